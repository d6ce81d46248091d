"""CPU: the host side of the thruster fault diagnosis on the two-stage wrench form (include/ftmpc.h, ftmpc_hull_offsets_batch,
ftmpc_simulate_wrench_diagnosis_batch, ftmpc_multi_simulate_wrench_diagnosis_batch; input_bounds.hull_offsets).

The input hull is a zonotope, so the facet normals of a pattern with fewer live thrusters are among those of the pattern it started
from and only the offsets change.  Checked here: the three entries are exported and no struct changed size; hull_offsets against
hull_tables on start patterns and against zonotope_hrep of every non-flat pattern of one to three faults on both vehicles; its flat
flag against the rank test on all 2 678 patterns of one to four faults; the oracle solves the same program on (start table,
recomputed offsets) as on the pattern's own table; the opt-in of the front end and its refusals.

Measured here: offsets against zonotope_hrep within 3.6e-15 (bound 1e-13); the smallest relative width of a non-flat pattern 5.3e-3,
the largest of a flat one 9.7e-16 (criterion 1e-9); oracle wrenches within 2.2e-13 f_max (bound 1e-9 f_max, the accuracy DESIGN.md
states for the polished float64 solution)."""
import ctypes as C
import subprocess
from itertools import combinations
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from ft_mpc_amd.controllers.tools.input_bounds import hull_normals, hull_offsets, hull_tables, zonotope_hrep
from oracle import qp_oracle as qo
from oracle import refmath as rm

ROOT = Path(__file__).resolve().parents[1]
NEW = ("ftmpc_hull_offsets_batch", "ftmpc_simulate_wrench_diagnosis_batch", "ftmpc_multi_simulate_wrench_diagnosis_batch")
F_MAX = rm.F_MAX
VEHICLES = {16: rm.allocation_matrix_16(), 8: rm.allocation_matrix_8()}


def _healthy_table(D):
    n = hull_normals(D, np.arange(D.shape[1]))
    A = np.vstack([n, -n])
    return A[np.lexsort(np.round(A, 7).T[::-1])]


def _spans(D, ub):
    G = D[:, ub > 0]
    return G.shape[1] >= 6 and np.linalg.matrix_rank(G, tol=1e-9 * np.abs(G).max()) == 6


def _patterns(NT, kmax, rng):
    """every pattern of 1..kmax dead or stuck thrusters: (ub, stuck), the stuck levels random in [0, f_max]"""
    for k in range(1, kmax + 1):
        for idx in combinations(range(NT), k):
            ub, stuck = np.full(NT, F_MAX), np.zeros(NT)
            ub[list(idx)] = 0.0
            stuck[list(idx)] = rng.uniform(0.0, F_MAX, k) * (rng.random(k) < 0.7)
            yield idx, ub, stuck


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_three_entries():
    from ft_mpc_amd import _lib
    _lib.build_library()
    lib = _lib.load_library()
    header = (ROOT / "include" / "ftmpc.h").read_text()
    for n in NEW:
        assert n in _lib.SYMBOLS and getattr(lib, n) is not None
        assert f"int {n}(" in header
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert lib.ftmpc_simulate_wrench_diagnosis_batch.argtypes[:-3] == lib.ftmpc_simulate_wrench_estimator_batch.argtypes
    assert lib.ftmpc_simulate_wrench_diagnosis_batch.argtypes[-3:] == [C.POINTER(_lib.ftmpc_diagnosis), dp, ip]
    assert lib.ftmpc_multi_simulate_wrench_diagnosis_batch.argtypes == lib.ftmpc_simulate_wrench_diagnosis_batch.argtypes
    assert lib.ftmpc_version() == 540


def test_no_campaign_struct_changed_size(tmp_path):
    from ft_mpc_amd import _lib
    names = dict(ftmpc_diagnosis=152, ftmpc_estimator=136, ftmpc_sensor=96, ftmpc_actuator=80, ftmpc_outcomes=120, ftmpc_plant_model=48,
                 ftmpc_mission=56, ftmpc_fault_schedule=56)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "ftmpc.h"\nint main(void){'
                   + "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names) + "return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for n, size in names.items():
        assert int(got[n]) == C.sizeof(getattr(_lib, n)) == size, n


# ---------------------------------------------------------------------------------------------------------------------------
# offsets
# ---------------------------------------------------------------------------------------------------------------------------
def test_offsets_equal_hull_tables_on_start_patterns():
    D = VEHICLES[16]
    _, ub, stuck, _ = qo.make_batch(600, 20, 16, 2, 5)
    T = hull_tables(D, ub, stuck, rows=32)                      # 26 facets, six padding rows
    ok = ~T["degenerate"]
    b, flat = hull_offsets(T["A"][T["set"]], D, ub, stuck)
    assert np.abs(b[ok] - T["b"][ok]).max() <= 1e-13 and (b[:, 26:] == 1.0).all()
    assert not flat[ok].any()
    # (a degenerate vehicle has no table of its own; on the healthy vehicle's normals its pattern shows as flat)
    assert np.array_equal(hull_offsets(_healthy_table(D), D, ub, stuck)[1], T["degenerate"]) and T["degenerate"].any()
    b1, f1 = hull_offsets(T["A"][T["set"][3]], D, ub[3], stuck[3])      # one vehicle, one table
    assert np.array_equal(b1, b[3]) and f1 is bool(flat[3])


@pytest.mark.parametrize("NT", [16, 8])
def test_offsets_on_the_healthy_table_are_every_patterns_own(NT):
    """Every non-flat pattern of one to three faults: each of the pattern's own normals is a row of the healthy table, and
    hull_offsets on that row is zonotope_hrep's offset."""
    D = VEHICLES[NT]
    A0 = _healthy_table(D)
    rng = np.random.default_rng(7920 + NT)
    worst, count = 0.0, 0
    for idx, ub, stuck in _patterns(NT, 3, rng):
        if not _spans(D, ub):
            continue
        A, b = zonotope_hrep(D, ub, stuck)
        b0, flat = hull_offsets(A0, D, ub, stuck)
        assert not flat, idx
        d = np.abs(A[:, None, :] - A0[None, :, :]).max(axis=2)
        row = d.argmin(axis=1)
        assert d.min(axis=1).max() <= 1e-9, idx                 # the subset property
        worst = max(worst, np.abs(b0[row] - b).max())
        # the rows that are no longer facets are valid for every corner of the new set: b0_r is the support function
        assert (b0 >= A0 @ (D @ (ub / 2 + stuck)) - 1e-12).all()
        count += 1
    print(f"NT = {NT}: {count} non-flat patterns, offsets within {worst:.2e} of zonotope_hrep")
    assert count == (666 if NT == 16 else 36)
    assert worst <= 1e-13


def test_flat_flag_is_the_rank_test():
    total, widths = 0, dict(flat=0.0, solid=np.inf)
    rng = np.random.default_rng(7930)
    for NT, D in VEHICLES.items():
        A0 = _healthy_table(D)
        c = np.abs(A0 @ D)
        a1 = np.abs(A0).sum(axis=1)
        for idx, ub, stuck in _patterns(NT, 4, rng):
            _, flat = hull_offsets(A0, D, ub, stuck)
            spans = _spans(D, ub)
            assert flat == (not spans), (NT, idx)
            rel = ((c @ ub) / (a1 * np.abs(D).max() * ub.max())).min()
            key = "solid" if spans else "flat"
            widths[key] = max(widths[key], rel) if key == "flat" else min(widths[key], rel)
            if NT == 16 and len(idx) == 2:
                assert flat == (idx in ((12, 13), (14, 15))), idx
            total += 1
    print(f"{total} patterns; smallest relative width of a non-flat pattern {widths['solid']:.2e}, largest of a flat one {widths['flat']:.2e}")
    assert total == 2678
    assert widths["solid"] > 1e-6 and widths["flat"] < 1e-12      # the criterion 1e-9 lies far from both


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle does not mind the redundant rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NT,nfault,seed", [(8, 1, 7910), (8, 2, 7911), (16, 2, 7912)])
def test_oracle_on_the_start_table_with_recomputed_offsets(NT, nfault, seed):
    N = 10
    cfg = qo.QPConfig(N=N, NT=NT)
    A0 = _healthy_table(cfg.D)
    x0, ub, stuck, xref = qo.make_batch(8, N, NT, nfault, seed)
    worst, done = 0.0, 0
    for b in range(8):
        b0, flat = hull_offsets(A0, cfg.D, ub[b], stuck[b])
        assert flat == (not _spans(cfg.D, ub[b]))
        if flat:
            continue
        own = zonotope_hrep(cfg.D, ub[b], stuck[b])
        _, T0, st0, it0, _ = qo.solve_wrench_instance(cfg, x0[b], ub[b], stuck[b], xref, hull=(A0, b0), mu_polish=1e-7)
        _, T1, st1, it1, _ = qo.solve_wrench_instance(cfg, x0[b], ub[b], stuck[b], xref, hull=own, mu_polish=1e-7)
        assert st0 == 0 and st1 == 0, (b, st0, st1)
        worst = max(worst, np.abs(T0 - T1).max() / F_MAX)
        done += 1
        print(f"  instance {b}: rows {A0.shape[0]} / {own[0].shape[0]}, iterations {it0} / {it1}")
    print(f"NT = {NT}, {nfault} faults: {done} non-flat instances, wrenches within {worst:.2e} f_max")
    assert done > 0 and worst <= 1e-9


# ---------------------------------------------------------------------------------------------------------------------------
# the front end: opt-in and refusals (raised before the library is reached, so a stand-in for the handle will do)
# ---------------------------------------------------------------------------------------------------------------------------
def test_front_end_opt_in_and_refusals():
    from ft_mpc_amd.batch import MPCConfig, _simulate
    N, NT, B, T = 15, 16, 4, 3
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 0, 3)
    obj = SimpleNamespace(cfg=MPCConfig(N=N, NT=NT), D=VEHICLES[16])
    xr = np.zeros((9, T + N))
    dg = dict(levels=(0.0, F_MAX), resid_sigma=(1e-2, 1e-2), threshold=18.0)

    def call(formulation, diagnosis, **kw):
        return _simulate(obj, False, x0, ub, stuck, xr, T, None, (0.0,) * 4, 0, False, 0, 8, 1e-9, formulation, None, 0.0, kw.get("faults"),
                         0, False, None, False, 0, None, diagnosis=diagnosis)
    with pytest.raises(ValueError, match="thruster formulation.*rebuild_hull"):
        call("wrench", dg)
    with pytest.raises(ValueError, match="thruster formulation"):
        call("wrench", dict(dg, rebuild_hull=False))
    for extra in (dict(rebuild_hull=True), dict(hull_b=np.ones((B, 26))), dict(no_hull=np.full(B, -1, np.int32))):
        with pytest.raises(ValueError, match="formulation='wrench'"):
            call("thruster", dict(dg, **extra))
    with pytest.raises(ValueError, match="no_hull"):
        call("wrench", dict(dg, rebuild_hull=True, no_hull=np.array([-1, -2, -1, -1], np.int32)))
    with pytest.raises(ValueError, match="no_hull"):
        call("wrench", dict(dg, rebuild_hull=True, no_hull=np.full(B + 1, -1, np.int32)))
    with pytest.raises(ValueError, match="unknown keys"):      # the common keys are still ft_mpc_amd.diagnosis.request's
        call("wrench", dict(dg, rebuild_hull=True, rebuild=True))
    with pytest.raises(ValueError, match="threshold"):
        call("wrench", dict(dg, rebuild_hull=True, threshold=0.0))
