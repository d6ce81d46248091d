"""CPU: the host side of the reference missions and the closed-loop cost (include/ftmpc.h, ftmpc_mission; ft_mpc_amd/missions.py;
ft_mpc_amd/outcomes.py closed_loop_cost): the four entries are exported, the ctypes struct has the layout gcc gives the header,
window against plain slicing, mission_tables' padding, phase_offsets' bounds and slice property, the cost restatement against
explicit loops written here from oracle.refmath, and the refusals Python raises before any call reaches the library."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import refmath as rm

ROOT = Path(__file__).resolve().parents[1]
NEW = ("ftmpc_simulate_mission_batch", "ftmpc_simulate_wrench_mission_batch", "ftmpc_multi_simulate_mission_batch",
       "ftmpc_multi_simulate_wrench_mission_batch")


def test_library_exports_the_mission_entries():
    from ft_mpc_amd import _lib
    _lib.build_library()
    lib = _lib.load_library()
    header = (ROOT / "include" / "ftmpc.h").read_text()
    for n in NEW:
        assert n in _lib.SYMBOLS and getattr(lib, n) is not None
        assert f"int {n}(" in header
    assert lib.ftmpc_version() >= 520
    # the last argument of each is the struct
    assert lib.ftmpc_simulate_mission_batch.argtypes[:-1] == lib.ftmpc_simulate_plant_batch.argtypes
    assert lib.ftmpc_simulate_wrench_mission_batch.argtypes[:-1] == lib.ftmpc_simulate_wrench_plant_batch.argtypes
    assert lib.ftmpc_multi_simulate_mission_batch.argtypes[:-1] == lib.ftmpc_multi_simulate_plant_batch.argtypes
    assert lib.ftmpc_multi_simulate_wrench_mission_batch.argtypes[:-1] == lib.ftmpc_multi_simulate_wrench_plant_batch.argtypes


def test_mission_struct_layout_matches_the_header(tmp_path):
    from ft_mpc_amd import _lib
    fields = [f for f, _ in _lib.ftmpc_mission._fields_]
    assert fields == ["struct_size", "n_tables", "n_cols", "xref", "uref", "table", "offset", "cost"]
    src = tmp_path / "layout.c"
    body = "".join(f'printf("{f} %zu\\n", offsetof(ftmpc_mission, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftmpc.h"\nint main(void){printf("sizeof %zu\\n", sizeof(ftmpc_mission));'
                   + body + 'printf("outcomes %zu\\n", sizeof(ftmpc_outcomes));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.ftmpc_mission) == 56
    for f in fields:
        assert int(got[f]) == getattr(_lib.ftmpc_mission, f).offset, f
    assert int(got["outcomes"]) == C.sizeof(_lib.ftmpc_outcomes) == 120        # no existing struct changed


# ---------------------------------------------------------------------------------------------------------------------------
# missions.py
# ---------------------------------------------------------------------------------------------------------------------------
def _mission(rng, K=3, Cn=50, B=11):
    return dict(tables=rng.standard_normal((K, 9, Cn)), utables=rng.standard_normal((K, 6, Cn)),
                table=(7 * np.arange(B) % K).astype(np.int32), offset=(5 * np.arange(B) % 23).astype(np.int32))


def test_window_is_plain_slicing():
    from ft_mpc_amd.missions import window
    m = _mission(np.random.default_rng(0))
    N = 10
    for b in range(11):
        for t in (0, 3, 16):
            k, o = int(m["table"][b]), int(m["offset"][b])
            xw, uw = window(m, b, t, N)
            assert xw.shape == (9, N + 1) and uw.shape == (6, N + 1)
            assert np.array_equal(xw, m["tables"][k][:, o + t:o + t + N + 1])
            assert np.array_equal(uw, m["utables"][k][:, o + t:o + t + N + 1])
    # defaults: table 0, offset 0, no uref
    xw, uw = window(dict(tables=m["tables"]), 4, 2, N)
    assert uw is None and np.array_equal(xw, m["tables"][0][:, 2:N + 3])
    with pytest.raises(ValueError):
        window(m, 9, 50 - 22 - N, N)          # offset 22: the last column would be 50


def test_error_columns_are_the_columns_the_header_names():
    from ft_mpc_amd.missions import error_columns
    m = _mission(np.random.default_rng(1))
    T = 9
    xr, ur = error_columns(m, 11, T)
    assert xr.shape == (T, 11, 9) and ur.shape == (T, 11, 6)
    for t in range(T):
        for b in range(11):
            k, o = int(m["table"][b]), int(m["offset"][b])
            assert np.array_equal(xr[t, b], m["tables"][k][:, o + t + 1])
            assert np.array_equal(ur[t, b], m["utables"][k][:, o + t])


def test_mission_tables_pads_with_the_last_column():
    from ft_mpc_amd.missions import mission_tables
    rng = np.random.default_rng(2)
    a, b, c = rng.standard_normal((9, 30)), rng.standard_normal((9, 12)), rng.standard_normal((9, 1))
    t = mission_tables([a, b, c])
    assert t.shape == (3, 9, 30) and t.dtype == np.float64
    assert np.array_equal(t[0], a)
    assert np.array_equal(t[1][:, :12], b) and np.array_equal(t[1][:, 12:], np.repeat(b[:, -1:], 18, axis=1))
    assert np.array_equal(t[2], np.repeat(c, 30, axis=1))
    # as the reference pads past the end of a trajectory (it then overwrites the rows 6:9 with omega_des)
    ext, _ = rm.assign_trajectory(b, 18)
    assert np.array_equal(t[1][0:6], ext[0:6])
    u = mission_tables([rng.standard_normal((6, 4)), rng.standard_normal((6, 7))], rows=6)
    assert u.shape == (2, 6, 7)
    with pytest.raises(ValueError):
        mission_tables([a, rng.standard_normal((8, 30))])
    with pytest.raises(ValueError):
        mission_tables([])


def test_phase_offsets_bounds_and_slices():
    from ft_mpc_amd.missions import phase_offsets
    whole = phase_offsets(96, 23, seed=5)
    assert whole.shape == (96,) and whole.dtype == np.int32
    assert whole.min() >= 0 and whole.max() < 23 and len(np.unique(whole)) > 12
    assert np.array_equal(np.concatenate([phase_offsets(40, 23, 5, index0=0), phase_offsets(56, 23, 5, index0=40)]), whole)
    assert not np.array_equal(phase_offsets(96, 23, seed=6), whole)
    assert (phase_offsets(50, 1, seed=5) == 0).all()
    with pytest.raises(ValueError):
        phase_offsets(4, 0, 1)


def test_phase_offsets_share_no_counter_with_the_plant_dispersion():
    """One seed for dispersion.sample and phase_offsets must give a phase that is independent of the plant: both draw from the same
    generator at counter v * 32 + component, so the phase needs a component of its own.  Checked structurally, and on the draws:
    for B independent uniform pairs the sample correlation has standard deviation 1 / sqrt(B); the bound is 5 of them (a shared
    counter gives a correlation of 1: floor(n u) against 2 u - 1)."""
    from ft_mpc_amd import dispersion as dsp
    from ft_mpc_amd.missions import phase_offsets
    taken = {dsp.C_MASS} | {dsp.C_INERTIA + i for i in range(3)} | {dsp.C_COM + i for i in range(3)} \
        | {dsp.C_FORCE + i for i in range(3)} | {dsp.C_TORQUE + i for i in range(3)} | {dsp.C_GAIN + i for i in range(16)}
    assert len(taken) == 29 and dsp.C_PHASE not in taken and 0 <= dsp.C_PHASE < dsp.STRIDE
    B, NT, n, seed = 4096, 16, 200, 5
    p = dsp.sample(B, NT, rm.allocation_matrix_16(), rm.INERTIA, rm.MASS, seed, mass_rel=0.1, inertia_rel=0.1, gain_rel=0.05,
                   com_offset=0.01, force=0.05, torque=0.005)
    off = phase_offsets(B, n, seed).astype(float)
    assert len(np.unique(off)) > n // 2
    bound = 5.0 / np.sqrt(B)
    worst = 0.0
    for name, a in p.items():
        a = np.asarray(a, float).reshape(B, -1)
        for k in range(a.shape[1]):
            if np.ptp(a[:, k]) > 0:
                worst = max(worst, abs(np.corrcoef(off, a[:, k])[0, 1]))
    print("largest |correlation| of the phase with a dispersed plant parameter:", worst, "bound", bound)
    assert worst < bound
    # what the bound would catch: the mass's own counter
    shared = np.floor(n * dsp.u01(seed, np.arange(B, dtype=np.uint64) * np.uint64(dsp.STRIDE) + np.uint64(dsp.C_MASS)))
    assert abs(np.corrcoef(shared, p["mass"])[0, 1]) > 0.99


# ---------------------------------------------------------------------------------------------------------------------------
# outcomes.closed_loop_cost against loops
# ---------------------------------------------------------------------------------------------------------------------------
def _histories(rng, T, B, NT):
    x = rng.standard_normal((T + 1, B, 13))
    x[..., 6:10] /= np.linalg.norm(x[..., 6:10], axis=-1, keepdims=True)
    u = rng.uniform(0, 3.4, (T, B, NT))
    pu = np.where(rng.random((T, B, NT)) < 0.2, 0.0, 3.4)
    ps = np.where(pu == 0, rng.uniform(0, 2, (T, B, NT)), 0.0)
    return x[0], x[1:], u, pu, ps


def _cost_loops(Q, R, P, D, fv, r, x0, xh, u, pu, ps, xcol, ucol, v_nq=None):
    T, B = xh.shape[:2]
    cost = np.zeros((B, 3))
    for b in range(B):
        for t in range(T):
            e = rm.robot_to_center(xh[t, b], r)[:9] - xcol(t, b)
            cost[b, 0] += sum(Q[i] * e[i] * e[i] for i in range(9))
            a = np.array([(u[t, b, i] if pu[t, b, i] > 0 else 0.0) + ps[t, b, i] for i in range(u.shape[2])])
            q = (x0[b] if t == 0 else xh[t - 1, b])[6:10]
            ur = ucol(t, b)
            w = D @ a - np.concatenate([rm.rot(q).T @ ur[:3], ur[3:]]) - np.concatenate([fv, np.zeros(3)])
            cost[b, 1] += sum(R[i] * w[i] * w[i] for i in range(6))
            cost[b, 2] = e @ P @ e + (0.0 if v_nq is None else v_nq(e))
    return cost


def test_closed_loop_cost_against_loops_per_vehicle_reference():
    from ft_mpc_amd.missions import error_columns
    from ft_mpc_amd.outcomes import closed_loop_cost
    rng = np.random.default_rng(3)
    T, B, NT = 7, 11, 8
    m = _mission(rng, B=B)
    x0, xh, u, pu, ps = _histories(rng, T, B, NT)
    A = rng.standard_normal((9, 9))
    P = A @ A.T
    D, r = rm.allocation_matrix_8(), rm.spiral_r()
    xr, ur = error_columns(m, B, T)
    got = closed_loop_cost(rm.Q_DIAG, rm.R_DIAG, P, D, rm.F_VIRT, r, x0, xh, u, pu, ps, xr, ur)
    ref = _cost_loops(rm.Q_DIAG, rm.R_DIAG, P, D, rm.F_VIRT, r, x0, xh, u, pu, ps,
                      lambda t, b: m["tables"][m["table"][b]][:, m["offset"][b] + t + 1],
                      lambda t, b: m["utables"][m["table"][b]][:, m["offset"][b] + t])
    print(np.abs(got - ref).max(), np.abs(ref).max())
    np.testing.assert_allclose(got, ref, rtol=1e-13, atol=1e-13)
    # the rotation matters and is the one of the state the step started from
    norot = closed_loop_cost(rm.Q_DIAG, rm.R_DIAG, P, D, rm.F_VIRT, r, xh[0], xh, u, pu, ps, xr, ur)
    assert np.abs(norot[:, 1] - ref[:, 1]).max() > 1e-3 and np.array_equal(norot[:, [0, 2]], got[:, [0, 2]])


def test_closed_loop_cost_shared_reference_terminal_terms_and_no_steps():
    from ft_mpc_amd.outcomes import closed_loop_cost
    rng = np.random.default_rng(4)
    T, B, NT = 5, 6, 16
    x0, xh, u, pu, ps = _histories(rng, T, B, NT)
    xt, ut = rng.standard_normal((9, T + 10)), rng.standard_normal((6, T + 10))
    P = np.diag(rng.uniform(1, 3, 9))
    D, r = rm.allocation_matrix_16(), rm.spiral_r()
    v_nq = lambda e: 0.3 * e[..., 0] ** 4 + np.sqrt(e[..., 4] ** 2 + 1e-3)
    got = closed_loop_cost(rm.Q_DIAG, rm.R_DIAG, P, D, rm.F_VIRT, r, x0, xh, u, pu[0], ps[0], xt, ut, v_nq)
    ref = _cost_loops(rm.Q_DIAG, rm.R_DIAG, P, D, rm.F_VIRT, r, x0, xh, u, np.repeat(pu[:1], T, 0), np.repeat(ps[:1], T, 0),
                      lambda t, b: xt[:, t + 1], lambda t, b: ut[:, t], v_nq)
    np.testing.assert_allclose(got, ref, rtol=1e-13, atol=1e-13)
    # without uref: zero
    got0 = closed_loop_cost(rm.Q_DIAG, rm.R_DIAG, P, D, rm.F_VIRT, r, x0, xh, u, pu, ps, xt)
    ref0 = _cost_loops(rm.Q_DIAG, rm.R_DIAG, P, D, rm.F_VIRT, r, x0, xh, u, pu, ps, lambda t, b: xt[:, t + 1], lambda t, b: np.zeros(6))
    np.testing.assert_allclose(got0, ref0, rtol=1e-13, atol=1e-13)
    # T = 0: zero
    none = closed_loop_cost(rm.Q_DIAG, rm.R_DIAG, P, D, rm.F_VIRT, r, x0, xh[:0], u[:0], pu[0], ps[0], xt)
    assert none.shape == (B, 3) and not none.any()


# ---------------------------------------------------------------------------------------------------------------------------
# what Python refuses before the library is called (no handle, no GPU: _mission_request and the argument check of _simulate)
# ---------------------------------------------------------------------------------------------------------------------------
def test_python_side_refusals():
    from ft_mpc_amd.batch import MPCConfig, _mission_request, _simulate
    B, T, N = 6, 4, 10
    good = dict(tables=np.zeros((2, 9, 40)), utables=np.zeros((2, 6, 40)), table=np.zeros(B, np.int32), offset=np.arange(B))
    ms, keep, cost = _mission_request(good, B, T, N, True)
    assert (ms.n_tables, ms.n_cols) == (2, 40) and cost.shape == (B, 3) and len(keep) == 4
    assert ms.struct_size == 56 and bool(ms.xref) and bool(ms.uref) and bool(ms.table) and bool(ms.offset) and bool(ms.cost)
    ms, keep, cost = _mission_request(None, B, T, N, True)           # the struct only asks for cost
    assert ms.n_tables == 0 and not bool(ms.xref) and not bool(ms.table) and cost.shape == (B, 3)
    ms, _, cost = _mission_request(dict(tables=good["tables"]), B, T, N, False)
    assert cost is None and not bool(ms.cost) and not bool(ms.uref) and not bool(ms.table) and not bool(ms.offset)
    bad = [
        dict(utables=good["utables"]),                                       # no tables
        dict(tables=np.zeros((2, 8, 40))),                                   # 8 rows
        dict(tables=np.zeros((9, 40))),                                      # one table without its axis
        dict(tables=np.zeros((0, 9, 40))),
        dict(tables=good["tables"], utables=np.zeros((2, 6, 39))),
        dict(tables=good["tables"], utables=np.zeros((1, 6, 40))),
        dict(tables=good["tables"], table=np.zeros(B + 1, np.int32)),
        dict(tables=good["tables"], offset=np.zeros(B)),                     # floats
        dict(tables=good["tables"], offset=np.zeros((B, 1), np.int32)),
        dict(tables=good["tables"], phase=np.zeros(B, np.int32)),            # unknown key
    ]
    for m in bad:
        with pytest.raises(ValueError):
            _mission_request(m, B, T, N, False)

    class Stub:      # _simulate refuses before it touches the handle
        cfg = MPCConfig(N=N, NT=8)
    args = (np.zeros((B, 13)), np.zeros((B, 8)), np.zeros((B, 8)))
    tail = (None, (0,) * 4, 0, False, 0, 8, 1e-9, "thruster", None, 0.0, None, 0, False, None, False, 0, None, None)
    with pytest.raises(ValueError, match="xref_traj"):
        _simulate(Stub(), False, *args, np.zeros((9, T + N)), T, *tail, good)
    with pytest.raises(ValueError, match="xref_traj"):
        _simulate(Stub(), False, *args, None, T, np.zeros((6, T + N)), *tail[1:], good)
    with pytest.raises(ValueError, match="mission"):
        _simulate(Stub(), False, *args, None, T, *tail, dict(tables=np.zeros((2, 8, 40))))
