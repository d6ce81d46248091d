"""GPU: every kernel family on a controller model without the default's structural zeros (tests/other_vehicle.py: dense inertia,
r and f_virt with three components, a dense terminal weight P, distinct Q / R entries, other dt, mass, rho and D).

Every other GPU test creates its handle with ftmpc_default_config's vehicle, where a dropped or transposed off-diagonal term, a
swapped r[0] / r[2] or P[i][j] read as P[j][i] multiplies a zero or meets its equal.  tests/test_other_vehicle_host.py shows on the
CPU that the oracle is right on this vehicle, that every constant put back to its default moves u0 of these batches by at least
1e-2 f_max, and that the batches with terminal-set / state-bound rows meet their conditions.  The layers, in the order to read a
failure in:

  A  linearise records (full-record, direction-split and four-share kernels; with and without a disturbance estimate), 1e-9 of scale
  B  the condensed QP of the fp32 build (2e-5 of scale) and of the float64 build (1e-11)
  C  the one-shot entry of every solve family against the oracle, at the tolerance DESIGN.md section 2 holds for that path
  D  the two cost kernels
  E  two short closed loops (plant step, warm-start shift, the linearisation in the loop)

Handles are made once per configuration and session; every batch is small (B <= 65) and every shape the smallest that reaches the
instantiation named.  Each test prints its worst figure before it asserts (DESIGN.md section 2 has them).

Found by layer A when it was written: with r[0] or r[2] non-zero the shares kernel (<double, 2>) gave records a few ulp (up to 7e-15)
from those of the full-record and one-direction kernels, all three within 1e-9 of the oracle.  The lever arm is now split in the
kernel so that its off-axis part is added in a fixed shape (CHANGELOG); the bit comparison of the three kernels below holds it."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))

from ft_mpc_amd import disturbances as DS
from ft_mpc_amd.controllers.tools.terminal_ingredients import load_terminal
from oracle import alloc_oracle as ao
from oracle import c_oracle as co
from oracle import closed_loop as cl
from oracle import qp_oracle as qo
from oracle import refmath as rm
import other_vehicle as ov
import wrench_state_rows as ws
from test_gpu_linearize_records import BLOCKS, REC, _batch, _check_against_oracle, _inputs
from test_gpu_wrench_sqp import cost_wrench

pytestmark = pytest.mark.gpu
F_MAX = rm.F_MAX
TOL_REC = 1e-9      # both sides float64, a stage ~1e3 operations: rounding ~1e-13; a dropped term is of order dt |w| J01 / J00 ~ 1e-3

_handles = {}


def _handle(factory, N, NT, fields=ov.ALL, **kw):
    """(handle, the equal QPConfig) of the other vehicle with the groups `fields` replaced; one handle per configuration and session"""
    vkw, q = ov.vehicle(N, NT, fields)
    key = repr((N, NT, tuple(fields), sorted((k, np.asarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v)) for k, v in kw.items())))
    if key not in _handles:
        _handles[key] = factory(**vkw, **kw)
    return _handles[key], q


def _term():
    t = load_terminal().term_set
    return t.A, t.b.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------
# A  linearise records
# ---------------------------------------------------------------------------------------------------------------------------
def _three(factory, N, NT, fields=ov.ALL, shares=16):
    """full-record kernel, direction-split kernel (the default), lin_split_max = shares (four shares of the directions for batches up
    to twice that, two shares up to five times: B = 24 and B = 65 at 16)"""
    full, q = _handle(factory, N, NT, fields, lin_split_max=-1)
    return (full, _handle(factory, N, NT, fields)[0], _handle(factory, N, NT, fields, lin_split_max=shares)[0]), q


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("N,NT,B", [(3, 8, 65), (2, 16, 24)])
def test_records_of_the_three_kernels_against_the_oracle(gpu_mpc_factory, N, NT, B, warm):
    handles, q = _three(gpu_mpc_factory, N, NT)
    d = _batch(B, N, NT)
    recs = [m.debug_records(**_inputs(d, warm)) for m in handles]
    assert recs[0].shape == (B, N, 152)
    for r in recs[1:]:
        assert np.array_equal(recs[0], r), np.argwhere(recs[0] != r)[:8]
    _check_against_oracle(recs[0], handles[0], d, warm, N, NT, range(B), cfg=q, tol=TOL_REC)
    assert np.array_equal(handles[0].P, q.P) and np.array_equal(handles[0].r, q.r)
    for m in handles:      # a zero estimate: the bits of the plain records
        assert np.array_equal(m.debug_records_disturbance(dist=np.zeros((B, 6)), **_inputs(d, warm)), recs[0])


@pytest.mark.parametrize("fields", ov.FIELDS)
def test_records_with_one_group_of_constants_replaced(gpu_mpc_factory, fields):
    """One group at a time, so that a failure of the test above names its constant (lin_split_max = 2: B = 5 takes two shares)."""
    N, NT, B = 2, 8, 5
    (full, split, shares), q = _three(gpu_mpc_factory, N, NT, (fields,), shares=2)
    d = _batch(B, N, NT)
    for warm in (False, True):
        ra = full.debug_records(**_inputs(d, warm))
        for other in (split, shares):
            rb = other.debug_records(**_inputs(d, warm))
            assert np.array_equal(ra, rb), np.argwhere(ra != rb)[:8]
        _check_against_oracle(ra, full, d, warm, N, NT, range(B), cfg=q, tol=TOL_REC)


def _rollout(cfg, r, x0, ub, stuck, warm, f, t, N):
    """c_0 .. c_N of the linearisation trajectory under the estimate and the gen of every stage (ft_mpc_amd.disturbances)"""
    c, gens = [DS.to_centre(x0, cfg, r)], []
    for k in range(N):
        u = np.where(ub > 0, np.clip(warm[k], 0.0, ub), 0.0)
        gens.append(np.asarray(cfg.D, float) @ (u + stuck))
        c.append(DS.centre_step(c[-1], gens[-1], f, t, cfg, r))
    return c, gens


@pytest.mark.parametrize("N,NT,B", [(3, 8, 65), (2, 16, 24)])
def test_records_with_a_disturbance_estimate(gpu_mpc_factory, N, NT, B):
    """As test_gpu_disturbances.py::test_what_the_solve_reads, at its bounds: W e against the restatement's rollout within BOUND_WE =
    1.3e-13 of max(1, |W e|) and never looser than 1e-3 of what the disturbance changes, R ut the undisturbed bits (no uref), the A
    and B blocks against central differences (step 1e-6) within 1e-7 of max(1, |block|)."""
    handles, q = _three(gpu_mpc_factory, N, NT)
    d = _batch(B, N, NT)
    inp = dict(x0=d["x0"], ub=d["ub"], stuck=d["stuck"], xref=d["xref"], warmU=d["W"].copy())
    rng = np.random.default_rng(29)
    dist = np.concatenate([rng.normal(size=(B, 3)) * 0.5, rng.normal(size=(B, 3)) * 0.05], axis=1)
    plain = handles[0].debug_records(**inp)
    recs = [m.debug_records_disturbance(dist=dist, **inp) for m in handles]
    for r in recs[1:]:
        assert np.array_equal(recs[0], r), np.argwhere(recs[0] != r)[:8]
    rec = recs[0]
    assert np.array_equal(rec[:, :, REC["RUT"]:REC["RUT"] + 6], plain[:, :, REC["RUT"]:REC["RUT"] + 6])
    cfg, r, xref = handles[0].cfg, handles[0].r, d["xref"].reshape(9, N + 1, order="F")
    worst_we, worst_blk, least_gap, h = 0.0, 0.0, np.inf, 1e-6
    for b in sorted({0, B // 2 + 1, B - 1}):      # (B // 2 is the batch's failed vehicle: included through the bits above)
        f, t = dist[b, 0:3], dist[b, 3:6]
        c, gens = _rollout(cfg, r, d["x0"][b], d["ub"][b], d["stuck"][b], d["W"][b], f, t, N)
        c0, _ = _rollout(cfg, r, d["x0"][b], d["ub"][b], d["stuck"][b], d["W"][b], 0 * f, 0 * t, N)
        for k in range(N):
            e, e0 = c[k + 1][0:9] - xref[:, k + 1], c0[k + 1][0:9] - xref[:, k + 1]
            we, we0 = (q.Q * e, q.Q * e0) if k + 1 < N else (q.P @ e, q.P @ e0)
            dv = np.abs(rec[b, k, REC["WE"]:REC["WE"] + 9] - we).max() / max(1.0, np.abs(we).max())
            gap = np.abs(we - we0).max() / max(1.0, np.abs(we).max())
            worst_we, least_gap = max(worst_we, dv), min(least_gap, gap)
            assert dv <= min(1.3e-13, 1e-3 * gap), (b, k, dv, gap)
            A, Bg = np.zeros((13, 13)), np.zeros((13, 6))
            for i in range(6, 13):
                dd = np.zeros(13)
                dd[i] = h
                A[:, i] = (DS.centre_step(c[k] + dd, gens[k], f, t, cfg, r) - DS.centre_step(c[k] - dd, gens[k], f, t, cfg, r)) / (2 * h)
            for i in range(6):
                dd = np.zeros(6)
                dd[i] = h
                Bg[:, i] = (DS.centre_step(c[k], gens[k] + dd, f, t, cfg, r) - DS.centre_step(c[k], gens[k] - dd, f, t, cfg, r)) / (2 * h)
            for name, (m, (r0, r1), (c0_, c1_)) in BLOCKS.items():
                ref = (A if m == "A" else Bg)[r0:r1, c0_:c1_]
                blk = rec[b, k, REC[name]:REC[name] + ref.size].reshape(ref.shape)
                dvb = np.abs(blk - ref).max() / max(1.0, np.abs(ref).max())
                worst_blk = max(worst_blk, dvb)
                assert dvb <= 1e-7, (b, k, name, dvb)
    print(f"other vehicle ({N}, {NT}): records under an estimate: W e within {worst_we:.2e}, blocks within {worst_blk:.2e} of central "
          f"differences; the estimate moves W e by at least {least_gap:.2e}")
    assert least_gap > 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# B  build
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol,tol_box", [("f32", 2e-5, 1e-6), ("f64", 1e-11, 1e-12)])
@pytest.mark.parametrize("nfault", [0, 1, 2])
def test_build_matches_oracle(gpu_mpc_factory, nfault, dtype, tol, tol_box):
    """fp32: the tolerances of test_gpu_parity.py::test_build_matches_oracle; float64: those of test_f64_kernel_reference_vehicle (the
    level at which a single entry of R is held, see test_other_vehicle_host.py)."""
    N, NT = 20, 8
    mpc, q = _handle(gpu_mpc_factory, N, NT, dtype=dtype)
    x0, ub, stuck, xref = ov.plain_batch(N, NT, nfault, 8)
    worst = [0.0, 0.0]
    for inst in (0, 3, 7):
        H, g, lo, hi = mpc.debug_build_qp(x0, ub, stuck, xref.reshape(-1, order="F"), inst)
        qp = qo.build_qp(q, x0[inst], ub[inst], stuck[inst], xref)
        assert H.shape == qp["H"].shape
        eH = np.abs(H - qp["H"]).max() / np.abs(qp["H"]).max()
        eg = np.abs(g - qp["g"]).max() / max(1.0, np.abs(qp["g"]).max())
        worst = [max(worst[0], eH), max(worst[1], eg)]
        assert eH <= tol and eg <= tol, (inst, eH, eg)
        assert np.allclose(lo, -qp["Ubar"], atol=tol_box) and np.allclose(hi, qp["ub"] - qp["Ubar"], atol=tol_box)
    print(f"other vehicle build {dtype} faults {nfault}: H within {worst[0]:.2e}, g within {worst[1]:.2e} of scale")


# ---------------------------------------------------------------------------------------------------------------------------
# C  every solve family
# ---------------------------------------------------------------------------------------------------------------------------
def _thruster_step(factory, N, NT, nf, B, tol_u0, tol_U, polish, kernel=None, **hkw):
    """solve() of one handle against the C oracle: every instance converged on both sides, u0 and U within the tolerances."""
    mpc, q = _handle(factory, N, NT, **hkw)
    x0, ub, stuck, xref = ov.plain_batch(N, NT, nf, B)
    if kernel is not None:
        mpc.set_profiling(True)
    out = mpc.solve(x0, ub, stuck, xref.reshape(-1, order="F"), return_U=True)
    if kernel is not None:
        ms = mpc.last_kernel_ms()
        mpc.set_profiling(False)
        assert any(kernel in k for k in ms), (kernel, ms)
    ref = co.solve_batch(q, x0, ub, stuck, xref, nthreads=4, max_iters=60, mu_stop=1e-13, polish=polish)
    assert (ref["status"] == 0).all()
    e0, eU = np.abs(out["u0"] - ref["u0"]).max() / F_MAX, np.abs(out["U"] - ref["U"]).max() / F_MAX
    print(f"other vehicle solve N={N} NT={NT} faults={nf} {hkw}: u0 within {e0:.2e}, U within {eU:.2e} f_max, iters {out['iters'].mean():.1f}")
    assert (out["status"] == 0).all(), out["status"]
    assert e0 <= tol_u0 and eU <= tol_U, (e0, eU)
    assert (out["u0"][ub == 0] == 0).all()


@pytest.mark.parametrize("N,nf,B", [(20, 2, 8), (20, 1, 8), (20, 0, 8), (3, 2, 16), (23, 2, 16)])
def test_kernel_2_eight_thrusters_fp32(gpu_mpc_factory, N, nf, B):
    """ftmpc_solve_f32_kernel<8>, <9>, <10> (n = 120, 140, 160 at N = 20), the scalar tail of the gradient sweeps (N = 3) and the MFMA
    form of struct_grad (N >= 22)."""
    nb = -(-N * (8 - nf) // 16)
    _thruster_step(gpu_mpc_factory, N, 8, nf, B, 1e-4, 1e-4, True, kernel=f"ftmpc_solve_f32_kernel<{max(nb, 8)}>")


@pytest.mark.parametrize("N,nf", [(11, 0), (11, 2), (17, 2)])
def test_kernel_10_sixteen_thrusters_fp32(gpu_mpc_factory, N, nf):
    """ftmpc_solve_wsw32_kernel<6> (6 N <= 96) and <8>: the QP through wrench space on one wave per instance."""
    _thruster_step(gpu_mpc_factory, N, 16, nf, 16, 1e-4, 1e-4, True, kernel="ftmpc_solve_wsw32_kernel")


@pytest.mark.parametrize("sel,nf,kernel", [("workgroup", 2, "ftmpc_solve_ws32_kernel"), ("workgroup", 0, "ftmpc_solve_ws32_kernel"),
                                           ("dense", 2, "ftmpc_solve_f32_kernel<10>"), ("dense", 0, "ftmpc_solve_wg32_kernel")])
def test_kernels_8_and_7_sixteen_thrusters_fp32(gpu_mpc_factory, sel, nf, kernel):
    """Kernel 8 takes the instances of ten and eleven blocks (n = 154 with two faults, 176 with none); with kernel_select = "dense" those
    of ten blocks stay on the one-wave kernel and kernel 7 takes the nominal vehicle."""
    _thruster_step(gpu_mpc_factory, 11, 16, nf, 16, 1e-4, 1e-4, True, kernel=kernel, kernel_select=sel)


@pytest.mark.parametrize("N,NT", [(3, 8), (17, 16), (25, 16)])
def test_kernel_12_float64(gpu_mpc_factory, N, NT):
    """ftmpc_solve_ric64_kernel<4>, <6>, <10> against the polished port."""
    _thruster_step(gpu_mpc_factory, N, NT, 2, 16, 1e-7, 1e-6, True, kernel="ftmpc_solve_ric64_kernel", dtype="f64", max_iters=40)


@pytest.mark.parametrize("sel,kernel", [("dense", "ftmpc_solve_f64_kernel"), ("workgroup", "ftmpc_solve_ws64_kernel")])
@pytest.mark.parametrize("N", [5, 7])
def test_kernels_3_and_9_float64(gpu_mpc_factory, N, sel, kernel):
    """The dense float64 kernel (MODE 0) and the float64 wrench-space kernel run the interior-point iteration to mu 1e-13 alone: held
    against the port without its polish."""
    _thruster_step(gpu_mpc_factory, N, 16, 2, 16, 1e-7, 1e-6, False, kernel=kernel, dtype="f64", max_iters=40, kernel_select=sel)


def _wrench_step(factory, N, NT, B, tol, iters_within, batch=None, term=False, state=False, **hkw):
    """solve_wrench() of one handle against the oracle's general-constraint solver instance by instance: the same verdicts, G within
    tol f_max where the oracle solves, non-zero status and finite outputs where it does not; u0 against the oracle's allocation of
    the oracle's tau0.  Returns (solved, instances with an active special row)."""
    extra = dict(terminal_set=True) if term else {}
    if state:
        extra.update(zip(("xlb", "xub"), ws.bounds()))
    mpc, q = _handle(factory, N, NT, **extra, **hkw)
    x0, ub, stuck, xref = ov.plain_batch(N, NT, 2, B) if batch is None else batch(q)
    out = mpc.solve_wrench(x0, ub, stuck, xref.reshape(-1, order="F"), return_G=True)
    At, bt = _term()
    solved = active = 0
    worst = worst_u = 0.0
    with np.errstate(all="ignore"):
        for b in range(B):
            if out["status"][b] == 3:      # the healthy thrusters do not span R^6: no hull on either side
                with pytest.raises(ValueError):
                    qo.zonotope_hrep(q.D, ub[b], stuck[b])
                continue
            if state:
                tau0, T, st, nit, qp = ws.solve_wrench_state_instance(q, x0[b], ub[b], stuck[b], xref, *ws.bounds())
            else:
                tau0, T, st, nit, qp = qo.solve_wrench_instance(q, x0[b], ub[b], stuck[b], xref, term_set=(At, bt) if term else None,
                                                                iters=60, mu_polish=1e-7)
            assert (out["status"][b] == 0) == (st == 0), (b, out["status"][b], st)
            assert np.isfinite(out["G"][b]).all() and np.isfinite(out["u0"][b]).all()
            if st != 0:
                continue
            solved += 1
            assert max(qo.kkt_general(qp["H"], qp["g"], qp["C"], qp["h"], qp["d"], qp["z"])) < 1e-7
            err = np.abs(out["G"][b] - T).max() / F_MAX
            worst = max(worst, err)
            assert err <= tol, (b, err)
            if iters_within is not None:
                assert abs(int(out["iters"][b]) - nit) <= iters_within, (b, out["iters"][b], nit)
            active += int((qp["z"][qp["nhull"]:] > (1e-6 if term else 0.0)).any()) if (term or state) else 0
            ref_u = ao.allocate(q.D, tau0 - q.D @ stuck[b], ub[b])[0]
            assert out["alloc_status"][b] == 0
            eu = np.abs(out["u0"][b] - ref_u).max() / F_MAX
            worst_u = max(worst_u, eu)
            assert eu <= max(tol, 1e-6), (b, eu)
            assert (out["u0"][b][ub[b] == 0] == 0).all() and (out["u0"][b] >= -1e-12).all() and (out["u0"][b] <= ub[b] + 1e-9).all()
    print(f"other vehicle solve_wrench N={N} NT={NT} term={term} state={state} {hkw}: solved {solved}/{B}, special rows active on "
          f"{active}, G within {worst:.2e}, u0 within {worst_u:.2e} f_max")
    return solved, active


@pytest.mark.parametrize("N", [5, 25])
def test_kernel_13_float64_two_stage(gpu_mpc_factory, N):
    """ftmpc_solve_ricw64_kernel<6> and <10> (the seam of pick_ricw64 is N = 24): wrenches, iterations, allocation."""
    solved, _ = _wrench_step(gpu_mpc_factory, N, 16, 16, 1e-6, 1, dtype="f64", max_iters=40)
    assert solved >= 12


@pytest.mark.parametrize("hkw,tol", [(dict(dtype="f32", max_iters=40), 1e-4), (dict(dtype="f64", max_iters=40, kernel_select="dense"), 1e-6)],
                         ids=["kernel-11", "kernel-3-mode-1"])
def test_kernels_11_and_3_two_stage(gpu_mpc_factory, hkw, tol):
    """Kernel 11 (fp32, one wave per instance) with its hand-over, and the dense float64 kernel's hull mode."""
    solved, _ = _wrench_step(gpu_mpc_factory, 5, 16, 16, tol, None, **hkw)
    assert solved >= 12


def _term_batch(q):
    t = ov.TERM
    return ov.near_terminal_set(q, t["B"], t["nf"], t["seed"], *_term(), t["scale"])


def test_kernel_13_with_the_terminal_set(gpu_mpc_factory):
    t = ov.TERM
    solved, active = _wrench_step(gpu_mpc_factory, t["N"], t["NT"], t["B"], 1e-6, None, batch=_term_batch, term=True, dtype="f64", max_iters=60)
    assert 2 * solved >= t["B"] and 4 * active >= t["B"], (solved, active)


@pytest.mark.parametrize("sel,kernel", [("riccati", "ftmpc_solve_ric64_kernel"), ("auto", "ftmpc_solve_f64_kernel")])
def test_kernels_12_and_3_with_the_terminal_set(gpu_mpc_factory, sel, kernel):
    """The thruster form with the 72 terminal rows: kernel 12's terminal-set instantiation and the dense kernel's MODE 2."""
    t = ov.TERM
    N, NT, B = t["N"], t["NT"], t["B"]
    At, bt = _term()
    mpc, q = _handle(gpu_mpc_factory, N, NT, dtype="f64", max_iters=60, terminal_set=True, kernel_select=sel)
    x0, ub, stuck, xref = _term_batch(q)
    mpc.set_profiling(True)
    out = mpc.solve(x0, ub, stuck, xref.reshape(-1, order="F"), return_U=True)
    ms = mpc.last_kernel_ms()
    mpc.set_profiling(False)
    assert any(kernel in k for k in ms), (kernel, ms)
    solved = active = 0
    worst = 0.0
    with np.errstate(all="ignore"):
        for b in range(B):
            _, U, st, _, qp = qo.solve_box_terminal_instance(q, x0[b], ub[b], stuck[b], xref, (At, bt), iters=60)
            assert (out["status"][b] == 0) == (st == 0), (b, out["status"][b], st)
            assert np.isfinite(out["U"][b]).all() and np.isfinite(out["u0"][b]).all()
            if st != 0:
                continue
            solved += 1
            assert max(qo.kkt_general(qp["H"], qp["g"], qp["C"], qp["h"], qp["d"], qp["z"])) < 1e-7
            err = np.abs(out["U"][b] - U).max() / F_MAX
            worst = max(worst, err)
            assert err <= 1e-6, (b, err)
            active += int((qp["z"][qp["nhull"]:] > 1e-6).any())
    print(f"other vehicle terminal set, thruster form, {sel}: solved {solved}/{B}, rows active on {active}, U within {worst:.2e} f_max")
    assert 2 * solved >= B and 4 * active >= B, (solved, active)


@pytest.mark.parametrize("shape", ov.STATE)
def test_kernel_13_with_state_bounds(gpu_mpc_factory, shape):
    N, NT, nf, B, seed = shape
    solved, active = _wrench_step(gpu_mpc_factory, N, NT, B, 1e-4, None, batch=lambda q: ov.near_state_bounds(q, B, nf, seed), state=True,
                                  dtype="f64", max_iters=60)
    assert 2 * solved >= B and 4 * active >= B, (solved, active)


@pytest.mark.parametrize("shape", ov.STATE)
def test_kernel_12_with_state_bounds(gpu_mpc_factory, shape):
    N, NT, nf, B, seed = shape
    xlb, xub = ws.bounds()
    mpc, q = _handle(gpu_mpc_factory, N, NT, dtype="f64", max_iters=60, xlb=xlb, xub=xub)
    x0, ub, stuck, xref = ov.near_state_bounds(q, B, nf, seed)
    out = mpc.solve(x0, ub, stuck, xref.reshape(-1, order="F"), return_U=True)
    solved = active = 0
    worst = 0.0
    with np.errstate(all="ignore"):
        for b in range(B):
            _, U, st, _, qp = qo.solve_box_state_instance(q, x0[b], ub[b], stuck[b], xref, xlb, xub, iters=60)
            assert (out["status"][b] == 0) == (st == 0), (b, out["status"][b], st)
            assert np.isfinite(out["U"][b]).all() and np.isfinite(out["u0"][b]).all()
            if st != 0:
                continue
            solved += 1
            assert max(qo.kkt_general(qp["H"], qp["g"], qp["C"], qp["h"], qp["d"], qp["z"])) < 1e-7
            err = np.abs(out["U"][b] - U).max() / F_MAX
            worst = max(worst, err)
            assert err <= 1e-4, (b, err)
            active += int(ws.active_state_rows(qp) > 0)
    print(f"other vehicle state bounds, thruster form, {shape}: solved {solved}/{B}, rows active on {active}, U within {worst:.2e} f_max")
    assert 2 * solved >= B and 4 * active >= B, (solved, active)


# ---------------------------------------------------------------------------------------------------------------------------
# D  cost kernels
# ---------------------------------------------------------------------------------------------------------------------------
class _TerminalCost:
    """e' P e with the handle's P plus the non-quadratic terms of config/terminal.yaml: what a handle with terminal_cost and its own
    P evaluates (the quadratic part travels as P)."""

    def __init__(self, P):
        self.P, self.T = P, load_terminal()

    def cost(self, e):
        return float(e @ self.P @ e) + self.T.cost(e, quadratic=False)


def _window(N, B=None):
    traj = rm.circle_trajectory(0.1, 10, radius=0.65, s_per_circle=40.0)
    xr_all, ur_all = rm.assign_trajectory(traj, N)
    return rm.trajectory_window(xr_all, ur_all, 0.5, N)


@pytest.mark.parametrize("tcost", [False, True], ids=["quadratic", "terminal-cost"])
def test_eval_cost_against_the_oracle(gpu_mpc_factory, tcost):
    """ftmpc_eval_cost_batch against qo.nlp_cost at the tolerance of test_cost_and_gradient_of_the_nonlinear_program (1e-10 relative)."""
    N, NT, B = 6, 8, 8
    mpc, q = _handle(gpu_mpc_factory, N, NT, **(dict(terminal_cost=True) if tcost else {}))
    tc = _TerminalCost(q.P).cost if tcost else None
    x0, ub, stuck, xref = ov.plain_batch(N, NT, 2, B)
    U = np.random.default_rng(1).uniform(0, F_MAX, (B, N, NT)) * (ub[:, None, :] > 0)
    xw, uw = _window(N)
    worst = 0.0
    for xr, ur in ((xref, None), (xw, uw)):
        J = mpc.eval_cost(x0, ub, stuck, xr.reshape(-1, order="F"), U, None if ur is None else ur.reshape(-1, order="F"))
        for b in range(B):
            ref = qo.nlp_cost(q, x0[b], ub[b], stuck[b], xr, U[b], ur, tc)
            worst = max(worst, abs(J[b] - ref) / abs(ref))
            assert J[b] == pytest.approx(ref, rel=1e-10), (b, J[b], ref)
    print(f"other vehicle eval_cost terminal_cost={tcost}: within {worst:.2e} relative")


@pytest.mark.parametrize("tcost", [False, True], ids=["quadratic", "terminal-cost"])
def test_eval_cost_wrench_against_its_restatement(gpu_mpc_factory, tcost):
    """ftmpc_eval_cost_wrench_batch against cost_wrench of test_gpu_wrench_sqp.py: cost 1e-10 relative, terminal violation 1e-12."""
    N, NT, B = 6, 16, 8
    term = _term()
    mpc, q = _handle(gpu_mpc_factory, N, NT, dtype="f64", terminal_set=True, **(dict(terminal_cost=True) if tcost else {}))
    tc = _TerminalCost(q.P) if tcost else None
    x0, ub, stuck, xref = ov.near_terminal_set(q, B, 2, 9506, *term, scale=1.5)
    G = ((ub / 2 + stuck) @ q.D.T)[:, None, :] + np.random.default_rng(N).uniform(-1.0, 1.0, (B, N, 6))
    xw, uw = _window(N)
    per_x, per_u = np.stack([xw.reshape(-1, order="F")] * B), np.stack([uw.reshape(-1, order="F")] * B)
    worst, nviol = 0.0, 0
    for xr, ur, xr_h, ur_h in ((xref.reshape(-1, order="F"), None, xref, None), (per_x, per_u, xw, uw)):
        J, V = mpc.eval_cost_wrench(x0, xr, G, uref=ur, return_tviol=True)
        for b in range(B):
            Jr, Vr, _ = cost_wrench(q, x0[b], xr_h, G[b], ur_h, tc, term)
            worst = max(worst, abs(J[b] - Jr) / abs(Jr))
            assert J[b] == pytest.approx(Jr, rel=1e-10), (b, J[b], Jr)
            assert abs(V[b] - Vr) <= 1e-12, (b, V[b], Vr)
            nviol += Vr > 0
    print(f"other vehicle eval_cost_wrench terminal_cost={tcost}: within {worst:.2e} relative, {nviol} points outside the set")
    assert nviol >= 4


# ---------------------------------------------------------------------------------------------------------------------------
# E  closed loops
# ---------------------------------------------------------------------------------------------------------------------------
def _hover_traj(N, T):
    xr = np.zeros((9, T + N))
    xr[8] = 0.6
    return xr


def test_thruster_loop_against_the_oracle_loop(gpu_mpc_factory):
    """ftmpc_simulate_batch on the float64 kernel against oracle/closed_loop.py:simulate at the tolerances of
    test_on_device_closed_loop_matches_oracle_loop_f64 (u 1e-6 N, x 1e-7)."""
    N, NT, B, T = 5, 16, 5, 6
    mpc, q = _handle(gpu_mpc_factory, N, NT, dtype="f64", max_iters=40)
    x0, ub, stuck, _ = ov.plain_batch(N, NT, 2, B)
    xr = _hover_traj(N, T)
    out = mpc.simulate(x0, ub, stuck, xr, T, seed=5, return_inputs=True)
    xo, uo = cl.simulate(q, x0, ub, stuck, xr, T, seed=5)
    eu, ex = np.abs(out["u"] - uo).max(), np.abs(out["x"] - xo).max()
    print(f"other vehicle thruster loop: u within {eu:.2e} N, x within {ex:.2e}")
    assert out["not_converged"].sum() == 0
    assert eu < 1e-6 and ex < 1e-7
    assert np.allclose(np.linalg.norm(out["x"][:, 6:10], axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("dtype,tol", [("f64", 1e-6), ("f32", 1e-4)])
def test_two_stage_loop_against_the_oracle_loop(gpu_mpc_factory, dtype, tol):
    """ftmpc_simulate_wrench_batch against oracle/closed_loop.py:simulate_wrench at the tolerances of
    test_on_device_two_stage_loop_against_the_oracle_loop."""
    N, NT, B, T = 5, 16, 5, 6
    mpc, q = _handle(gpu_mpc_factory, N, NT, dtype=dtype, max_iters=60)
    x0, ub, stuck, _ = ov.plain_batch(N, NT, 2, B)
    xr = _hover_traj(N, T)
    out = mpc.simulate(x0, ub, stuck, xr, T, seed=21, return_inputs=True, formulation="wrench")
    xo, uo, _, sto, asto = cl.simulate_wrench(q, x0, ub, stuck, xr, T, seed=21)
    assert (sto == 0).all() and (asto == 0).all()
    e0, eu, ex = np.abs(out["u"][0] - uo[0]).max() / F_MAX, np.abs(out["u"] - uo).max() / F_MAX, np.abs(out["x"] - xo).max()
    print(f"other vehicle two-stage loop {dtype}: first u within {e0:.2e}, u within {eu:.2e} f_max, x within {ex:.2e}")
    assert out["not_converged"].sum() == 0 and out["alloc_failed"].sum() == 0
    assert e0 <= tol and eu <= 2 * tol and ex <= 2 * tol
