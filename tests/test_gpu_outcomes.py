"""GPU: per-vehicle campaign outcomes reduced on the device (ftmpc_outcome_kernel; ftmpc_simulate_outcomes_batch,
ftmpc_simulate_wrench_outcomes_batch), the campaign-wide noise counter (index0 / index_total) and the closed loops on the
multi-GPU driver (ftmpc_multi_simulate_*).

The NumPy reference below is written from oracle/refmath.robot_to_center and the definitions of include/ftmpc.h (ftmpc_outcomes);
it does not use ft_mpc_amd/outcomes.py.  Floats: rtol 1e-12 + atol 1e-12 (sums of at most 12 terms of a few roundings each, added
in the same order; FMA contraction is the only source of difference).  Integers: exact -- every band tolerance is the midpoint of
two neighbouring recorded norms and the tests assert that no recorded norm / terminal-row residual lies within 1e-9 of a threshold."""
import ctypes as C

import numpy as np
import pytest

import ft_mpc_amd
from ft_mpc_amd import _lib
from ft_mpc_amd._lib import FtmpcError
from ft_mpc_amd.controllers.tools.terminal_ingredients import load_terminal
from ft_mpc_amd.sharding import MultiGPUMPC
from oracle import qp_oracle as qo
from oracle import refmath as rm
from test_gpu_wrench import _near_terminal_set

pytestmark = pytest.mark.gpu
DT = 0.1
FLOATS = ("err_int", "err_max", "impulse")
INTS = ("settle_step", "tset_step", "unsolved", "first_unsolved", "alloc_failed")


def _hover(N, T):
    xr = np.zeros((9, T + N))
    xr[8] = 0.6
    return xr


def _errors(x_hist, xr):
    """e [T,B,9] = robot_to_center(x_{t+1})[0:9] - xref[:, t+1]."""
    T, B = x_hist.shape[:2]
    r = rm.spiral_r()
    e = np.empty((T, B, 9))
    for t in range(T):
        for b in range(B):
            e[t, b] = rm.robot_to_center(x_hist[t, b], r)[:9] - xr[:, t + 1]
    return e


def _norms(e):
    return np.stack([np.linalg.norm(e[..., 3 * j:3 * j + 3], axis=-1) for j in range(3)], axis=-1)


def _plant_patterns(ub, stuck, faults, T):
    pu, ps = np.repeat(ub[None], T, 0), np.repeat(stuck[None], T, 0)
    for b in range(ub.shape[0]):
        for k in range(faults["onset"].shape[1]):
            on = faults["onset"][b, k]
            if on >= 0:
                pu[on:, b], ps[on:, b] = faults["ub"][b, k], faults["stuck"][b, k]
    return pu, ps


def _reference(x_hist, u_hist, status_hist, xr, pu, ps, tol=None, term=None):
    T, B = x_hist.shape[:2]
    e = _errors(x_hist, xr)
    nrm = _norms(e)
    out = dict(err_int=np.zeros((B, 3)), err_max=nrm.max(axis=0), impulse=np.zeros((B, 2)))
    cmd = np.where(pu > 0.0, u_hist, 0.0)
    for t in range(T):
        out["err_int"] += DT * nrm[t] ** 2
        out["impulse"][:, 0] += DT * (cmd[t] + ps[t]).sum(axis=1)
        out["impulse"][:, 1] += DT * cmd[t].sum(axis=1)
    if tol is not None:
        assert np.abs(nrm - np.asarray(tol)).min() > 1e-9
        outside = (nrm > np.asarray(tol)).any(axis=-1)
        out["settle_step"] = np.array([max([t + 1 for t in range(T) if outside[t, b]], default=0) for b in range(B)], np.int32)
    if term is not None:
        res = np.einsum("rj,tbj->tbr", term[0], e) - term[1]
        assert np.abs(res).min() > 1e-9
        inside = (res <= 0).all(axis=-1)
        out["tset_step"] = np.array([next((t for t in range(T) if inside[t, b]), -1) for b in range(B)], np.int32)
    bad = status_hist != 0
    out["unsolved"] = bad.sum(axis=0).astype(np.int32)
    out["first_unsolved"] = np.array([next((t for t in range(T) if bad[t, b]), -1) for b in range(B)], np.int32)
    return out


def _compare(got, ref):
    for k in FLOATS:
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-12, atol=1e-12, err_msg=k)
    for k in INTS:
        if k in ref:
            assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (k, got[k], ref[k])


def _band(nrm):
    """Per norm the midpoint of two neighbouring recorded values next to the median of the last step's: about half of the
    vehicles end inside."""
    tol = []
    for j in range(3):
        s = np.unique(nrm[..., j])
        k = min(np.searchsorted(s, np.median(nrm[-1, :, j])), len(s) - 2)
        tol.append(0.5 * (s[k] + s[k + 1]))
    return tuple(tol)


def _bits(a, b, keys):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def term():
    t = load_terminal().term_set
    return t, np.asarray(t.A, float).reshape(-1, 9), np.asarray(t.b, float).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------
# the thruster batch of cases 1, 2, 4, 5: one event per vehicle at steps 3..8, detected two steps late on half of the vehicles,
# the broken thruster stuck on every third
# ---------------------------------------------------------------------------------------------------------------------------
def _thruster_batch(B, N, seed=11):
    NT, T = 8, 12
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 0, seed)
    onset = (3 + np.arange(B) % 6).astype(np.int32)[:, None]
    eub, est = np.repeat(ub[:, None], 1, 1).copy(), np.zeros((B, 1, NT))
    for b in range(B):
        eub[b, 0, b % NT] = 0.0
        est[b, 0, b % NT] = 1.7 if b % 3 == 0 else 0.0
    delay = np.where(np.arange(B) % 2 == 0, 2, 0)
    return dict(N=N, NT=NT, T=T, B=B, x0=x0, ub=ub, stuck=stuck, xr=_hover(N, T), faults=dict(onset=onset, ub=eub, stuck=est),
                delay=delay, seed=5)


def _run(mpc, bt, lo=0, hi=None, **kw):
    hi = bt["B"] if hi is None else hi
    f = {k: v[lo:hi] for k, v in bt["faults"].items()}
    return mpc.simulate(bt["x0"][lo:hi], bt["ub"][lo:hi], bt["stuck"][lo:hi], bt["xr"], bt["T"], noise=(1e-3,) * 4, seed=bt["seed"],
                        faults=f, detect_delay=bt["delay"][lo:hi], return_inputs=True, return_states=True, **kw)


@pytest.fixture(scope="module")
def case1(gpu_mpc_factory, term):
    bt = _thruster_batch(96, 10)
    mpc = gpu_mpc_factory(N=10, NT=8, dtype="f32", terminal_set=term[0], terminal_set_active=False)
    plain = _run(mpc, bt)                                           # the _faults_ entry
    tol = _band(_norms(_errors(plain["x_hist"], bt["xr"])))
    out = _run(mpc, bt, outcomes=dict(tol_pos=tol[0], tol_vel=tol[1], tol_rate=tol[2]), return_status=True)
    return bt, mpc, plain, tol, out


def test_thruster_outcomes_equal_numpy_from_the_runs_own_histories(case1, term):
    bt, _, _, tol, out = case1
    o = out["outcomes"]
    assert sorted(o) == sorted(FLOATS + INTS[:4])                 # the thruster form has no alloc_failed
    pu, ps = _plant_patterns(bt["ub"], bt["stuck"], bt["faults"], bt["T"])
    assert (pu != bt["ub"]).any() and (ps[-1] > 0).any()
    ref = _reference(out["x_hist"], out["u"], out["status_hist"], bt["xr"], pu, ps, tol, term[1:])
    for k in FLOATS + INTS[:4]:
        print(k, np.abs(np.asarray(o[k], float) - ref[k]).max())
    _compare(o, ref)
    assert (o["settle_step"] < bt["T"]).any() and (o["settle_step"] == bt["T"]).any()
    assert not np.allclose(o["impulse"][:, 0], o["impulse"][:, 1])         # a stuck thruster delivers what nobody commanded
    assert o["unsolved"].sum() == out["not_converged"].sum()


def test_asking_for_outcomes_changes_nothing_thruster(case1):
    _, _, plain, _, out = case1
    assert "outcomes" not in plain and "status_hist" not in plain
    _bits(out, plain, ("x", "u", "x_hist", "not_converged"))


def test_unsolved_steps_per_vehicle(gpu_mpc_factory):
    """max_iters = 5 is the smallest cap with mixed statuses on this batch: at 4 every solve of the run ends at the cap (status 1
    on all 12 x 96), at 5 about 1 % finish, at 6 a third, from 13 on all of them."""
    bt = _thruster_batch(96, 10)
    out = _run(gpu_mpc_factory(N=10, NT=8, dtype="f32", max_iters=5), bt, outcomes=True, return_status=True)
    sh = out["status_hist"]
    assert (sh == 0).any() and (sh != 0).any()
    bad = sh != 0
    assert np.array_equal(out["outcomes"]["unsolved"], bad.sum(axis=0))
    assert np.array_equal(out["outcomes"]["first_unsolved"], np.where(bad.any(axis=0), bad.argmax(axis=0), -1))
    assert np.array_equal(bad.sum(axis=1), out["not_converged"])
    assert "tset_step" not in out["outcomes"] and "settle_step" not in out["outcomes"]


# ---------------------------------------------------------------------------------------------------------------------------
# the wrench batch of cases 3, 4, 6: float64 handle with the terminal set, half of the states well inside the set, half far out
# ---------------------------------------------------------------------------------------------------------------------------
def _wrench_batch(term):
    N, NT, B, T = 15, 16, 40, 10
    _, At, bt_ = term
    from ft_mpc_amd import faults as fl
    D = rm.allocation_matrix_16()

    def group(seed, scale):
        """B / 2 vehicles with an event each: the first healthy thruster whose loss (stuck at 0.5) leaves the hull full-dimensional;
        candidates without one (their two initial faults already flatten the hull) are dropped."""
        x0, ub, stuck, xref = _near_terminal_set(B // 2 + 6, N, NT, 2, seed, At, bt_, scale)
        keep, eub, est = [], [], []
        for b in range(x0.shape[0]):
            for k in np.flatnonzero(ub[b] > 0):
                eu, es = ub[b:b + 1, None].copy(), stuck[b:b + 1, None].copy()
                eu[0, 0, k], es[0, 0, k] = 0.0, 0.5
                if not fl.fault_hull_tables(D, ub[b:b + 1], stuck[b:b + 1], eu, es, np.array([[2]], np.int32))["degenerate"].any():
                    keep.append(b)
                    eub.append(eu[0])
                    est.append(es[0])
                    break
        keep = keep[:B // 2]
        assert len(keep) == B // 2
        return x0[keep], ub[keep], stuck[keep], np.array(eub[:B // 2]), np.array(est[:B // 2]), xref
    near, far = group(9941, 0.5), group(9942, 8.0)
    x0, ub, stuck, eub, est = (np.concatenate([a, b]) for a, b in zip(near[:5], far[:5]))
    xref = near[5]
    xr = np.concatenate([xref, np.repeat(xref[:, -1:], T - 1, axis=1)], axis=1)
    onset = (2 + np.arange(B) % 5).astype(np.int32)[:, None]
    return dict(N=N, NT=NT, T=T, B=B, x0=x0, ub=ub, stuck=stuck, xr=xr, faults=dict(onset=onset, ub=eub, stuck=est), seed=9)


def _run_wrench(mpc, bt, **kw):
    return mpc.simulate(bt["x0"], bt["ub"], bt["stuck"], bt["xr"], bt["T"], noise=(1e-4,) * 4, seed=bt["seed"], faults=bt["faults"],
                        formulation="wrench", return_inputs=True, return_states=True, **kw)


@pytest.fixture(scope="module")
def case3(gpu_mpc_factory, term):
    bt = _wrench_batch(term)
    mpc = gpu_mpc_factory(N=15, NT=16, dtype="f64", max_iters=60, terminal_set=term[0])
    plain = _run_wrench(mpc, bt)
    out = _run_wrench(mpc, bt, outcomes=True, return_status=True)
    return bt, mpc, plain, out


def test_wrench_outcomes(case3, term):
    bt, _, _, out = case3
    o = out["outcomes"]
    pu, ps = _plant_patterns(bt["ub"], bt["stuck"], bt["faults"], bt["T"])
    ref = _reference(out["x_hist"], out["u"], out["status_hist"], bt["xr"], pu, ps, None, term[1:])
    _compare(o, ref)
    assert (o["tset_step"] == -1).any() and (o["tset_step"] >= 0).any()
    assert o["alloc_failed"].sum() == out["alloc_failed"].sum() and o["alloc_failed"].shape == (bt["B"],)
    assert o["unsolved"].sum() == out["not_converged"].sum()


def test_asking_for_outcomes_changes_nothing_wrench(case3):
    _, _, plain, out = case3
    _bits(out, plain, ("x", "u", "x_hist", "not_converged", "alloc_failed"))


def test_outputs_the_form_or_the_config_does_not_have_are_refused(gpu_mpc_factory, case1):
    bt, with_rows, _, _, _ = case1
    with pytest.raises(FtmpcError) as e:
        _run(with_rows, bt, outcomes=dict(fields=["alloc_failed"]))
    assert e.value.code == -1 and "alloc_failed" in str(e.value)
    with pytest.raises(FtmpcError) as e:
        _run(gpu_mpc_factory(N=10, NT=8, dtype="f32"), bt, outcomes=dict(fields=["tset_step"]))
    assert e.value.code == -1 and "tset_step" in str(e.value) and "term_rows" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------------
# 5: slices of a campaign are the campaign
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [10, 20])
def test_slices_with_the_campaign_index_equal_the_whole(N):
    bt = _thruster_batch(96, N)
    B = bt["B"]

    def fresh(lo, hi, **kw):
        mpc = ft_mpc_amd.BatchedMPC(N=N, NT=8, dtype="f32")
        try:
            return _run(mpc, bt, lo, hi, outcomes=True, return_status=True, **kw)
        finally:
            mpc.close()
    whole = fresh(0, B)
    parts = [fresh(0, 40, index0=0, index_total=B), fresh(40, B, index0=40, index_total=B)]
    assert np.array_equal(np.concatenate([p["x"] for p in parts]), whole["x"])
    for k in ("x_hist", "u", "status_hist"):
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), whole[k]), k
    for k in whole["outcomes"]:
        assert np.array_equal(np.concatenate([p["outcomes"][k] for p in parts]), whole["outcomes"][k]), k
    assert np.array_equal(parts[0]["not_converged"] + parts[1]["not_converged"], whole["not_converged"])
    local = fresh(40, B)                                          # its own counter: other noise
    assert not np.array_equal(local["x"], whole["x"][40:])


# ---------------------------------------------------------------------------------------------------------------------------
# 6: the multi-GPU driver
# ---------------------------------------------------------------------------------------------------------------------------
def _same(multi, serial):
    _bits(multi, serial, [k for k in ("x", "u", "x_hist", "not_converged", "alloc_failed", "status_hist") if k in serial])
    assert sorted(multi["outcomes"]) == sorted(serial["outcomes"])
    _bits(multi["outcomes"], serial["outcomes"], serial["outcomes"])


def test_multi_driver_equals_one_handle_thruster(gpu_mpc_factory):
    bt = _thruster_batch(100, 20)
    bt["T"] = 8
    bt["xr"] = _hover(20, 8)
    bt["faults"]["onset"] = np.minimum(bt["faults"]["onset"], 6)
    kw = dict(outcomes=dict(tol_pos=1.0, tol_vel=0.3, tol_rate=0.1), return_status=True)
    serial = _run(gpu_mpc_factory(N=20, NT=8, dtype="f32"), bt, **kw)
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=20, NT=8, dtype="f32"), devices=[0, 0, 0])
    try:
        assert [m.shard_bounds(100, g) for g in range(3)] == [(0, 33), (33, 66), (66, 100)]
        _same(_run(m, bt, **kw), serial)
        # refusals: the campaign index belongs to the driver; more slots than vehicles
        from ft_mpc_amd.batch import _simulate
        with pytest.raises(FtmpcError) as e:
            _simulate(m, True, bt["x0"], bt["ub"], bt["stuck"], bt["xr"], bt["T"], None, (1e-3,) * 4, 5, False, 0, 8, 1e-9, "thruster", None,
                      0.0, None, 0, False, True, False, 7, None)
        assert e.value.code == -1 and "index0" in str(e.value)
        with pytest.raises(FtmpcError) as e:
            m.simulate(bt["x0"][:2], bt["ub"][:2], bt["stuck"][:2], bt["xr"], bt["T"], outcomes=True)
        assert e.value.code == -1 and "slots" in str(e.value)
    finally:
        m.close()


@pytest.mark.parametrize("slots", [1, 2])
def test_multi_driver_equals_one_handle_wrench(case3, term, slots):
    bt, _, _, serial = case3
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=15, NT=16, dtype="f64", max_iters=60, terminal_set=term[0]), devices=[0] * slots)
    try:
        _same(_run_wrench(m, bt, outcomes=True, return_status=True), serial)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7: refusals of the struct
# ---------------------------------------------------------------------------------------------------------------------------
def test_struct_refusals(gpu_mpc_factory):
    bt = _thruster_batch(4, 10)
    mpc = gpu_mpc_factory(N=10, NT=8, dtype="f32")
    with pytest.raises(FtmpcError) as e:
        _run(mpc, bt, outcomes=True, index0=3, index_total=5)
    assert e.value.code == -1 and "index_total" in str(e.value)
    with pytest.raises(FtmpcError) as e:
        _run(mpc, bt, outcomes=True, index0=-1, index_total=8)
    assert e.value.code == -1 and "index0" in str(e.value)
    with pytest.raises(FtmpcError) as e:
        _run(mpc, bt, outcomes=dict(fields=["settle_step"]))
    assert e.value.code == -1 and "tol_pos" in str(e.value)
    with pytest.raises(FtmpcError) as e:
        _run(mpc, bt, outcomes=dict(fields=["settle_step"], tol_pos=0.1, tol_vel=float("inf"), tol_rate=0.1))
    assert e.value.code == -1 and "tol_vel" in str(e.value)
    # a struct of another size, straight at the C entry
    oc = _lib.ftmpc_outcomes(struct_size=C.sizeof(_lib.ftmpc_outcomes) - 8)
    x = bt["x0"].copy()
    dp = C.POINTER(C.c_double)
    nz = np.full(4, 1e-3)
    xr = np.ascontiguousarray(bt["xr"].reshape(-1, order="F"))
    rc = mpc.lib.ftmpc_simulate_outcomes_batch(mpc._h, 4, bt["T"], x.ctypes.data_as(dp), bt["ub"].ctypes.data_as(dp), bt["stuck"].ctypes.data_as(dp),
                                               xr.ctypes.data_as(dp), None, nz.ctypes.data_as(dp), C.c_uint64(1), 0, 8, 1e-9, None, None, None,
                                               None, C.byref(oc))
    assert rc == -1 and b"struct_size" in mpc.lib.ftmpc_last_error(mpc._h)
    assert np.array_equal(x, bt["x0"])
