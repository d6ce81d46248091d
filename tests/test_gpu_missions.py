"""GPU: reference missions and the closed-loop cost in the on-device closed loops (ftmpc_ref_window_kernel,
ftmpc_outcome_mission_kernel; ftmpc_simulate_mission_batch, ftmpc_simulate_wrench_mission_batch, ftmpc_multi_simulate_*_mission_batch;
BatchedMPC.simulate(mission=..., outcomes=dict(cost=True))).

The NumPy references are written here from oracle.refmath and the definitions of include/ftmpc.h (ftmpc_mission, ftmpc_outcomes);
they use neither ft_mpc_amd/missions.py nor ft_mpc_amd/outcomes.py.

A  one table is the shared loop, bit for bit; so are mission = NULL and n_tables = 0 / cost = NULL through ctypes.
B  a mission over contiguous groups is the existing shared entry called once per group as a slice of the campaign, bit for bit.
C  interleaved tables and offsets against a loop around the float64 C oracle (per-instance windows), with the tolerances of
   tests/test_gpu_closed_loop.py; vehicles on the hover table end exactly where the all-hover run puts them, the others elsewhere.
D  the records of ftmpc_outcomes under a mission against NumPy from the run's own histories with each vehicle's own column.
   Floats rtol 1e-12 + atol 1e-12 (sums of at most 12 terms of a few roundings each, added in the same order; FMA contraction is
   the only source of difference), integers exact: thresholds are midpoints of neighbouring recorded values and no recorded value
   lies within 1e-9 of one.
E  cost against NumPy from the run's own x0, x_hist, u and the PLANT's patterns, same bound: per step at most 9 + 6 + 81 products,
   added in step order.
F  the multi-GPU driver equals one handle bit for bit, cost included.
G  every refusal of the header, on a handle and on the driver."""
import ctypes as C

import numpy as np
import pytest

import ft_mpc_amd
from ft_mpc_amd import _lib
from ft_mpc_amd._lib import FtmpcError
from ft_mpc_amd.batch import _outcome_request
from ft_mpc_amd.controllers.tools.terminal_ingredients import load_terminal
from ft_mpc_amd.faults import normalize_schedule
from ft_mpc_amd.sharding import MultiGPUMPC
from oracle import c_oracle as co
from oracle import closed_loop as cl
from oracle import qp_oracle as qo
from oracle import refmath as rm
from test_gpu_outcomes import _band, _compare, _norms, _plant_patterns, _thruster_batch

pytestmark = pytest.mark.gpu
DT = 0.1
NOISE = (1e-3,) * 4
COLS = 64                      # columns per table: the largest offset (22) + T (12) + N (20) = 54 fits
STATE = ("x", "u", "x_hist", "not_converged", "status_hist")
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _tables(cols=COLS):
    """tables [3,9,cols], utables [3,6,cols]: hover; a circle of radius 0.5 m and period 40 s with its velocity and
    uref[0:3] = mass * acceleration; a line at 0.05 m/s.  omega = (0, 0, 0.6) on all."""
    t = DT * np.arange(cols)
    xt, ut = np.zeros((3, 9, cols)), np.zeros((3, 6, cols))
    xt[:, 8] = 0.6
    R, om = 0.5, 2 * np.pi / 40.0
    xt[1, 0], xt[1, 1] = R * np.cos(om * t) - R, R * np.sin(om * t)
    xt[1, 3], xt[1, 4] = -R * om * np.sin(om * t), R * om * np.cos(om * t)
    ut[1, 0], ut[1, 1] = -rm.MASS * R * om * om * np.cos(om * t), -rm.MASS * R * om * om * np.sin(om * t)
    xt[2, 0], xt[2, 3] = 0.05 * t, 0.05
    return xt, ut


XT, UT = _tables()


def _interleaved(B):
    return (7 * np.arange(B) % 3).astype(np.int32), (5 * np.arange(B) % 23).astype(np.int32)


def _columns(table, offset, T):
    """(xcol [T,B,9]: column offset + t + 1 of each vehicle's table, ucol [T,B,6]: column offset + t)."""
    B = len(table)
    xc, uc = np.empty((T, B, 9)), np.empty((T, B, 6))
    for t in range(T):
        for b in range(B):
            xc[t, b], uc[t, b] = XT[table[b]][:, offset[b] + t + 1], UT[table[b]][:, offset[b] + t]
    return xc, uc


def _sim(mpc, bt, lo=0, hi=None, xr=None, ur=None, mission=None, **kw):
    """bt: dict(x0, ub, stuck, T, seed[, faults, delay]) -- the vehicles [lo, hi) of it."""
    hi = len(bt["x0"]) if hi is None else hi
    f = None if bt.get("faults") is None else {k: v[lo:hi] for k, v in bt["faults"].items()}
    d = 0 if bt.get("delay") is None else bt["delay"][lo:hi]
    return mpc.simulate(bt["x0"][lo:hi], bt["ub"][lo:hi], bt["stuck"][lo:hi], xr, bt["T"], uref_traj=ur, noise=bt.get("noise", NOISE),
                        seed=bt["seed"], faults=f, detect_delay=d, return_inputs=True, return_states=True, mission=mission, **kw)


def _same(a, b, keys=STATE):
    for k in keys:
        if k in b or k in a:
            assert np.array_equal(a[k], b[k]), k
    if keys is STATE and ("outcomes" in b or "outcomes" in a):
        assert sorted(a["outcomes"]) == sorted(b["outcomes"])
        for k in b["outcomes"]:
            assert np.array_equal(a["outcomes"][k], b["outcomes"][k]), k


@pytest.fixture(scope="module")
def term():
    t = load_terminal().term_set
    return t, np.asarray(t.A, float).reshape(-1, 9), np.asarray(t.b, float).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------
# A: one table is the shared loop
# ---------------------------------------------------------------------------------------------------------------------------
def _c_call(obj, multi, bt, xr, ur, ms, oc=None, wrench=None):
    """The thruster mission entry straight through ctypes (handle or driver): (rc, message, dict(x, u, x_hist, not_converged))."""
    B, T, NT = len(bt["x0"]), bt["T"], bt["ub"].shape[1]
    x = np.ascontiguousarray(bt["x0"], dtype=np.float64).copy()
    ub, stuck = np.ascontiguousarray(bt["ub"], dtype=np.float64), np.ascontiguousarray(bt["stuck"], dtype=np.float64)
    nz = np.asarray(bt.get("noise", NOISE), float)
    uh, xh, bad = np.zeros((T, B, NT)), np.zeros((T, B, 13)), np.zeros(T, np.int32)
    sched, keep = None, None
    if bt.get("faults") is not None:
        onset, detect, eub, est = keep = normalize_schedule(bt["faults"], B, NT, T, bt["delay"])
        sched = _lib.ftmpc_fault_schedule(struct_size=C.sizeof(_lib.ftmpc_fault_schedule), n_events=onset.shape[1], onset=onset.ctypes.data_as(ip),
                                          detect=detect.ctypes.data_as(ip), ub=eub.ctypes.data_as(dp), stuck=est.ctypes.data_as(dp))
    xr = None if xr is None else np.ascontiguousarray(np.asarray(xr, float).reshape(-1, order="F"))
    ur = None if ur is None else np.ascontiguousarray(np.asarray(ur, float).reshape(-1, order="F"))
    p = lambda a, ct=dp: None if a is None else a.ctypes.data_as(ct)
    fn = obj.lib.ftmpc_multi_simulate_mission_batch if multi else obj.lib.ftmpc_simulate_mission_batch
    rc = fn(obj._h, B, T, p(x), p(ub), p(stuck), p(xr), p(ur), p(nz), C.c_uint64(bt["seed"]), 0, 8, 1e-9,
            C.byref(sched) if sched is not None else None, p(uh), p(xh), p(bad, ip), C.byref(oc) if oc is not None else None, None,
            C.byref(ms) if ms is not None else None)
    msg = (obj.lib.ftmpc_multi_last_error(obj._h) if multi else obj.lib.ftmpc_last_error(obj._h)).decode()
    return rc, msg, dict(x=x, u=uh, x_hist=xh, not_converged=bad)


@pytest.fixture(scope="module")
def caseA(gpu_mpc_factory, term):
    bt = _thruster_batch(96, 10)
    mpc = gpu_mpc_factory(N=10, NT=8, dtype="f32", terminal_set=term[0], terminal_set_active=False)
    kw = dict(outcomes=dict(tol_pos=1.0, tol_vel=0.3, tol_rate=0.1), return_status=True)
    shared = _sim(mpc, bt, xr=bt["xr"], plant={}, **kw)                      # the _plant_ entry
    return bt, mpc, kw, shared


def test_one_table_is_the_shared_loop(caseA):
    bt, mpc, kw, shared = caseA
    assert "tset_step" in shared["outcomes"] and "settle_step" in shared["outcomes"]
    one = _sim(mpc, bt, mission=dict(tables=bt["xr"][None]), **kw)
    _same(one, shared)
    # more columns than T + N, and a table number / offset of zero given explicitly
    two = _sim(mpc, bt, mission=dict(tables=XT[:1], table=np.zeros(96, np.int32), offset=np.zeros(96, np.int32)), **kw)
    _same(two, shared)


def test_null_mission_and_empty_mission_are_the_plant_entry(caseA):
    bt, mpc, kw, shared = caseA
    for ms in (None, _lib.ftmpc_mission(struct_size=C.sizeof(_lib.ftmpc_mission))):
        oc, orec, sh = _outcome_request(mpc, 96, bt["T"], False, kw["outcomes"], True, 0, None)
        rc, msg, out = _c_call(mpc, False, bt, bt["xr"], None, ms, oc)
        assert rc == 0, msg
        out.update(outcomes=orec, status_hist=sh)
        _same(out, shared)


# ---------------------------------------------------------------------------------------------------------------------------
# B: groups are slices
# ---------------------------------------------------------------------------------------------------------------------------
def _groups_equal_slices(make, N, bt, groups, **kw):
    """One mission call over contiguous groups [(lo, hi, table, offset)] against one call of the shared entry per group, each a slice
    index0 = lo of the campaign with the group's columns as xref_traj / uref_traj.  Every call on a fresh handle."""
    B, T = len(bt["x0"]), bt["T"]
    table, offset = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for lo, hi, k, o in groups:
        table[lo:hi], offset[lo:hi] = k, o

    def fresh(f):
        mpc = make()
        try:
            return f(mpc)
        finally:
            mpc.close()
    whole, replayed = fresh(lambda m: (_sim(m, bt, mission=dict(tables=XT, utables=UT, table=table, offset=offset), outcomes=True,
                                            return_status=True, **kw), m.sqp_graph_launches()))
    parts = [fresh(lambda m: _sim(m, bt, lo, hi, xr=XT[k][:, o:o + T + N], ur=UT[k][:, o:o + T + N], outcomes=True, return_status=True,
                                  index0=lo, index_total=B, **kw)) for lo, hi, k, o in groups]
    assert np.array_equal(np.concatenate([p["x"] for p in parts]), whole["x"])
    for k in ("x_hist", "u", "status_hist"):
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), whole[k]), k
    for k in whole["outcomes"]:
        assert np.array_equal(np.concatenate([p["outcomes"][k] for p in parts]), whole["outcomes"][k]), k
    for k in ("not_converged", "alloc_failed"):
        if k in whole:
            assert np.array_equal(sum(p[k] for p in parts), whole[k]), k
    # the groups do fly different things
    assert not np.array_equal(whole["x_hist"][:, groups[0][0]], whole["x_hist"][:, groups[1][0]])
    return whole, replayed


@pytest.mark.parametrize("N", [10, 20])
def test_groups_are_slices_thruster(N):
    bt = _thruster_batch(96, N)
    _groups_equal_slices(lambda: ft_mpc_amd.BatchedMPC(N=N, NT=8, dtype="f32"), N, bt,
                         [(0, 24, 0, 0), (24, 48, 1, 0), (48, 72, 1, 7), (72, 96, 2, 20)])


def _wrench_batch24(T=8):
    x0, ub, stuck, _ = qo.make_batch(24, 15, 16, 1, 77)        # one fault keeps every hull full-dimensional
    return dict(x0=x0, ub=ub, stuck=stuck, T=T, seed=9)


GROUPS3 = [(0, 8, 0, 0), (8, 16, 1, 3), (16, 24, 2, 11)]


@pytest.mark.parametrize("sqp_iters", [0, 2])
def test_groups_are_slices_wrench(sqp_iters):
    _groups_equal_slices(lambda: ft_mpc_amd.BatchedMPC(N=15, NT=16, dtype="f64", max_iters=60), 15, _wrench_batch24(), GROUPS3,
                         formulation="wrench", sqp_iters=sqp_iters)


def test_groups_are_slices_thruster_sqp():
    """B = 24 <= 512: from the third step on the SQP of a step may be replayed from its recorded graph (the window pointer no longer
    moves with the step); the result must be that of the direct launches of the per-group calls, whose pointer moves."""
    x0, ub, stuck, _ = qo.make_batch(24, 10, 8, 1, 78)
    bt = dict(x0=x0, ub=ub, stuck=stuck, T=6, seed=9)
    _, replayed = _groups_equal_slices(lambda: ft_mpc_amd.BatchedMPC(N=10, NT=8, dtype="f32"), 10, bt, GROUPS3, sqp_iters=3)
    print("steps replayed from the graph:", replayed)
    assert replayed == bt["T"] - 2


# ---------------------------------------------------------------------------------------------------------------------------
# C: against the oracle loop with interleaved assignment
# ---------------------------------------------------------------------------------------------------------------------------
def _oracle_loop(qcfg, x0, ub, stuck, table, offset, T, seed):
    N, NT = qcfg.N, qcfg.NT
    x = np.array(x0, float)
    B = x.shape[0]
    warm, us, ok = None, np.zeros((T, B, NT)), True
    for t in range(T):
        xw = np.stack([XT[table[b]][:, offset[b] + t:offset[b] + t + N + 1].reshape(-1, order="F") for b in range(B)])
        uw = np.stack([UT[table[b]][:, offset[b] + t:offset[b] + t + N + 1].reshape(-1, order="F") for b in range(B)])
        out = co.solve_batch(qcfg, x, ub, stuck, xw, uref=uw, warmU=warm, max_iters=60, nthreads=4)
        ok = ok and (out["status"] == 0).all()
        us[t] = out["u0"]
        warm = np.concatenate([out["U"][:, 1:], np.zeros((B, 1, NT))], axis=1)
        for b in range(B):
            x[b] = co.plant_step(qcfg, x[b], out["u0"][b], ub[b], stuck[b])
        idx = (np.uint64(t) * np.uint64(B) + np.arange(B, dtype=np.uint64))[:, None] * np.uint64(13) + np.arange(13, dtype=np.uint64)[None, :]
        x = x + 1e-3 * cl.u01(seed, idx)
        x[:, 6:10] /= np.linalg.norm(x[:, 6:10], axis=1, keepdims=True)
    return x, us, ok


@pytest.mark.parametrize("dtype,N,NT,B,T,tol_u,tol_x", [("f64", 15, 16, 6, 12, 1e-6, 1e-7), ("f32", 20, 8, 24, 8, 5e-4 * 3.4, 1e-4)])
def test_interleaved_mission_against_the_oracle_loop(gpu_mpc_factory, dtype, N, NT, B, T, tol_u, tol_x):
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 2, 99)
    table, offset = _interleaved(B)
    assert len(set(table)) == 3 and (np.diff(table) < 0).any()                # not sorted
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype=dtype, max_iters=40) if dtype == "f64" else gpu_mpc_factory(N=N, NT=NT)
    bt = dict(x0=x0, ub=ub, stuck=stuck, T=T, seed=5)
    out = _sim(mpc, bt, mission=dict(tables=XT, utables=UT, table=table, offset=offset))
    xo, uo, ok = _oracle_loop(qo.QPConfig(N=N, NT=NT), x0, ub, stuck, table, offset, T, 5)
    print("max |u - oracle|", np.abs(out["u"] - uo).max(), "max |x - oracle|", np.abs(out["x"] - xo).max())
    assert ok and out["not_converged"].sum() == 0
    assert np.abs(out["u"] - uo).max() < tol_u
    assert np.abs(out["x"] - xo).max() < tol_x
    # both effects: the hover table at any offset is the all-hover run, the other tables are not
    hover = _sim(mpc, bt, xr=XT[0][:, :T + N], ur=UT[0][:, :T + N])
    on0 = table == 0
    assert (offset[on0] > 0).any()
    assert np.array_equal(out["x"][on0], hover["x"][on0]) and np.array_equal(out["u"][:, on0], hover["u"][:, on0])
    moved = np.abs(out["x"][~on0] - hover["x"][~on0]).max(axis=1)
    print("tables 1, 2 against the all-hover run: min", moved.min())
    assert (moved > 1e-3).all()


# ---------------------------------------------------------------------------------------------------------------------------
# D, E: records and cost under the three-table mission on batch A's schedule
# ---------------------------------------------------------------------------------------------------------------------------
def _errors(x_hist, xcol):
    T, B = x_hist.shape[:2]
    r = rm.spiral_r()
    return np.array([[rm.robot_to_center(x_hist[t, b], r)[:9] - xcol[t, b] for b in range(B)] for t in range(T)])


def _records(e, u_hist, status_hist, pu, ps, tol=None, term=None):
    T, B = e.shape[:2]
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


def _cost(D, P, x0, x_hist, u_hist, pu, ps, xcol, ucol, v_nq=None):
    """cost [B,3] of the header from histories: e'diag(Q)e and w'diag(R)w summed in step order, V of the last error."""
    T, B = x_hist.shape[:2]
    r = rm.spiral_r()
    fv = np.concatenate([rm.F_VIRT, np.zeros(3)])
    cost = np.zeros((B, 3))
    for b in range(B):
        for t in range(T):
            e = rm.robot_to_center(x_hist[t, b], r)[:9] - xcol[t, b]
            cost[b, 0] += float(np.sum(rm.Q_DIAG * e * e))
            a = np.where(pu[t, b] > 0.0, u_hist[t, b], 0.0) + ps[t, b]
            q = (x0[b] if t == 0 else x_hist[t - 1, b])[6:10]
            w = D @ a - np.concatenate([rm.rot(q).T @ ucol[t, b, :3], ucol[t, b, 3:]]) - fv
            cost[b, 1] += float(np.sum(rm.R_DIAG * w * w))
            cost[b, 2] = e @ P @ e + (0.0 if v_nq is None else v_nq(e))
    return cost


def _show(name, got, ref):
    print(f"{name}: max |got - ref| = {np.abs(got - ref).max():.3e}, max |ref| = {np.abs(ref).max():.3e}")


@pytest.fixture(scope="module")
def caseD(caseA, term):
    bt, mpc, _, _ = caseA
    B, T = 96, bt["T"]
    table, offset = _interleaved(B)
    ms = dict(tables=XT, utables=UT, table=table, offset=offset)
    xcol, ucol = _columns(table, offset, T)
    plain = _sim(mpc, bt, mission=ms)
    tol = _band(_norms(_errors(plain["x_hist"], xcol)))
    oc = dict(tol_pos=tol[0], tol_vel=tol[1], tol_rate=tol[2])
    rec = _sim(mpc, bt, mission=ms, outcomes=oc, return_status=True)
    cost = _sim(mpc, bt, mission=ms, outcomes=dict(oc, cost=True), return_status=True)
    return bt, mpc, xcol, ucol, tol, plain, rec, cost


def test_records_under_a_mission_equal_numpy_with_each_vehicles_own_column(caseD, term):
    bt, _, xcol, _, tol, plain, rec, _ = caseD
    _same(rec, plain, ("x", "u", "x_hist", "not_converged"))
    o = rec["outcomes"]
    assert sorted(o) == sorted(("err_int", "err_max", "impulse", "settle_step", "tset_step", "unsolved", "first_unsolved"))
    pu, ps = _plant_patterns(bt["ub"], bt["stuck"], bt["faults"], bt["T"])
    e = _errors(rec["x_hist"], xcol)
    ref = _records(e, rec["u"], rec["status_hist"], pu, ps, tol, term[1:])
    for k in ref:
        _show(k, np.asarray(o[k], float), ref[k])
    _compare(o, ref)
    assert (o["settle_step"] < bt["T"]).any() and (o["settle_step"] == bt["T"]).any()
    # measured against the shared hover column instead, the records of the vehicles on the other tables are others
    hov = _records(_errors(rec["x_hist"], np.broadcast_to(XT[0][:, 0], xcol.shape)), rec["u"], rec["status_hist"], pu, ps)
    assert np.abs(hov["err_int"] - o["err_int"]).max() > 1e-6


def test_cost_under_a_mission(caseD):
    bt, mpc, xcol, ucol, _, _, rec, out = caseD
    # asking for cost changes no other output bit
    got = out["outcomes"].pop("cost")
    _same(out, rec)
    assert got.shape == (96, 3) and got.dtype == np.float64
    pu, ps = _plant_patterns(bt["ub"], bt["stuck"], bt["faults"], bt["T"])
    ref = _cost(rm.allocation_matrix_8(), mpc.P, bt["x0"], out["x_hist"], out["u"], pu, ps, xcol, ucol)
    _show("cost", got, ref)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    assert (ref > 0).all() and np.abs(ucol).max() > 0.1
    # without the rotated uref the stage term of the vehicles on the circle is another
    nour = _cost(rm.allocation_matrix_8(), mpc.P, bt["x0"], out["x_hist"], out["u"], pu, ps, xcol, np.zeros_like(ucol))
    on1 = _interleaved(96)[0] == 1
    assert (np.abs(nour[on1, 1] - ref[on1, 1]) > 1e-9 * ref[on1, 1]).all() and np.array_equal(nour[~on1], ref[~on1])
    # the PLANT's pattern: with the controller's (switched at the detection step) the vehicles whose fault is detected late differ
    late = bt["delay"] > 0
    cu, cs = _plant_patterns(bt["ub"], bt["stuck"], dict(bt["faults"], onset=bt["faults"]["onset"] + bt["delay"][:, None]), bt["T"])
    ctrl = _cost(rm.allocation_matrix_8(), mpc.P, bt["x0"], out["x_hist"], out["u"], cu, cs, xcol, ucol)
    miss = np.abs(ctrl[:, 1] - got[:, 1]) > 1e-12 + 1e-12 * np.abs(got[:, 1])
    assert not miss[~late].any() and miss[late].sum() >= late.sum() // 2, (miss[late].sum(), late.sum())


def test_cost_with_the_shared_reference(caseA):
    """n_tables = 0: the struct only asks for cost; the call's xref_traj / uref_traj (here the circle) are every vehicle's."""
    bt, mpc, kw, _ = caseA
    T, N = bt["T"], 10
    xr, ur = XT[1][:, 5:5 + T + N], UT[1][:, 5:5 + T + N]
    base = _sim(mpc, bt, xr=xr, ur=ur, plant={}, **kw)
    out = _sim(mpc, bt, xr=xr, ur=ur, outcomes=dict(kw["outcomes"], cost=True), return_status=True)
    got = out["outcomes"].pop("cost")
    _same(out, base)
    only = _sim(mpc, bt, xr=xr, ur=ur, outcomes=dict(fields=["cost"]))
    assert sorted(only["outcomes"]) == ["cost"] and np.array_equal(only["outcomes"]["cost"], got)
    pu, ps = _plant_patterns(bt["ub"], bt["stuck"], bt["faults"], T)
    xcol = np.broadcast_to(xr[:, 1:T + 1].T[:, None, :], (T, 96, 9))
    ucol = np.broadcast_to(ur[:, :T].T[:, None, :], (T, 96, 6))
    ref = _cost(rm.allocation_matrix_8(), mpc.P, bt["x0"], out["x_hist"], out["u"], pu, ps, xcol, ucol)
    _show("cost", got, ref)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    assert "cost" not in _sim(mpc, bt, xr=xr, ur=ur, outcomes=True)["outcomes"]          # outcomes=True keeps today's set


def test_cost_wrench_form(gpu_mpc_factory):
    bt = _wrench_batch24()
    table, offset = np.zeros(24, np.int32), np.zeros(24, np.int32)
    for lo, hi, k, o in GROUPS3:
        table[lo:hi], offset[lo:hi] = k, o
    mpc = gpu_mpc_factory(N=15, NT=16, dtype="f64", max_iters=60)
    ms = dict(tables=XT, utables=UT, table=table, offset=offset)
    base = _sim(mpc, bt, mission=ms, formulation="wrench", outcomes=True, return_status=True)
    out = _sim(mpc, bt, mission=ms, formulation="wrench", outcomes=dict(cost=True), return_status=True)
    got = out["outcomes"].pop("cost")
    _same(out, base)
    assert np.array_equal(out["alloc_failed"], base["alloc_failed"])
    xcol, ucol = _columns(table, offset, bt["T"])
    pu, ps = np.repeat(bt["ub"][None], bt["T"], 0), np.repeat(bt["stuck"][None], bt["T"], 0)
    ref = _cost(rm.allocation_matrix_16(), mpc.P, bt["x0"], out["x_hist"], out["u"], pu, ps, xcol, ucol)
    _show("cost", got, ref)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)


def _v_nq(tc):
    """V_nq of include/ftmpc.h (ftmpc_config.tc_*): const + sum_t coef_t prod_j e_j^exp_tj + sum_r coef_r (prod_j e_j^exp_rj + eps_r)^pow_r."""
    t = tc.device_tables(_lib.MAX_TCOST, _lib.MAX_TCOST)
    pe, re_ = np.asarray(t["poly_exp"]).reshape(-1, 9), np.asarray(t["root_exp"]).reshape(-1, 9)

    def f(e):
        v = float(t["const"])
        for c, ex in zip(t["poly_coef"], pe):
            v += c * np.prod(e ** ex)
        for c, ex, eps, pw in zip(t["root_coef"], re_, t["root_eps"], t["root_pow"]):
            v += c * (np.prod(e ** ex) + eps) ** pw
        return v
    return f


def test_cost_with_terminal_cost_terms(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 70, 5
    tc = load_terminal()
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32", terminal_cost=tc)
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 1, 31)
    table, offset = _interleaved(B)
    bt = dict(x0=x0, ub=ub, stuck=stuck, T=T, seed=3)
    out = _sim(mpc, bt, mission=dict(tables=XT, utables=UT, table=table, offset=offset), outcomes=dict(fields=["cost"]))
    got = out["outcomes"]["cost"]
    xcol, ucol = _columns(table, offset, T)
    pu, ps = np.repeat(ub[None], T, 0), np.repeat(stuck[None], T, 0)
    f = _v_nq(tc)
    ref = _cost(rm.allocation_matrix_8(), mpc.P, x0, out["x_hist"], out["u"], pu, ps, xcol, ucol, f)
    quad = _cost(rm.allocation_matrix_8(), mpc.P, x0, out["x_hist"], out["u"], pu, ps, xcol, ucol)
    _show("cost", got, ref)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    assert np.abs(quad[:, 2] - ref[:, 2]).min() > 1e-9                        # the terms are there


# ---------------------------------------------------------------------------------------------------------------------------
# F: the multi-GPU driver
# ---------------------------------------------------------------------------------------------------------------------------
def test_multi_driver_equals_one_handle(gpu_mpc_factory):
    bt = _thruster_batch(100, 20)
    bt["T"] = 8
    bt["faults"]["onset"] = np.minimum(bt["faults"]["onset"], 6)
    table, offset = _interleaved(100)
    ms = dict(tables=XT, utables=UT, table=table, offset=offset)
    kw = dict(outcomes=dict(tol_pos=1.0, tol_vel=0.3, tol_rate=0.1, cost=True), return_status=True)
    serial = _sim(gpu_mpc_factory(N=20, NT=8, dtype="f32"), bt, mission=ms, **kw)
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=20, NT=8, dtype="f32"), devices=[0, 0, 0])
    try:
        multi = _sim(m, bt, mission=ms, **kw)
        assert "cost" in multi["outcomes"] and multi["outcomes"]["cost"].all()
        _same(multi, serial)
        # the shared reference with cost through the driver
        xr = XT[2][:, :8 + 20]
        _same(_sim(m, bt, xr=xr, **kw), _sim(gpu_mpc_factory(N=20, NT=8, dtype="f32"), bt, xr=xr, **kw))
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# G: refusals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multi", [False, True])
def test_refusals(gpu_mpc_factory, multi):
    N, NT, B, T = 10, 8, 6, 4
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 0, 1)
    bt = dict(x0=x0, ub=ub, stuck=stuck, T=T, seed=1)
    obj = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f32"), devices=[0, 0]) if multi else gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    size = C.sizeof(_lib.ftmpc_mission)
    cols = 20                                                               # T + N = 14
    xt = np.ascontiguousarray(XT[:, :, :cols].transpose(0, 2, 1))
    ut = np.ascontiguousarray(UT[:, :, :cols].transpose(0, 2, 1))
    hover = XT[0][:, :T + N]
    v = 4                                                                   # the offending vehicle: in the second shard of the driver
    zeros, cost = np.zeros(B, np.int32), np.zeros((B, 3))

    def arr(val):
        a = zeros.copy()
        a[v] = val
        return a

    def ms(**kw):
        kw = {k: (a.ctypes.data_as(ip if a.dtype == np.int32 else dp) if isinstance(a, np.ndarray) else a) for k, a in kw.items()}
        return _lib.ftmpc_mission(**dict(dict(struct_size=size, n_tables=3, n_cols=cols, xref=xt.ctypes.data_as(dp)), **kw))
    nan_x, nan_u = xt.copy(), ut.copy()
    nan_x[1, 7, 2], nan_u[2, 3, 5] = np.nan, np.inf
    tbl_hi, tbl_lo, off_lo, off_hi = arr(3), arr(-1), arr(-1), arr(7)       # 7 + 14 > 20
    cases = [
        (ms(struct_size=size - 8), None, None, ("struct_size",)),
        (ms(n_tables=-1), None, None, ("n_tables",)),
        (ms(xref=None), None, None, ("xref",)),
        (ms(n_cols=T + N - 1), None, None, ("n_cols",)),
        (ms(), hover, None, ("xref_traj",)),
        (ms(), None, np.zeros((6, T + N)), ("uref_traj",)),
        (ms(table=tbl_hi), None, None, ("table", f"vehicle {v}")),
        (ms(table=tbl_lo), None, None, ("table", f"vehicle {v}")),
        (ms(offset=off_lo), None, None, ("offset", f"vehicle {v}")),
        (ms(offset=off_hi), None, None, ("offset", f"vehicle {v}")),
        (ms(xref=nan_x), None, None, ("xref", "table 1", "non-finite")),
        (ms(uref=nan_u), None, None, ("uref", "table 2", "non-finite")),
        (ms(n_tables=0, xref=None, cost=cost), None, None, ("xref_traj",)),
        (ms(n_tables=0, xref=None, cost=cost, table=zeros), hover, None, ("table",)),
        (ms(n_tables=0, xref=None, cost=cost, offset=zeros), hover, None, ("offset",)),
    ]
    try:
        for m, xr, ur, words in cases:
            rc, msg, out = _c_call(obj, multi, bt, xr, ur, m)
            assert rc == -1 and "ftmpc_mission" in msg and all(w in msg for w in words), (words, msg)
            assert np.array_equal(out["x"], x0)
        # ... and the accepted forms of the same call: tables with the largest offset that fits, cost alone
        rc, msg, _ = _c_call(obj, multi, bt, None, None, ms(offset=arr(6), uref=ut, cost=cost))
        assert rc == 0 and cost.all(), msg
        rc, msg, _ = _c_call(obj, multi, bt, hover, None, ms(n_tables=0, xref=None, cost=cost))
        assert rc == 0, msg
        # through Python: the library's refusal arrives as an FtmpcError
        with pytest.raises(FtmpcError) as e:
            _sim(obj, bt, mission=dict(tables=XT[:, :, :cols], table=tbl_hi))
        assert e.value.code == -1 and "table" in str(e.value) and f"vehicle {v}" in str(e.value)
        with pytest.raises(FtmpcError) as e:
            _sim(obj, bt, mission=dict(tables=XT[:, :, :T + N - 1]))
        assert e.value.code == -1 and "n_cols" in str(e.value)
        # the wrench entries (their own argument order, their own null-buffer guard): a vehicle's table, a vehicle's offset, and cost
        # alone with a table given
        for bad, words in ((dict(table=tbl_hi), ("table", f"vehicle {v}")), (dict(offset=off_hi), ("offset", f"vehicle {v}")),
                           (dict(utables=np.where(np.arange(cols) == 5, np.inf, UT[:, :, :cols])), ("uref", "non-finite"))):
            with pytest.raises(FtmpcError) as e:
                _sim(obj, bt, formulation="wrench", mission=dict(tables=XT[:, :, :cols], **bad))
            assert e.value.code == -1 and "ftmpc_mission" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    finally:
        if multi:
            obj.close()
