"""GPU: the disturbance estimate on the two-stage wrench form (ftmpc_cost_wrench_kernel<1>, the DIST instantiations of
ftmpc_linearize_kernel about warmG; ftmpc_simulate_wrench_disturbance_batch, ftmpc_multi_simulate_wrench_disturbance_batch,
ftmpc_eval_cost_wrench_disturbance_batch, ftmpc_solve_wrench_disturbance_batch, ftmpc_solve_sqp_wrench_disturbance_batch;
BatchedMPC.simulate(formulation="wrench", disturbance=dict(..., wrench=True)), eval_cost_wrench / solve_wrench / solve_sqp_wrench
with dist=).

The filter and the diagnosis are the thruster form's (tests/test_gpu_disturbances.py, whose BOUND holds here: the filter kernels are
unchanged); new are the wrench cost kernel under the estimate and the loop that hands d^_{t|t} to the wrench QP and the wrench SQP.

1  a zero estimate is the plain entry, disturbance = NULL the _wrench_diagnosis_ entry; 2  the cost under the estimate against a
restatement (disturbances.rollout_centre + the oracle's cost pieces); 3  torque equivalence; 4  the SQP solves the disturbed program;
5  one QP about a stationary point stays there; 6  loop plumbing; 7  replay; 8  an exact estimate closes the model; 9  continued runs,
slices and device slots; 10  refusals; 11  it does its job.

The 16-thruster vehicle with its 26-row hull, N = 15 (N = 5 where a test differentiates numerically), float64 handle unless said."""
import ctypes as C
import time

import numpy as np
import pytest

import ft_mpc_amd
from ft_mpc_amd import _lib
from ft_mpc_amd import diagnosis as DG
from ft_mpc_amd import disturbances as DS
from ft_mpc_amd.controllers.tools.input_bounds import hull_tables
from ft_mpc_amd.controllers.tools.terminal_ingredients import load_terminal
from ft_mpc_amd.sharding import MultiGPUMPC
from oracle import qp_oracle as qo
from oracle import refmath as rm
from test_disturbances_host import DIST_G, EST_G
from test_gpu_diagnosis import _on_orbit, _shift
from test_gpu_disturbances import BALL, BOUND, P0D, QD, _bad_structs, _priors
from test_gpu_disturbances import _check_replay as _check_filter_replay
from test_gpu_estimators import EALL, _sensor
from test_gpu_estimators import _spec as _est_spec
from test_gpu_outcomes import _errors, _hover
from test_gpu_wrench_diagnosis import D16, F_MAX, N, NT, NOISE, SIGMA, ZERO, _check_hull_state, _dspec, _mpc, _p, _two_faults16, _wentry

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)
N5 = 5
# (4), (5): the estimate the SQP is asked to compensate.  Chosen on the CPU with the oracle's wrench solve (qp_oracle.solve_wrench_instance
# iterated six times from D stuck on _on_orbit(B, 51), N = 5, hover reference, healthy vehicle): the nominal solutions leave every hull
# row inactive by at least 0.609 N (B = 65; 0.614 N for B = 9) on rows of unit normals, and this estimate moves the compensating wrench
# by |f^| = 0.36 N and |t^| = 0.027 N m, well inside that margin
F_SQP = np.array([0.25, -0.20, 0.15])
T_SQP = np.array([0.020, -0.015, 0.010])
# (11): the plant's force and torque, see test_it_does_its_job
FORCE_W = np.array([0.90, -0.60, 0.75])
TORQUE_W = np.array([0.060, -0.045, 0.030])
T_JOB = 59


def _dist(compensate=True, **kw):
    return dict(dict(p0=P0D, proc_sigma=QD, compensate=compensate, fields=BALL, wrench=True), **kw)


def _sim(mpc, x0, ub, stuck, T, sen, est, dist, hull, seed=5, noise=NOISE, xr=None, n=N, **kw):
    L = sen.get("latency", 0) if sen is not None and sen.get("predict") else 0
    xr = _hover(n, T + L) if xr is None else xr
    return mpc.simulate(x0, ub, stuck, xr, T, noise=noise, seed=seed, return_inputs=True, return_states=True, sensor=sen, estimator=est,
                        disturbance=dist, formulation="wrench", hull=hull, **kw)


def _window_refs(B, n):
    """a per-vehicle reference window with uref (stride 9 (n+1) / 6 (n+1)) of a circle, as tests/test_gpu_wrench_sqp.py builds it"""
    traj = rm.circle_trajectory(0.1, 10, radius=0.65, s_per_circle=40.0)
    xr_all, ur_all = rm.assign_trajectory(traj, n)
    xw, uw = rm.trajectory_window(xr_all, ur_all, 0.5, n)
    return np.stack([xw.reshape(-1, order="F")] * B), np.stack([uw.reshape(-1, order="F")] * B), xw, uw


def _random_dist(B, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.normal(size=(B, 3)) * 0.5 * scale, rng.normal(size=(B, 3)) * 0.05 * scale], axis=1)


def cost_wrench_dist(cfg, mcfg, x0, xref, G, f, t, uref=None, T=None, term=None):
    """(J, terminal-set violation, centre states) of the COMMANDED wrench sequence G [n,6] along the rollout under the estimate
    (disturbances.rollout_centre); the cost terms, the non-quadratic terminal cost and the violation as cost_wrench of
    tests/test_gpu_wrench_sqp.py takes them from the oracle's pieces.  cfg: the oracle's QPConfig, mcfg: the handle's MPCConfig."""
    n = cfg.N
    xref = np.asarray(xref, float).reshape(9, n + 1)
    X = DS.rollout_centre(rm.robot_to_center(x0, cfg.r), G, f, t, mcfg, cfg.r)
    fv = np.concatenate([cfg.f_virt, np.zeros(3)])
    J, viol = 0.0, 0.0
    for k in range(n):
        ur = np.zeros(6)
        if uref is not None:
            u_r = np.asarray(uref, float).reshape(6, n + 1)[:, k]
            ur = np.concatenate([rm.rot(X[k][9:13]).T @ u_r[0:3], u_r[3:6]])
        ut = np.asarray(G[k], float) - ur - fv
        J += ut @ (cfg.R * ut)
        e = X[k + 1][0:9] - xref[:, k + 1]
        if k + 1 < n:
            J += e @ (cfg.Q * e)
        else:
            J += float(T.cost(e)) if T is not None else e @ cfg.P @ e
            if term is not None:
                viol = float(np.maximum(term[0] @ e - term[1], 0.0).sum())
    return float(J), viol, X


# ---------------------------------------------------------------------------------------------------------------------------
# (1) a zero estimate is the parent
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tset", [False, True], ids=["no-set", "terminal-set"])
def test_zero_estimate_gives_the_bits_of_the_plain_entries(gpu_mpc_factory, tset):
    """B = 65 (crosses a wave; with backtracks = 7 the line search's 455 lanes are no multiple of 64), with and without uref."""
    B = 65
    T = load_terminal()
    kw = dict(terminal_set=T.term_set, terminal_cost=T) if tset else {}
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, **kw)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, 1, 9610)
    hull = hull_tables(D16, ub, stuck)
    assert not hull["degenerate"].any()
    cfg = qo.QPConfig(N=N, NT=NT)
    rng = np.random.default_rng(5)
    G = ((ub / 2 + stuck) @ cfg.D.T)[:, None, :] + rng.uniform(-1.0, 1.0, (B, N, 6))
    per_x, per_u, _, _ = _window_refs(B, N)
    zero = np.zeros((B, 6))
    for xr, ur in ((xref.reshape(-1, order="F"), None), (per_x, per_u)):
        a = mpc.eval_cost_wrench(x0, xr, G, uref=ur, return_tviol=True)
        b = mpc.eval_cost_wrench(x0, xr, G, uref=ur, return_tviol=True, dist=zero)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.isfinite(a[0]).all()
        a = mpc.solve_wrench(x0, ub, stuck, xr, uref=ur, return_G=True, hull=hull)
        b = mpc.solve_wrench(x0, ub, stuck, xr, uref=ur, return_G=True, hull=hull, dist=zero)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        W = np.ascontiguousarray(G)
        a = mpc.solve_sqp_wrench(x0, ub, stuck, xr, uref=ur, warmG=W, hull=hull, sqp_iters=3, backtracks=7, return_X=True)
        b = mpc.solve_sqp_wrench(x0, ub, stuck, xr, uref=ur, warmG=W, hull=hull, sqp_iters=3, backtracks=7, return_X=True, dist=zero)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        assert (a["sqp_iters"] > 0).any()
        # and a non-zero estimate is another program
        c = mpc.solve_wrench(x0, ub, stuck, xr, uref=ur, return_G=True, hull=hull, dist=_random_dist(B, 7))
        assert not np.array_equal(c["G"], mpc.solve_wrench(x0, ub, stuck, xr, uref=ur, return_G=True, hull=hull)["G"])


def test_zero_estimate_on_an_fp32_handle(gpu_mpc_factory):
    B = 65
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32", max_iters=60)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, 1, 9611)
    hull = hull_tables(D16, ub, stuck)
    xr = xref.reshape(-1, order="F")
    a = mpc.solve_wrench(x0, ub, stuck, xr, return_G=True, hull=hull)
    b = mpc.solve_wrench(x0, ub, stuck, xr, return_G=True, hull=hull, dist=np.zeros((B, 6)))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    a = mpc.solve_sqp_wrench(x0, ub, stuck, xr, hull=hull, sqp_iters=2, backtracks=7)
    b = mpc.solve_sqp_wrench(x0, ub, stuck, xr, hull=hull, sqp_iters=2, backtracks=7, dist=np.zeros((B, 6)))
    for k in a:
        if a[k] is not None:
            assert np.array_equal(a[k], b[k]), k


def test_null_disturbance_gives_the_bits_of_the_wrench_diagnosis_entry(gpu_mpc_factory):
    """On a handle and on three device slots, with a sensor, an estimator and a rebuild_hull diagnosis in the call."""
    B, T = 65, 4
    x0, ub, stuck = qo.make_batch(B, N, NT, 1, 16)[:3]
    hull = hull_tables(D16, ub, stuck)
    H = NT * 2
    se = _lib.ftmpc_sensor(struct_size=C.sizeof(_lib.ftmpc_sensor), latency=2, predict=0, seed=9)
    for k in range(4):
        se.sigma[k] = SIGMA[k]

    def structs():
        eh, lh = np.zeros((T, B, 13)), np.zeros((T, B, H))
        es = _lib.ftmpc_estimator(struct_size=C.sizeof(_lib.ftmpc_estimator), every=1, est_hist=eh.ctypes.data_as(dp))
        dg = _lib.ftmpc_diagnosis(struct_size=C.sizeof(_lib.ftmpc_diagnosis), every=1, n_levels=2, max_detect=2, threshold=18.0,
                                  llr_hist=lh.ctypes.data_as(dp))
        for k in range(4):
            es.p0[k] = es.meas_sigma[k] = SIGMA[k]
            es.proc_sigma[k] = 0.1 * SIGMA[k]
        dg.levels[0], dg.levels[1] = 0.0, F_MAX
        dg.resid_sigma[0], dg.resid_sigma[1] = DG.default_sigma(SIGMA, NOISE)
        return es, dg, eh, lh
    mpc = _mpc(gpu_mpc_factory)
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f64", max_iters=60), devices=[0, 0, 0])
    try:
        for obj in (mpc, m):
            es, dg, eh0, lh0 = structs()
            hb0, nh0 = np.zeros_like(hull["b"]), np.full(B, -1, np.int32)
            rc, err, ref = _wentry(obj, "wrench_diagnosis_batch", x0, ub, stuck, hull, T, 7,
                                   (None, None, None, C.byref(se), C.byref(es), C.byref(dg), _p(hb0), _p(nh0, ip)))
            assert rc == 0, err
            es2, dg2, eh1, lh1 = structs()
            hb1, nh1 = np.zeros_like(hull["b"]), np.full(B, -1, np.int32)
            rc, err, out = _wentry(obj, "wrench_disturbance_batch", x0, ub, stuck, hull, T, 7,
                                   (None, None, None, C.byref(se), C.byref(es2), C.byref(dg2), _p(hb1), _p(nh1, ip), None))
            assert rc == 0, err
            for k in ref:
                assert np.array_equal(out[k], ref[k]), k
            assert np.array_equal(eh1, eh0) and np.array_equal(lh1, lh0) and eh0.any() and out["u"].any()
            assert np.array_equal(hb1, hb0) and np.array_equal(nh1, nh0)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (2) the cost under the estimate, (3) torque equivalence
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [9, 65])
def test_cost_under_the_estimate_against_the_restatement(gpu_mpc_factory, B):
    """1e-10 relative, the bound tests/test_gpu_wrench_sqp.py holds the plain kernel to; the violation within 1e-12 as there.  The
    estimates (2 N, 0.2 N m per axis, normal: these states start up to 2 m off the reference and their costs are in the thousands)
    move every cost by at least 1e-3 relative against dist = 0, asserted.
    Measured on an MI355X: worst relative deviation 7.7e-16 (B = 9) and 1.2e-15 (B = 65); the estimate moves the cost by at least
    8e-2 (B = 9) and 5.9e-3 (B = 65) relative."""
    T = load_terminal()
    term = (T.term_set.A, T.term_set.b.reshape(-1))
    with_tc = gpu_mpc_factory(N=N, NT=NT, dtype="f64", terminal_set=T.term_set, terminal_cost=T)
    plain = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60)
    cfg = qo.QPConfig(N=N, NT=NT)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, 2, 9500 + B)
    rng = np.random.default_rng(B)
    G = ((ub / 2 + stuck) @ cfg.D.T)[:, None, :] + rng.uniform(-1.0, 1.0, (B, N, 6))
    per_x, per_u, xw, uw = _window_refs(B, N)
    dist = _random_dist(B, 31 + B, scale=4.0)
    worst, least = 0.0, np.inf
    for mpc, tc, tm in ((with_tc, T, term), (plain, None, None)):
        for (xr, ur, xr_h, ur_h) in ((xref.reshape(-1, order="F"), None, xref, None), (per_x, per_u, xw, uw)):
            J, V = mpc.eval_cost_wrench(x0, xr, G, uref=ur, return_tviol=True, dist=dist)
            J0 = mpc.eval_cost_wrench(x0, xr, G, uref=ur)
            for b in range(B):
                Jr, Vr, _ = cost_wrench_dist(cfg, mpc.cfg, x0[b], xr_h, G[b], dist[b, 0:3], dist[b, 3:6], ur_h, tc, tm)
                worst = max(worst, abs(J[b] - Jr) / abs(Jr))
                least = min(least, abs(J[b] - J0[b]) / abs(J0[b]))
                assert J[b] == pytest.approx(Jr, rel=1e-10), (b, J[b], Jr)
                assert abs(V[b] - Vr) <= 1e-12 * max(1.0, Vr), (b, V[b], Vr)
                assert abs(J[b] - J0[b]) >= 1e-3 * abs(J0[b]), (b, J[b], J0[b])
    print(f"cost under the estimate, B = {B}: worst relative deviation {worst:.3e}; the estimate moves the cost by at least {least:.3e}")


def test_torque_equivalence(gpu_mpc_factory):
    """uref = None, f^ = 0: the model sees tau + t^, so cost(G; t^) = cost_plain(G + [0; t^]) + sum_k sum_{g >= 3} R_g (G_kg^2 -
    (G_kg + t^_g)^2) (ur and f_virt have no torque part), and the violation is the same bits: the two rollouts are the same
    additions.  1e-12 relative, as tests/test_gpu_wrench_sqp.py:283.  Measured on an MI355X: 2.1e-16 relative, the correction up to
    2.4e-6 of the cost, the violations the same bits (all 65 points lie outside the terminal set)."""
    B = 65
    T = load_terminal()
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f64", terminal_set=T.term_set, terminal_cost=T)
    cfg = qo.QPConfig(N=N, NT=NT)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, 2, 9620)
    rng = np.random.default_rng(17)
    G = ((ub / 2 + stuck) @ cfg.D.T)[:, None, :] + rng.uniform(-1.0, 1.0, (B, N, 6))
    dist = _random_dist(B, 19)
    dist[:, 0:3] = 0.0
    xr = xref.reshape(-1, order="F")
    J, V = mpc.eval_cost_wrench(x0, xr, G, return_tviol=True, dist=dist)
    Gs = G.copy()
    Gs[:, :, 3:6] += dist[:, None, 3:6]
    Jp, Vp = mpc.eval_cost_wrench(x0, xr, Gs, return_tviol=True)
    corr = (cfg.R[3:6] * (G[:, :, 3:6] ** 2 - Gs[:, :, 3:6] ** 2)).sum(axis=(1, 2))
    rel = np.abs(J - (Jp + corr)) / np.abs(J)
    print(f"torque equivalence: worst relative deviation {rel.max():.3e}; the correction is up to {np.abs(corr / J).max():.3e} of the cost, "
          f"{int((V > 0).sum())} of {B} points outside the terminal set")
    assert rel.max() <= 1e-12
    assert np.array_equal(V, Vp)
    assert np.abs(corr / J).max() > 1e-9 and np.abs(J - mpc.eval_cost_wrench(x0, xr, G)).min() > 0


# ---------------------------------------------------------------------------------------------------------------------------
# (4) the SQP solves the disturbed program, (5) one QP about a stationary point stays there
# ---------------------------------------------------------------------------------------------------------------------------
def _sqp_setup(B):
    x0 = _on_orbit(B, 51)
    ub, stuck = np.full((B, NT), F_MAX), np.zeros((B, NT))
    hull = hull_tables(D16, ub, stuck)
    xr = np.ascontiguousarray(_hover(N5, 1)[:, :N5 + 1].reshape(-1, order="F"))
    dist = np.tile(np.r_[F_SQP, T_SQP], (B, 1))
    return x0, ub, stuck, hull, xr, dist


def _gradient(mpc, x0, xr, G, dist, h=1e-5):
    """central differences of the cost entry over all 6 n directions, every point a row of ONE call: [B, 6 n].  The cost is close to
    quadratic in G (the dynamics are affine in the wrench but for the attitude coupling), so the truncation h^2 |J'''| / 6 is far
    below the rounding 2^-53 |J| / h = 1e-10 for |J| of ten."""
    B, n = G.shape[0], G.shape[1]
    m = 6 * n
    E = np.eye(m).reshape(m, n, 6) * h
    pts = np.concatenate([G[:, None] + E[None], G[:, None] - E[None]], axis=1).reshape(B * 2 * m, n, 6)
    J = mpc.eval_cost_wrench(np.repeat(x0, 2 * m, axis=0), xr, pts, dist=None if dist is None else np.repeat(dist, 2 * m, axis=0))
    J = J.reshape(B, 2, m)
    return (J[:, 0] - J[:, 1]) / (2 * h)


@pytest.mark.parametrize("B", [9, 65])
def test_the_sqp_solves_the_disturbed_program(gpu_mpc_factory, B):
    """N = 5, hover reference, states near its orbit, healthy vehicle, no terminal set, no state bounds, backtracks = 7 (B * 7 lanes:
    no multiple of 64), sqp_iters = 10, every hull row inactive at every returned solution (asserted, no instance excluded).
    (1) the reported cost is the cost entry at the returned G under the estimate (1e-12 relative) and cost <= cost0;
    (2) the max-norm of the central-difference gradient of the disturbed cost at G* is at most 10 x what the PLAIN entry leaves at its
        own solution under the plain cost (the parent's solver is the reference; the margin covers the different iterate path);
    (3) the same gradient at the plain solution under the disturbed cost is at least 100 x larger: the estimate matters, so (2) fails
        if the linearisation, the merit of the line search or the final cost ignored it.
    Measured on an MI355X: B = 9: |grad| 5.1e-6 at the disturbed solution, 4.5e-6 the plain entry's at its own (ratio 1.2), 32.7 the
    disturbed cost's at the plain solution; B = 65: 6.6e-6, 3.6e-6 (ratio 1.8) and 32.6; 3.2 - 3.3 major iterations against 3.0; the two
    solutions differ by up to 0.059 N."""
    mpc = gpu_mpc_factory(N=N5, NT=NT, dtype="f64", max_iters=60)
    x0, ub, stuck, hull, xr, dist = _sqp_setup(B)
    kw = dict(hull=hull, sqp_iters=10, backtracks=7, tol=1e-12)
    plain = mpc.solve_sqp_wrench(x0, ub, stuck, xr, **kw)
    got = mpc.solve_sqp_wrench(x0, ub, stuck, xr, dist=dist, **kw)
    for o in (plain, got):
        assert (o["status"] == 0).all() and (o["alloc_status"] == 0).all()
        for b in range(B):      # every hull row inactive at every stage
            A = hull["A"][hull["set"][b]]
            assert (o["G"][b] @ A.T - hull["b"][b] < -1e-3).all(), b
    J = mpc.eval_cost_wrench(x0, xr, got["G"], dist=dist)
    assert np.abs(got["cost"] - J).max() <= 1e-12 * np.abs(J).max() and (np.abs(got["cost"] - J) <= 1e-12 * np.abs(J)).all()
    assert (got["cost"] <= got["cost0"]).all() and (got["sqp_iters"] > 0).all()
    assert np.array_equal(got["cost0"], mpc.eval_cost_wrench(x0, xr, np.zeros((B, N5, 6)), dist=dist))      # (start: D stuck = 0)
    g_plain = np.abs(_gradient(mpc, x0, xr, plain["G"], None)).max()
    g_dist = np.abs(_gradient(mpc, x0, xr, got["G"], dist)).max()
    g_cross = np.abs(_gradient(mpc, x0, xr, plain["G"], dist)).max(axis=1).min()
    print(f"wrench SQP under the estimate, B = {B}: |grad| at its solution {g_dist:.3e}, the plain entry's at its own {g_plain:.3e}; the "
          f"disturbed cost's gradient at the plain solution is at least {g_cross:.3e}; major iterations {got['sqp_iters'].mean():.1f} "
          f"against {plain['sqp_iters'].mean():.1f}; |G* - G_plain| up to {np.abs(got['G'] - plain['G']).max():.3e}")
    assert g_dist <= 10.0 * g_plain
    assert g_cross >= 100.0 * g_plain


@pytest.mark.parametrize("B", [9, 65])
def test_one_qp_about_a_stationary_point_stays_there(gpu_mpc_factory, B):
    """solve_wrench(warmG = G*, dist) returns G* within 10 x the distance the plain pair (plain G*, dist = 0) shows, and
    solve_wrench(warmG = G*, dist = 0) moves at least 100 x farther.  Measured on an MI355X: B = 9: the plain pair moves 4.8e-7 N,
    the disturbed pair 2.8e-7 N, the disturbed point under dist = 0 at least 4.0e-2 N; B = 65: 3.8e-7, 7.1e-7 and 3.5e-2 N."""
    mpc = gpu_mpc_factory(N=N5, NT=NT, dtype="f64", max_iters=60)
    x0, ub, stuck, hull, xr, dist = _sqp_setup(B)
    kw = dict(hull=hull, sqp_iters=10, backtracks=7, tol=1e-12)
    Gp = mpc.solve_sqp_wrench(x0, ub, stuck, xr, **kw)["G"]
    Gd = mpc.solve_sqp_wrench(x0, ub, stuck, xr, dist=dist, **kw)["G"]

    def moved(G, d):
        out = mpc.solve_wrench(x0, ub, stuck, xr, warmG=np.ascontiguousarray(G.copy()), return_G=True, hull=hull, dist=d)
        assert (out["status"] == 0).all()
        return np.abs(out["G"] - G).max(axis=(1, 2))
    base, stay, leave = moved(Gp, None), moved(Gd, dist), moved(Gd, np.zeros((B, 6)))
    print(f"one QP about the stationary point, B = {B}: plain pair moves {base.max():.3e}, the disturbed pair {stay.max():.3e}, the disturbed "
          f"point under dist = 0 at least {leave.min():.3e}")
    assert stay.max() <= 10.0 * base.max()
    assert leave.min() >= 100.0 * base.max()


# ---------------------------------------------------------------------------------------------------------------------------
# (6) loop plumbing, T = 1
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sqp_iters", [0, 2])
def test_the_loops_first_command_is_the_standalone_solve(gpu_mpc_factory, sqp_iters):
    """Handed force / torque, p0 = 0, zero noise: u_hist[0] is the command of solve_wrench (sqp_iters = 0) or solve_sqp_wrench
    (sqp_iters = 2) from the estimate of step 0 under d^_{0|0}, allocation included, bit for bit; with compensate = 0 the bits are
    those of the run with the estimator only."""
    B = 65
    x0, ub, stuck = qo.make_batch(B, N, NT, 1, 21)[:3]
    hull = hull_tables(D16, ub, stuck)
    mpc = _mpc(gpu_mpc_factory)
    d = _random_dist(B, 23)
    est = dict(every=1, p0=ZERO, proc_sigma=ZERO, meas_sigma=SIGMA, xhat=x0, fields=("est",))
    spec = dict(p0=(0.0, 0.0), proc_sigma=(0.0, 0.0), force=d[:, 0:3], torque=d[:, 3:6])
    on = _sim(mpc, x0, ub, stuck, 1, None, est, _dist(True, **spec), hull, noise=ZERO, sqp_iters=sqp_iters)
    seen = on["estimator"]["est"][0]
    d0 = np.concatenate([on["disturbance"]["force_hist"][0], on["disturbance"]["torque_hist"][0]], axis=1)
    assert np.array_equal(d0, d) and np.abs(seen - x0).max() <= 1e-15
    win = np.ascontiguousarray(_hover(N, 1)[:, :N + 1].reshape(-1, order="F"))
    if sqp_iters == 0:
        alone = mpc.solve_wrench(seen, ub, stuck, win, hull=hull, dist=d0)
        nominal = mpc.solve_wrench(seen, ub, stuck, win, hull=hull)
    else:
        alone = mpc.solve_sqp_wrench(seen, ub, stuck, win, hull=hull, sqp_iters=sqp_iters, dist=d0)
        nominal = mpc.solve_sqp_wrench(seen, ub, stuck, win, hull=hull, sqp_iters=sqp_iters)
    assert (alone["alloc_status"] == 0).all()
    assert np.array_equal(on["u"][0], alone["u0"])
    assert not np.array_equal(alone["u0"], nominal["u0"])
    off = _sim(mpc, x0, ub, stuck, 1, None, est, _dist(False, **spec), hull, noise=ZERO, sqp_iters=sqp_iters)
    only = mpc.simulate(x0, ub, stuck, _hover(N, 1), 1, noise=ZERO, seed=5, return_inputs=True, return_states=True, estimator=est,
                        formulation="wrench", hull=hull, sqp_iters=sqp_iters)
    assert np.array_equal(off["u"], only["u"]) and np.array_equal(off["x"], only["x"])
    assert np.array_equal(off["u"][0], nominal["u0"])
    assert np.array_equal(off["disturbance"]["force_hist"], on["disturbance"]["force_hist"])


# ---------------------------------------------------------------------------------------------------------------------------
# (7) replay
# ---------------------------------------------------------------------------------------------------------------------------
def _detected_schedule(out, ub, stuck, dg):
    """the controller's pattern as a schedule with no delay: an event per detection, at its step, with the pattern after it"""
    do = out["diagnosis"]
    B = ub.shape[0]
    det = DG.detections_of(do["step"], do["thruster"], do["level"])
    K = max(1, max(len(d) for d in det))
    onset = np.full((B, K), -1, np.int32)
    eub, est = np.repeat(ub[:, None], K, 1).copy(), np.repeat(stuck[:, None], K, 1).copy()
    for b in range(B):
        for k in range(len(det[b])):
            onset[b, k] = det[b][k][0]
            eub[b, k], est[b, k] = DG.pattern(ub[b], stuck[b], det[b][:k + 1], dg["levels"])
    return dict(onset=onset, ub=eub, stuck=est), det


def _check_decisions(out, x0, ub, stuck, dg, cfg, step0=0):
    """the detections and the returned pattern against diagnosis.replay of the run's own measurements and applied commands under the
    recorded estimates (force=, torque=); returns the largest deviation of llr_hist"""
    do, bo = out["diagnosis"], out["disturbance"]
    B = ub.shape[0]
    so = out.get("sensor") or {}
    meas = so["meas"] if "meas" in so else np.concatenate([x0[None], out["x_hist"][:-1]])
    got = DG.detections_of(do["step"], do["thruster"], do["level"])
    dev = 0.0
    for b in range(B):
        r = DG.replay(meas[:, b], out["u"][:, b], ub[b], stuck[b], dg, cfg, step0=step0, force=bo["force_hist"][:, b],
                      torque=bo["torque_hist"][:, b])
        assert got[b] == r["detections"], (b, got[b], r["detections"])
        assert np.array_equal(do["ub"][b], r["ub_end"]) and np.array_equal(do["stuck"][b], r["stuck_end"]), b
        dev = max(dev, (np.abs(do["llr_hist"][:, b] - r["llr_hist"]) / np.maximum(1.0, np.abs(r["llr_hist"]))).max())
    return dev


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("B", [1, 65, 96])
def test_replay_from_the_runs_own_histories(gpu_mpc_factory, B, every):
    """Noise, a biased sensor with latency 2 and the filter predicting, a two-fault schedule that moves the plant only, a rebuild_hull
    diagnosis, handed priors with a full covariance, a constant plant force and torque; sqp_iters = 0, and 2 for B = 65.  The filter
    against disturbances.replay under the controller's own pattern of each step (its detections), within BOUND of
    tests/test_gpu_disturbances.py; the decisions identical to diagnosis.replay(force=, torque=); hull_b / no_hull from the detections.
    Measured on an MI355X, maxima over the cases (the fp32 handle's test below included), in the scales of that file: est 6.0e-15, pred
    9.5e-15, force 1.1e-14, torque 7.7e-14, xhat 7.4e-15, cov 5.8e-14, cross 2.4e-15, cov_d 3.1e-16 (BOUND 4.7e-12); llr_hist within
    5.5e-13 of the definition; 99 to 170 detections on B = 65 and 96, 57 to 92 vehicles with new offsets, 5 to 16 without a hull."""
    T = 12
    bt = _two_faults16(B)
    mpc = _mpc(gpu_mpc_factory)
    hull = hull_tables(D16, bt["ub"], bt["stuck"])
    sen = _sensor(B, NT)
    pe, pd = _priors(bt["x0"])
    est = _est_spec(every, fields=EALL, **pe)
    dist = _dist(**pd)
    dg = _dspec(every)
    plant = dict(force=np.tile(FORCE_W, (B, 1)), torque=np.tile(TORQUE_W, (B, 1)))
    for sqp in ((0, 2) if B == 65 else (0,)):
        out = _sim(mpc, bt["x0"], bt["ub"], bt["stuck"], T, sen, est, dist, hull, faults=bt["faults"], diagnosis=dg, plant=plant,
                   sqp_iters=sqp)
        assert sorted(out["disturbance"]) == ["cov", "cross", "force", "force_hist", "torque", "torque_hist"]
        assert "hull_b" in out["diagnosis"] and "no_hull" in out["diagnosis"]
        sched, det = _detected_schedule(out, bt["ub"], bt["stuck"], dg)
        _check_filter_replay(out, bt["x0"], bt["ub"], bt["stuck"], sen, est, dist, mpc.cfg, faults=sched, delay=0)
        dev = _check_decisions(out, bt["x0"], bt["ub"], bt["stuck"], dg, mpc.cfg)
        moved, flat = _check_hull_state(mpc, out, bt["ub"], bt["stuck"], hull, dg)
        print(f"B = {B}, every = {every}, sqp_iters = {sqp}: {sum(len(d) for d in det)} detections, llr_hist within {dev:.3e}, {moved} vehicles "
              f"with new offsets, {flat} without a hull")
        assert np.isfinite(out["x"]).all() and out["u"].any()


def test_replay_on_an_fp32_handle(gpu_mpc_factory):
    B, T = 65, 12
    bt = _two_faults16(B)
    mpc = _mpc(gpu_mpc_factory, "f32")
    hull = hull_tables(D16, bt["ub"], bt["stuck"])
    sen = _sensor(B, NT)
    pe, pd = _priors(bt["x0"])
    est, dist, dg = _est_spec(3, fields=EALL, **pe), _dist(**pd), _dspec(3)
    out = _sim(mpc, bt["x0"], bt["ub"], bt["stuck"], T, sen, est, dist, hull, faults=bt["faults"], diagnosis=dg)
    sched, _ = _detected_schedule(out, bt["ub"], bt["stuck"], dg)
    _check_filter_replay(out, bt["x0"], bt["ub"], bt["stuck"], sen, est, dist, mpc.cfg, faults=sched, delay=0)
    _check_decisions(out, bt["x0"], bt["ub"], bt["stuck"], dg, mpc.cfg)
    _check_hull_state(mpc, out, bt["ub"], bt["stuck"], hull, dg)


# ---------------------------------------------------------------------------------------------------------------------------
# (8) an exact estimate closes the model
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sqp_iters", [0, 2])
def test_exact_estimate_closes_the_model(gpu_mpc_factory, sqp_iters):
    """The plant's own force and torque handed over with zero covariances, a trivial sensor, no noise: the filter is a chained RK4 of
    the truth's own model (est[t] = x_hist[t-1] within 1e-12, the thruster test's bound), every CUSUM statistic is exactly 0 and
    nothing is detected, with and without compensation.  Measured on an MI355X: 4.4e-16 (sqp_iters = 0), 3.3e-16 (sqp_iters = 2)."""
    B, T = 96 if sqp_iters == 0 else 32, 12 if sqp_iters == 0 else 6
    x0, ub, stuck = qo.make_batch(B, N, NT, 1, 12)[:3]
    hull = hull_tables(D16, ub, stuck)
    force, torque = np.tile(FORCE_W, (B, 1)), np.tile(TORQUE_W, (B, 1))
    est = dict(every=1, p0=ZERO, proc_sigma=ZERO, meas_sigma=SIGMA, xhat=x0, fields=EALL)
    dg = _dspec()
    mpc = _mpc(gpu_mpc_factory)
    for comp in (True, False):
        dist = _dist(comp, p0=(0.0, 0.0), proc_sigma=(0.0, 0.0), force=force, torque=torque)
        out = _sim(mpc, x0, ub, stuck, T, None, est, dist, hull, noise=ZERO, diagnosis=dg, plant=dict(force=force, torque=torque),
                   sqp_iters=sqp_iters)
        eo, do, bo = out["estimator"], out["diagnosis"], out["disturbance"]
        worst = np.abs(eo["est"][1:] - out["x_hist"][:-1]).max()
        print(f"exact estimate (sqp_iters = {sqp_iters}, compensate = {comp}): max |est[t] - x_hist[t-1]| = {worst:.3e}")
        np.testing.assert_allclose(eo["est"][1:], out["x_hist"][:-1], rtol=0, atol=1e-12)
        assert np.array_equal(bo["force_hist"], np.repeat(force[None], T, 0)) and np.array_equal(bo["torque"], torque)
        assert not bo["cross"].any() and not bo["cov"].any()
        assert not do["llr_hist"].any()
        assert (do["step"] < 0).all() and np.array_equal(do["ub"], ub) and np.array_equal(do["hull_b"], hull["b"])
        assert out["u"].any()


# ---------------------------------------------------------------------------------------------------------------------------
# (9) continued runs, slices of a campaign and device slots
# ---------------------------------------------------------------------------------------------------------------------------
GROUPS = (("estimator", ("xhat", "cov")), ("disturbance", ("force", "torque", "cross", "cov")),
          ("diagnosis", ("state", "llr", "step", "thruster", "level", "ub", "stuck", "hull_b", "no_hull")))


def _resume(faults, ub, stuck, k):
    """the schedule as a call that starts k steps later sees it (_shift), with one more event in front that fires at the call's step
    0 on every vehicle and holds the pattern the PLANT has by then.  The call's own ub / stuck are the controller's pattern, which a
    false alarm of the first part moves away from the plant's (with sqp_iters = 2 one vehicle raises one before its first fault)."""
    sh = _shift(faults, k)
    B = ub.shape[0]
    pu, ps = ub.copy(), stuck.copy()
    for b in range(B):
        for e in range(faults["onset"].shape[1]):
            if 0 <= faults["onset"][b, e] < k:
                pu[b], ps[b] = faults["ub"][b, e], faults["stuck"][b, e]
    return dict(onset=np.concatenate([np.zeros((B, 1), np.int32), sh["onset"]], axis=1).astype(np.int32),
                ub=np.concatenate([pu[:, None], sh["ub"]], axis=1), stuck=np.concatenate([ps[:, None], sh["stuck"]], axis=1))


@pytest.mark.parametrize("sqp_iters", [0, 2])
def test_continued_runs_equal_the_whole(gpu_mpc_factory, sqp_iters):
    """T = 12 against 6 + 6 with force, torque, cross, cov, xhat, cov, pending, step0 = 6, the diagnosis' carry-over and hull_b /
    no_hull handed over, no process noise, every = 3, compensate = 1: bit for bit.  The handed estimates lie near the plant's values
    (tests/test_gpu_disturbances.py explains why); the second call's schedule starts with the plant's pattern of step 6 (_resume)."""
    B = 65 if sqp_iters == 0 else 33
    bt = _two_faults16(B)
    x0, ub, stuck, faults = bt["x0"], bt["ub"], bt["stuck"], bt["faults"]
    mpc = _mpc(gpu_mpc_factory)
    hull = hull_tables(D16, ub, stuck)
    sen = _sensor(B, NT)
    xr = _hover(N, 12 + 2)
    pe, pd = _priors(x0, near=(FORCE_W, TORQUE_W))
    plant = dict(force=np.tile(FORCE_W, (B, 1)), torque=np.tile(TORQUE_W, (B, 1)))
    est, dist, dg = _est_spec(3, fields=EALL, **pe), _dist(**pd), _dspec(3)
    kw = dict(noise=ZERO, diagnosis=dg, plant=plant, sqp_iters=sqp_iters)
    whole = _sim(mpc, x0, ub, stuck, 12, sen, est, dist, hull, xr=xr, faults=faults, **kw)
    first = _sim(mpc, x0, ub, stuck, 6, sen, est, dist, hull, xr=xr[:, :6 + N + 2], faults=faults, **kw)
    fd, fb = first["diagnosis"], first["disturbance"]
    sen2 = dict(sen, pending=first["sensor"]["pending"], step0=6)
    est2 = dict(est, xhat=first["estimator"]["xhat"], cov=first["estimator"]["cov"])
    dist2 = dict(dist, force=fb["force"], torque=fb["torque"], cross=fb["cross"], cov=fb["cov"])
    dg2 = dict(dg, state=fd["state"], llr=fd["llr"], detect=(fd["step"], fd["thruster"], fd["level"]), hull_b=fd["hull_b"], no_hull=fd["no_hull"])
    second = _sim(mpc, first["x"], fd["ub"], fd["stuck"], 6, sen2, est2, dist2, hull, xr=xr[:, 6:], faults=_resume(faults, ub, stuck, 6),
                  **dict(kw, diagnosis=dg2))
    assert np.array_equal(second["x"], whole["x"])
    for k in ("x_hist", "u"):
        assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    for grp, keys in (("sensor", ("meas", "pred")), ("estimator", ("est",)), ("disturbance", ("force_hist", "torque_hist")),
                      ("diagnosis", ("llr_hist",))):
        for k in keys:
            assert np.array_equal(np.concatenate([first[grp][k], second[grp][k]]), whole[grp][k]), (grp, k)
    for grp, keys in GROUPS + (("sensor", ("pending",)),):
        for k in keys:
            assert np.array_equal(second[grp][k], whole[grp][k]), (grp, k)
    assert whole["disturbance"]["force_hist"][-1].any() and (whole["diagnosis"]["step"] >= 0).any()


def test_slices_and_device_slots_equal_the_whole():
    B, T = 65, 10
    bt = _two_faults16(B)
    hull = hull_tables(D16, bt["ub"], bt["stuck"])
    sen = _sensor(B, NT)
    pe, pd = _priors(bt["x0"])
    est, dist, dg = _est_spec(3, fields=EALL, **pe), _dist(**pd), _dspec(3)

    def run(mpc, lo=0, hi=B, **kw):
        f = {k: v[lo:hi] for k, v in bt["faults"].items()}
        s = dict(sen, bias=sen["bias"][lo:hi], pending=sen["pending"][lo:hi])
        e = dict(est, xhat=est["xhat"][lo:hi], cov=est["cov"][lo:hi])
        d = dict(dist, **{k: dist[k][lo:hi] for k in ("force", "torque", "cross", "cov")})
        h = dict(hull, set=hull["set"][lo:hi], b=hull["b"][lo:hi], degenerate=hull["degenerate"][lo:hi])
        return _sim(mpc, bt["x0"][lo:hi], bt["ub"][lo:hi], bt["stuck"][lo:hi], T, s, e, d, h, faults=f, diagnosis=dg, **kw)

    def fresh(lo, hi, **kw):
        mpc = ft_mpc_amd.BatchedMPC(N=N, NT=NT, dtype="f64", max_iters=60)
        try:
            return run(mpc, lo, hi, **kw)
        finally:
            mpc.close()
    whole = fresh(0, B)
    parts = [fresh(0, 27, index0=0, index_total=B), fresh(27, B, index0=27, index_total=B)]
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f64", max_iters=60), devices=[0, 0, 0])
    try:
        multi = run(m)
        multi_sqp = run(m, sqp_iters=2)
    finally:
        m.close()
    assert np.array_equal(np.concatenate([p["x"] for p in parts]), whole["x"]) and np.array_equal(multi["x"], whole["x"])
    for k in ("x_hist", "u"):
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), whole[k]), k
        assert np.array_equal(multi[k], whole[k]), k
    hist = ("est", "force_hist", "torque_hist", "llr_hist")
    for grp, keys in GROUPS + (("estimator", ("est", "err_sq")), ("disturbance", ("force_hist", "torque_hist")), ("diagnosis", ("llr_hist",))):
        for k in keys:
            assert np.array_equal(np.concatenate([p[grp][k] for p in parts], axis=1 if k in hist else 0), whole[grp][k]), (grp, k)
            assert np.array_equal(multi[grp][k], whole[grp][k]), (grp, k)
    assert whole["disturbance"]["force_hist"][-1].any() and (whole["diagnosis"]["step"] >= 0).any()
    # the wrench SQP on the driver: the bits of one handle
    mpc = ft_mpc_amd.BatchedMPC(N=N, NT=NT, dtype="f64", max_iters=60)
    try:
        one_sqp = run(mpc, sqp_iters=2)
    finally:
        mpc.close()
    assert np.array_equal(multi_sqp["x"], one_sqp["x"]) and np.array_equal(multi_sqp["u"], one_sqp["u"])
    assert np.array_equal(multi_sqp["disturbance"]["force_hist"], one_sqp["disturbance"]["force_hist"])
    assert not np.array_equal(one_sqp["u"], whole["u"])


# ---------------------------------------------------------------------------------------------------------------------------
# (10) refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _wdentry(obj, x0, ub, stuck, hull, T, tail, fs=None, sqp_iters=0, n=N):
    """the wrench disturbance entry through ctypes with the structs `tail` after the outcomes"""
    B = ub.shape[0]
    multi = isinstance(obj, MultiGPUMPC)
    oc = _lib.ftmpc_outcomes(struct_size=C.sizeof(_lib.ftmpc_outcomes))
    x, uh, xh = x0.copy(), np.zeros((T, B, NT)), np.zeros((T, B, 13))
    bad, abad = np.zeros(T, np.int32), np.zeros(T, np.int32)
    xr, nz = np.ascontiguousarray(_hover(n, T + 2).reshape(-1, order="F")), np.array(NOISE)
    A, hs, hb = (np.ascontiguousarray(hull[k], dtype=t) for k, t in (("A", np.float64), ("set", np.int32), ("b", np.float64)))
    f = getattr(obj.lib, ("ftmpc_multi_simulate_" if multi else "ftmpc_simulate_") + "wrench_disturbance_batch")
    rc = f(obj._h, B, T, _p(x), _p(ub), _p(stuck), _p(A), A.shape[0], _p(hs, ip), _p(hb), int(hull["rows"]), _p(xr), None, _p(nz),
           C.c_uint64(1), sqp_iters, 8, 1e-9, 0.0, fs, _p(uh), _p(xh), _p(bad, ip), _p(abad, ip), C.byref(oc), *tail)
    err = (obj.lib.ftmpc_multi_last_error if multi else obj.lib.ftmpc_last_error)(obj._h)
    return rc, err, dict(x=x, u=uh)


def test_refusals(gpu_mpc_factory):
    """FTMPC_ERR_ARG on a handle and on the driver, the field named, x untouched: everything the thruster entry refuses of the struct
    (with sqp_iters = 2: the count itself is served here), no estimator, what the wrench diagnosis entry refuses, state bounds with
    sqp_iters > 0; the thruster entry keeps refusing sqp_iters > 0; what the front end refuses itself."""
    B, T = 12, 2
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 0, 20)
    hull = hull_tables(D16, ub, stuck)
    mpc = _mpc(gpu_mpc_factory)
    cfgm = ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f64", max_iters=60)
    m = MultiGPUMPC(cfgm, devices=[0, 0, 0])
    xh = np.tile(np.r_[np.zeros(9), 1.0, np.zeros(3)], (B, 1))

    def estimator(with_xhat=False):
        es = _lib.ftmpc_estimator(struct_size=C.sizeof(_lib.ftmpc_estimator), every=1)
        for k in range(4):
            es.p0[k] = es.proc_sigma[k] = es.meas_sigma[k] = SIGMA[k]
        if with_xhat:
            es.xhat = xh.ctypes.data_as(dp)
        return es
    good = _lib.ftmpc_disturbance(struct_size=C.sizeof(_lib.ftmpc_disturbance), compensate=1)
    dgood = _lib.ftmpc_diagnosis(struct_size=C.sizeof(_lib.ftmpc_diagnosis), every=1, n_levels=2, max_detect=2, threshold=18.0)
    dgood.levels[0], dgood.levels[1] = 0.0, F_MAX
    dgood.resid_sigma[0], dgood.resid_sigma[1] = DG.default_sigma(SIGMA, NOISE)
    on = np.full((B, 1), 1, np.int32)
    fub, fst = ub[:, None].copy(), stuck[:, None].copy()
    evs, evb = np.zeros((B, 1), np.int32), np.ascontiguousarray(hull["b"][:, None])

    def schedule(**kw):
        return _lib.ftmpc_fault_schedule(struct_size=C.sizeof(_lib.ftmpc_fault_schedule), n_events=1, onset=_p(on, ip), ub=_p(fub), stuck=_p(fst), **kw)
    v = B - 2
    nh_bad = np.full(B, -1, np.int32)
    nh_bad[v] = -2
    try:
        for obj in (mpc, m):
            def refused(tail, field, vehicle=None, **kw):
                rc, err, out = _wdentry(obj, x0, ub, stuck, hull, T, tail, **kw)
                assert rc == -1 and field.encode() in err, (field, rc, err)
                if vehicle is not None:
                    assert f"vehicle {vehicle} ".encode() in err, err
                assert np.array_equal(out["x"], x0)
            for field, veh, needs_xhat, db, keep in _bad_structs(B):
                es = estimator(needs_xhat)
                for sqp in (0, 2):
                    refused((None, None, None, None, C.byref(es), None, None, None, C.byref(db)), f"ftmpc_disturbance.{field}", veh, sqp_iters=sqp)
            refused((None, None, None, None, None, None, None, None, C.byref(good)), "estimator")
            # what the wrench diagnosis entry refuses
            es = estimator()
            tail = (None, None, None, None, C.byref(es), C.byref(dgood), None, None, C.byref(good))
            refused(tail, "ftmpc_fault_schedule.hull_set must be NULL", fs=C.byref(schedule(hull_set=_p(evs, ip))))
            refused(tail, "ftmpc_fault_schedule.hull_b must be NULL", fs=C.byref(schedule(hull_b=_p(evb))))
            refused((None, None, None, None, C.byref(es), C.byref(dgood), None, _p(nh_bad, ip), C.byref(good)), "no_hull_step", vehicle=v)
            es2 = estimator()
            es2.every = 2
            refused((None, None, None, None, C.byref(es2), C.byref(dgood), None, None, C.byref(good)), "ftmpc_diagnosis.every")
            refused((None, None, None, None, C.byref(es), None, None, None, C.byref(good)), "SQP", sqp_iters=-1)
            # a good struct is accepted, sqp_iters = 0 and 2
            for sqp in (0, 2):
                rc, err, out = _wdentry(obj, x0, ub, stuck, hull, T, (None, None, None, None, C.byref(es), None, None, None, C.byref(good)), sqp_iters=sqp)
                assert rc == 0, err
                assert not np.array_equal(out["x"], x0) and out["u"].any()
        # state bounds with sqp_iters > 0, as without the struct (sqp_iters = 0 is served: kernel 13 has the state rows)
        sb = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, xub=np.full(13, 50.0))
        ms = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f64", max_iters=60, xub=np.full(13, 50.0)), devices=[0, 0, 0])
        try:
            for obj in (sb, ms):
                es = estimator()
                rc, err, out = _wdentry(obj, x0, ub, stuck, hull, T, (None, None, None, None, C.byref(es), None, None, None, C.byref(good)), sqp_iters=2)
                assert rc == -1 and b"state_bounds" in err and np.array_equal(out["x"], x0), err
        finally:
            ms.close()
        # the thruster entry keeps its refusal, and the front end its own without the key
        th = gpu_mpc_factory(N=10, NT=8, dtype="f32")
        x8, ub8, st8, _ = qo.make_batch(B, 10, 8, 0, 20)
        with pytest.raises(ValueError, match="sqp_iters must be 0"):
            th.simulate(x8, ub8, st8, _hover(10, T), T, disturbance=dict(p0=P0D, proc_sigma=QD), estimator=_est_spec(), sqp_iters=2)
        est = _est_spec()
        for kw in (dict(disturbance=_dist(wrench=False), estimator=est), dict(disturbance=_dist(), estimator=None),
                   dict(disturbance=_dist(p0=(1.0, -1.0)), estimator=est), dict(disturbance=_dist(wrench=2), estimator=est)):
            with pytest.raises(ValueError):
                mpc.simulate(x0, ub, stuck, _hover(N, T), T, formulation="wrench", hull=hull, **kw)
        with pytest.raises(ValueError, match="formulation must be 'wrench'"):
            mpc.simulate(x0, ub, stuck, _hover(N, T), T, disturbance=_dist(), estimator=est)
        with pytest.raises(_lib.FtmpcError) as e:
            mpc.eval_cost_wrench(x0, _hover(N, 1)[:, :N + 1].reshape(-1, order="F"), np.zeros((B, N, 6)), dist=np.full((B, 6), np.nan))
        assert e.value.code == -1 and "dist" in str(e.value)
        # both objects give the same bits
        sen = _sensor(B, NT)
        pe, pd = _priors(x0)
        e2, d2 = _est_spec(fields=EALL, **pe), _dist(**pd)
        a, b = (_sim(o, x0, ub, stuck, T, sen, e2, d2, hull, sqp_iters=2) for o in (mpc, m))
        assert np.array_equal(a["x"], b["x"])
        for k in a["disturbance"]:
            assert np.array_equal(a["disturbance"][k], b["disturbance"][k]), k
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (11) it does its job
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,sqp_iters", [(96, 0), (32, 2)])
def test_it_does_its_job(gpu_mpc_factory, B, sqp_iters):
    """Vehicles on the hover reference's orbit, zero noise, a trivial sensor, a constant plant force and torque, the filter gains of
    tests/test_disturbances_host.py::test_filter_converges_on_synthetic_data, T = 59.  compensate = 1: every vehicle's f^ and t^ end
    within 10 % of the plant's and the mean position error of the last five steps is at most a third of the same run's without
    `disturbance` (test G's bound on the thruster form, where 0.196 was measured).  With the diagnosis on and no fault the
    compensated run makes no more detections than the uncompensated one.
    Measured on an MI355X (0.4 s per case): B = 96, sqp_iters = 0: |f^ - f| / |f| <= 2.9e-5, |t^ - t| / |t| <= 5.0e-6; mean position
    error of the last five steps 0.110 m with the estimate, 0.923 m without, ratio 0.119; detections 0 with, 192 without (two per
    vehicle: the uncompensated drift is a residual to every CUSUM test); the largest hull row value of an applied command -0.327 N (no
    row active), no allocation failed.  B = 32, sqp_iters = 2: 2.7e-5, 4.9e-6; 0.102 m against 0.844 m, ratio 0.120; detections 0
    against 64; -0.300 N.
    Why this force and this T: they are test G's of the thruster form (|f| = 1.32 N, |t| = 0.081 N m, T = 59, chosen there so that the
    disturbance's part of the error dominates the loop's own within the run).  On the wrench form (N = 15, 16 thrusters) the loop's own
    error is smaller than on that test's N = 10 handle, so the same choice leaves more room: the ratio is 0.12 where the thruster form
    measured 0.196, and the commanded wrench stays 0.3 N inside the nearest hull row although the controller now commands f_virt plus
    the compensation of 1.32 N."""
    T = T_JOB
    assert 12 < T < 60
    t0 = time.perf_counter()
    x0 = _on_orbit(B, 31)
    ub, stuck = np.full((B, NT), F_MAX), np.zeros((B, NT))
    hull = hull_tables(D16, ub, stuck)
    F, Tq = np.asarray(FORCE_W), np.asarray(TORQUE_W)
    plant = dict(force=np.tile(F, (B, 1)), torque=np.tile(Tq, (B, 1)))
    mpc = _mpc(gpu_mpc_factory)
    xr = _hover(N, T)
    est = dict(EST_G, fields=("est",))
    dg = _dspec()
    on = _sim(mpc, x0, ub, stuck, T, None, est, dict(DIST_G, compensate=True, fields=BALL, wrench=True), hull, noise=ZERO, plant=plant,
              diagnosis=dg, sqp_iters=sqp_iters)
    off = mpc.simulate(x0, ub, stuck, xr, T, noise=ZERO, seed=5, return_inputs=True, return_states=True, estimator=est, plant=plant,
                       diagnosis=dg, formulation="wrench", hull=hull, sqp_iters=sqp_iters)
    ef = np.linalg.norm(on["disturbance"]["force"] - F, axis=1) / np.linalg.norm(F)
    et = np.linalg.norm(on["disturbance"]["torque"] - Tq, axis=1) / np.linalg.norm(Tq)
    e_on = np.linalg.norm(_errors(on["x_hist"], xr)[-5:, :, 0:3], axis=2).mean()
    e_off = np.linalg.norm(_errors(off["x_hist"], xr)[-5:, :, 0:3], axis=2).mean()
    n_on, n_off = int((on["diagnosis"]["step"] >= 0).sum()), int((off["diagnosis"]["step"] >= 0).sum())
    # the commanded wrench stays inside the hull: tau_0 = D (u + stuck) of every applied command against the call's rows
    tau = on["u"] @ D16.T
    slack = max((tau[:, b] @ hull["A"][hull["set"][b]].T - hull["b"][b]).max() for b in range(B))
    print(f"it does its job (B = {B}, sqp_iters = {sqp_iters}): |f^ - f| / |f| <= {ef.max():.3e}, |t^ - t| / |t| <= {et.max():.3e}; mean position "
          f"error of the last 5 steps {e_on:.4e} m with the estimate, {e_off:.4e} m without, ratio {e_on / e_off:.3f}; detections {n_on} "
          f"with, {n_off} without; largest hull row value of a command {slack:.3f}; alloc_failed {int(on['alloc_failed'].sum())}; "
          f"{time.perf_counter() - t0:.1f} s")
    assert ef.max() <= 0.1 and et.max() <= 0.1
    assert e_on <= e_off / 3.0
    assert n_on <= n_off
    assert slack < 0.0 and on["alloc_failed"].sum() == 0
