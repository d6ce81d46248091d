"""GPU: the line-search SQP on the reference's own nonlinear program -- the generalized-force decision with the input hull at
every stage, the 72-row terminal set, the full terminal cost and RK4 dynamics (spiraling_mpc.py:87-238, IPOPT at :346):
ftmpc_eval_cost_wrench_batch, ftmpc_solve_sqp_wrench_batch, ftmpc_simulate_wrench_batch_ex and SpiralingController.solve_mpc with
formulation="wrench".
Checker: `sqp_wrench` below, a NumPy restatement built from the oracle's pieces -- build_qp_wrench, the non-quadratic terminal
gradient through GN (as qp_oracle.sqp_linesearch adds it), ipm_general as solve_wrench_instance calls it, refmath.rk4 /
centre_dx_dt for the cost -- with the merit J + sigma * terminal-set violation and the same line search."""
import numpy as np
import pytest

from ft_mpc_amd.controllers.tools.input_bounds import hull_tables
from ft_mpc_amd.controllers.tools.terminal_ingredients import load_terminal
from oracle import alloc_oracle as ao
from oracle import qp_oracle as qo
from oracle import refmath as rm

pytestmark = pytest.mark.gpu
F_MAX = rm.F_MAX
SIGMA = 1e5      # the library's default merit weight (include/ftmpc.h ftmpc_solve_sqp_wrench_batch)


# ---- NumPy reference of the wrench SQP (one instance) ----
def cost_wrench(cfg, x0, xref, G, uref=None, T=None, term=None):
    """(J, terminal-set violation, centre states [N+1, 13]) of the total-wrench sequence G [N, 6] along the nonlinear rollout."""
    N = cfg.N
    xref = np.asarray(xref, float).reshape(9, N + 1)
    c = rm.robot_to_center(x0, cfg.r)
    X = [c]
    fv = np.concatenate([cfg.f_virt, np.zeros(3)])
    J, viol = 0.0, 0.0
    for k in range(N):
        gen = np.asarray(G[k], float)
        ur = np.zeros(6)
        if uref is not None:
            u_r = np.asarray(uref, float).reshape(6, N + 1)[:, k]
            ur = np.concatenate([rm.rot(c[9:13]).T @ u_r[0:3], u_r[3:6]])
        ut = gen - ur - fv
        J += ut @ (cfg.R * ut)
        c = rm.rk4(lambda s: rm.centre_dx_dt(s, gen, cfg.r, cfg.mass, cfg.J), c, cfg.dt)
        X.append(c)
        e = c[0:9] - xref[:, k + 1]
        if k + 1 < N:
            J += e @ (cfg.Q * e)
        else:
            J += float(T.cost(e)) if T is not None else e @ cfg.P @ e
            if term is not None:
                viol = float(np.maximum(term[0] @ e - term[1], 0.0).sum())
    return float(J), viol, np.array(X)


def sqp_wrench(cfg, x0, ub, stuck, xref, uref=None, warmG=None, T=None, term=None, sigma=SIGMA, sqp_iters=10, backtracks=8,
               tol=1e-9, iters=60):
    """The semantics of ftmpc_solve_sqp_wrench_batch for one instance.  Returns dict(G, cost, cost0, tviol, merits (one per accepted
    step, the start first), sqp_iters, status, margin (the smallest |phi_t - threshold| / (1 + |phi|) of any line-search decision),
    lam (largest terminal-row multiplier of the QPs))."""
    N = cfg.N
    G = np.tile(cfg.D @ np.asarray(stuck, float), (N, 1)) if warmG is None else np.asarray(warmG, float).reshape(N, 6).copy()
    J, v, _ = cost_wrench(cfg, x0, xref, G, uref, T, term)
    phi = J + sigma * v
    out = dict(cost0=J, merits=[phi], sqp_iters=0, status=0, margin=np.inf, lam=0.0)
    for _ in range(sqp_iters):
        qp = qo.build_qp_wrench(cfg, x0, ub, stuck, xref, uref, G, None, term)
        if T is not None:
            qp["g"] = qp["g"] + qp["GN"].T @ T.grad(qp["eN"], quadratic=False)
        d, s, z, nit, st = qo.ipm_general(qp["H"], qp["g"], qp["C"], qp["h"], qp["d0"], qp["nhull"], iters=iters, mu_stop=1e-10,
                                          mu_polish=1e-7)
        out["status"] = st
        if st == 2:
            break
        if term is not None and z.size > qp["nhull"]:
            out["lam"] = max(out["lam"], float(z[qp["nhull"]:].max()))
        step = qp["Tbar"] + d.reshape(N, 6) - G
        thr = phi - tol * (1.0 + abs(phi))
        accepted = False
        for j in range(backtracks):
            Gt = G + 2.0 ** -j * step
            Jt, vt, _ = cost_wrench(cfg, x0, xref, Gt, uref, T, term)
            pt = Jt + sigma * vt
            out["margin"] = min(out["margin"], abs(pt - thr) / (1.0 + abs(phi)))
            if pt < thr:
                G, J, v, phi, accepted = Gt, Jt, vt, pt, True
                break
        if not accepted:
            break
        out["sqp_iters"] += 1
        out["merits"].append(phi)
    out.update(G=G, cost=J, tviol=v)
    return out


def near_terminal_set(B, N, NT, nf, seed, At, bt, scale=2.0):
    """Random poses / faults whose orbit-centre tracking error starts on `scale` times the boundary of the terminal set:
    for some of them the set is reachable within the horizon (often with active rows), for others it is not."""
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, nf, seed)
    rng = np.random.default_rng(seed + 1)
    r = rm.spiral_r()
    for b in range(B):
        e = rng.standard_normal(9)
        e *= scale / max((At @ e / bt).max(), 1e-9)
        R = rm.rot(x0[b, 6:10])
        w = rm.OMEGA_DES + e[6:9]
        x0[b, 0:3] = e[0:3] - R.T @ r                    # robot_to_center (spiral_model.py:103-109) inverted
        x0[b, 3:6] = e[3:6] - R.T @ np.cross(w, r)
        x0[b, 10:13] = w
    return x0, ub, stuck, xref


def parity_batch(B=40, seed=9600):
    """N = 15, 16 thrusters, two faults: half random poses, half near the terminal set (hull-spanning instances only)."""
    N, NT = 15, 16
    term = load_terminal().term_set
    At, bt = term.A, term.b.reshape(-1)
    xa, ua, sa, xref = qo.make_batch(B // 2, N, NT, 2, seed)
    xb, ub_, sb, _ = near_terminal_set(B - B // 2, N, NT, 2, seed + 7, At, bt, scale=1.5)
    x0, ub, stuck = np.vstack([xa, xb]), np.vstack([ua, ub_]), np.vstack([sa, sb])
    keep = ~hull_tables(qo.QPConfig(N=N, NT=NT).D, ub, stuck)["degenerate"]
    return x0[keep], ub[keep], stuck[keep], xref, (At, bt)


# ---- GPU tests ----
@pytest.mark.parametrize("N", [15, 20])
def test_cost_and_terminal_violation(gpu_mpc_factory, N):
    NT, B = 16, 64
    T = load_terminal()
    term = (T.term_set.A, T.term_set.b.reshape(-1))
    with_tc = gpu_mpc_factory(N=N, NT=NT, dtype="f64", terminal_set=T.term_set, terminal_cost=T)
    plain = gpu_mpc_factory(N=N, NT=NT, dtype="f64", terminal_set=T.term_set)
    cfg = qo.QPConfig(N=N, NT=NT)
    x0, ub, stuck, xref = near_terminal_set(B, N, NT, 2, 9500 + N, *term, scale=1.5)
    rng = np.random.default_rng(N)
    G = ((ub / 2 + stuck) @ cfg.D.T)[:, None, :] + rng.uniform(-1.0, 1.0, (B, N, 6))
    traj = rm.circle_trajectory(0.1, 10, radius=0.65, s_per_circle=40.0)
    xr_all, ur_all = rm.assign_trajectory(traj, N)
    xw, uw = rm.trajectory_window(xr_all, ur_all, 0.5, N)
    per_x = np.stack([xw.reshape(-1, order="F")] * B)            # a per-window reference (stride 9 (N+1))
    per_u = np.stack([uw.reshape(-1, order="F")] * B)
    nviol = 0
    for mpc, tc in ((with_tc, T), (plain, None)):
        for (xr, ur, xr_h, ur_h) in ((xref.reshape(-1, order="F"), None, xref, None), (per_x, per_u, xw, uw)):
            J, V = mpc.eval_cost_wrench(x0, xr, G, uref=ur, return_tviol=True)
            for b in range(B):
                Jr, Vr, _ = cost_wrench(cfg, x0[b], xr_h, G[b], ur_h, tc, term)
                assert J[b] == pytest.approx(Jr, rel=1e-10), (b, J[b], Jr)
                assert abs(V[b] - Vr) <= 1e-12, (b, V[b], Vr)
                nviol += Vr > 0
    assert nviol >= 8      # (some of the points lie outside the set)


def test_sqp_parity_float64(gpu_mpc_factory):
    N, NT = 15, 16
    T = load_terminal()
    x0, ub, stuck, xref, term = parity_batch()
    B = x0.shape[0]
    assert B >= 32
    cfg = qo.QPConfig(N=N, NT=NT)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, terminal_set=T.term_set, terminal_cost=T)
    out = mpc.solve_sqp_wrench(x0, ub, stuck, xref.reshape(-1, order="F"), sqp_iters=10, backtracks=8)
    hull = hull_tables(cfg.D, ub, stuck)
    excluded, progressed = [], 0
    for b in range(B):
        ref = sqp_wrench(cfg, x0[b], ub[b], stuck[b], xref, T=T, term=term, sqp_iters=10, backtracks=8)
        assert all(m1 < m0 for m0, m1 in zip(ref["merits"], ref["merits"][1:]))      # the merit never increases
        assert out["cost0"][b] == pytest.approx(ref["cost0"], rel=1e-10)
        if ref["margin"] <= 1e-10:
            excluded.append(b)
            continue
        assert out["sqp_iters"][b] == ref["sqp_iters"], (b, out["sqp_iters"][b], ref["sqp_iters"])
        progressed += ref["sqp_iters"] >= 2
        assert np.abs(out["G"][b] - ref["G"]).max() / F_MAX <= 1e-6, (b, np.abs(out["G"][b] - ref["G"]).max())
        assert out["cost"][b] == pytest.approx(ref["cost"], rel=1e-9)
        assert abs(out["tviol"][b] - ref["tviol"]) <= 1e-9
        A = hull["A"][hull["set"][b]]
        assert (out["G"][b] @ A.T - hull["b"][b] <= 1e-9 * F_MAX).all()      # hull rows at every stage
        want = out["tau0"][b] - cfg.D @ stuck[b]
        assert np.array_equal(out["tau0"][b], out["G"][b][0]) and out["alloc_status"][b] == 0
        assert np.abs(out["u0"][b] - ao.allocate(cfg.D, want, ub[b])[0]).max() / F_MAX <= 1e-6
    print(f"wrench SQP parity: {B} instances, {len(excluded)} excluded (line-search decision within 1e-10 of the threshold)")
    assert len(excluded) <= 1, excluded
    assert progressed >= B // 4


def test_one_iteration_is_the_wrench_step(gpu_mpc_factory):
    """sqp_iters = 1 with the full step accepted: the QP of solve_wrench from the same warm start, one step."""
    N, NT = 15, 16
    T = load_terminal()
    x0, ub, stuck, xref, _ = parity_batch(B=32, seed=9700)
    B = x0.shape[0]
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, terminal_set=T.term_set, terminal_cost=T)
    cfg = qo.QPConfig(N=N, NT=NT)
    rng = np.random.default_rng(3)
    W = np.ascontiguousarray(((ub / 2 + stuck) @ cfg.D.T)[:, None, :] + rng.uniform(-0.1, 0.1, (B, N, 6)))
    out = mpc.solve_sqp_wrench(x0, ub, stuck, xref.reshape(-1, order="F"), warmG=W, sqp_iters=1)
    one = mpc.solve_wrench(x0, ub, stuck, xref.reshape(-1, order="F"), warmG=W.copy(), return_G=True)
    full = 0
    for b in range(B):
        if out["sqp_iters"][b] != 1 or one["status"][b] == 2:
            continue
        step = np.abs(out["G"][b] - W[b]).max()
        if np.abs(out["G"][b] - one["G"][b]).max() > 0.5 * step:
            continue      # (a shorter step was accepted)
        full += 1
        assert np.abs(out["G"][b] - one["G"][b]).max() / F_MAX <= 1e-12, b
        # (the allocation stops at a residual of 1e-8 (1 + |tau|): the commands agree to that, not to the last bit)
        assert np.abs(out["u0"][b] - one["u0"][b]).max() / F_MAX <= 1e-7, b
    assert full >= B // 2, full


def test_fp32_handle_against_float64(gpu_mpc_factory):
    """Kernel 11 with its hand-over in every QP against the float64 handle.  Measured on this batch: worst merit gap 2.0e-7 relative,
    no terminal violation where the float64 run has none; one borderline instance whose first QP the fp32 handle finds infeasible
    (status 2: the SQP stops at its start point) and the float64 handle does not -- the reachability verdicts of the two kernels may
    differ on such instances (tests/test_gpu_wrench.py)."""
    N, NT = 15, 16
    T = load_terminal()
    x0, ub, stuck, xref, _ = parity_batch(B=128, seed=9800)
    xr = xref.reshape(-1, order="F")
    kw = dict(N=N, NT=NT, max_iters=60, terminal_set=T.term_set, terminal_cost=T)
    o64 = gpu_mpc_factory(dtype="f64", **kw).solve_sqp_wrench(x0, ub, stuck, xr)
    o32 = gpu_mpc_factory(dtype="f32", **kw).solve_sqp_wrench(x0, ub, stuck, xr)
    same = (o64["sqp_iters"] > 0) == (o32["sqp_iters"] > 0)       # (both left the start point, or neither)
    phi = lambda o: o["cost"] + SIGMA * o["tviol"]
    rel = np.abs(phi(o32) - phi(o64))[same] / np.abs(phi(o64))[same]
    inside = same & (o64["tviol"] <= 1e-9)
    print(f"fp32 handle: {int((~same).sum())} borderline verdicts, worst relative merit gap {rel.max():.2e}, worst terminal "
          f"violation where float64 has none {o32['tviol'][inside].max():.2e}")
    assert (~same).sum() <= 1, np.flatnonzero(~same)
    assert rel.max() <= 1e-5, (rel.max(), int(np.flatnonzero(same)[rel.argmax()]))
    assert o32["tviol"][inside].max() <= 1e-5
    assert (o32["alloc_status"] == 0).all()
    assert (o32["u0"] >= -1e-12).all() and (o32["u0"] <= ub + 1e-9).all()


def test_closed_loop_equals_the_step_by_step_loop(gpu_mpc_factory):
    from oracle import c_oracle as co
    from oracle import closed_loop as cl
    N, NT, B, T = 15, 16, 6, 5
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60)
    cfg = qo.QPConfig(N=N, NT=NT)
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 2, 9900)
    ub[0] = 3.4; stuck[0] = 0.0
    xr = np.zeros((9, T + N))
    xr[8] = 0.6
    out = mpc.simulate(x0, ub, stuck, xr, T, seed=5, return_inputs=True, formulation="wrench", sqp_iters=3)
    assert out["alloc_failed"].sum() == 0
    x = x0.copy()
    amp = np.repeat(np.full(4, 1e-3), [3, 3, 4, 3])
    warm = None
    for t in range(T):
        step = mpc.solve_sqp_wrench(x, ub, stuck, np.ascontiguousarray(xr[:, t:t + N + 1]).reshape(-1, order="F"), warmG=warm, sqp_iters=3)
        assert (step["alloc_status"] == 0).all()
        assert np.abs(step["u0"] - out["u"][t]).max() < 1e-8, t
        warm = np.ascontiguousarray(np.concatenate([step["G"][:, 1:], step["G"][:, -1:]], axis=1))
        for b in range(B):
            x[b] = co.plant_step(cfg, x[b], step["u0"][b], ub[b], stuck[b])
        idx = (np.uint64(t) * np.uint64(B) + np.arange(B, dtype=np.uint64))[:, None] * np.uint64(13) + np.arange(13, dtype=np.uint64)[None, :]
        x = x + amp[None, :] * cl.u01(5, idx)
        x[:, 6:10] /= np.linalg.norm(x[:, 6:10], axis=1, keepdims=True)
    assert np.abs(out["x"] - x).max() < 1e-8


def test_controller_solve_mpc_in_the_wrench_formulation():
    from ft_mpc_amd.controllers.spiraling_mpc import SpiralingController
    from ft_mpc_amd.models.spiral_model import SpiralModel
    from ft_mpc_amd.models.sys_model import SystemModel
    from ft_mpc_amd.util.broken_thruster import BrokenThruster
    params = {"horizon": 15, "param_set": "P1", "P1": {"Q": [1, 1, 1, 1, 1, 1, 2, 2, 2], "R": [0.1, 0.1, 0.1, 0.01, 0.01, 0.01]},
              "max_iters": 60, "formulation": "wrench", "terminal_set": True}
    m = SystemModel(0.1)
    m.set_fault(BrokenThruster(10, 1.0))
    m.set_fault(BrokenThruster(11, 0.4))
    sm = SpiralModel.from_system_model(m)
    c0 = sm.robot_to_center(np.array([0.05, -0.02, 0.03, 0.01, 0.02, -0.01, 0.0, 0.0, 0.0, 1.0, 0.01, -0.02, 0.62]))
    res = {}
    for it in (1, 5):
        ctrl = SpiralingController(sm, dict(params, sqp_iters=it), None, quiet=True)
        ctrl.load_trajectory("hover", 10)
        xs, us, _, cost, status = ctrl.solve_mpc(c0)
        assert len(xs) == 16 and len(us) == 15 and all(u.shape == (6,) for u in us) and all(x.shape == (13,) for x in xs)
        assert np.abs(xs[0] - c0).max() <= 1e-12
        assert status == "Solve_Succeeded"
        G = ctrl.optimal_wrench
        J = ctrl.mpc.eval_cost_wrench(sm.center_to_robot(c0)[None], ctrl.x_sp.reshape(-1), G[None], uref=ctrl.u_sp.reshape(-1))[0]
        assert cost == pytest.approx(J, rel=1e-12)
        fv = np.concatenate([ctrl.spiral_params.f_virt, np.zeros(3)])
        assert np.abs(us[0] - (G[0] - fv)).max() <= 1e-12      # (hover: u_ref = 0)
        res[it] = cost
        ctrl.mpc.close()
    assert res[5] <= res[1]


def test_bad_arguments_are_refused(gpu_mpc_factory):
    from ft_mpc_amd._lib import FtmpcError
    N, NT = 15, 16
    x0, ub, stuck, xref = qo.make_batch(4, N, NT, 1, 5)
    xr = xref.reshape(-1, order="F")
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f64")
    for kw in (dict(sqp_iters=-1), dict(backtracks=0)):
        with pytest.raises(FtmpcError) as e:
            mpc.solve_sqp_wrench(x0, ub, stuck, xr, **kw)
        assert e.value.code == -1
    hull = hull_tables(qo.QPConfig(N=N, NT=NT).D, ub, stuck)
    bad = dict(hull, set=np.full(4, hull["A"].shape[0], np.int32))
    with pytest.raises(FtmpcError) as e:
        mpc.solve_sqp_wrench(x0, ub, stuck, xr, hull=bad)
    assert e.value.code == -1
    sb = gpu_mpc_factory(N=N, NT=NT, dtype="f64", xub=np.full(13, 50.0))
    with pytest.raises(FtmpcError) as e:
        sb.solve_sqp_wrench(x0, ub, stuck, xr)
    assert e.value.code == -1
