"""GPU: the reference's optional STATE BOUNDS on its own formulation -- the generalized-force program with the input hull
(spiraling_mpc.py:129-130,179-185 beside :133-137,175-177).  The HIP path is kernel 13's state-bound instantiation
(ftmpc_solve_ricw64_kernel<*, false, true>: a diagonal barrier term on the state weight of the bounded stage and an entry of its
state-linear term); the checker is tests/wrench_state_rows.py -- the same rows written out DENSE through the sensitivities behind
the hull rows of oracle/qp_oracle.py:build_qp_wrench, ipm_general with its active-set polish, certified by KKT residuals: the EXACT
solution.  Tolerance: 1e-4 f_max on the whole-horizon wrenches (this mode stops at mu 1e-10 and has no
polish; on the CPU the unpolished iterate is up to 3.6e-5 f_max from the polished one on these batches).

Measured (MI355X, both handle dtypes alike): worst 4.7e-6 / 2.2e-6 / 2.8e-6 / 3.6e-5 f_max on the wrenches of the four batches, 4.6e-6 on
tau0, rows violated by at most 4e-16; the same instances solved (15 / 14 / 11 / 5) and active (7 / 5 / 6 / 1) as the oracle."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))

from oracle import c_oracle as co
from oracle import qp_oracle as qo
from oracle import refmath as rm
import wrench_state_rows as ws

pytestmark = pytest.mark.gpu
F_MAX = rm.F_MAX
GOLD = Path(__file__).parent / "golden"
TOL = 1e-4


def _check_allocation(cfg, out, b, ub, stuck):
    want = out["tau0"][b] - cfg.D @ stuck[b]
    assert out["alloc_status"][b] == 0
    assert np.abs(cfg.D @ out["u0"][b] - want).max() <= 1e-7 * (1 + np.abs(want).max())
    assert (out["u0"][b][ub[b] == 0] == 0).all() and (out["u0"][b] >= -1e-12).all() and (out["u0"][b] <= ub[b] + 1e-9).all()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", ws.BATCHES)
def test_wrench_state_bounds_against_the_oracle(gpu_mpc_factory, shape, dtype):
    N, NT, nf, B, seed = shape
    xlb, xub = ws.bounds()
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype=dtype, max_iters=60, xlb=xlb, xub=xub)
    free = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60)
    cfg = qo.QPConfig(N=N, NT=NT)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, nf, seed)
    xr = xref.reshape(-1, order="F")
    out = mpc.solve_wrench(x0, ub, stuck, xr, return_G=True)
    ref = free.solve_wrench(x0, ub, stuck, xr, return_G=True)
    assert not (out["status"] == 3).any()      # (no flat hulls in these batches)
    solved = active = 0
    worst = worst0 = viol = 0.0
    with np.errstate(all="ignore"):
        for b in range(B):
            tau0, T, st, _, qp = ws.solve_wrench_state_instance(cfg, x0[b], ub[b], stuck[b], xref, xlb, xub)
            assert (out["status"][b] == 0) == (st == 0), (b, out["status"][b], st)
            assert np.isfinite(out["G"][b]).all() and np.isfinite(out["tau0"][b]).all() and np.isfinite(out["u0"][b]).all()
            if st != 0:
                continue
            solved += 1
            assert max(qo.kkt_general(qp["H"], qp["g"], qp["C"], qp["h"], qp["d"], qp["z"])) < 1e-7
            err, err0 = np.abs(out["G"][b] - T).max() / F_MAX, np.abs(out["tau0"][b] - tau0).max() / F_MAX
            worst, worst0 = max(worst, err), max(worst0, err0)
            # the state rows hold along the linearised prediction of the GPU's wrenches (the test's own rows)
            nh = qp["nhull"]
            res = qp["C"][nh:] @ (out["G"][b] - qp["Tbar"]).reshape(-1) - qp["h"][nh:]
            viol = max(viol, res.max())
            na = ws.active_state_rows(qp)
            diff = np.abs(out["G"][b] - ref["G"][b]).max() / F_MAX
            print(f"  b={b} err={err:.2e} tau0={err0:.2e} rows={res.max():.2e} active={na} vs_free={diff:.2e} it={out['iters'][b]}")
            assert err <= TOL and err0 <= TOL, (b, err, err0)
            assert res.max() <= 1e-8, (b, res.max())
            active += int(na > 0)
            if na > 0:
                assert diff > 1e-5, (b, diff)      # the rows matter
            _check_allocation(cfg, out, b, ub, stuck)
    print(f"{shape} {dtype}: solved {solved}/{B} active {active} worst G {worst:.2e} tau0 {worst0:.2e} f_max, rows {viol:.2e}")
    assert (solved, active) == ws.COUNTS[shape]


def test_wrench_state_bounds_against_golden(gpu_mpc_factory):
    d = np.load(GOLD / "qp_wrench_state_n15.npz")
    mpc = gpu_mpc_factory(N=int(d["N"]), NT=int(d["NT"]), dtype="f32", max_iters=60, xlb=d["xlb"], xub=d["xub"])
    out = mpc.solve_wrench(d["x0"], d["ub"], d["stuck"], d["xref"].reshape(-1, order="F"), return_G=True)
    ok = d["status"] == 0
    assert np.array_equal(out["status"] == 0, ok) and ok.sum() == 15 and (d["active_rows"][ok] > 0).sum() == 7
    print("golden: worst", np.abs(out["G"][ok] - d["G"][ok]).max() / F_MAX)
    assert np.abs(out["G"][ok] - d["G"][ok]).max() / F_MAX <= TOL
    assert np.isfinite(out["G"]).all() and np.isfinite(out["u0"]).all()


def test_no_finite_bound_is_the_plain_problem_and_one_sided_bounds(gpu_mpc_factory):
    """All bounds infinite: the state-bound instantiation returns plain kernel 13's solution (no rows; mu 1e-10 without polish against
    the polished result); an upper bound alone (the reference fills the missing side with infinities, spiraling_mpc.py:181-182)
    against the oracle."""
    N, NT, B = 20, 8, 12
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, 1, 5128)
    xr = xref.reshape(-1, order="F")
    plain = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60).solve_wrench(x0, ub, stuck, xr, return_G=True)
    none = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, xub=np.full(13, np.inf)).solve_wrench(x0, ub, stuck, xr, return_G=True)
    assert (plain["status"] == 0).all() and (none["status"] == 0).all()
    print("no finite bound vs plain:", np.abs(none["G"] - plain["G"]).max() / F_MAX)
    assert np.abs(none["G"] - plain["G"]).max() / F_MAX <= 2e-5
    xub = np.full(13, np.inf)
    xub[3:6] = 0.9
    one = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, xub=xub).solve_wrench(x0, ub, stuck, xr, return_G=True)
    cfg = qo.QPConfig(N=N, NT=NT)
    solved = 0
    with np.errstate(all="ignore"):
        for b in range(B):
            _, T, st, _, _ = ws.solve_wrench_state_instance(cfg, x0[b], ub[b], stuck[b], xref, None, xub)
            assert (one["status"][b] == 0) == (st == 0)
            assert np.isfinite(one["G"][b]).all()
            if st == 0:
                solved += 1
                assert np.abs(one["G"][b] - T).max() / F_MAX <= TOL, (b, np.abs(one["G"][b] - T).max() / F_MAX)
    assert solved >= B // 2


def _hover_traj(N, T):
    xr = np.zeros((9, T + N))
    xr[8] = 0.6
    return xr


def _centre_speed(cfg, x):
    return np.array([np.abs(rm.robot_to_center(x[b], cfg.r)[3:6]).max() for b in range(x.shape[0])])


def test_bounded_two_stage_loop_equals_the_step_by_step_loop_and_keeps_the_velocity_bound(gpu_mpc_factory):
    """ftmpc_simulate_wrench_batch on a state-bound handle against solve_wrench per step on that handle with the oracle's plant step
    and the repeat-last warm-start shift (noise off).  |v| <= 0.7: two vehicles of this batch exceed it in the unbounded loop (0.87 and
    0.93 m/s on the CPU oracle's loop); under the bound every step's PREDICTED states respect it."""
    N, NT, B, T, VB = 15, 16, 6, 6, 0.7
    xub, xlb = np.full(13, np.inf), np.full(13, -np.inf)
    xub[3:6], xlb[3:6] = VB, -VB
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, xlb=xlb, xub=xub)
    free = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60)
    cfg = qo.QPConfig(N=N, NT=NT)
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 2, 8500)
    xr = _hover_traj(N, T)
    quiet = (0.0, 0.0, 0.0, 0.0)
    out = mpc.simulate(x0, ub, stuck, xr, T, noise=quiet, return_inputs=True, formulation="wrench")
    assert out["not_converged"].sum() == 0 and out["alloc_failed"].sum() == 0
    unb = free.simulate(x0, ub, stuck, xr, T, noise=quiet, formulation="wrench", return_states=True)
    vfree = np.max([_centre_speed(cfg, unb["x_hist"][t]) for t in range(T)], axis=0)
    assert (vfree > VB + 0.1).sum() >= 2, vfree      # the bound is one the plain controller breaks
    x = x0.copy()
    warm = None
    vmax = np.zeros(B)
    for t in range(T):
        lin = None if warm is None else warm.copy()      # (solve_wrench overwrites its warm start with the solution)
        step = mpc.solve_wrench(x, ub, stuck, np.ascontiguousarray(xr[:, t:t + N + 1]).reshape(-1, order="F"), warmG=warm, return_G=True)
        assert (step["status"] == 0).all() and (step["alloc_status"] == 0).all()
        assert np.abs(step["u0"] - out["u"][t]).max() < 1e-8, t
        for b in range(B):      # the bound along the linearised prediction of this step's wrenches
            Cx, hx, _ = ws.state_rows(cfg, x[b], stuck[b], xlb, xub, warmG=None if lin is None else lin[b])
            Tbar = np.tile(cfg.D @ stuck[b], (N, 1)) if lin is None else lin[b]
            assert (Cx @ (step["G"][b] - Tbar).reshape(-1) <= hx + 1e-8).all(), (t, b)
        warm = np.ascontiguousarray(np.concatenate([step["G"][:, 1:], step["G"][:, -1:]], axis=1))
        for b in range(B):
            x[b] = co.plant_step(cfg, x[b], step["u0"][b], ub[b], stuck[b])
        x[:, 6:10] /= np.linalg.norm(x[:, 6:10], axis=1, keepdims=True)
        vmax = np.maximum(vmax, _centre_speed(cfg, x))
    assert np.abs(out["x"] - x).max() < 1e-8
    print("centre speed, unbounded loop:", vfree.round(3), "bounded:", vmax.round(3))
    assert (vmax <= VB + 0.02).all()      # (the plant is the nonlinear one: the bound holds on the prediction, nearly on the run)


def test_bounded_two_stage_loop_with_a_fault_that_starts_mid_run(gpu_mpc_factory):
    N, NT, B, T = 15, 16, 4, 6
    xlb, xub = ws.bounds()
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, xlb=xlb, xub=xub)
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 1, 8600)
    eub, est = ub.copy(), stuck.copy()
    for b in range(B):      # one more thruster breaks at step 2 or 3, stuck at half thrust
        i = int(np.flatnonzero(ub[b] > 0)[b])
        eub[b, i], est[b, i] = 0.0, 1.7
    faults = dict(onset=(2 + np.arange(B) % 2).astype(np.int32)[:, None], ub=eub[:, None, :], stuck=est[:, None, :])
    out = mpc.simulate(x0, ub, stuck, _hover_traj(N, T), T, noise=(0.0,) * 4, return_inputs=True, formulation="wrench", faults=faults,
                       detect_delay=1, return_states=True)
    assert np.isfinite(out["x"]).all() and np.isfinite(out["u"]).all() and np.isfinite(out["x_hist"]).all()
    assert out["not_converged"].shape == (T,) and (out["not_converged"] >= 0).all() and (out["not_converged"] <= B).all()
    assert (out["u"] >= -1e-9).all() and (out["u"] <= 3.4 + 1e-9).all()
    print("not_converged per step:", out["not_converged"], "alloc_failed:", out["alloc_failed"])


def test_what_has_no_state_rows_is_refused(gpu_mpc_factory):
    from ft_mpc_amd._lib import FtmpcError
    N, NT, B, T = 15, 16, 4, 2
    xlb, xub = ws.bounds()
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, 1, 5)
    xr = xref.reshape(-1, order="F")
    sb = gpu_mpc_factory(N=N, NT=NT, dtype="f64", xlb=xlb, xub=xub)
    with pytest.raises(FtmpcError) as e:
        sb.solve_sqp_wrench(x0, ub, stuck, xr)
    assert e.value.code == -1
    with pytest.raises(FtmpcError) as e:
        sb.simulate(x0, ub, stuck, _hover_traj(N, T), T, formulation="wrench", sqp_iters=2)
    assert e.value.code == -1
    with pytest.raises(FtmpcError) as e:
        sb.simulate(x0, ub, stuck, _hover_traj(N, T), T, formulation="wrench", sqp_iters=2, return_states=True)
    assert e.value.code == -1
    dense = gpu_mpc_factory(N=N, NT=NT, dtype="f64", kernel_select="dense", xlb=xlb, xub=xub)
    with pytest.raises(FtmpcError) as e:
        dense.solve_wrench(x0, ub, stuck, xr)
    assert e.value.code == -1
    with pytest.raises(FtmpcError) as e:
        dense.simulate(x0, ub, stuck, _hover_traj(N, T), T, formulation="wrench")
    assert e.value.code == -1


def test_controller_wrench_formulation_with_xub_xlb(gpu_mpc_factory):
    """SpiralingController takes the reference's own keys params["xub"] / params["xlb"] on formulation "wrench"."""
    import yaml
    from ft_mpc_amd import _lib
    from ft_mpc_amd.controllers.spiraling_mpc import SpiralingController
    from ft_mpc_amd.models.sys_model import SystemModel
    from ft_mpc_amd.util.controller_debug import ControllerDebug
    params = yaml.safe_load(open(Path(_lib.__file__).parent / "config" / "reactive.yaml"))["tuning"]["spiraling"]
    xlb, xub = ws.bounds(0.5, 1.2)
    m = SystemModel(0.1)
    ctl = SpiralingController(m, dict(params, xub=xub, xlb=xlb, formulation="wrench"), ControllerDebug(), quiet=True)
    ctl.load_trajectory("hover", 10)
    x = np.array([1.0, 0.0, 1.0, 0.3, 0.1, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.6])
    u = ctl.get_control(x, 0.0)
    assert u.shape == (16,) and np.isfinite(u).all() and (u >= -1e-9).all() and (u <= 3.4 + 1e-9).all()
    ctl.mpc.close()
    with pytest.raises(ValueError):
        SpiralingController(m, dict(params, xub=xub, xlb=xlb, formulation="wrench", sqp_iters=3), ControllerDebug(), quiet=True)
