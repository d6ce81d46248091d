"""GPU: the terminal set on the thruster-space Riccati kernel (ftmpc_solve_ric64_kernel<NV, false, true>).

The thruster form with the 72 rows of config/terminal.yaml used to live on the dense float64 kernel alone (N * NT <= 256, N <= 16
for the 16-thruster reference vehicle).  Kernel 12's terminal-set instantiations take every horizon up to 40: the rows are a 9 x 9
term on the terminal weight of the Riccati recursion and a 9-vector on the terminal state-linear term.  Checked here:
  * parity with oracle/qp_oracle.py:solve_box_terminal_instance instance by instance at N = 17 (n = 272, the first size the
    dense kernel refused; NV = 6), N = 20 and N = 40 (NV = 10), reachable and unreachable sets;
  * A/B against the dense kernel's general-row mode at N = 15 (NV = 4) through kernel_select = "riccati";
  * the rows matter; the persistent loop; the callers of the thruster-space step (fp32 handle, closed loop, on-device SQP);
  * what stays refused.
Tolerance: 1e-6 f_max on the whole horizon, the project's float64 general-row tolerance."""
import numpy as np
import pytest

from ft_mpc_amd._lib import FtmpcError
from ft_mpc_amd.controllers.tools.terminal_ingredients import load_terminal
from oracle import qp_oracle as qo
from oracle import refmath as rm
from test_gpu_wrench import _near_terminal_set

pytestmark = pytest.mark.gpu
F_MAX = rm.F_MAX
TOL = 1e-6
NT = 16
RIC, DENSE = "ftmpc_solve_ric64_kernel", "ftmpc_solve_f64_kernel"


@pytest.fixture(scope="module")
def term():
    t = load_terminal().term_set
    return t, t.A, t.b.reshape(-1)


def _oracle(N, x0, ub, stuck, xref, At, bt):
    cfg = qo.QPConfig(N=N, NT=NT)
    with np.errstate(all="ignore"):
        return qo.solve_box_terminal_instance(cfg, x0, ub, stuck, xref, (At, bt), iters=60)


def _inside_box(U, ub):
    return np.isfinite(U).all() and (U >= 0).all() and (U <= ub[None, :] + 1e-9).all()


@pytest.mark.parametrize("N,B,seed,scale,min_solved,min_active,some_unreachable",
                         [(17, 12, 9901, 2.0, 12, 4, False), (17, 12, 9901, 6.0, 4, 2, True), (20, 12, 9902, 8.0, 4, 2, True),
                          (40, 8, 9903, 2.0, 8, 6, False), (40, 8, 9903, 12.0, 2, 1, True)])
def test_parity_with_the_oracle(gpu_mpc_factory, term, N, B, seed, scale, min_solved, min_active, some_unreachable):
    t, At, bt = term
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, terminal_set=t)
    x0, ub, stuck, xref = _near_terminal_set(B, N, NT, 2, seed, At, bt, scale)
    mpc.set_profiling(True)
    out = mpc.solve(x0, ub, stuck, xref.reshape(-1, order="F"), return_U=True)
    assert RIC in mpc.last_kernel_ms() and DENSE not in mpc.last_kernel_ms()
    mpc.set_profiling(False)
    solved = active = 0
    worst = 0.0
    for b in range(B):
        _, U, st, nit, qp = _oracle(N, x0[b], ub[b], stuck[b], xref, At, bt)
        print(f"N={N} scale={scale} b={b}: oracle st={st} it={nit}  gpu st={out['status'][b]} it={out['iters'][b]}"
              f"  |dU|/f_max={np.abs(out['U'][b] - U).max() / F_MAX:.2e}")
        assert (out["status"][b] == 0) == (st == 0), (b, out["status"][b], st)
        if st != 0:
            assert _inside_box(out["U"][b], ub[b]), b
            continue
        solved += 1
        assert max(qo.kkt_general(qp["H"], qp["g"], qp["C"], qp["h"], qp["d"], qp["z"])) < 1e-7, b
        err = np.abs(out["U"][b] - U).max() / F_MAX
        worst = max(worst, err)
        assert err <= TOL, (b, err)
        d = (out["U"][b][:, qp["act"]]).reshape(-1) - qp["Ubar"]
        assert (At @ (qp["eN"] + qp["GN"] @ d) <= bt + 1e-7).all(), b      # the set holds on the GPU solution
        active += int((qp["z"][qp["nhull"]:] > 1e-6).any())
    print(f"N={N} scale={scale}: solved {solved}/{B}, active rows on {active}, worst |dU|/f_max {worst:.2e}")
    assert solved >= min_solved and active >= min_active
    assert (solved < B) == some_unreachable


def test_ab_against_the_dense_kernel(gpu_mpc_factory, term):
    """N = 15: both kernels serve the shape.  kernel_select = "riccati" takes kernel 12 (NV = 4), the default keeps kernel 3."""
    t, At, bt = term
    N, B = 15, 24
    x0, ub, stuck, xref = _near_terminal_set(B, N, NT, 2, 31, At, bt, scale=1.5)
    xr = xref.reshape(-1, order="F")
    res = {}
    for sel, name, other in (("riccati", RIC, DENSE), ("auto", DENSE, RIC)):
        mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, terminal_set=t, kernel_select=sel)
        mpc.set_profiling(True)
        res[sel] = mpc.solve(x0, ub, stuck, xr, return_U=True)
        ms = mpc.last_kernel_ms()
        assert name in ms and other not in ms, (sel, ms)
    a, d = res["riccati"], res["auto"]
    assert np.array_equal(a["status"], d["status"]), (a["status"], d["status"])
    both = a["status"] == 0
    assert both.sum() >= 6
    err = np.abs(a["U"][both] - d["U"][both]).max() / F_MAX
    print(f"A/B N=15: solved {both.sum()}/{B}, |dU|/f_max {err:.2e}, iters riccati {a['iters'].mean():.1f} dense {d['iters'].mean():.1f}")
    assert err <= TOL, err
    assert np.isfinite(a["U"]).all()


def test_the_rows_matter(gpu_mpc_factory, term):
    t, At, bt = term
    N, B = 20, 12
    x0, ub, stuck, xref = _near_terminal_set(B, N, NT, 2, 9902, At, bt, 8.0)
    xr = xref.reshape(-1, order="F")
    out = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, terminal_set=t).solve(x0, ub, stuck, xr, return_U=True)
    free = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60).solve(x0, ub, stuck, xr, return_U=True)
    ok = out["status"] == 0
    assert ok.sum() >= 4
    assert np.abs(free["U"][ok] - out["U"][ok]).max() / F_MAX > 1e-4


def test_persistent_loop(gpu_mpc_factory, term):
    """More than twice as many instances as the persistent grid has waves (eight resident waves on each of the 256 CUs: 2 048, the
    host launches min(B, grid)): every wave pulls two or more instances from the shared cursor, far states (set unreachable) and
    near-set states mixed half and half, and each must start from clean per-instance state -- the rows of term_A, q_N, psi_N, m9,
    GN GN', the row tail of the slot, the polish flag."""
    t, At, bt = term
    N, B = 17, 4608
    x0, ub, stuck, xref = _near_terminal_set(B, N, NT, 2, 9911, At, bt, 2.0)
    far = qo.make_batch(B, N, NT, 2, 9911)[0]
    x0[1::2] = far[1::2]
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, terminal_set=t)
    out = mpc.solve(x0, ub, stuck, xref.reshape(-1, order="F"), return_U=True)
    assert np.isfinite(out["U"]).all() and np.isfinite(out["u0"]).all()
    assert (out["status"][0::2] == 0).sum() >= B // 4
    checked = 0
    for b in np.linspace(0, B - 1, 16).astype(int):      # a sample spread over the batch: eight near-set, eight far instances
        _, U, st, nit, qp = _oracle(N, x0[b], ub[b], stuck[b], xref, At, bt)
        assert (out["status"][b] == 0) == (st == 0), (b, out["status"][b], st)
        if st == 0:
            checked += 1
            assert np.abs(out["U"][b] - U).max() / F_MAX <= TOL, (b, np.abs(out["U"][b] - U).max() / F_MAX)
    assert checked >= 4      # (at scale 2.0 the oracle reaches the set from every near-set start of the parity batch: half the sample's eight)


def test_callers_of_the_thruster_step(gpu_mpc_factory, term):
    t, At, bt = term
    N, B, T = 17, 8, 3
    x0, ub, stuck, xref = _near_terminal_set(B, N, NT, 2, 9921, At, bt, 1.5)
    xr = xref.reshape(-1, order="F")
    m32 = gpu_mpc_factory(N=N, NT=NT, dtype="f32", max_iters=60, terminal_set=t)
    m64 = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, terminal_set=t)
    a, b = m32.solve(x0, ub, stuck, xr, return_U=True), m64.solve(x0, ub, stuck, xr, return_U=True)
    assert np.array_equal(a["U"], b["U"]) and np.array_equal(a["status"], b["status"])      # the form is float64 whatever the dtype
    assert (b["status"] == 0).sum() >= 4
    # closed loop: the first step is the solve above (constant reference window, as _near_terminal_set's xref)
    traj = np.concatenate([xref, np.repeat(xref[:, -1:], T - 1, axis=1)], axis=1)
    for m in (m32, m64):
        sim = m.simulate(x0, ub, stuck, traj, T, noise=(0.0, 0.0, 0.0, 0.0), return_inputs=True)
        assert np.isfinite(sim["x"]).all() and np.isfinite(sim["u"]).all()
        assert np.abs(sim["u"][0] - b["u0"]).max() <= 1e-12
        sq = m.solve_sqp_device(x0, ub, stuck, xr, sqp_iters=2)
        assert np.isfinite(sq["cost"]).all() and np.isfinite(sq["cost0"]).all() and np.isfinite(sq["U"]).all()
        assert (sq["cost"] <= sq["cost0"]).all()


@pytest.mark.parametrize("N", [17, 41])
def test_dense_beyond_its_limit_is_still_refused(gpu_mpc_factory, term, N):
    t, At, bt = term
    x0, ub, stuck, xref = qo.make_batch(2, N, NT, 2, 5)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, terminal_set=t, kernel_select="dense")
    with pytest.raises(FtmpcError) as e:
        mpc.solve(x0, ub, stuck, xref.reshape(-1, order="F"))
    assert "N <= 40" in str(e.value) and "256" in str(e.value)


def test_debug_build_qp_on_a_handle_beyond_the_dense_limit(gpu_mpc_factory, term):
    """The dump (H, g, box) of a terminal-set handle at N = 17 comes from the dense kernel's box mode, whose slots such a handle
    allocates on first use: it is the dump of a handle without the set, and the solve afterwards still runs on kernel 12."""
    t, At, bt = term
    N, B = 17, 4
    x0, ub, stuck, xref = _near_terminal_set(B, N, NT, 2, 9931, At, bt, 1.5)
    xr = xref.reshape(-1, order="F")
    with_set = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60, terminal_set=t)
    before = with_set.solve(x0, ub, stuck, xr, return_U=True)
    a = with_set.debug_build_qp(x0, ub, stuck, xr, 1)
    b = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60).debug_build_qp(x0, ub, stuck, xr, 1)
    assert a[0].shape[0] == a[1].size > 0
    for p, q in zip(a, b):
        assert np.array_equal(p, q)
    after = with_set.solve(x0, ub, stuck, xr, return_U=True)
    assert np.array_equal(before["U"], after["U"]) and np.array_equal(before["status"], after["status"])
