"""CPU checks of the checker of the state bounds on the generalized-force formulation (tests/wrench_state_rows.py): its rows are the
derivative of the oracle's linearised prediction, the batches the GPU test uses contain what it asserts on (solved instances,
active state rows, bounds that cannot be met), and the committed fixture re-solves to the same verdicts."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))

from oracle import qp_oracle as qo
from oracle import refmath as rm
import wrench_state_rows as ws

GOLD = Path(__file__).parent / "golden"
F_MAX = rm.F_MAX


def _predict(cfg, x0, stuck, d):
    """Linearised prediction c_1 .. c_N of the wrench sequence Tbar + d (Tbar = D stuck): cbar_j + dx_j, dx_{k+1} = A_k dx_k + Bg_k d_k."""
    cbar, A, Bg, _ = qo.linearize_wrench(cfg, x0, stuck)
    dx = np.zeros(13)
    out = np.zeros((cfg.N, 13))
    for k in range(cfg.N):
        dx = A[k] @ dx + Bg[k] @ d[6 * k:6 * k + 6]
        out[k] = cbar[k + 1] + dx
    return out


def test_state_rows_are_the_derivative_of_the_linearised_prediction():
    N, NT = 15, 16
    cfg = qo.QPConfig(N=N, NT=NT)
    x0, ub, stuck, _ = qo.make_batch(2, N, NT, 2, 5115)
    xlb, xub = ws.bounds()
    rng = np.random.default_rng(1)
    for b in range(2):
        Cx, hx, srow = ws.state_rows(cfg, x0[b], stuck[b], xlb, xub)
        assert len(srow) == (N - 1) * 12 and Cx.shape == (len(srow), 6 * N)
        assert srow[0] == (1, 3, 1) and srow[1] == (1, 3, -1) and srow[12] == (2, 3, 1)      # stage, component, upper then lower
        base = _predict(cfg, x0[b], stuck[b], np.zeros(6 * N))
        for (j, i, sg), c, hh in zip(srow, Cx, hx):
            assert hh == pytest.approx((xub[i] - base[j - 1][i]) if sg > 0 else (base[j - 1][i] - xlb[i]), abs=1e-12)
            assert np.all(c[6 * j:] == 0)      # stage j depends on the wrenches of the stages before it only
        # central differences of the prediction in random directions (the prediction is affine in d: exact up to rounding)
        for _ in range(3):
            v = rng.standard_normal(6 * N)
            fd = (_predict(cfg, x0[b], stuck[b], 0.5 * v) - _predict(cfg, x0[b], stuck[b], -0.5 * v))
            want = np.array([sg * fd[j - 1][i] for (j, i, sg) in srow])
            assert np.abs(Cx @ v - want).max() <= 1e-10 * (1 + np.abs(want).max())
    # one-sided and absent bounds
    one = np.full(13, np.inf)
    one[3:6] = 1.2
    assert len(ws.state_rows(cfg, x0[0], stuck[0], None, one)[2]) == (N - 1) * 3
    assert ws.state_rows(cfg, x0[0], stuck[0])[0].shape == (0, 6 * N)


@pytest.mark.parametrize("shape", ws.BATCHES)
def test_the_batches_have_solved_active_and_unsolvable_instances(shape):
    N, NT, nf, B, seed = shape
    cfg = qo.QPConfig(N=N, NT=NT)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, nf, seed)
    xlb, xub = ws.bounds()
    solved = active = 0
    with np.errstate(all="ignore"):
        for b in range(B):
            _, T, st, _, qp = ws.solve_wrench_state_instance(cfg, x0[b], ub[b], stuck[b], xref, xlb, xub)
            if st != 0:
                continue
            solved += 1
            assert max(qo.kkt_general(qp["H"], qp["g"], qp["C"], qp["h"], qp["d"], qp["z"])) < 1e-7
            if ws.active_state_rows(qp) > 0:
                active += 1
                _, T0, st0, _, _ = qo.solve_wrench_instance(cfg, x0[b], ub[b], stuck[b], xref)
                assert st0 == 0 and np.abs(T - T0).max() / F_MAX > 1e-5      # the rows matter
    assert (solved, active) == ws.COUNTS[shape]


def test_the_fixture_resolves_to_the_same_verdicts():
    d = np.load(GOLD / "qp_wrench_state_n15.npz")
    N, NT = int(d["N"]), int(d["NT"])
    cfg = qo.QPConfig(N=N, NT=NT)
    B = d["x0"].shape[0]
    assert (N, NT, 2, B, 5115) == ws.BATCHES[0]
    assert int((d["status"] == 0).sum()) == 15 and int((d["active_rows"] > 0).sum()) == 7
    with np.errstate(all="ignore"):
        for b in range(B):
            _, T, st, _, qp = ws.solve_wrench_state_instance(cfg, d["x0"][b], d["ub"][b], d["stuck"][b], d["xref"], d["xlb"], d["xub"])
            assert st == d["status"][b]
            if st == 0:
                assert np.abs(T - d["G"][b]).max() / F_MAX <= 1e-9
                assert ws.active_state_rows(qp) == d["active_rows"][b]
