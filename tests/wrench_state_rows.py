"""Checker of the STATE BOUNDS on the generalized-force formulation (helper of test_wrench_state_bounds_host.py and
test_gpu_wrench_state_bounds.py; not a test module).

The reference's wrench program carries the optional rows  xlb <= c_j <= xub  on the orbit-centre state of the stages j = 1 .. N-1
(spiraling_mpc.py:129-130,179-185).  Here they are written out DENSE through the sensitivities of the linearised prediction,
G_{k+1} = A_k G_k, G_{k+1}[:, 6k:6k+6] = Bg_k (c_j ~ cbar_j + G_j d), and appended to the hull rows of
oracle/qp_oracle.py:build_qp_wrench in the order of build_qp_box_state: stage, component, upper then lower.  ipm_general treats
them as it treats every row beyond `nhull` (slack max(residual, 0.1), carried primal residual) and finishes with its active-set
polish: the exact solution, certified by kkt_general."""
import numpy as np

from oracle import qp_oracle as qo

# (N, NT, faults, B, seed) of the batches the tests use, and what the oracle finds on them with bounds():
# instances solved (status 0), instances with an active state row
BATCHES = [(15, 16, 2, 16, 5115), (20, 16, 2, 16, 5120), (20, 8, 1, 12, 5128), (33, 16, 2, 6, 5133)]
COUNTS = {(15, 16, 2, 16, 5115): (15, 7), (20, 16, 2, 16, 5120): (14, 5), (20, 8, 1, 12, 5128): (11, 6), (33, 16, 2, 6, 5133): (5, 1)}


def bounds(v=0.9, w=1.6):
    """|v| <= v, |omega| <= w on the centre state [p, v, omega, q]; every other component free."""
    xub, xlb = np.full(13, np.inf), np.full(13, -np.inf)
    xub[3:6], xlb[3:6] = v, -v
    xub[6:9], xlb[6:9] = w, -w
    return xlb, xub


def state_rows(cfg, x0, stuck, xlb=None, xub=None, warmG=None):
    """(C_x [m, 6N], h_x [m], srow) of the finite state rows: +G_j[i] d <= xub[i] - cbar_j[i], -G_j[i] d <= cbar_j[i] - xlb[i]."""
    N = cfg.N
    xub = np.full(13, np.inf) if xub is None else np.asarray(xub, float).reshape(13)
    xlb = np.full(13, -np.inf) if xlb is None else np.asarray(xlb, float).reshape(13)
    cbar, A, Bg, _ = qo.linearize_wrench(cfg, x0, stuck, warmG)
    G = np.zeros((13, 6 * N))
    rows, hs, srow = [], [], []
    for k in range(N):
        G = A[k] @ G
        G[:, 6 * k:6 * k + 6] = Bg[k]      # now G = d c_{k+1} / d T
        if k + 1 < N:
            for i in range(13):
                if np.isfinite(xub[i]):
                    rows.append(G[i].copy()); hs.append(xub[i] - cbar[k + 1][i]); srow.append((k + 1, i, 1))
                if np.isfinite(xlb[i]):
                    rows.append(-G[i]); hs.append(cbar[k + 1][i] - xlb[i]); srow.append((k + 1, i, -1))
    Cx = np.array(rows).reshape(len(rows), 6 * N)
    return Cx, np.array(hs, float), srow


def build_qp_wrench_state(cfg, x0, ub, stuck, xref, xlb=None, xub=None, uref=None, warmG=None, hull=None):
    """build_qp_wrench plus the state rows after the hull rows (`nhull` stays the number of hull rows)."""
    qp = qo.build_qp_wrench(cfg, x0, ub, stuck, xref, uref, warmG, hull)
    Cx, hx, srow = state_rows(cfg, x0, stuck, xlb, xub, warmG)
    qp.update(C=np.vstack([qp["C"], Cx]), h=np.concatenate([qp["h"], hx]), srow=srow)
    return qp


def solve_wrench_state_instance(cfg, x0, ub, stuck, xref, xlb=None, xub=None, uref=None, warmG=None, hull=None, iters=60, mu_stop=1e-10,
                                polish=True):
    """Returns (tau0 (6,), T (N,6), status, iterations, qp dict with d, z, s)."""
    qp = build_qp_wrench_state(cfg, x0, ub, stuck, xref, xlb, xub, uref, warmG, hull)
    d, s, z, nit, st = qo.ipm_general(qp["H"], qp["g"], qp["C"], qp["h"], qp["d0"], qp["nhull"], iters=iters, mu_stop=mu_stop, polish=polish)
    T = qp["Tbar"] + (d.reshape(cfg.N, 6) if st != 2 else 0.0)
    qp.update(d=d, z=z, s=s)
    return T[0].copy(), T, st, nit, qp


def active_state_rows(qp):
    """Number of state rows with a positive multiplier at the (polished) solution."""
    return int((qp["z"][qp["nhull"]:] > 0).sum())
