"""Per-vehicle outcomes of a fault campaign on the host: the reductions of ftmpc_outcome_kernel (include/ftmpc.h, ftmpc_outcomes;
BatchedMPC.simulate(outcomes=...)) in NumPy for callers who already hold the histories, and the figures a campaign report prints.

Per loop step t, with x_{t+1} = x_hist[t], e = robot_to_center(x_{t+1})[0:9] - xref_traj[:, t+1] (spiral_model.py:91-109) and
ep, ev, ew the Euclidean norms of e[0:3], e[3:6], e[6:9]; the definitions are those of the header."""
import numpy as np


def plant_patterns(ub, stuck, faults, T, detect_delay=0):
    """The PLANT's pattern at every step under a fault schedule (the last event with onset <= t, else the initial pattern):
    (ub [T,B,NT], stuck [T,B,NT]).  faults as BatchedMPC.simulate takes it, or None."""
    ub, stuck = np.asarray(ub, float), np.asarray(stuck, float)
    B, NT = ub.shape
    pu, ps = np.broadcast_to(ub, (T, B, NT)).copy(), np.broadcast_to(stuck, (T, B, NT)).copy()
    if faults is not None:
        from .faults import normalize_schedule
        onset, _, eub, est = normalize_schedule(faults, B, NT, T, detect_delay)
        for e in range(onset.shape[1]):      # slots are sorted by onset: a later slot overrides
            on = onset[:, e]
            for b in np.flatnonzero(on >= 0):
                pu[on[b]:, b], ps[on[b]:, b] = eub[b, e], est[b, e]
    return pu, ps


def _rot(x):
    """World -> body rotation matrices [..., 3, 3] of the states x [..., 13] (util/utils.py:4-19)."""
    qx, qy, qz, qw = (x[..., 6 + i] for i in range(4))
    R = np.empty(x.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = qx * qx - qy * qy - qz * qz + qw * qw, 2 * (qx * qy + qz * qw), 2 * (qx * qz - qy * qw)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2 * (qx * qy - qz * qw), -qx * qx + qy * qy - qz * qz + qw * qw, 2 * (qy * qz + qx * qw)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2 * (qx * qz + qy * qw), 2 * (qy * qz - qx * qw), -qx * qx - qy * qy + qz * qz + qw * qw
    return R


def centre_state(x_hist, r):
    """robot_to_center(x_hist[t])[0:9], [T,B,9]: the orbit-centre [p, v, omega] of every state."""
    x = np.asarray(x_hist, float)
    R = _rot(x)                              # robot_to_center applies the transpose
    r = np.asarray(r, float).reshape(3)
    w = x[..., 10:13]
    pos = x[..., 0:3] + np.einsum("tbji,j->tbi", R, r)
    vel = x[..., 3:6] + np.einsum("tbji,tbj->tbi", R, np.cross(w, r))
    return np.concatenate([pos, vel, w], axis=-1)


def centre_error(x_hist, xref_traj, r):
    """e [T,B,9] = robot_to_center(x_hist[t])[0:9] - xref_traj[:, t+1]."""
    T = np.shape(x_hist)[0]
    return centre_state(x_hist, r) - np.asarray(xref_traj, float)[:, 1:T + 1].T[:, None, :]


def closed_loop_cost(Q, R, P, D, f_virt, r, x0, x_hist, u_hist, plant_ub, plant_stuck, xref, uref=None, v_nq=None):
    """The device's `cost` outcome [B,3] from histories (include/ftmpc.h, ftmpc_mission.cost), summed in step order:
      cost[:, 0] = sum_t e_{t+1}' diag(Q) e_{t+1}
      cost[:, 1] = sum_t w_t' diag(R) w_t,   w_t = D a_t - [Rot(q_t)^T uref_t[0:3]; uref_t[3:6]] - [f_virt; 0]
      cost[:, 2] = e_T' P e_T (+ v_nq(e_T))
    Q [9], R [6], P [9,9], D [6,NT], f_virt [3], r [3]: the handle's (BatchedMPC.cfg.Q / .R / .f_virt, BatchedMPC.P / .D / .r).
    x0 [B,13] the states the loop started from, x_hist [T,B,13], u_hist [T,B,NT] (commanded), plant_ub / plant_stuck [B,NT] or
    [T,B,NT] (plant_patterns).  xref: what x_hist[t] is measured against -- [T,B,9] per vehicle (missions.error_columns), or a shared
    trajectory 9 x (>= T+1), whose column t + 1 it is; uref: [T,B,6] per vehicle (the column of step t), a shared 6 x (>= T), or None
    (zero).  v_nq: the non-quadratic terminal-cost terms as a function of e [B,9] -> [B], or None."""
    x_hist = np.asarray(x_hist, float)
    T, B = x_hist.shape[:2]
    u = np.asarray(u_hist, float)
    pu = np.broadcast_to(np.asarray(plant_ub, float), u.shape)
    ps = np.broadcast_to(np.asarray(plant_stuck, float), u.shape)
    Q, R, P = np.asarray(Q, float).reshape(9), np.asarray(R, float).reshape(6), np.asarray(P, float).reshape(9, 9)
    D = np.asarray(D, float).reshape(6, -1)
    fv = np.concatenate([np.asarray(f_virt, float).reshape(3), np.zeros(3)])
    xref = np.asarray(xref, float)
    if xref.ndim == 2:
        xref = np.broadcast_to(xref[:, 1:T + 1].T[:, None, :], (T, B, 9))
    if uref is not None:
        uref = np.asarray(uref, float)
        if uref.ndim == 2:
            uref = np.broadcast_to(uref[:, :T].T[:, None, :], (T, B, 6))
    e = centre_state(x_hist, r) - xref
    start = np.concatenate([np.asarray(x0, float).reshape(1, B, 13), x_hist[:-1]], axis=0) if T else x_hist      # the state step t started from
    Rq = _rot(start)
    a = np.where(pu > 0.0, u, 0.0) + ps
    cost = np.zeros((B, 3))
    for t in range(T):
        cost[:, 0] += (Q * e[t] * e[t]).sum(axis=-1)
        w = a[t] @ D.T - fv
        if uref is not None:
            w[:, 0:3] -= np.einsum("bji,bj->bi", Rq[t], uref[t, :, 0:3])
            w[:, 3:6] -= uref[t, :, 3:6]
        cost[:, 1] += (R * w * w).sum(axis=-1)
    if T:
        cost[:, 2] = np.einsum("bi,ij,bj->b", e[-1], P, e[-1])
        if v_nq is not None:
            cost[:, 2] += v_nq(e[-1])
    return cost


def outcomes_from_history(cfg, x_hist, u_hist, status_hist, xref_traj, plant_ub, plant_stuck, tol=None, term=None,
                          alloc_status_hist=None):
    """The device's outcome records from histories: x_hist [T,B,13], u_hist [T,B,NT] (commanded), status_hist [T,B], xref_traj
    9 x (>= T+1), plant_ub / plant_stuck [B,NT] or [T,B,NT] (plant_patterns).  tol: (tol_pos, tol_vel, tol_rate) for settle_step;
    term: (A [rows,9], b [rows]) for tset_step; alloc_status_hist [T,B] for alloc_failed.  cfg: an MPCConfig (dt, mass, f_virt, r).
    Returns a dict of arrays named and shaped as BatchedMPC.simulate(outcomes=...) returns them."""
    x_hist = np.asarray(x_hist, float)
    T, B = x_hist.shape[:2]
    u = np.asarray(u_hist, float)
    pu = np.broadcast_to(np.asarray(plant_ub, float), u.shape)
    ps = np.broadcast_to(np.asarray(plant_stuck, float), u.shape)
    r = cfg.r
    if r is None:       # spiral_parameters.py:39
        r = np.linalg.norm(cfg.f_virt) / (cfg.mass * 0.6 ** 2) * np.array([0.0, 1.0, 0.0])
    e = centre_error(x_hist, xref_traj, r)
    n2 = np.stack([(e[..., 3 * j:3 * j + 3] ** 2).sum(axis=-1) for j in range(3)], axis=-1)      # [T,B,3]
    nrm = np.sqrt(n2)
    out = dict(err_int=np.zeros((B, 3)), err_max=nrm.max(axis=0) if T else np.zeros((B, 3)), impulse=np.zeros((B, 2)))
    cmd = np.where(pu > 0.0, u, 0.0)
    for t in range(T):      # in step order, as the device adds them
        out["err_int"] += cfg.dt * n2[t]
        out["impulse"][:, 0] += cfg.dt * (cmd[t] + ps[t]).sum(axis=-1)
        out["impulse"][:, 1] += cfg.dt * cmd[t].sum(axis=-1)
    steps = np.arange(T)[:, None]
    if tol is not None:
        outside = ~(nrm <= np.asarray(tol, float).reshape(3)).all(axis=-1)
        out["settle_step"] = np.where(outside, steps + 1, 0).max(axis=0, initial=0).astype(np.int32)
    if term is not None:
        A, b = np.asarray(term[0], float).reshape(-1, 9), np.asarray(term[1], float).reshape(-1)
        inside = (np.einsum("rj,tbj->tbr", A, e) <= b).all(axis=-1)
        out["tset_step"] = np.where(inside.any(axis=0), inside.argmax(axis=0), -1).astype(np.int32)
    bad = np.asarray(status_hist) != 0
    out["unsolved"] = bad.sum(axis=0).astype(np.int32)
    out["first_unsolved"] = np.where(bad.any(axis=0), bad.argmax(axis=0), -1).astype(np.int32)
    if alloc_status_hist is not None:
        out["alloc_failed"] = (np.asarray(alloc_status_hist) != 0).sum(axis=0).astype(np.int32)
    return out


def summarize(outcomes, T=None, quantiles=(0.5, 0.9, 0.99)):
    """What a campaign report prints: the number of vehicles, the fraction that recovered (settle_step < T when T and settle_step are
    given), the fraction with an unsolved step, the fraction that entered the terminal set, and the quantiles of settle_step (over the
    recovered), tset_step (over those that entered), err_max, err_int and impulse."""
    q = list(quantiles)
    B = len(outcomes["unsolved"]) if "unsolved" in outcomes else len(next(iter(outcomes.values())))
    rep = dict(vehicles=int(B), quantiles=q)

    def quant(a):
        a = np.asarray(a, float)
        return np.quantile(a, q, axis=0).tolist() if a.shape[0] else None
    if "settle_step" in outcomes and T is not None:
        ok = np.asarray(outcomes["settle_step"]) < T
        rep["recovered_fraction"] = float(ok.mean()) if B else 0.0
        rep["settle_step"] = quant(np.asarray(outcomes["settle_step"])[ok])
    if "tset_step" in outcomes:
        inn = np.asarray(outcomes["tset_step"]) >= 0
        rep["tset_fraction"] = float(inn.mean()) if B else 0.0
        rep["tset_step"] = quant(np.asarray(outcomes["tset_step"])[inn])
    if "unsolved" in outcomes:
        rep["unsolved_fraction"] = float((np.asarray(outcomes["unsolved"]) > 0).mean()) if B else 0.0
    if "alloc_failed" in outcomes:
        rep["alloc_failed_fraction"] = float((np.asarray(outcomes["alloc_failed"]) > 0).mean()) if B else 0.0
    for k in ("err_max", "err_int", "impulse"):
        if k in outcomes:
            rep[k] = quant(outcomes[k])
    return rep
