"""Sensor bias estimation on the host: NumPy restatements of what BatchedMPC.simulate(bias_estimate=...) runs on the device
(include/ftmpc.h, ftmpc_bias_estimate; csrc/ftmpc_sim.hip, ftmpc_filter_bias_kernel; csrc/ftmpc_bias_block.h).

The navigation filter of ft_mpc_amd.estimators augmented by six states per vehicle: b_v^ [3], a constant bias of the velocity
measurement (m/s), and b_w^ [3], a constant bias of the rate measurement (rad/s) -- the channels 3..5 and 9..11 of sensor["bias"].
Position tells the filter what the velocity is and attitude what the rate is, so both are observable from the kinematics alone; a
constant position or attitude bias is not, and stays in the estimate.

The textbook form (the definition; update_natural / propagate_natural): error coordinates (dp, dv, dtheta, dw, db_v, db_w), 18 in
all; y_v = v + b_v + n, y_w = w + b_w + n, so H = [I_12, HB]; Phi = diag(Phi_xx, I_6); Q = diag(proc_sigma_x[g]^2, proc_sigma_b^2).
The form the device runs (update / propagate / propagate_split): the MEASURED coordinates m = (dp, dv + db_v, dtheta, dw + db_w)
with b unchanged, P^m = T18 P T18'.  There H = [I 0], Phi^m = [[Phi_xx, E], [0, I]] with E = (I - Phi_xx) HB and Q^m = T18 Q T18'.
The covariance travels in measured coordinates, in the three pieces of ft_mpc_amd.disturbances (pack / unpack):
  P_mm  the estimator's 78 packed doubles,   P_mb  [12,6] row-major (72),   P_bb  the packed upper triangle (21).
replay runs the loop's augmented filter for one vehicle from the recorded measurements and applied commands.

Not estimated: a position or attitude bias; the bias states together with the disturbance states of ft_mpc_amd.disturbances."""
from __future__ import annotations

import numpy as np

from . import estimators as _est
from .disturbances import NC, ND, NDD, _IU6, pack, unpack  # noqa: F401  (the pieces have the disturbance pieces' layout)
from .estimators import _G, generalized_force, residual, retract
from .sensors import predict as _predict

_GB = np.array((0, 0, 0, 1, 1, 1))                  # bias coordinate -> group: velocity, rate
FIELDS = ("bias_hist", "state")

HB = np.zeros((12, 6))                              # d y / d b: the velocity and the rate channels
HB[3:6, 0:3] = np.eye(3)
HB[9:12, 3:6] = np.eye(3)
T18 = np.eye(18)                                    # (x, b) -> (m, b)
T18[0:12, 12:18] = HB


def to_measured_dense(P):
    """[..., 18, 18] in the textbook coordinates -> the same covariance in measured coordinates, T18 P T18'."""
    return T18 @ np.asarray(P, dtype=np.float64) @ T18.T


def from_measured_dense(Pm):
    """The inverse of to_measured_dense: T18^-1 P^m T18^-T."""
    Ti = np.linalg.inv(T18)
    return Ti @ np.asarray(Pm, dtype=np.float64) @ Ti.T


def to_measured(cov, cross, cov_b):
    """(cov [..., 78], cross [..., 72], cov_b [..., 21]) of the textbook coordinates -> the three pieces in measured coordinates."""
    return pack(to_measured_dense(unpack(cov, cross, cov_b)))


def from_measured(cov, cross, cov_b):
    """The inverse of to_measured."""
    return pack(from_measured_dense(unpack(cov, cross, cov_b)))


def with_bias(x, b):
    """x~ [13]: x with v + b_v and w + b_w (what the sensor reports of x under the bias b [6])."""
    out = np.array(x, dtype=np.float64).reshape(13)
    b = np.asarray(b, dtype=np.float64).reshape(6)
    out[3:6] += b[0:3]
    out[10:13] += b[3:6]
    return out


def prior(est_spec, bias_spec, cov=None):
    """P^m [18,18] of a call that is handed no cross: the bias prior diag(p0_b^2) independent of the state error, whose covariance is
    cov ([78] or [12,12]; None: diag(est_spec p0^2)); formed as the library forms it (the additions on P_mm's diagonal, HB's ones
    times p0_b^2 in P_mb)."""
    p0 = np.asarray(est_spec["p0"], dtype=np.float64).reshape(4)
    pb = np.asarray(bias_spec["p0"], dtype=np.float64).reshape(2)[_GB] ** 2
    Pxx = np.diag(p0[_G] ** 2) if cov is None else (_est.unpack(cov) if np.size(cov) == _est.NP else np.array(cov, dtype=np.float64).reshape(12, 12))
    P = np.zeros((18, 18))
    P[0:12, 0:12] = Pxx + HB @ np.diag(pb) @ HB.T
    P[0:12, 12:18] = HB * pb[None, :]
    P[12:18, 0:12] = P[0:12, 12:18].T
    P[12:18, 12:18] = np.diag(pb)
    return P


def update(x, b, Pm, y, meas_sigma):
    """The device form.  (x^+, b^+, P^m+) from the prior (x [13], b [6], P^m [18,18] in measured coordinates) and the measurement y
    [13]: the estimator's twelve scalar updates on the residual y [-] x~ with H = [I 0], each over all 18 coordinates; then
    x^ <- x^ [+] delta_m with HB delta_b taken off v^ and w^ (delta_x = delta_m - HB delta_b), b^ += delta_b."""
    P = np.array(Pm, dtype=np.float64).reshape(18, 18)
    R = np.asarray(meas_sigma, dtype=np.float64).reshape(4)[_G] ** 2
    b = np.asarray(b, dtype=np.float64).reshape(6)
    r = residual(y, with_bias(x, b))
    d = np.zeros(18)
    for j in range(12):
        sj = P[j, j] + R[j]
        k = P[:, j] / sj
        d = d + k * (r[j] - d[j])
        P = P - sj * np.outer(k, k)
    xn = retract(x, d[0:12])
    xn[3:6] -= d[12:15]
    xn[10:13] -= d[15:18]
    return xn, b + d[12:18], P


def update_natural(x, b, P, y, meas_sigma):
    """The textbook form.  (x^+, b^+, P+) in the coordinates (dp, dv, dtheta, dw, db_v, db_w): the twelve sequential scalar updates in
    channel order, each over all 18 coordinates with row h_j of H = [I_12, HB]; x^ <- x^ [+] delta[0:12], b^ += delta[12:18]."""
    P = np.array(P, dtype=np.float64).reshape(18, 18)
    R = np.asarray(meas_sigma, dtype=np.float64).reshape(4)[_G] ** 2
    b = np.asarray(b, dtype=np.float64).reshape(6)
    H = np.hstack([np.eye(12), HB])
    r = residual(y, with_bias(x, b))
    d = np.zeros(18)
    for j in range(12):
        h = H[j]
        Ph = P @ h
        sj = h @ Ph + R[j]
        k = Ph / sj
        d = d + k * (r[j] - h @ d)
        P = P - sj * np.outer(k, k)
    return retract(x, d[0:12]), b + d[12:18], P


def e_block(Phi_xx):
    """E [12,6] = (I - Phi_xx) HB: (p, b_v) = -dt I, (theta, b_w) = -dt I, (w, b_w) = I - W; nothing in the v rows."""
    return (np.eye(12) - np.asarray(Phi_xx, dtype=np.float64)) @ HB


def propagate_split(Pmm, Pmb, Pbb, Phi_xx, Qx, Qb):
    """The three pieces after P^m <- Phi^m P^m Phi^m' + Q^m, formed as the device forms them: Y = Phi_xx P_mb, Z = E P_bb;
    P_mm' = (Phi_xx P_mm Phi_xx' + Qx) + (Y E' + E Y' + Z E' + HB diag(Qb) HB'),  P_mb' = Y + Z + HB diag(Qb),  P_bb' = P_bb + Qb.
    Qx [12], Qb [6]: the diagonals of the textbook Q."""
    E = e_block(Phi_xx)
    Y = Phi_xx @ Pmb
    Z = E @ Pbb
    Qb = np.asarray(Qb, dtype=np.float64).reshape(6)
    return ((Phi_xx @ Pmm @ Phi_xx.T + np.diag(Qx)) + (Y @ E.T + E @ Y.T + Z @ E.T + HB @ np.diag(Qb) @ HB.T), Y + Z + HB * Qb[None, :],
            Pbb + np.diag(Qb))


def _q(proc_sigma_x, proc_sigma_b):
    return (np.asarray(proc_sigma_x, dtype=np.float64).reshape(4)[_G] ** 2, np.asarray(proc_sigma_b, dtype=np.float64).reshape(2)[_GB] ** 2)


def propagate(x, b, Pm, u, ub, stuck, proc_sigma_x, proc_sigma_b, cfg):
    """The device form.  (x^-, P^m-) of the next step from the posterior (x [13], b [6], P^m [18,18]) under the command u [NT] and the
    controller's pattern: the mean takes the estimator's RK4 step (the bias does not enter the dynamics), b stays."""
    P = np.asarray(Pm, dtype=np.float64).reshape(18, 18)
    Phi = np.eye(12) + float(cfg.dt) * _est.jacobian(x, generalized_force(u, ub, stuck, cfg), cfg)
    Qx, Qb = _q(proc_sigma_x, proc_sigma_b)
    Pmm, Pmb, Pbb = propagate_split(P[0:12, 0:12], P[0:12, 12:18], P[12:18, 12:18], Phi, Qx, Qb)
    return _predict(x, np.asarray(u, dtype=np.float64).reshape(1, -1), ub, stuck, cfg), np.block([[Pmm, Pmb], [Pmb.T, Pbb]])


def propagate_natural(x, b, P, u, ub, stuck, proc_sigma_x, proc_sigma_b, cfg):
    """The textbook form.  Phi = diag(Phi_xx, I_6), P <- Phi P Phi' + diag(Qx, Qb); the mean as in propagate."""
    P = np.asarray(P, dtype=np.float64).reshape(18, 18)
    Phi = np.eye(18)
    Phi[0:12, 0:12] += float(cfg.dt) * _est.jacobian(x, generalized_force(u, ub, stuck, cfg), cfg)
    Qx, Qb = _q(proc_sigma_x, proc_sigma_b)
    return (_predict(x, np.asarray(u, dtype=np.float64).reshape(1, -1), ub, stuck, cfg),
            Phi @ P @ Phi.T + np.diag(np.concatenate([Qx, Qb])))


def replay(meas, u_applied, ub, stuck, est_spec, bias_spec, cfg, xhat=None, cov=None, bias=None, cross=None, cov_b=None, step0=0,
           latency=0, tail=None):
    """The loop's augmented filter for ONE vehicle, in the device form.  meas [T,13]: the y_t; u_applied [T,NT]: the a_t (u_hist); ub,
    stuck [NT] or [T,NT]: the controller's pattern of each step; est_spec: dict(every, p0, proc_sigma, meas_sigma) of the estimator;
    bias_spec: dict(p0 (2,), proc_sigma (2,)); xhat / cov / bias / cross / cov_b: the priors handed to the call (with cross: cov is
    P_mm as it stands; without: see prior); latency d > 0 with tail [d,NT] also gives pred [T,13].
    Returns dict(est [T,13], bias [T,6] (the b^_{t|t}), pred [T,13] | None, and the priors of step T in measured coordinates: xhat
    [13], cov [78], bias_end [6], cross [72], cov_b [21])."""
    meas = np.asarray(meas, dtype=np.float64).reshape(-1, 13)
    T = meas.shape[0]
    u = np.asarray(u_applied, dtype=np.float64).reshape(T, -1)
    NT = u.shape[1]
    ub = np.broadcast_to(np.asarray(ub, dtype=np.float64), (T, NT))
    stuck = np.broadcast_to(np.asarray(stuck, dtype=np.float64), (T, NT))
    every = int(est_spec.get("every", 1))
    p0 = np.asarray(est_spec["p0"], dtype=np.float64).reshape(4)
    p0b = np.asarray(bias_spec["p0"], dtype=np.float64).reshape(2)
    d = int(latency)
    queue = None
    if d > 0 and tail is not None:
        queue = np.concatenate([u, np.asarray(tail, dtype=np.float64).reshape(d, NT)])
    if cross is None:
        P = prior(est_spec, bias_spec, cov)
    else:
        P = unpack(_est.pack(np.diag(p0[_G] ** 2)) if cov is None else (cov if np.size(cov) == _est.NP else _est.pack(np.reshape(cov, (12, 12)))),
                   cross, np.diag(p0b[_GB] ** 2)[_IU6] if cov_b is None else cov_b)
    x = None if xhat is None else np.array(xhat, dtype=np.float64).reshape(13)
    b = np.zeros(6) if bias is None else np.array(bias, dtype=np.float64).reshape(6)
    est, bh = np.empty((T, 13)), np.empty((T, 6))
    pred = np.empty((T, 13)) if queue is not None else None
    for k in range(T):
        if x is None:
            x = meas[k].copy()
            x[3:6] -= b[0:3]
            x[10:13] -= b[3:6]
        elif (int(step0) + k) % every == 0:
            x, b, P = update(x, b, P, meas[k], est_spec["meas_sigma"])
        est[k], bh[k] = x, b
        if pred is not None:
            pred[k] = _predict(x, queue[k:k + d], ub[k], stuck[k], cfg)
        x, P = propagate(x, b, P, u[k], ub[k], stuck[k], est_spec["proc_sigma"], bias_spec["proc_sigma"], cfg)
    c78, c72, c21 = pack(P)
    return dict(est=est, bias=bh, pred=pred, xhat=x, cov=c78, bias_end=b, cross=c72, cov_b=c21)


def request(bias_estimate, B, T, estimator=None, disturbance=None):
    """The checks BatchedMPC.simulate makes on a bias_estimate dict before the call reaches the library (the library's own refusals,
    raised from Python too); returns the dict with defaults filled in: p0 (2,), proc_sigma (2,), bias [B,6] | None, cross [B,72] |
    None, cov [B,21] | None, fields."""
    spec = dict(bias_estimate)
    out = dict(p0=spec.pop("p0", None), proc_sigma=spec.pop("proc_sigma", None), bias=spec.pop("bias", None), cross=spec.pop("cross", None),
               cov=spec.pop("cov", None), fields=tuple(spec.pop("fields", FIELDS)))
    if spec:
        raise ValueError(f"bias_estimate: unknown keys {sorted(spec)}")
    if estimator is None:
        raise ValueError("bias_estimate needs an estimator: the bias states augment its filter")
    if disturbance is not None:
        raise ValueError("bias_estimate together with disturbance: 24 filter states are not served")
    for name in ("p0", "proc_sigma"):
        if out[name] is None:
            raise ValueError(f"bias_estimate['{name}'] is required: 2 values (velocity bias m/s, rate bias rad/s)")
        out[name] = np.asarray(out[name], dtype=np.float64)
        if out[name].shape != (2,) or not (np.isfinite(out[name]).all() and (out[name] >= 0).all()):
            raise ValueError(f"bias_estimate['{name}'] must be 2 finite values >= 0")
    if any(n not in FIELDS for n in out["fields"]):
        raise ValueError(f"bias_estimate['fields'] must be among {list(FIELDS)}")
    if out["cross"] is not None:
        if out["bias"] is None:
            raise ValueError("bias_estimate['cross'] requires bias_estimate['bias']")
        if estimator.get("xhat") is None:
            raise ValueError("bias_estimate['cross'] requires estimator['xhat']")
    if out["cov"] is not None and out["cross"] is None:
        raise ValueError("bias_estimate['cov'] requires bias_estimate['cross']")
    for name, shape in (("bias", (B, 6)), ("cross", (B, NC)), ("cov", (B, NDD))):
        if out[name] is not None:
            a = np.asarray(out[name], dtype=np.float64)
            if name == "cross" and a.shape == (B, 12, ND):
                a = a.reshape(B, NC)
            if name == "cov" and a.shape == (B, ND, ND):
                a = a[:, _IU6[0], _IU6[1]]
            out[name] = np.array(a, dtype=np.float64)           # a copy: the call writes into it
            if out[name].shape != shape or not np.isfinite(out[name]).all():
                raise ValueError(f"bias_estimate['{name}'] must be finite with shape {shape}")
    if out["cov"] is not None and (out["cov"][:, np.cumsum([0, 6, 5, 4, 3, 2])] < 0).any():
        raise ValueError("bias_estimate['cov'] has a negative diagonal entry")
    return out
