"""Disturbance estimation on the host: NumPy restatements of what BatchedMPC.simulate(disturbance=...) runs on the device
(include/ftmpc.h, ftmpc_disturbance; csrc/ftmpc_sim.hip, ftmpc_filter_dist_kernel and ftmpc_diagnose_dist_kernel; csrc/ftmpc_linearize.hip,
the DIST instantiations).

The navigation filter of ft_mpc_amd.estimators augmented by six states per vehicle: f^ [3], a constant force in the inertial frame (N),
and t^ [3], a constant torque in the body frame (N m) -- the frames and units of plant["force"] / plant["torque"].  The error
coordinates are (dp, dv, dtheta, dw, df, dt), 18 in all; the covariance travels in three pieces (pack / unpack):
  P_xx  the estimator's 78 packed doubles,   P_xd  [12,6] row-major (72),   P_dd  the packed upper triangle (21).
  model_step   one RK4 step of the model with the estimate, v' = (Rot(q)^T F + f^) / m, w' = J^-1 (tau + t^ - w x J w), renormalised
  centre_step  the same for the orbit-centre state c = [p, v, w, q] the linearise kernel rolls out (no renormalisation)
  update       H = [I 0], R = diag(meas_sigma[g]^2): the estimator's twelve sequential scalar updates over all 18 coordinates
  propagate    Phi = [[Phi_xx, Phi_xd], [0, I]], Phi_xd = dt [0; I / m; 0; J^-1] in the blocks (v, f) and (w, t);
               P <- Phi P Phi' + diag(proc_sigma_x^2, proc_sigma_d^2); the mean takes model_step, f^ and t^ stay
  rollout_centre  centre_step stage by stage under per-stage commanded wrenches: what the wrench cost kernel rolls out under the
               estimate (the two-stage wrench form, disturbance["wrench"] = True, with one QP or the wrench SQP per step)
replay runs the loop's augmented filter for one vehicle from the recorded measurements and applied commands.

Not estimated: m, J, D (a gain or centre-of-mass error shows up as a command-dependent part of (f^, t^)).  An undetected stuck thruster
is a constant body wrench: a slow t^ absorbs its torque signature over time, so proc_sigma of the disturbance has to be small against
the diagnosis' detection time."""
from __future__ import annotations

import numpy as np

from . import estimators as _est
from .estimators import _G, _cfg_model, generalized_force, residual, retract
from .sensors import _omega

ND = 6                                              # disturbance states
NC, NDD = 72, 21                                    # entries of P_xd, packed entries of P_dd
_IU6 = np.triu_indices(ND)
_GD = np.array((0, 0, 0, 1, 1, 1))                  # disturbance coordinate -> group: force, torque
FIELDS = ("force_hist", "torque_hist", "state")


def _rot(q):
    """Rot(q): inertial -> body, so that v' = Rot(q)^T F / m (the matrix of plant_f, transposed)."""
    return _est._body_to_inertial(q).T


def _rk4(rhs, x, dt):
    k1 = rhs(x)
    k2 = rhs(x + 0.5 * dt * k1)
    k3 = rhs(x + 0.5 * dt * k2)
    k4 = rhs(x + dt * k3)
    return x + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)


def model_step(x, gen, f, t, cfg):
    """x [13] after one RK4 step of cfg.dt of the model with the estimate under the generalised force gen [6] (body frame), the
    force f [3] (inertial) and the torque t [3] (body) held over the step; the quaternion renormalised."""
    _, m, J = _cfg_model(cfg)
    gen = np.asarray(gen, dtype=np.float64).reshape(6)
    f = np.asarray(f, dtype=np.float64).reshape(3)
    t = np.asarray(t, dtype=np.float64).reshape(3)

    def rhs(x):
        v, q, w = x[3:6], x[6:10], x[10:13]
        return np.concatenate([v, (_rot(q).T @ gen[0:3] + f) / m, 0.5 * _omega(w) @ q, np.linalg.solve(J, gen[3:6] + t - np.cross(w, J @ w))])
    x = _rk4(rhs, np.array(x, dtype=np.float64).reshape(13), float(cfg.dt))
    x[6:10] /= np.linalg.norm(x[6:10])
    return x


def centre_r(cfg):
    """The orbit-centre offset r [3] of the config (cfg.r, or the library's default)."""
    if getattr(cfg, "r", None) is not None:
        return np.asarray(cfg.r, dtype=np.float64).reshape(3)
    import ctypes as C

    from . import _lib
    c = _lib.ftmpc_config()
    _lib.load_library().ftmpc_default_config(C.byref(c), int(cfg.N), int(cfg.NT))
    return np.array(list(c.r))


def to_centre(x, cfg, r=None):
    """c = [p + Rot(q)^T r, v + Rot(q)^T (w x r), w, q] [13] of the vehicle state x [13]: what the linearise kernel starts from."""
    r = centre_r(cfg) if r is None else np.asarray(r, dtype=np.float64).reshape(3)
    x = np.asarray(x, dtype=np.float64).reshape(13)
    RT = _rot(x[6:10]).T
    return np.concatenate([x[0:3] + RT @ r, x[3:6] + RT @ np.cross(x[10:13], r), x[10:13], x[6:10]])


def centre_step(c, gen, f, t, cfg, r=None):
    """c [13] = [p, v, w, q] of the orbit centre after one RK4 step of cfg.dt (no renormalisation) under gen [6] with the estimate:
    w' = J^-1 (tau + t - w x J w),  v' = Rot(q)^T (F / m + w' x r + w x (w x r)) + f / m."""
    _, m, J = _cfg_model(cfg)
    r = centre_r(cfg) if r is None else np.asarray(r, dtype=np.float64).reshape(3)
    gen = np.asarray(gen, dtype=np.float64).reshape(6)
    f = np.asarray(f, dtype=np.float64).reshape(3)
    t = np.asarray(t, dtype=np.float64).reshape(3)

    def rhs(s):
        v, w, q = s[3:6], s[6:9], s[9:13]
        dw = np.linalg.solve(J, gen[3:6] + t - np.cross(w, J @ w))
        ab = gen[0:3] / m + np.cross(dw, r) + np.cross(w, np.cross(w, r))
        return np.concatenate([v, _rot(q).T @ ab + f / m, dw, 0.5 * _omega(w) @ q])
    return _rk4(rhs, np.array(c, dtype=np.float64).reshape(13), float(cfg.dt))


def rollout_centre(c0, G, f, t, cfg, r=None):
    """[N+1, 13] centre states c_0 .. c_N under the per-stage COMMANDED wrenches G [N,6] with the estimate (f [3] inertial, t [3]
    body) held over the horizon: centre_step applied stage by stage from c0 [13] -- the rollout of the linearise kernel's DIST
    instantiations about warmG = G and of the wrench cost kernel under the estimate (its out_X)."""
    G = np.asarray(G, dtype=np.float64).reshape(-1, 6)
    r = centre_r(cfg) if r is None else r
    X = np.empty((G.shape[0] + 1, 13))
    X[0] = np.asarray(c0, dtype=np.float64).reshape(13)
    for k in range(G.shape[0]):
        X[k + 1] = centre_step(X[k], G[k], f, t, cfg, r)
    return X


def retract18(x, f, t, d):
    """(x [+] d[0:12], f + d[12:15], t + d[15:18])."""
    d = np.asarray(d, dtype=np.float64).reshape(18)
    return retract(x, d[0:12]), np.asarray(f, dtype=np.float64) + d[12:15], np.asarray(t, dtype=np.float64) + d[15:18]


def jacobian(x, gen, cfg):
    """A [18,18] of the error dynamics about x [13] under gen [6]: the estimator's A in the x block, (v, f) = I / m and
    (w, t) = J^-1 in the cross block, zero rows for the disturbance (it is constant).  It does not depend on (f^, t^): the force is
    inertial and the torque enters w' additively."""
    _, m, J = _cfg_model(cfg)
    A = np.zeros((18, 18))
    A[0:12, 0:12] = _est.jacobian(x, gen, cfg)
    A[3:6, 12:15] = np.eye(3) / m
    A[9:12, 15:18] = np.linalg.inv(J)
    return A


def update(x, f, t, P, y, meas_sigma):
    """(x^+, f^+, t^+, P+) from the prior (x [13], f [3], t [3], P [18,18]) and the measurement y [13]: twelve scalar updates in
    channel order, each over all 18 coordinates."""
    P = np.array(P, dtype=np.float64).reshape(18, 18)
    R = np.asarray(meas_sigma, dtype=np.float64).reshape(4)[_G] ** 2
    r = residual(y, x)
    d = np.zeros(18)
    for j in range(12):
        sj = P[j, j] + R[j]
        k = P[:, j] / sj
        d = d + k * (r[j] - d[j])
        P = P - sj * np.outer(k, k)
    return (*retract18(x, f, t, d), P)


def propagate_split(Pxx, Pxd, Pdd, Phi_xx, Phi_xd, Qx, Qd):
    """The three pieces after P <- Phi P Phi' + diag(Qx, Qd) with Phi = [[Phi_xx, Phi_xd], [0, I]], formed as the device forms them:
    Y = Phi_xx P_xd, Z = Phi_xd P_dd;  P_xx' = (Phi_xx P_xx Phi_xx' + Qx) + (Y Phi_xd' + Phi_xd Y' + Z Phi_xd'),  P_xd' = Y + Z,
    P_dd' = P_dd + Qd."""
    Y = Phi_xx @ Pxd
    Z = Phi_xd @ Pdd
    return (Phi_xx @ Pxx @ Phi_xx.T + np.diag(Qx)) + (Y @ Phi_xd.T + Phi_xd @ Y.T + Z @ Phi_xd.T), Y + Z, Pdd + np.diag(Qd)


def propagate(x, f, t, P, u, ub, stuck, proc_sigma_x, proc_sigma_d, cfg):
    """(x^-, P-) of the next step from the posterior (x [13], f, t [3], P [18,18]) under the command u [NT] and the controller's
    pattern; f and t do not change."""
    P = np.asarray(P, dtype=np.float64).reshape(18, 18)
    gen = generalized_force(u, ub, stuck, cfg)
    Phi = np.eye(18) + float(cfg.dt) * jacobian(x, gen, cfg)
    Qx = np.asarray(proc_sigma_x, dtype=np.float64).reshape(4)[_G] ** 2
    Qd = np.asarray(proc_sigma_d, dtype=np.float64).reshape(2)[_GD] ** 2
    Pxx, Pxd, Pdd = propagate_split(P[0:12, 0:12], P[0:12, 12:18], P[12:18, 12:18], Phi[0:12, 0:12], Phi[0:12, 12:18], Qx, Qd)
    return model_step(x, gen, f, t, cfg), np.block([[Pxx, Pxd], [Pxd.T, Pdd]])


def pack(P):
    """[..., 18, 18] -> (cov [..., 78], cross [..., 72], cov_d [..., 21])."""
    P = np.asarray(P, dtype=np.float64)
    return (_est.pack(P[..., 0:12, 0:12]), np.ascontiguousarray(P[..., 0:12, 12:18]).reshape(P.shape[:-2] + (NC,)),
            np.ascontiguousarray(P[..., 12:18, 12:18][..., _IU6[0], _IU6[1]]))


def unpack(cov, cross, cov_d):
    """(cov [..., 78], cross [..., 72], cov_d [..., 21]) -> [..., 18, 18], symmetric."""
    Pxx = _est.unpack(cov)
    Pxd = np.asarray(cross, dtype=np.float64).reshape(Pxx.shape[:-2] + (12, ND))
    pd = np.asarray(cov_d, dtype=np.float64)
    Pdd = np.zeros(pd.shape[:-1] + (ND, ND))
    Pdd[..., _IU6[0], _IU6[1]] = pd
    Pdd[..., _IU6[1], _IU6[0]] = pd
    P = np.zeros(Pxx.shape[:-2] + (18, 18))
    P[..., 0:12, 0:12], P[..., 0:12, 12:18], P[..., 12:18, 12:18] = Pxx, Pxd, Pdd
    P[..., 12:18, 0:12] = np.swapaxes(Pxd, -1, -2)
    return P


def predict(x, f, t, cmds, ub, stuck, cfg):
    """x^ [13] propagated over the rows of cmds [d,NT] with the model with the estimate (the filter's prediction over the queue)."""
    x = np.array(x, dtype=np.float64).reshape(13)
    for u in np.asarray(cmds, dtype=np.float64).reshape(-1, int(np.size(ub))):
        x = model_step(x, generalized_force(u, ub, stuck, cfg), f, t, cfg)
    return x


def replay(meas, u_applied, ub, stuck, est_spec, dist_spec, cfg, xhat=None, cov=None, force=None, torque=None, cross=None, cov_d=None,
           step0=0, latency=0, tail=None):
    """The loop's augmented filter for ONE vehicle.  meas [T,13]: the y_t; u_applied [T,NT]: the a_t (u_hist); ub, stuck [NT] or
    [T,NT]: the controller's pattern of each step; est_spec: dict(every, p0, proc_sigma, meas_sigma) of the estimator; dist_spec:
    dict(p0 (2,), proc_sigma (2,)); xhat / cov / force / torque / cross / cov_d: the priors handed to the call; latency d > 0 with
    tail [d,NT] also gives pred [T,13].
    Returns dict(est [T,13], force [T,3], torque [T,3] (the f^_{t|t}, t^_{t|t}), pred [T,13] | None, and the priors of step T: xhat
    [13], cov [78], force_end [3], torque_end [3], cross [72], cov_d [21])."""
    meas = np.asarray(meas, dtype=np.float64).reshape(-1, 13)
    T = meas.shape[0]
    u = np.asarray(u_applied, dtype=np.float64).reshape(T, -1)
    NT = u.shape[1]
    ub = np.broadcast_to(np.asarray(ub, dtype=np.float64), (T, NT))
    stuck = np.broadcast_to(np.asarray(stuck, dtype=np.float64), (T, NT))
    every = int(est_spec.get("every", 1))
    p0 = np.asarray(est_spec["p0"], dtype=np.float64).reshape(4)
    p0d = np.asarray(dist_spec["p0"], dtype=np.float64).reshape(2)
    d = int(latency)
    queue = None
    if d > 0 and tail is not None:
        queue = np.concatenate([u, np.asarray(tail, dtype=np.float64).reshape(d, NT)])
    P = unpack(_est.pack(np.diag(p0[_G] ** 2)) if cov is None else (cov if np.size(cov) == _est.NP else _est.pack(np.reshape(cov, (12, 12)))),
               np.zeros(NC) if cross is None else cross,
               np.diag(p0d[_GD] ** 2)[_IU6] if cov_d is None else cov_d)
    x = None if xhat is None else np.array(xhat, dtype=np.float64).reshape(13)
    f = np.zeros(3) if force is None else np.array(force, dtype=np.float64).reshape(3)
    t = np.zeros(3) if torque is None else np.array(torque, dtype=np.float64).reshape(3)
    est, fh, th = np.empty((T, 13)), np.empty((T, 3)), np.empty((T, 3))
    pred = np.empty((T, 13)) if queue is not None else None
    for k in range(T):
        if x is None:
            x = meas[k].copy()
        elif (int(step0) + k) % every == 0:
            x, f, t, P = update(x, f, t, P, meas[k], est_spec["meas_sigma"])
        est[k], fh[k], th[k] = x, f, t
        if pred is not None:
            pred[k] = predict(x, f, t, queue[k:k + d], ub[k], stuck[k], cfg)
        x, P = propagate(x, f, t, P, u[k], ub[k], stuck[k], est_spec["proc_sigma"], dist_spec["proc_sigma"], cfg)
    c78, c72, c21 = pack(P)
    return dict(est=est, force=fh, torque=th, pred=pred, xhat=x, cov=c78, force_end=f, torque_end=t, cross=c72, cov_d=c21)


def request(disturbance, B, T, estimator=None, sqp_iters=0, formulation="thruster"):
    """The checks BatchedMPC.simulate makes on a disturbance dict before the call reaches the library (the library's own refusals,
    raised from Python too); returns the dict with defaults filled in: p0 (2,), proc_sigma (2,), compensate (bool), force / torque
    [B,3] | None, cross [B,72] | None, cov [B,21] | None, fields, wrench (bool).
    The opt-in key wrench=True asks for the two-stage wrench form (ftmpc_simulate_wrench_disturbance_batch): formulation must then be
    "wrench" and sqp_iters >= 0 is accepted (the wrench SQP's cost kernel knows the estimate).  Without the key the call is the
    thruster form's with one QP per step, and the wrench formulation and sqp_iters > 0 are refused as before."""
    spec = dict(disturbance)
    out = dict(p0=spec.pop("p0", None), proc_sigma=spec.pop("proc_sigma", None), compensate=spec.pop("compensate", True),
               force=spec.pop("force", None), torque=spec.pop("torque", None), cross=spec.pop("cross", None), cov=spec.pop("cov", None),
               fields=tuple(spec.pop("fields", FIELDS)))
    wrench = spec.pop("wrench", False)
    if spec:
        raise ValueError(f"disturbance: unknown keys {sorted(spec)}")
    if wrench not in (0, 1, True, False):
        raise ValueError(f"disturbance['wrench'] must be 0 / 1 (False / True), not {wrench}")
    out["wrench"] = bool(wrench)
    if out["wrench"]:
        if formulation != "wrench":
            raise ValueError("disturbance['wrench'] = True asks for the two-stage wrench form: formulation must be 'wrench'")
    elif formulation != "thruster":
        raise ValueError("disturbance: thruster formulation only (the two-stage wrench form has no disturbance entry)")
    if estimator is None:
        raise ValueError("disturbance needs an estimator: the disturbance states augment its filter")
    if int(sqp_iters) > 0 and not out["wrench"]:
        raise ValueError("disturbance: sqp_iters must be 0 (the cost kernels of the SQP do not know the estimate)")
    if int(sqp_iters) < 0:
        raise ValueError("disturbance: sqp_iters must be >= 0")
    if out["compensate"] not in (0, 1, True, False):
        raise ValueError(f"disturbance['compensate'] must be 0 / 1 (False / True), not {out['compensate']}")
    out["compensate"] = bool(out["compensate"])
    for name in ("p0", "proc_sigma"):
        if out[name] is None:
            raise ValueError(f"disturbance['{name}'] is required: 2 values (force N, torque N m)")
        out[name] = np.asarray(out[name], dtype=np.float64)
        if out[name].shape != (2,) or not (np.isfinite(out[name]).all() and (out[name] >= 0).all()):
            raise ValueError(f"disturbance['{name}'] must be 2 finite values >= 0")
    if any(n not in FIELDS for n in out["fields"]):
        raise ValueError(f"disturbance['fields'] must be among {list(FIELDS)}")
    if out["cross"] is not None:
        if out["force"] is None or out["torque"] is None:
            raise ValueError("disturbance['cross'] requires disturbance['force'] and disturbance['torque']")
        if estimator.get("xhat") is None:
            raise ValueError("disturbance['cross'] requires estimator['xhat']")
    if out["cov"] is not None and out["cross"] is None:
        raise ValueError("disturbance['cov'] requires disturbance['cross']")
    for name, shape in (("force", (B, 3)), ("torque", (B, 3)), ("cross", (B, NC)), ("cov", (B, NDD))):
        if out[name] is not None:
            a = np.asarray(out[name], dtype=np.float64)
            if name == "cross" and a.shape == (B, 12, ND):
                a = a.reshape(B, NC)
            if name == "cov" and a.shape == (B, ND, ND):
                a = a[:, _IU6[0], _IU6[1]]
            out[name] = np.array(a, dtype=np.float64)           # a copy: the call writes into it
            if out[name].shape != shape or not np.isfinite(out[name]).all():
                raise ValueError(f"disturbance['{name}'] must be finite with shape {shape}")
    if out["cov"] is not None and (out["cov"][:, np.cumsum([0, 6, 5, 4, 3, 2])] < 0).any():
        raise ValueError("disturbance['cov'] has a negative diagonal entry")
    return out
