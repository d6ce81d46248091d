"""The navigation filter on the host: NumPy restatements of what BatchedMPC.simulate(estimator=...) runs on the device between the
sensor and the solve (include/ftmpc.h, ftmpc_estimator; csrc/ftmpc_sim.hip, ftmpc_filter_kernel).

A multiplicative (error-state) extended Kalman filter per vehicle.  The mean x^ [13] has the layout of x; the covariance P [12,12] is
over the error coordinates delta = (dp, dv, dtheta, dw) of the retraction
    x [+] delta = (p + dp, v + dv, rotate(q, dtheta), w + dw)            (sensors.rotate: body-frame rotation vector)
and travels packed: 78 doubles, upper triangle, row-major (pack / unpack).
  residual  y [-] x^: differences, and for the attitude the theta with rotate(q^, theta) = y_q
  update    H = I, R = diag(meas_sigma[g]^2): twelve sequential scalar updates in channel order on d = 0, then x^ <- x^ [+] d
  propagate Phi = I + dt A(x^, gen), P <- Phi P Phi' + diag(proc_sigma[g]^2), x^ <- one RK4 step of the controller's model, renormalised
replay runs the loop's filter for one vehicle from the recorded measurements and applied commands; steady_state iterates the covariance
recursion at a fixed linearisation point.

The filter is told neither the plant's dispersion nor the actuator: its model is the controller's (cfg's mass, J, D) under the
controller's fault pattern."""
from __future__ import annotations

import numpy as np

from .sensors import GROUPS, predict, rotate

NP = 78                                             # packed entries of P
_IU = np.triu_indices(12)
_G = np.array(GROUPS)


def _cfg_model(cfg):
    D = cfg.D
    if D is None:
        from .models.sys_model import allocation_matrix_16, allocation_matrix_8
        D = allocation_matrix_16() if cfg.NT == 16 else allocation_matrix_8()
    return np.asarray(D, dtype=np.float64).reshape(6, -1), float(cfg.mass), np.asarray(cfg.J, dtype=np.float64).reshape(3, 3)


def generalized_force(u, ub, stuck, cfg):
    """gen [6] = D ((ub > 0 ? u : 0) + stuck) of the config's D: what the filter's model is driven by."""
    D = _cfg_model(cfg)[0]
    a = np.where(np.asarray(ub) > 0, np.asarray(u, dtype=np.float64).reshape(-1), 0.0) + np.asarray(stuck, dtype=np.float64).reshape(-1)
    return D @ a


def _skew(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def _xi(q):
    """Xi(q) [4,3] with Omega(theta) q = Xi(q) theta."""
    x, y, z, w = q
    return np.array([[w, -z, y], [z, w, -x], [-y, x, w], [-x, -y, -z]])


def _body_to_inertial(q):
    """M(q): the matrix plant_f applies to F / m."""
    x, y, z, w = q
    return np.array([[x * x - y * y - z * z + w * w, 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), -x * x + y * y - z * z + w * w, 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), -x * x - y * y + z * z + w * w]])


def retract(x, d):
    """x [+] d: x [13], d [12]."""
    x = np.asarray(x, dtype=np.float64).reshape(13)
    d = np.asarray(d, dtype=np.float64).reshape(12)
    out = x.copy()
    out[0:6] += d[0:6]
    out[6:10] = rotate(x[6:10], d[6:9])
    out[10:13] += d[9:12]
    return out


def residual(y, x):
    """y [-] x [12]: the d with x [+] d = y (attitude: |d_theta| <= pi; y_q and -y_q are the same attitude)."""
    y = np.asarray(y, dtype=np.float64).reshape(13)
    x = np.asarray(x, dtype=np.float64).reshape(13)
    r = np.empty(12)
    r[0:6] = y[0:6] - x[0:6]
    r[9:12] = y[10:13] - x[10:13]
    c = float(x[6:10] @ y[6:10])
    s = _xi(x[6:10]).T @ y[6:10]
    if c < 0:
        c, s = -c, -s
    n = float(np.sqrt(s @ s))
    r[6:9] = 2.0 * s if n < 1e-8 else (2.0 * np.arctan2(n, c) / n) * s
    return r


def jacobian(x, gen, cfg):
    """A [12,12] of the error dynamics d' = A d about x [13] under gen [6]: blocks (p,v) = I, (theta,w) = I,
    (v,theta) = -M [F/m]x, (theta,theta) = -[w]x, (w,w) = J^-1 ([J w]x - [w]x J)."""
    _, m, J = _cfg_model(cfg)
    x = np.asarray(x, dtype=np.float64).reshape(13)
    gen = np.asarray(gen, dtype=np.float64).reshape(6)
    w = x[10:13]
    A = np.zeros((12, 12))
    A[0:3, 3:6] = np.eye(3)
    A[3:6, 6:9] = -_body_to_inertial(x[6:10]) @ _skew(gen[0:3] / m)
    A[6:9, 6:9] = -_skew(w)
    A[6:9, 9:12] = np.eye(3)
    A[9:12, 9:12] = np.linalg.solve(J, _skew(J @ w) - _skew(w) @ J)
    return A


def update(x, P, y, meas_sigma):
    """(x^+, P+) from the prior (x [13], P [12,12]) and the measurement y [13]: the twelve scalar updates in channel order."""
    P = np.array(P, dtype=np.float64).reshape(12, 12)
    R = np.asarray(meas_sigma, dtype=np.float64).reshape(4)[_G] ** 2
    r = residual(y, x)
    d = np.zeros(12)
    for j in range(12):
        sj = P[j, j] + R[j]
        k = P[:, j] / sj
        d = d + k * (r[j] - d[j])
        P = P - sj * np.outer(k, k)
    return retract(x, d), P


def propagate(x, P, u, ub, stuck, proc_sigma, cfg):
    """(x^-, P-) of the next step from the posterior (x [13], P [12,12]) under the command u [NT] and the controller's pattern."""
    P = np.asarray(P, dtype=np.float64).reshape(12, 12)
    Phi = np.eye(12) + float(cfg.dt) * jacobian(x, generalized_force(u, ub, stuck, cfg), cfg)
    Pn = Phi @ P @ Phi.T + np.diag(np.asarray(proc_sigma, dtype=np.float64).reshape(4)[_G] ** 2)
    return predict(x, np.asarray(u, dtype=np.float64).reshape(1, -1), ub, stuck, cfg), Pn


def pack(P):
    """[..., 12, 12] -> [..., 78]: the upper triangle, row-major."""
    return np.ascontiguousarray(np.asarray(P, dtype=np.float64)[..., _IU[0], _IU[1]])


def unpack(p):
    """[..., 78] -> [..., 12, 12], symmetric."""
    p = np.asarray(p, dtype=np.float64)
    P = np.zeros(p.shape[:-1] + (12, 12))
    P[..., _IU[0], _IU[1]] = p
    P[..., _IU[1], _IU[0]] = p
    return P


def replay(meas, u_applied, ub, stuck, spec, cfg, xhat=None, cov=None, step0=0, latency=0, tail=None):
    """The loop's filter for ONE vehicle.  meas [T,13]: the y_t; u_applied [T,NT]: the a_t (u_hist); ub, stuck [NT] or [T,NT]: the
    controller's pattern of each step; spec: dict(every, p0, proc_sigma, meas_sigma); xhat [13] / cov [78] or [12,12]: the priors
    handed to the call; latency d > 0 with tail [d,NT] (the commands still waiting at the end: the returned pending) also gives
    pred [T,13], x^_{t|t} propagated over the d commands queued at step t.
    Returns dict(est [T,13], pred [T,13] | None, xhat [13], cov [78]): what the device returns."""
    meas = np.asarray(meas, dtype=np.float64).reshape(-1, 13)
    T = meas.shape[0]
    u = np.asarray(u_applied, dtype=np.float64).reshape(T, -1)
    NT = u.shape[1]
    ub = np.broadcast_to(np.asarray(ub, dtype=np.float64), (T, NT))
    stuck = np.broadcast_to(np.asarray(stuck, dtype=np.float64), (T, NT))
    every = int(spec.get("every", 1))
    p0 = np.asarray(spec["p0"], dtype=np.float64).reshape(4)
    d = int(latency)
    queue = None
    if d > 0 and tail is not None:
        queue = np.concatenate([u, np.asarray(tail, dtype=np.float64).reshape(d, NT)])
    P = np.diag(p0[_G] ** 2) if cov is None else (unpack(cov) if np.size(cov) == NP else np.array(cov, dtype=np.float64).reshape(12, 12))
    x = None if xhat is None else np.array(xhat, dtype=np.float64).reshape(13)
    est = np.empty((T, 13))
    pred = np.empty((T, 13)) if queue is not None else None
    for t in range(T):
        if x is None:
            x = meas[t].copy()
        elif (int(step0) + t) % every == 0:
            x, P = update(x, P, meas[t], spec["meas_sigma"])
        est[t] = x
        if pred is not None:
            pred[t] = predict(x, queue[t:t + d], ub[t], stuck[t], cfg)
        x, P = propagate(x, P, u[t], ub[t], stuck[t], spec["proc_sigma"], cfg)
    return dict(est=est, pred=pred, xhat=x, cov=pack(P))


def steady_state(spec, x, gen, cfg, iters=2000, tol=1e-13):
    """The fixed point of the covariance recursion about x [13] under gen [6]: P_{t|t} [12,12] right after an update, with `every`
    time updates between two updates.  Iterates until the relative change falls below tol (or iters)."""
    every = int(spec.get("every", 1))
    R = np.asarray(spec["meas_sigma"], dtype=np.float64).reshape(4)[_G] ** 2
    Q = np.diag(np.asarray(spec["proc_sigma"], dtype=np.float64).reshape(4)[_G] ** 2)
    Phi = np.eye(12) + float(cfg.dt) * jacobian(x, gen, cfg)
    P = np.diag(R)
    for _ in range(int(iters)):
        Pm = P
        for _ in range(every):
            Pm = Phi @ Pm @ Phi.T + Q
        Pn = Pm - Pm @ np.linalg.solve(Pm + np.diag(R), Pm)
        Pn = 0.5 * (Pn + Pn.T)
        done = np.abs(Pn - P).max() <= tol * np.abs(Pn).max()
        P = Pn
        if done:
            break
    return P


def request(estimator, B, T):
    """The checks BatchedMPC.simulate makes on an estimator dict before the call reaches the library; returns the dict with defaults
    filled in: every, p0, proc_sigma, meas_sigma (4,), xhat [B,13] | None, cov [B,78] | None, fields."""
    spec = dict(estimator)
    out = dict(every=spec.pop("every", 1), p0=spec.pop("p0", None), proc_sigma=spec.pop("proc_sigma", None),
               meas_sigma=spec.pop("meas_sigma", None), xhat=spec.pop("xhat", None), cov=spec.pop("cov", None),
               fields=tuple(spec.pop("fields", ())))
    if spec:
        raise ValueError(f"estimator: unknown keys {sorted(spec)}")
    if int(out["every"]) != out["every"] or int(out["every"]) < 1:
        raise ValueError(f"estimator['every'] must be an integer >= 1, not {out['every']}")
    out["every"] = int(out["every"])
    for name in ("p0", "proc_sigma", "meas_sigma"):
        if out[name] is None:
            raise ValueError(f"estimator['{name}'] is required: 4 values (position, velocity, attitude, rate)")
        out[name] = np.asarray(out[name], dtype=np.float64)
        low_ok = (out[name] > 0) if name == "meas_sigma" else (out[name] >= 0)
        if out[name].shape != (4,) or not (np.isfinite(out[name]).all() and low_ok.all()):
            raise ValueError(f"estimator['{name}'] must be 4 finite values " + ("> 0" if name == "meas_sigma" else ">= 0"))
    if any(f not in ("est", "err_sq", "xhat", "cov") for f in out["fields"]):
        raise ValueError("estimator['fields'] must be among ['est', 'err_sq', 'xhat', 'cov']")
    if out["cov"] is not None and out["xhat"] is None:
        raise ValueError("estimator['cov'] requires estimator['xhat']")
    if out["xhat"] is not None:
        out["xhat"] = np.array(out["xhat"], dtype=np.float64)           # a copy: the call writes into it
        if out["xhat"].shape != (B, 13) or not np.isfinite(out["xhat"]).all():
            raise ValueError(f"estimator['xhat'] must be finite with shape {(B, 13)}")
    if out["cov"] is not None:
        cov = np.asarray(out["cov"], dtype=np.float64)
        if cov.shape == (B, 12, 12):
            cov = pack(cov)
        out["cov"] = np.array(cov, dtype=np.float64)
        if out["cov"].shape != (B, NP) or not np.isfinite(out["cov"]).all():
            raise ValueError(f"estimator['cov'] must be finite with shape {(B, NP)} (packed) or {(B, 12, 12)}")
        if (unpack(out["cov"])[:, np.arange(12), np.arange(12)] < 0).any():
            raise ValueError("estimator['cov'] has a negative diagonal entry")
    return out
