"""Measurement dropouts, outliers and the gated filter on the host: NumPy restatements of what BatchedMPC.simulate(outage=...) runs on
the device between the sensor and the solve (include/ftmpc.h, ftmpc_outage; csrc/ftmpc_sim.hip, ftmpc_outage_kernel,
ftmpc_filter_gated_kernel, ftmpc_diagnose_gated_kernel).

Per vehicle the availability of the measurement is a two-state Markov chain over the campaign steps c = step0 + t,
    lost_c = u_0 < p_loss      when available at c - 1,        lost_c = not (u_0 < p_recover)      when lost at c - 1,
overridden inside a scripted window [from, to); its stationary loss fraction is p_loss / (p_loss + p_recover) and an outage lasts
1 / p_recover steps in the mean (chain_params / chain_stats convert).  An available measurement carries an outlier in group k
(position, velocity, attitude, rate) with probability p_outlier[k]: three Gaussian errors of outlier_sigma[k] on the group's channels,
applied as the sensor applies its own.  The draws come from the library's counter function: vehicle g of a campaign of index_total
draws u_s = u01(seed, 32 (c index_total + g) + s); s = 0 the chain, 1 + k the outlier of group k, 8 + 2 j and 9 + 2 j the Box-Muller
pair of channel j.

The filter's update runs on the steps c % every == 0 where the vehicle is available; inside it a channel whose innovation e has
e^2 > gate^2 (P_jj + R_j) is left out (gated_update, replay).  The diagnosis skips a lost step altogether
(diagnosis.replay(avail=...)); outliers reach it ungated."""
from __future__ import annotations

import numpy as np

from .dispersion import u01
from .estimators import NP, _G, pack, predict, propagate, residual, retract, unpack
from .sensors import rotate

DRAWS = 32                                          # counters per (step, vehicle)
FIELDS = ("avail", "outlier", "gate", "meas", "state", "rejected", "outliers")


def chain_params(loss_fraction, mean_length):
    """(p_loss, p_recover) of the chain whose stationary loss fraction and mean outage length (steps, >= 1) are the given ones."""
    f, m = float(loss_fraction), float(mean_length)
    if not (0.0 <= f < 1.0) or not m >= 1.0:
        raise ValueError("loss_fraction must be in [0, 1) and mean_length >= 1")
    p_recover = 1.0 / m
    p_loss = f * p_recover / (1.0 - f)
    if not p_loss < 1.0:
        raise ValueError(f"no chain has a loss fraction of {f} with outages of {m} steps (p_loss would be {p_loss})")
    return p_loss, p_recover


def chain_stats(p_loss, p_recover):
    """(stationary loss fraction, mean outage length in steps) of the chain: p_loss / (p_loss + p_recover), 1 / p_recover."""
    p_loss, p_recover = float(p_loss), float(p_recover)
    return p_loss / (p_loss + p_recover), 1.0 / p_recover


def _four(v):
    return np.broadcast_to(np.asarray(v, dtype=np.float64), (4,)).copy()


def draw(y, t, run, p_loss=0.0, p_recover=1.0, p_outlier=0.0, outlier_sigma=0.0, seed=0, window=None, step0=0, index0=0,
         index_total=None, init=False):
    """One step of the chain, the window and the outliers for a batch.  y [B,13]: the y_t the sense kernel formed; run [B] int: the
    length of each vehicle's current outage before this step (0: available); window [B,2] int or None; init: the first step of a
    call without estimator['xhat'] (available, nothing drawn).  Vehicle b is number index0 + b of a campaign of index_total
    (default B).  Returns dict(y [B,13] after the step, avail [B] int32 (1 / 0), run [B] int32, outlier [B] int32 (bit k: group k))."""
    y = np.array(y, dtype=np.float64).reshape(-1, 13)
    B = y.shape[0]
    run_prev = np.asarray(run, dtype=np.int64).reshape(B)
    bits = np.zeros(B, np.int32)
    if init:
        return dict(y=y, avail=np.ones(B, np.int32), run=np.zeros(B, np.int32), outlier=bits)
    total = B if index_total is None else int(index_total)
    c = int(step0) + int(t)
    p_out, sig = _four(p_outlier), _four(outlier_sigma)
    with np.errstate(over="ignore"):
        k0 = (np.uint64(c) * np.uint64(total) + np.uint64(int(index0)) + np.arange(B, dtype=np.uint64)) * np.uint64(DRAWS)
        u0 = u01(seed, k0)
        lost = np.where(run_prev > 0, ~(u0 < float(p_recover)), u0 < float(p_loss))
        if window is not None:
            w = np.asarray(window, dtype=np.int64).reshape(B, 2)
            lost = lost | ((w[:, 0] <= c) & (c < w[:, 1]))
        for g in range(4):
            if p_out[g] > 0:
                hit = ~lost & (u01(seed, k0 + np.uint64(1 + g)) < p_out[g])
                bits[hit] |= 1 << g
        for b in np.nonzero(bits)[0]:
            e = np.zeros(12)
            for j in range(12):
                if bits[b] >> (j // 3) & 1:
                    u1, u2 = u01(seed, k0[b] + np.uint64(8 + 2 * j)), u01(seed, k0[b] + np.uint64(9 + 2 * j))
                    e[j] = sig[j // 3] * np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)
            if bits[b] & 1:
                y[b, 0:3] += e[0:3]
            if bits[b] & 2:
                y[b, 3:6] += e[3:6]
            if bits[b] & 4:
                y[b, 6:10] = rotate(y[b, 6:10], e[6:9])
            if bits[b] & 8:
                y[b, 10:13] += e[9:12]
    run_new = np.where(lost, run_prev + 1, 0).astype(np.int32)
    return dict(y=y, avail=(~lost).astype(np.int32), run=run_new, outlier=bits)


def gated_update(x, P, y, meas_sigma, avail=True, gate=0.0):
    """estimators.update with availability and the innovation gate: (x^+, P+, mask) from the prior (x [13], P [12,12]) and y [13].
    Not available: the prior comes back, mask 0.  Channel j with e = r_j - d_j, s_j = P_jj + R_j and gate > 0, e^2 > gate^2 s_j is
    rejected: d and P stay, bit j of mask is set.  With gate = 0 and avail it is estimators.update bit for bit."""
    P = np.array(P, dtype=np.float64).reshape(12, 12)
    if not avail:
        return np.array(x, dtype=np.float64).reshape(13), P, 0
    R = np.asarray(meas_sigma, dtype=np.float64).reshape(4)[_G] ** 2
    gsq = float(gate) * float(gate)
    r = residual(y, x)
    d = np.zeros(12)
    mask = 0
    for j in range(12):
        sj = P[j, j] + R[j]
        e = r[j] - d[j]
        if gsq > 0 and e * e > gsq * sj:
            mask |= 1 << j
            continue
        k = P[:, j] / sj
        d = d + k * e
        P = P - sj * np.outer(k, k)
    return retract(x, d), P, mask


def replay(meas, avail, u_applied, ub, stuck, spec, cfg, gate=0.0, xhat=None, cov=None, step0=0, latency=0, tail=None):
    """estimators.replay driven by the availability and the gate, for ONE vehicle.  meas [T,13]: the y_t of the outage's meas_hist;
    avail [T] (None: always available); the rest as estimators.replay.  Returns its dict plus gate [T] int32 (bit j: channel j was
    rejected at step t) and rejected [4] (channel-steps per group)."""
    meas = np.asarray(meas, dtype=np.float64).reshape(-1, 13)
    T = meas.shape[0]
    avail = np.ones(T, bool) if avail is None else np.asarray(avail).reshape(T).astype(bool)
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
    masks, rejected = np.zeros(T, np.int32), np.zeros(4, np.int64)
    for t in range(T):
        if x is None:
            x = meas[t].copy()
        elif (int(step0) + t) % every == 0:
            x, P, masks[t] = gated_update(x, P, meas[t], spec["meas_sigma"], avail[t], gate)
            for g in range(4):
                rejected[g] += bin(int(masks[t]) >> (3 * g) & 7).count("1")
        est[t] = x
        if pred is not None:
            pred[t] = predict(x, queue[t:t + d], ub[t], stuck[t], cfg)
        x, P = propagate(x, P, u[t], ub[t], stuck[t], spec["proc_sigma"], cfg)
    return dict(est=est, pred=pred, xhat=x, cov=pack(P), gate=masks, rejected=rejected)


def request(outage, B, T, estimator=None, disturbance=None, bias_estimate=None):
    """The checks BatchedMPC.simulate makes on an outage dict before the call reaches the library (the library's own refusals, raised
    here as ValueError); returns the dict with defaults filled in: seed, p_loss, p_recover, p_outlier (4,), outlier_sigma (4,), gate,
    window [B,2] int32 | None, state [B,3] | None, rejected [B,4] | None, outliers [B,4] | None (copies: the call writes into them),
    fields."""
    spec = dict(outage)
    out = dict(seed=int(spec.pop("seed", 0)), p_loss=spec.pop("p_loss", 0.0), p_recover=spec.pop("p_recover", 1.0),
               p_outlier=spec.pop("p_outlier", 0.0), outlier_sigma=spec.pop("outlier_sigma", 0.0), gate=spec.pop("gate", 0.0),
               window=spec.pop("window", None), state=spec.pop("state", None), rejected=spec.pop("rejected", None),
               outliers=spec.pop("outliers", None), fields=tuple(spec.pop("fields", ())))
    if spec:
        raise ValueError(f"outage: unknown keys {sorted(spec)}")
    if estimator is None:
        raise ValueError("outage needs an estimator: the availability and the gate act on its filter")
    if disturbance is not None:
        raise ValueError("outage together with disturbance: the disturbance filter has no gated form")
    if bias_estimate is not None:
        raise ValueError("outage together with bias_estimate: the bias filter has no gated form")
    out["p_loss"], out["p_recover"], out["gate"] = float(out["p_loss"]), float(out["p_recover"]), float(out["gate"])
    if not 0.0 <= out["p_loss"] < 1.0:
        raise ValueError(f"outage['p_loss'] must be in [0, 1), not {out['p_loss']}")
    if not 0.0 < out["p_recover"] <= 1.0:
        raise ValueError(f"outage['p_recover'] must be in (0, 1], not {out['p_recover']}")
    for name in ("p_outlier", "outlier_sigma"):
        try:
            out[name] = _four(out[name])
        except ValueError:
            raise ValueError(f"outage['{name}'] must be one value or 4 (position, velocity, attitude, rate)") from None
    if not ((out["p_outlier"] >= 0) & (out["p_outlier"] <= 1)).all():
        raise ValueError("outage['p_outlier'] must be in [0, 1]")
    if not (np.isfinite(out["outlier_sigma"]).all() and (out["outlier_sigma"] >= 0).all()):
        raise ValueError("outage['outlier_sigma'] must be finite and >= 0")
    if not (np.isfinite(out["gate"]) and out["gate"] >= 0):
        raise ValueError("outage['gate'] must be finite and >= 0 (0: no gate)")
    if any(f not in FIELDS for f in out["fields"]):
        raise ValueError(f"outage['fields'] must be among {list(FIELDS)}")
    if out["window"] is not None:
        out["window"] = np.ascontiguousarray(out["window"], dtype=np.int32)
        if out["window"].shape != (B, 2):
            raise ValueError(f"outage['window'] must have shape {(B, 2)}: [from, to) in campaign steps")
    for name, width in (("state", 3), ("rejected", 4), ("outliers", 4)):
        if out[name] is not None:
            out[name] = np.array(out[name], dtype=np.int32)
            if out[name].shape != (B, width) or (out[name] < 0).any():
                raise ValueError(f"outage['{name}'] must have shape {(B, width)} and no negative entry")
    return out
