"""Navigation errors and command latency on the host: NumPy restatements of what BatchedMPC.simulate(sensor=...) forms on the device
(include/ftmpc.h, ftmpc_sensor; csrc/ftmpc_sim.hip, ftmpc_sense_kernel).

The plant keeps the truth x_t.  Before the solve of loop step t the controller is handed a measurement y_t of it:
    y_p = p + bias[0:3] + sigma[0] z_{0:3}          y_v = v + bias[3:6] + sigma[1] z_{3:6}
    theta = bias[6:9] + sigma[2] z_{6:9}            y_q = cos(|theta|/2) q + s Omega(theta) q, renormalised
    y_w = w + bias[9:12] + sigma[3] z_{9:12}
with z standard normal draws from counters (gauss), a constant bias per vehicle (sample_bias) and theta a body-frame rotation vector.
The command solved at step t acts at step t + d; with predict the controller first propagates y_t over the d commands still waiting,
by its own model (predict), and solves from there for the window d columns later.

The controller is told neither the plant's dispersion nor the actuator; the prediction uses the controller's fault pattern."""
from __future__ import annotations

import numpy as np

from .dispersion import STRIDE, plant_step, u01

# sample_bias needs 12 draws per vehicle and dispersion.py leaves two components free (14 and 15), so it takes component 14 as the
# root of a second-level counter, (vehicle * STRIDE + 14) * 13 + channel, under a seed of its own derived from the caller's: a bias
# then shares no draw with dispersion.sample or missions.phase_offsets even when one seed serves all three
C_BIAS = 14
CHANNELS = 12
GROUPS = (0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3)      # channel -> sigma / scale group: position, velocity, attitude, rate


def gauss(seed, idx):
    """Standard normal from the counters 2 idx and 2 idx + 1 of the library's uniform generator (Box-Muller):
    sqrt(-2 log(1 - u1)) cos(2 pi u2)."""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        u1 = u01(seed, np.uint64(2) * idx)
        u2 = u01(seed, np.uint64(2) * idx + np.uint64(1))
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)


def _omega(w):
    wx, wy, wz = w
    return np.array([[0.0, wz, -wy, wx], [-wz, 0.0, wx, wy], [wy, -wx, 0.0, wz], [-wx, -wy, -wz, 0.0]])


def rotate(q, theta):
    """q [4] turned by the body-frame rotation vector theta [3]: the closed form q(1) of q' = 1/2 Omega(theta) q, renormalised."""
    q = np.asarray(q, dtype=np.float64).reshape(4)
    theta = np.asarray(theta, dtype=np.float64).reshape(3)
    n = float(np.sqrt(theta @ theta))
    s = 0.5 if n < 1e-8 else np.sin(0.5 * n) / n
    y = np.cos(0.5 * n) * q + s * (_omega(theta) @ q)
    return y / np.sqrt(y @ y)


def measure(x, t, sigma=(0.0, 0.0, 0.0, 0.0), bias=None, seed=0, step0=0, index0=0, index_total=None):
    """y [B,13] of the truths x [B,13] at loop step t: vehicle b is number index0 + b of a campaign of index_total (default B), its
    channel j draws from the counter ((step0 + t) index_total + index0 + b) 12 + j.  bias [B,12] or None; a sigma of zero draws
    nothing for its group."""
    x = np.array(x, dtype=np.float64).reshape(-1, 13)
    B = x.shape[0]
    total = B if index_total is None else int(index_total)
    sigma = np.asarray(sigma, dtype=np.float64).reshape(4)
    e = np.zeros((B, CHANNELS)) if bias is None else np.array(bias, dtype=np.float64).reshape(B, CHANNELS)
    g = np.uint64(int(index0)) + np.arange(B, dtype=np.uint64)
    with np.errstate(over="ignore"):
        c = ((np.uint64(int(step0) + int(t)) * np.uint64(total) + g)[:, None] * np.uint64(CHANNELS)
             + np.arange(CHANNELS, dtype=np.uint64)[None, :])
    z = gauss(seed, c)
    for j in range(CHANNELS):
        if sigma[GROUPS[j]] > 0:
            e[:, j] += sigma[GROUPS[j]] * z[:, j]
    y = x.copy()
    y[:, 0:3] += e[:, 0:3]
    y[:, 3:6] += e[:, 3:6]
    y[:, 10:13] += e[:, 9:12]
    for b in range(B):
        y[b, 6:10] = rotate(x[b, 6:10], e[b, 6:9])
    return y


def predict(y, cmds, ub, stuck, cfg=None):
    """x^ [13] from the measurement y [13] of ONE vehicle: one RK4 step of cfg.dt of the controller's model (cfg's mass, J and D)
    per row of cmds [d,NT], the commands that act before the one being solved for, under the controller's pattern ub / stuck; the
    quaternion is renormalised after each step.  cfg: an MPCConfig or BatchedMPC.cfg (default MPCConfig with NT = len(ub))."""
    if cfg is None:
        from .batch import MPCConfig
        cfg = MPCConfig(NT=int(np.size(ub)))
    x = np.array(y, dtype=np.float64).reshape(13)
    for u in np.asarray(cmds, dtype=np.float64).reshape(-1, int(np.size(ub))):
        x = plant_step(x, u, ub, stuck, {}, cfg)
        x[6:10] /= np.linalg.norm(x[6:10])
    return x


def sample_bias(B, scales, seed, index0=0):
    """bias [B,12] for BatchedMPC.simulate(sensor=dict(bias=...)), uniform in [-scales[k], scales[k]) per group k (position m,
    velocity m/s, attitude rad, rate rad/s) for the vehicles [index0, index0 + B) of a campaign, keyed by (seed, index0 + b,
    channel) alone: sample_bias(96, ..)[40:96] is sample_bias(56, .., index0=40) bit for bit.  A scale of zero gives zero exactly."""
    scales = np.asarray(scales, dtype=np.float64).reshape(4)
    v = np.uint64(int(index0)) + np.arange(B, dtype=np.uint64)
    with np.errstate(over="ignore"):
        # second-level counter: component C_BIAS of the vehicle picks a stream, the channel a draw in it
        idx = (v[:, None] * np.uint64(STRIDE) + np.uint64(C_BIAS)) * np.uint64(CHANNELS + 1) + np.arange(CHANNELS, dtype=np.uint64)[None, :]
    u = 2.0 * u01((int(seed) ^ 0x5E5E5E5E5E5E5E5E) & ((1 << 64) - 1), idx) - 1.0
    return scales[list(GROUPS)][None, :] * u


def request(sensor, B, T, NT):
    """The checks BatchedMPC.simulate makes on a sensor dict before the call reaches the library; returns the dict with defaults
    filled in: sigma (4,), bias [B,12] | None, seed, step0, latency, predict, pending [B,latency,NT] | None, fields."""
    spec = dict(sensor)
    out = dict(sigma=np.asarray(spec.pop("sigma", (0.0,) * 4), dtype=np.float64), bias=spec.pop("bias", None), seed=int(spec.pop("seed", 0)),
               step0=int(spec.pop("step0", 0)), latency=int(spec.pop("latency", 0)), predict=spec.pop("predict", False),
               pending=spec.pop("pending", None), fields=tuple(spec.pop("fields", ())))
    if spec:
        raise ValueError(f"sensor: unknown keys {sorted(spec)}")
    if out["sigma"].shape != (4,) or not (np.isfinite(out["sigma"]).all() and (out["sigma"] >= 0).all()):
        raise ValueError("sensor['sigma'] must be 4 finite values >= 0 (position, velocity, attitude, rate)")
    if not 0 <= out["latency"] <= 8:
        raise ValueError(f"sensor['latency'] must be in [0, 8], not {out['latency']}")
    if out["predict"] not in (False, True, 0, 1):
        raise ValueError("sensor['predict'] must be False or True")
    out["predict"] = bool(out["predict"])
    if out["step0"] < 0:
        raise ValueError("sensor['step0'] must be >= 0")
    if any(f not in ("meas", "pred", "pending") for f in out["fields"]):
        raise ValueError("sensor['fields'] must be among ['meas', 'pred', 'pending']")
    if "pred" in out["fields"] and not out["predict"]:
        raise ValueError("sensor: the field pred belongs to predict=True")
    if out["latency"] == 0 and (out["pending"] is not None or "pending" in out["fields"]):
        raise ValueError("sensor: pending belongs to latency > 0")
    if out["bias"] is not None:
        out["bias"] = np.ascontiguousarray(out["bias"], dtype=np.float64)
        if out["bias"].shape != (B, CHANNELS) or not np.isfinite(out["bias"]).all():
            raise ValueError(f"sensor['bias'] must be finite with shape {(B, CHANNELS)}")
    if out["pending"] is not None:
        out["pending"] = np.array(out["pending"], dtype=np.float64)      # a copy: the call writes into it
        if out["pending"].shape != (B, out["latency"], NT) or not np.isfinite(out["pending"]).all():
            raise ValueError(f"sensor['pending'] must be finite with shape {(B, out['latency'], NT)}")
    return out
