"""A disturbance that varies over the run, on the host: NumPy restatements of what BatchedMPC.simulate(environment=...) runs on the
device right before every plant step (include/ftmpc.h, ftmpc_environment; csrc/ftmpc_sim.hip, ftmpc_environment_kernel;
csrc/ftmpc_env.h, the per-vehicle step).

The wrench held over plant step c = step0 + t (force in the inertial frame [0:3], torque in the body frame [3:6]) is
    w_c = base + g_c + p_c + k_c
base the call's plant["force"] / ["torque"]; g six independent first-order Gauss-Markov processes, exactly discretised,
    g_{c+1,j} = phi_a g_{c,j} + sigma_a sqrt(1 - phi_a^2) n_{c,j},   phi_a = exp(-dt / tau_a),   a = 0 force, 1 torque,
started from a handed state or from a stationary draw; p_c = amp sin(2 pi c dt / period + phase); k_c a kick while from <= c < to.
The draws come from the library's counter function: vehicle g of a campaign of index_total draws u_s = u01(seed, 32 (c index_total + g)
+ s); the Gaussian of the slot pair (s, s + 1) is sqrt(-2 log(1 - u_s)) cos(2 pi u_{s+1}); s = 2 j the innovation of component j,
s = 16 + 2 j its stationary start.

wrench is one step, replay a whole run from the seed, request the validation of the dict, sample a campaign's amplitudes, phases and
kicks keyed by the vehicle number (a slice of a campaign draws what the whole campaign draws for the same vehicles)."""
from __future__ import annotations

import numpy as np

from .dispersion import u01

DRAWS = 32                                          # counters per (step, vehicle)
TWO_PI = 6.283185307179586
FIELDS = ("wrench", "state", "est_err_sq")
# draws of `sample`, per vehicle v: counter v * STRIDE + component
STRIDE = 32
C_AMP_FORCE, C_AMP_TORQUE, C_PHASE, C_KICK, C_FROM, C_LENGTH = 0, 3, 6, 7, 13, 14


def _two(v):
    return np.broadcast_to(np.asarray(v, dtype=np.float64), (2,)).copy()


def process(sigma, tau, dt):
    """(phi [2], innov [2]) of the exactly discretised processes: exp(-dt / tau), sigma sqrt(1 - phi^2); sigma_a = 0 switches the
    process off (tau_a is not looked at, phi_a = 0), as the library does."""
    sigma, tau = _two(sigma), _two(tau)
    phi = np.zeros(2)
    for a in range(2):
        if sigma[a] > 0:
            phi[a] = np.exp(-float(dt) / tau[a])
    return phi, sigma * np.sqrt(1.0 - phi * phi)


def _counter(B, c, index0, index_total):
    total = B if index_total is None else int(index_total)
    with np.errstate(over="ignore"):
        return np.uint64(int(c)) * np.uint64(total) + np.uint64(int(index0)) + np.arange(B, dtype=np.uint64)


def gauss(seed, k, s):
    """The Gaussian of the slot pair (s, s + 1) of the counters k [B]."""
    with np.errstate(over="ignore"):
        i = np.asarray(k, dtype=np.uint64) * np.uint64(DRAWS) + np.uint64(int(s))
        u1, u2 = u01(seed, i), u01(seed, i + np.uint64(1))
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(TWO_PI * u2)


def stationary(B, sigma, seed=0, c=0, index0=0, index_total=None):
    """g [B,6] of a stationary start at campaign step c: sigma_a times the Gaussian of the slots 16 + 2 j, 17 + 2 j."""
    sigma = _two(sigma)
    k = _counter(B, c, index0, index_total)
    g = np.zeros((B, 6))
    for j in range(6):
        if sigma[j // 3] > 0:
            g[:, j] = sigma[j // 3] * gauss(seed, k, 16 + 2 * j)
    return g


def wrench(c, g, dt, sigma=0.0, tau=1.0, seed=0, base=None, amp=None, phase=None, period=1.0, kick=None, window=None, index0=0,
           index_total=None, B=None):
    """One step of a batch at campaign step c.  g [B,6]: the Gauss-Markov state of this step, or None for a stationary start (B then
    comes from the keyword or from whichever array is given);
    base [B,6] | None (plant force, then torque); amp [B,6] | None (amp_force, then amp_torque; zeros where one is not given);
    phase [B] | None; kick [B,6] | None with window [B,2] int.  Vehicle b is number index0 + b of a campaign of index_total (default
    B).  Returns (w [B,6], the wrench held over this plant step, and g_next [B,6], the state of step c + 1)."""
    sigma = _two(sigma)
    phi, innov = process(sigma, tau, dt)
    if B is None:
        B = next((np.shape(a)[0] for a in (g, base, amp, phase, kick, window) if a is not None), None)
        if B is None:
            raise ValueError("wrench: B is needed where no array is given")
    k = _counter(B, c, index0, index_total)
    g = stationary(B, sigma, seed, c, index0, index_total) if g is None else np.array(g, dtype=np.float64).reshape(B, 6)
    w = (np.zeros((B, 6)) if base is None else np.array(base, dtype=np.float64).reshape(B, 6)) + g
    if amp is not None:
        ph = np.zeros(B) if phase is None else np.asarray(phase, dtype=np.float64).reshape(B)
        s = np.sin(TWO_PI * (float(int(c)) * float(dt) / float(period)) + ph)
        w = w + np.asarray(amp, dtype=np.float64).reshape(B, 6) * s[:, None]
    if kick is not None:
        win = np.asarray(window, dtype=np.int64).reshape(B, 2)
        on = (win[:, 0] <= int(c)) & (int(c) < win[:, 1])
        w = w + np.where(on[:, None], np.asarray(kick, dtype=np.float64).reshape(B, 6), 0.0)
    g_next = np.empty((B, 6))
    for j in range(6):
        a = j // 3
        g_next[:, j] = phi[a] * g[:, j] + (innov[a] * gauss(seed, k, 2 * j) if sigma[a] > 0 else 0.0)
    return w, g_next


def amplitudes(B, amp_force=None, amp_torque=None):
    """amp [B,6] from the two optional [B,3] arrays (None when neither is given)."""
    if amp_force is None and amp_torque is None:
        return None
    amp = np.zeros((B, 6))
    if amp_force is not None:
        amp[:, 0:3] = np.asarray(amp_force, dtype=np.float64).reshape(B, 3)
    if amp_torque is not None:
        amp[:, 3:6] = np.asarray(amp_torque, dtype=np.float64).reshape(B, 3)
    return amp


def replay(B, T, dt, environment, plant=None, index0=0, index_total=None):
    """A whole run from the seed: the environment dict of BatchedMPC.simulate (what `request` accepts) over T steps of B vehicles, on
    top of plant["force"] / ["torque"].  Returns dict(wrench [T,B,6], state [B,6]: g of step step0 + T)."""
    r = request(environment, B, T, in_call=False)
    base = None
    if plant is not None and (plant.get("force") is not None or plant.get("torque") is not None):
        base = np.zeros((B, 6))
        if plant.get("force") is not None:
            base[:, 0:3] = np.asarray(plant["force"], dtype=np.float64).reshape(B, 3)
        if plant.get("torque") is not None:
            base[:, 3:6] = np.asarray(plant["torque"], dtype=np.float64).reshape(B, 3)
    amp = amplitudes(B, r["amp_force"], r["amp_torque"])
    g = r["state"]
    hist = np.empty((T, B, 6))
    for t in range(T):
        hist[t], g = wrench(r["step0"] + t, g, dt, r["sigma"], r["tau"], r["seed"], base, amp, r["phase"], r["period"], r["kick"],
                            r["window"], index0, index_total, B)
    return dict(wrench=hist, state=g)


def request(environment, B, T, sensor=None, disturbance=None, in_call=True):
    """The checks BatchedMPC.simulate makes on an environment dict before the call reaches the library (the library's own refusals,
    raised here as ValueError naming the field; in_call=False, as replay uses it, leaves out the one against the rest of the call:
    est_err_sq needing a disturbance); returns the dict with defaults filled in: seed, step0, sigma (2,), tau (2,), period,
    amp_force / amp_torque [B,3] | None, phase [B] | None, kick [B,6] | None, window [B,2] int32 | None, state [B,6] | None,
    est_err_sq [B,2] | None (copies: the call writes into them), fields."""
    spec = dict(environment)
    out = dict(seed=int(spec.pop("seed", 0)), step0=int(spec.pop("step0", 0)), sigma=spec.pop("sigma", 0.0), tau=spec.pop("tau", 1.0),
               period=float(spec.pop("period", 1.0)), amp_force=spec.pop("amp_force", None), amp_torque=spec.pop("amp_torque", None),
               phase=spec.pop("phase", None), kick=spec.pop("kick", None), window=spec.pop("window", None),
               state=spec.pop("state", None), est_err_sq=spec.pop("est_err_sq", None), fields=tuple(spec.pop("fields", ())))
    if spec:
        raise ValueError(f"environment: unknown keys {sorted(spec)}")
    if out["step0"] < 0:
        raise ValueError("environment['step0'] must be >= 0")
    if sensor is not None and int(sensor.get("step0", 0)) != out["step0"]:
        raise ValueError(f"environment['step0'] is {out['step0']}, sensor['step0'] is {int(sensor.get('step0', 0))}: one campaign "
                         "clock per call")
    for name in ("sigma", "tau"):
        try:
            out[name] = _two(out[name])
        except ValueError:
            raise ValueError(f"environment['{name}'] must be one value or 2 (force, torque)") from None
    if not (np.isfinite(out["sigma"]).all() and (out["sigma"] >= 0).all()):
        raise ValueError("environment['sigma'] must be finite and >= 0")
    for a in range(2):
        if out["sigma"][a] > 0 and not (np.isfinite(out["tau"][a]) and out["tau"][a] > 0):
            raise ValueError(f"environment['tau'][{a}] must be positive and finite where sigma is > 0")
    if any(f not in FIELDS for f in out["fields"]):
        raise ValueError(f"environment['fields'] must be among {list(FIELDS)}")
    if (out["amp_force"] is not None or out["amp_torque"] is not None) and not (np.isfinite(out["period"]) and out["period"] > 0):
        raise ValueError("environment['period'] must be positive and finite where an amplitude is given")
    for name, shape in (("amp_force", (B, 3)), ("amp_torque", (B, 3)), ("phase", (B,)), ("kick", (B, 6)), ("state", (B, 6)),
                        ("est_err_sq", (B, 2))):
        if out[name] is not None:
            out[name] = np.array(out[name], dtype=np.float64)
            if out[name].shape != shape or not np.isfinite(out[name]).all():
                raise ValueError(f"environment['{name}'] must have shape {shape} and finite entries")
    if out["kick"] is not None and out["window"] is None:
        raise ValueError("environment['kick'] needs environment['window']: [from, to) in campaign steps")
    if out["window"] is not None:
        out["window"] = np.ascontiguousarray(out["window"], dtype=np.int32)
        if out["window"].shape != (B, 2):
            raise ValueError(f"environment['window'] must have shape {(B, 2)}: [from, to) in campaign steps")
    if (out["est_err_sq"] is not None or "est_err_sq" in out["fields"]) and disturbance is None and in_call:
        raise ValueError("environment['est_err_sq'] needs a disturbance estimate (`disturbance`) in the same call")
    if out["est_err_sq"] is not None and (out["est_err_sq"] < 0).any():
        raise ValueError("environment['est_err_sq'] must have no negative entry")
    return out


def _pm1(seed, vehicles, comp, n):
    idx = vehicles[:, None] * np.uint64(STRIDE) + (np.uint64(comp) + np.arange(n, dtype=np.uint64))[None, :]
    return 2.0 * u01(seed, idx) - 1.0


def sample(B, seed, index0=0, amp_force=0.0, amp_torque=0.0, kick_force=0.0, kick_torque=0.0, kick_from=(0, 0), kick_length=(0, 0)):
    """Amplitudes, phases, kick windows and kick vectors of the vehicles [index0, index0 + B) of a campaign, as keys of an
    `environment` dict:
      amp_force  [B,3] = amp_force u_k (N),   amp_torque [B,3] = amp_torque u_k (N m),   phase [B] uniform in [0, 2 pi)
      kick       [B,6] = (kick_force u_k, kick_torque u_k),   window [B,2]: from uniform in kick_from = (lo, hi) inclusive, length
                 uniform in kick_length = (lo, hi) inclusive (campaign steps; length 0: no kick)
    with every u uniform in [-1, 1), keyed by (seed, index0 + b, component) alone: sample(B=96)[40:96] is sample(B=56, index0=40) bit
    for bit.  A half-width of zero leaves that key out (amplitudes) or gives zeros (kick)."""
    v = np.uint64(int(index0)) + np.arange(B, dtype=np.uint64)
    out = {}
    if amp_force:
        out["amp_force"] = float(amp_force) * _pm1(seed, v, C_AMP_FORCE, 3)
    if amp_torque:
        out["amp_torque"] = float(amp_torque) * _pm1(seed, v, C_AMP_TORQUE, 3)
    if amp_force or amp_torque:
        out["phase"] = TWO_PI * u01(seed, v * np.uint64(STRIDE) + np.uint64(C_PHASE))
    if kick_force or kick_torque:
        k = _pm1(seed, v, C_KICK, 6)
        k[:, 0:3] *= float(kick_force)
        k[:, 3:6] *= float(kick_torque)
        f0, f1 = (int(a) for a in kick_from)
        l0, l1 = (int(a) for a in kick_length)
        if f1 < f0 or l1 < l0 or f0 < 0 or l0 < 0:
            raise ValueError("kick_from and kick_length must be (lo, hi) with 0 <= lo <= hi")
        start = f0 + np.floor(u01(seed, v * np.uint64(STRIDE) + np.uint64(C_FROM)) * (f1 - f0 + 1)).astype(np.int64)
        length = l0 + np.floor(u01(seed, v * np.uint64(STRIDE) + np.uint64(C_LENGTH)) * (l1 - l0 + 1)).astype(np.int64)
        out["kick"] = k
        out["window"] = np.stack([start, start + length], axis=1).astype(np.int32)
    return out
