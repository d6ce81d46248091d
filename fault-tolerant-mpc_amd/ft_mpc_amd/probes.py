"""Probe pulses on the host: NumPy restatements of what BatchedMPC.simulate(probe=...) runs on the device after every solve
(include/ftmpc.h, ftmpc_probe; csrc/ftmpc_probe.h, the host / device functions ftmpc_probe_kernel is made of).

The diagnosis is passive: a dead thruster that is not commanded has no signature, and a thruster the controller was told to leave
alone can never clear itself.  The probe fires a thruster that has been quiet.  Per vehicle and step, with (ub_c, stuck_c) the
controller's pattern, u the solve's command:
  listed     thruster i is off and the newest entry for i in the vehicle's detection list has a level below n_levels
  probeable  live (ub_c,i > 0), or listed under reinstate
  idle       e_i = ub_c,i > 0 ? u_i : 0,  idle_i = (probeable and e_i < quiet) ? idle_i + 1 : 0  (a NaN command compares false)
  candidate  the probeable thruster with the largest idle_i among those with idle_i >= idle_steps and, when capped,
             pulses_i < max_pulses; the lowest index on a tie; at most one per vehicle and step
  pulse      live: u_i = min(u_i + amp, ub_c,i); listed: u_i = amp; pulses_i += 1, impulse += (u_i,new - e_i) dt, idle_i = 0
step is one vehicle's step, replay a whole run from the commands the loop recorded.  The hypothesis "listed thruster i is healthy"
that reinstate adds to the decision rule is restated in ft_mpc_amd.diagnosis (test_step and replay with probe=).

The pulse is not wrench-neutral (the controller corrects its effect on the next step); a thruster stuck at the level it is commanded
at still has no signature; the parameters are uniform over the call; a PWM actuator swallows a pulse below its minimum on-time;
MultiGPUMPC has no probe."""
from __future__ import annotations

import numpy as np

FIELDS = ("thruster_hist", "idle", "pulses", "impulse", "pacc", "health", "reinstated")
_CARRIED = (("idle", np.int32, True), ("pulses", np.int32, True), ("impulse", np.float64, False), ("pacc", np.float64, True),
            ("health", np.float64, True), ("reinstated", np.int32, False))


def request(probe, B, T, NT, diagnosis):
    """The checks BatchedMPC.simulate makes on a probe dict before the call reaches the library (the library's own refusals, raised
    from Python too, each naming its ftmpc_probe field); diagnosis: the call's diagnosis dict or None.  Returns the dict with defaults
    filled in: amp, quiet, idle_steps, max_pulses, reinstate, restore_ub, idle / pulses [B,NT] | None, impulse [B] | None,
    pacc / health [B,NT] | None, reinstated [B] | None (copies: the call writes into them), fields."""
    spec = dict(probe)
    out = dict(amp=spec.pop("amp", None), quiet=spec.pop("quiet", 0.0), idle_steps=spec.pop("idle_steps", None),
               max_pulses=spec.pop("max_pulses", 0), reinstate=spec.pop("reinstate", False), restore_ub=spec.pop("restore_ub", None),
               fields=spec.pop("fields", None))
    for name, _, _ in _CARRIED:
        out[name] = spec.pop(name, None)
    if spec:
        raise ValueError(f"probe: unknown keys {sorted(spec)}")
    if diagnosis is None:
        raise ValueError("probe: the call has no diagnosis whose pattern and detection list the probe reads (ftmpc_probe needs ftmpc_diagnosis)")
    has_state = (diagnosis.get("state") is not None
                 or any(f in ("detect", "state") for f in diagnosis.get("fields", ("detect", "pattern", "llr_hist", "state"))))
    if out["fields"] is None:
        out["fields"] = tuple(f for f in FIELDS if f not in ("pacc", "health") or has_state)
    out["fields"] = tuple(out["fields"])
    if any(f not in FIELDS for f in out["fields"]):
        raise ValueError(f"probe['fields'] must be among {list(FIELDS)}")

    def number(name):
        try:
            return float(out[name])
        except (TypeError, ValueError):
            raise ValueError(f"probe[{name!r}] must be one number (ftmpc_probe.{name})") from None

    def integer(name, low):
        v = out[name]
        if v is None or isinstance(v, bool) or int(v) != v or int(v) < low:
            raise ValueError(f"probe[{name!r}] must be an integer >= {low}, not {v} (ftmpc_probe.{name})")
        return int(v)

    out["amp"] = number("amp")
    if not (np.isfinite(out["amp"]) and out["amp"] > 0):
        raise ValueError("probe['amp'] must be finite and > 0 (ftmpc_probe.amp)")
    out["quiet"] = number("quiet")
    if not 0 <= out["quiet"] < out["amp"]:
        raise ValueError("probe['quiet'] must lie in [0, amp) (ftmpc_probe.quiet)")
    out["idle_steps"] = integer("idle_steps", 1)
    out["max_pulses"] = integer("max_pulses", 0)
    if out["reinstate"] not in (0, 1, False, True):
        raise ValueError(f"probe['reinstate'] must be 0 or 1 (False or True), not {out['reinstate']} (ftmpc_probe.reinstate)")
    out["reinstate"] = bool(out["reinstate"])
    if out["reinstate"]:
        out["restore_ub"] = number("restore_ub")
        if not (np.isfinite(out["restore_ub"]) and out["restore_ub"] > 0):
            raise ValueError("probe['restore_ub'] must be finite and > 0 when reinstate is set (ftmpc_probe.restore_ub)")
    else:
        out["restore_ub"] = 0.0 if out["restore_ub"] is None else number("restore_ub")
    for name, dtype, wide in _CARRIED:
        if out[name] is None:
            continue
        a = out[name] = np.array(out[name], dtype=dtype)
        shape = (B, NT) if wide else (B,)
        if a.shape != shape or not np.isfinite(a).all() or (a < 0).any():
            raise ValueError(f"probe[{name!r}] must have shape {shape} and no negative or non-finite entry (ftmpc_probe.{name})")
    for name in ("pacc", "health"):
        if (out[name] is not None or name in out["fields"]) and not has_state:
            raise ValueError(f"probe[{name!r}] requires the diagnosis' state (diagnosis['state'], or 'state' or 'detect' among its "
                             f"fields): ftmpc_probe.{name} without ftmpc_diagnosis.state")
    return out


def listed(ub, detections, n_levels):
    """[NT] bool: thruster i is off in the controller's pattern ub [NT] and the newest entry for i in detections
    [(step, thruster, level)], oldest first, has a level below n_levels (an entry at n_levels is a reinstatement)."""
    ub = np.asarray(ub, dtype=np.float64).reshape(-1)
    newest = {}
    for _, i, l in detections:
        if i >= 0:
            newest[int(i)] = int(l)
    out = np.zeros(ub.size, bool)
    for i, l in newest.items():
        out[i] = (not ub[i] > 0) and l < int(n_levels)
    return out


def step(u, ub, idle, pulses, lst, spec, dt):
    """One vehicle's probe step.  u [NT]: the solve's command; ub [NT]: the controller's pattern; idle, pulses [NT]: the counters;
    lst [NT] bool: `listed`; spec: dict(amp, quiet, idle_steps, max_pulses=0, reinstate=False); dt: the step.
    Returns dict(u [NT] the command with the pulse, idle, pulses (new arrays), thruster (the pulsed one, or -1), impulse (what the
    pulse adds, N s))."""
    u = np.array(u, dtype=np.float64).reshape(-1)
    ub = np.asarray(ub, dtype=np.float64).reshape(-1)
    idle = np.array(idle, dtype=np.int64).reshape(-1)
    pulses = np.array(pulses, dtype=np.int64).reshape(-1)
    amp, quiet = float(spec["amp"]), float(spec.get("quiet", 0.0))
    need, cap = int(spec["idle_steps"]), int(spec.get("max_pulses", 0))
    live = ub > 0
    probeable = live | (np.asarray(lst, bool).reshape(-1) if spec.get("reinstate", False) else False)
    e = np.where(live, u, 0.0)
    with np.errstate(invalid="ignore"):
        still = probeable & (e < quiet)
    idle = np.where(still, idle + 1, 0)
    ok = probeable & (idle >= need) & ((pulses < cap) if cap > 0 else True)
    thruster, impulse = -1, 0.0
    if ok.any():
        thruster = int(np.argmax(np.where(ok, idle, -1)))      # (the first of equal maxima)
        new = min(u[thruster] + amp, ub[thruster]) if live[thruster] else amp
        impulse = (new - e[thruster]) * float(dt)
        u[thruster] = new
        pulses[thruster] += 1
        idle[thruster] = 0
    return dict(u=u, idle=idle, pulses=pulses, thruster=thruster, impulse=float(impulse))


def replay(commands, thruster_hist, ub_hist, listed_hist, spec, dt, idle=None, pulses=None, impulse=0.0, solved=None):
    """The probe of a whole run for ONE vehicle, from what the loop recorded.  commands [T,NT]: the command of every step as it
    entered the latency ring, the pulse included (u_hist; with a latency of d steps row t of u_hist is the command of step t - d,
    and the last d commands are the sensor's `pending`); thruster_hist [T]; ub_hist [T,NT]: the controller's pattern of every
    step (ft_mpc_amd.diagnosis.replay: ub); listed_hist [T,NT] bool (`listed` of every step; None: nothing is listed); idle, pulses
    [NT], impulse: what a previous call returned; solved [T,NT] | None: the solve's commands before the pulse, where they are known.
    The recorded command of a pulsed thruster is the command after the pulse; the one before it is taken from `solved`, or is
    commands - amp where the pulse was not clipped by ub (a clipped pulse on a live thruster without `solved` is refused: the
    command before it cannot be told).  Every other thruster's command is the solve's.
    Returns dict(thruster_hist [T] (the rule's own candidates: equal to the input when the run followed the rule), idle, pulses
    [NT], impulse, idle_hist [T,NT] (after each step))."""
    cmd = np.asarray(commands, dtype=np.float64)
    T, NT = cmd.shape
    th = np.asarray(thruster_hist).reshape(T)
    ubh = np.asarray(ub_hist, dtype=np.float64).reshape(T, NT)
    lh = np.zeros((T, NT), bool) if listed_hist is None else np.asarray(listed_hist, bool).reshape(T, NT)
    idle = np.zeros(NT, np.int64) if idle is None else np.array(idle, dtype=np.int64).reshape(NT)
    pulses = np.zeros(NT, np.int64) if pulses is None else np.array(pulses, dtype=np.int64).reshape(NT)
    impulse = float(impulse)
    amp = float(spec["amp"])
    got, ih = np.full(T, -1, np.int64), np.empty((T, NT), np.int64)
    for t in range(T):
        u = cmd[t].copy()
        j = int(th[t])
        if solved is not None:
            u = np.asarray(solved, dtype=np.float64)[t].copy()
        elif j >= 0:
            if not ubh[t, j] > 0:
                u[j] = 0.0                                   # (a listed thruster: the solve's command does not count, e = 0)
            elif cmd[t, j] < ubh[t, j]:
                u[j] = cmd[t, j] - amp
            else:
                raise ValueError(f"probes.replay: the pulse of step {t} on thruster {j} was clipped by ub; pass solved=")
        r = step(u, ubh[t], idle, pulses, lh[t], spec, dt)
        idle, pulses, got[t] = r["idle"], r["pulses"], r["thruster"]
        if r["thruster"] >= 0 and solved is None and ubh[t, r["thruster"]] > 0 and r["thruster"] == j:
            r["impulse"] = (cmd[t, j] - u[j]) * float(dt)      # (the recorded command, not u - amp + amp)
        impulse += r["impulse"]
        ih[t] = idle
    return dict(thruster_hist=got, idle=idle, pulses=pulses, impulse=impulse, idle_hist=ih)
