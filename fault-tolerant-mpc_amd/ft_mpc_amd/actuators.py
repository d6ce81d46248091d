"""Pulsed (PWM) thrusters and valve lag on the host: NumPy restatements of what BatchedMPC.simulate(actuator=...) integrates
(include/ftmpc.h, ftmpc_actuator; csrc/ftmpc_sim.hip, ftmpc_plant_step_act_kernel).

The plant's step of length dt is cut into S sub-steps of h = dt / S.  Per thruster i, with the plant's pattern ub_i / stuck_i and the
command u_i of the step:
    proportional   target g_ij = ub_i > 0 ? u_i : 0 in every sub-step j (unclipped)
    PWM            duty d_i = ub_i > 0 ? clip(u_i / ub_i, 0, 1) : 0,  ticks k_i = floor(d_i S + 0.5), 0 where below min_on;
                   g_ij = ub_i for s_i <= j < s_i + k_i, else 0, with s_i = 0 | (S - k_i) // 2 | S - k_i (leading | centred | trailing)
    valve lag      a_i carried over sub-steps and steps; with (E, K) the on-pair where g_ij > a_i, else the off-pair:
                   m_ij = g_ij + (a_i - g_ij) K (mean force of the sub-step), then a_i = g_ij + (a_i - g_ij) E
    thrust         m_ij + stuck_i (a jammed-open valve has no lag and no modulation), held over one RK4 step of length h

The controller is not told about any of this: it keeps commanding a proportional thruster."""
from __future__ import annotations

import numpy as np

ALIGN = {"leading": 0, "centred": 1, "trailing": 2}


def min_on_ticks(seconds, dt, S):
    """The smallest whole number of ticks of h = dt / S that lasts at least `seconds` (a valve's minimum on-time), at most S."""
    h = float(dt) / int(S)
    return int(min(int(S), max(0, int(np.ceil(float(seconds) / h - 1e-12)))))


def ticks(u, ub, S, min_on=0):
    """k [.., NT] int32: on-time of a step in ticks of h = dt / S for commands u under the plant's pattern ub."""
    u, ub = np.asarray(u, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    live = ub > 0
    d = np.where(live, np.minimum(np.maximum(u / np.where(live, ub, 1.0), 0.0), 1.0), 0.0)
    k = np.floor(d * int(S) + 0.5).astype(np.int32)
    return np.where(k < int(min_on), 0, k).astype(np.int32)


def targets(k, ub, S, align="leading"):
    """g [S, .., NT]: the PWM target of every sub-step, ub inside the on-window [s, s + k) and 0 outside."""
    k, ub = np.asarray(k), np.asarray(ub, dtype=np.float64)
    S = int(S)
    a = ALIGN[align] if isinstance(align, str) else int(align)
    s = np.zeros_like(k) if a == 0 else ((S - k) // 2 if a == 1 else S - k)
    j = np.arange(S).reshape((S,) + (1,) * k.ndim)
    return np.where((j >= s) & (j < s + k), np.where(ub > 0, ub, 0.0), 0.0)


def lag_constants(h, tau_on=0.0, tau_off=0.0):
    """(E_on, K_on, E_off, K_off): E = exp(-h / tau), K = -expm1(-h / tau) tau / h; E = K = 0 for tau = 0 (no lag)."""
    out = []
    for tau in (float(tau_on), float(tau_off)):
        if tau < 0 or not np.isfinite(tau):
            raise ValueError("a time constant must be finite and >= 0")
        out += [np.exp(-h / tau), -np.expm1(-h / tau) * tau / h] if tau > 0 else [0.0, 0.0]
    return tuple(out)


def substep_forces(g, state, consts):
    """The valves through the sub-steps: g [S, .., NT] targets, state [.., NT] valve states at the start, consts = lag_constants(..).
    Returns (m [S, .., NT] mean force of every sub-step, state [.., NT] at the end)."""
    E_on, K_on, E_off, K_off = consts
    a = np.array(state, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    m = np.empty_like(g)
    for j in range(g.shape[0]):
        on = g[j] > a
        m[j] = g[j] + (a - g[j]) * np.where(on, K_on, K_off)
        a = g[j] + (a - g[j]) * np.where(on, E_on, E_off)
    return m, a


def _normalise(actuator):
    spec = dict(actuator)
    mode = spec.get("mode", "proportional")
    if mode not in ("proportional", "pwm"):
        raise ValueError("actuator['mode'] must be 'proportional' or 'pwm'")
    S = int(spec.get("substeps", 1))
    if not 1 <= S <= 64:
        raise ValueError("actuator['substeps'] must be in [1, 64]")
    min_on = int(spec.get("min_on", 0))
    if not 0 <= min_on <= S:
        raise ValueError("actuator['min_on'] must be in [0, substeps]")
    align = spec.get("align", "leading")
    if align not in ALIGN:
        raise ValueError(f"actuator['align'] must be one of {sorted(ALIGN)}")
    if mode == "proportional" and (min_on != 0 or align != "leading"):
        raise ValueError("actuator: min_on and align belong to mode='pwm'")
    return mode, S, min_on, align, float(spec.get("tau_on", 0.0)), float(spec.get("tau_off", 0.0))


def step(x, u, ub, stuck, actuator, state=None, plant=None, cfg=None):
    """One plant step of ONE vehicle under an actuator: x [13], command u [NT], the plant's pattern ub / stuck [NT], `actuator` the
    dict of BatchedMPC.simulate, state [NT] the valve states (None: 0).  plant: a row of the `plant` dict (what is missing is cfg's),
    cfg: an MPCConfig (None: the reference's constants for len(u) thrusters).  No noise, no renormalisation.
    Returns dict(x [13], state [NT], applied [NT] = (1/S) sum_j (m_ij + stuck_i), ticks [NT] | None, delivered = sum_j h sum_i (..))."""
    from .dispersion import _omega, _rot
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    ub = np.asarray(ub, dtype=np.float64).reshape(-1)
    stuck = np.asarray(stuck, dtype=np.float64).reshape(-1)
    NT = u.size
    if cfg is None:
        from .batch import MPCConfig
        cfg = MPCConfig(NT=NT)
    plant = {} if plant is None else plant
    D = plant.get("D")
    if D is None:
        D = cfg.D
    if D is None:
        from .models.sys_model import allocation_matrix_16, allocation_matrix_8
        D = allocation_matrix_16() if NT == 16 else allocation_matrix_8()
    D = np.asarray(D, dtype=np.float64).reshape(6, NT)
    mass = float(plant["mass"]) if plant.get("mass") is not None else float(cfg.mass)
    J = np.asarray(plant["J"] if plant.get("J") is not None else cfg.J, dtype=np.float64).reshape(3, 3)
    f = np.asarray(plant["force"], dtype=np.float64).reshape(3) if plant.get("force") is not None else np.zeros(3)
    t = np.asarray(plant["torque"], dtype=np.float64).reshape(3) if plant.get("torque") is not None else np.zeros(3)
    mode, S, min_on, align, tau_on, tau_off = _normalise(actuator)
    h = float(cfg.dt) / S
    k = None
    if mode == "pwm":
        k = ticks(u, ub, S, min_on)
        g = targets(k, ub, S, align)
    else:
        g = np.broadcast_to(np.where(ub > 0, u, 0.0), (S, NT))
    m, a = substep_forces(g, np.zeros(NT) if state is None else state, lag_constants(h, tau_on, tau_off))
    x = np.asarray(x, dtype=np.float64).reshape(13)
    delivered = 0.0
    for j in range(S):
        thrust = m[j] + stuck
        gen = D @ thrust
        F, tau = gen[0:3], gen[3:6] + t

        def rhs(x):
            v, q, w = x[3:6], x[6:10], x[10:13]
            return np.concatenate([v, (_rot(q).T @ F + f) / mass, 0.5 * _omega(w) @ q, np.linalg.solve(J, tau - np.cross(w, J @ w))])
        k1 = rhs(x)
        k2 = rhs(x + h / 2 * k1)
        k3 = rhs(x + h / 2 * k2)
        k4 = rhs(x + h * k3)
        x = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        delivered += h * thrust.sum()
    return dict(x=x, state=a, applied=(m + stuck).sum(axis=0) / S, ticks=k, delivered=delivered)
