"""Thruster faults that start mid-run: the host side of the fault schedule of the on-device closed loops
(include/ftmpc.h, ftmpc_fault_schedule; BatchedMPC.simulate(faults=...)).

A schedule gives every vehicle up to E events.  Event e carries the FULL pattern after it (ub / stuck as
SystemModel.set_fault leaves them), an onset step (the plant switches) and a detection step >= onset (the
controller switches, and repairs its warm start for the new constraints).  onset = -1 marks an unused slot."""
import numpy as np

from .controllers.tools.input_bounds import hull_tables

F_MAX = 3.4  # sys_model.py:60
HULL_MARGIN = 1e-8   # relative facet margin of the wrench warm-start repair (the tau_0 rule of ftmpc_solve_sqp_wrench_batch)


def schedule_from_failures(actuator_failures, dt, NT=16, max_thrust=F_MAX):
    """Reference-style config (reactive.yaml: actuator_failures[] of act_id, intensity, start_time in seconds) -> the initial
    pattern and a one-vehicle schedule.  Failures at step 0 go into the initial pattern; the others become events at step
    round(start_time / dt), those of the same step merged into one.  Events are cumulative, as SystemModel.set_fault: the pattern
    after an event holds every failure up to it.  Returns (ub [NT], stuck [NT], faults) with faults = dict(onset [E] int,
    ub [E,NT], stuck [E,NT]), which BatchedMPC.simulate broadcasts over the batch."""
    fs = sorted(actuator_failures, key=lambda f: float(f.get("start_time", 0.0)))
    ub, stuck = np.full(NT, float(max_thrust)), np.zeros(NT)
    onset, ubs, stucks = [], [], []
    for f in fs:
        step = int(round(float(f.get("start_time", 0.0)) / dt))
        if step < 0:
            raise ValueError("actuator failure with a negative start_time")
        i = int(f["act_id"])
        if not 0 <= i < NT:
            raise ValueError(f"act_id {i} outside [0, {NT})")
        if step == 0:
            ub[i], stuck[i] = 0.0, float(f["intensity"]) * max_thrust
            continue
        if not onset or onset[-1] != step:
            onset.append(step)
            ubs.append((ubs[-1] if ubs else ub).copy())
            stucks.append((stucks[-1] if stucks else stuck).copy())
        ubs[-1][i], stucks[-1][i] = 0.0, float(f["intensity"]) * max_thrust
    E = len(onset)
    return ub, stuck, dict(onset=np.asarray(onset, np.int32).reshape(E), ub=np.asarray(ubs, float).reshape(E, NT),
                           stuck=np.asarray(stucks, float).reshape(E, NT))


def normalize_schedule(faults, B, NT, T=None, detect_delay=0):
    """faults dict(onset [B,E] or [E], ub [B,E,NT] or [E,NT], stuck likewise) and detect_delay (int, [B] or [B,E]) -> C-contiguous
    (onset [B,E] int32, detect [B,E] int32, ub [B,E,NT], stuck [B,E,NT]); unused slots (onset -1) keep detect -1."""
    onset = np.asarray(faults["onset"])
    E = onset.shape[-1] if onset.ndim else 0
    if E == 0:
        z = np.zeros((B, 0), np.int32)
        return z, z.copy(), np.zeros((B, 0, NT)), np.zeros((B, 0, NT))
    onset = np.ascontiguousarray(np.broadcast_to(onset.reshape(-1, E) if onset.ndim == 2 else onset.reshape(E), (B, E)), np.int32)
    ub = np.ascontiguousarray(np.broadcast_to(np.asarray(faults["ub"], float).reshape(-1, E, NT), (B, E, NT)))
    stuck = np.ascontiguousarray(np.broadcast_to(np.asarray(faults["stuck"], float).reshape(-1, E, NT), (B, E, NT)))
    d = np.asarray(detect_delay, np.int64)
    if d.ndim == 1:
        d = d[:, None]
    delay = np.broadcast_to(d, (B, E))
    if (delay < 0).any():
        raise ValueError("detect_delay must be >= 0")
    detect = np.ascontiguousarray(np.where(onset >= 0, onset + delay, -1), np.int32)
    return onset, detect, ub, stuck


def fault_hull_tables(D, ub, stuck, ev_ub, ev_stuck, onset):
    """hull_tables over the initial pattern and every used event pattern stacked together, split back: dict(A, set [B], b [B,rows],
    rows, degenerate [B] (any pattern of that vehicle flat), ev_set [B,E], ev_b [B,E,rows]).  Unused slots (onset < 0) get the
    initial pattern's set and offsets."""
    ub, stuck = np.asarray(ub, float), np.asarray(stuck, float)
    B, NT = ub.shape
    E = ev_ub.shape[1]
    used = (np.asarray(onset) >= 0)[:, :, None]
    pu = np.where(used, ev_ub, ub[:, None, :])
    ps = np.where(used, ev_stuck, stuck[:, None, :])
    allu = np.concatenate([ub[None], pu.transpose(1, 0, 2)]).reshape(-1, NT)
    alls = np.concatenate([stuck[None], ps.transpose(1, 0, 2)]).reshape(-1, NT)
    h = hull_tables(D, allu, alls)
    rows = h["rows"]
    sets = h["set"].reshape(E + 1, B)
    bs = h["b"].reshape(E + 1, B, rows)
    deg = h["degenerate"].reshape(E + 1, B).any(axis=0)
    return dict(A=h["A"], set=np.ascontiguousarray(sets[0]), b=np.ascontiguousarray(bs[0]), rows=rows, degenerate=deg,
                ev_set=np.ascontiguousarray(sets[1:].T, np.int32), ev_b=np.ascontiguousarray(bs[1:].transpose(1, 0, 2)))


def clip_warm(U, ub):
    """Thruster-form warm-start repair: U [..., N, NT] clipped elementwise to [0, ub] (ub [..., NT])."""
    return np.minimum(np.maximum(U, 0.0), np.asarray(ub, float)[..., None, :])


def pull_into_hull(G, D, ub, stuck, A, b, margin=HULL_MARGIN):
    """Wrench-form warm-start repair of ONE vehicle: every stage of G [N,6] pulled towards the hull centre D (ub/2 + stuck) by the
    smallest factor that leaves every facet a (A g <= b) the relative margin `margin` of its slack at the centre; a stage that
    keeps the margin is returned unchanged.  The rule of ftmpc_sqpw_tau0_kernel applied to every stage."""
    G = np.array(G, float).reshape(-1, 6)
    ctr = np.asarray(D, float) @ (0.5 * np.asarray(ub, float) + np.asarray(stuck, float))
    s0 = b - A @ ctr
    for k in range(G.shape[0]):
        st = b - A @ G[k]
        bad = (st < margin * s0) & (s0 > st)
        if bad.any():
            eps = np.max((margin * s0[bad] - st[bad]) / (s0[bad] - st[bad]) * 1.0001)
            G[k] = ctr + (1.0 - eps) * (G[k] - ctr)
    return G
