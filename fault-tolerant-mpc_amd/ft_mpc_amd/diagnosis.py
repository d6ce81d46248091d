"""Thruster fault diagnosis on the host: NumPy restatements of what BatchedMPC.simulate(diagnosis=...) runs on the device before every
solve (include/ftmpc.h, ftmpc_diagnosis; csrc/ftmpc_sim.hip, ftmpc_diagnose_kernel).

Per vehicle a bank of one-sided CUSUM tests, one per hypothesis "thruster i is stuck at level l" (index i L + l; a dead thruster is
level 0), on a parity residual: the measurement y_t against xt, the open-loop prediction of the controller's model from the last used
measurement.  With n the model steps since that measurement and acc_i the sum over them of the effective command of thruster i:
  signature   delta = n levels[l] - acc_i,  a_v = (dt / m) D[0:3, i] delta,  a_w = dt J^-1 D[3:6, i] delta
  test_step   r = y [-] xt,  rho_v = M(q~)' r[3:6],  r_w = r[9:12],  s = resid_sigma^2 + n drift_sigma^2 (velocity, rate),
              z = (a_v . rho_v - |a_v|^2 / 2) / s_v + (a_w . r_w - |a_w|^2 / 2) / s_w,  llr = max(0, llr + z); 0 where ub_c,i == 0
  decision    the largest statistic above the threshold is detected (a tie: the lowest index): ub_c,i = 0, stuck_c,i = levels[l],
              every statistic of the vehicle back to 0
  propagate   xt <- one RK4 step of the model under c_i = ub_c,i > 0 ? a_t,i : 0 and stuck_c, acc += c, n += 1
replay runs the loop's diagnosis for one vehicle from the recorded measurements and applied commands.

The signature is first order in dt; a dead thruster that is not commanded has none, and neither has a thruster stuck at the level it
is commanded at; with isolation= (include/ftmpc.h, ftmpc_isolation; csrc/ftmpc_isolate.h) the decision gets a consistency gate on the
fit q_h = q_0 - 2 z_h, confirmation over `persist` tests and the revision of a detected thruster's level; a fault that starts inside a window of every > 1 steps shows only a part of its signature in that window's test; a
detection is withdrawn only under a reinstating probe (probe=, include/ftmpc.h, ftmpc_probe; ft_mpc_amd.probes), which pulses a detected
thruster and adds the hypotheses "listed thruster i is healthy"; position and attitude are not used; the diagnosis is told neither the plant's dispersion nor the
actuator."""
from __future__ import annotations

import numpy as np

from .estimators import _body_to_inertial, _cfg_model, residual
from .sensors import predict

MAX_LEVELS = 4
MAX_DETECT = 8          # FTMPC_MAX_FAULT_EVENTS
FIELDS = ("detect", "pattern", "llr_hist", "state")
ISO_FIELDS = ("lead", "voided", "revised", "fit")


def default_sigma(sensor_sigma, noise=(0.0, 0.0, 0.0, 0.0)):
    """resid_sigma (2,) for a sensor with standard deviations sensor_sigma (4,) and process noise amplitudes noise (4,):
    sqrt(2 sigma^2 + noise^2) for the velocity and rate groups (the residual is a difference of two measurements)."""
    s = np.asarray(sensor_sigma, dtype=np.float64).reshape(4)
    a = np.asarray(noise, dtype=np.float64).reshape(4)
    return np.sqrt(2.0 * s[[1, 3]] ** 2 + a[[1, 3]] ** 2)


def signature(n, acc, levels, cfg):
    """(a_v [NT,L,3], a_w [NT,L,3]): what "thruster i stuck at level l over the last n steps" adds to the body-frame velocity and
    to the rate, against a model that applied acc [NT] in sum."""
    D, m, J = _cfg_model(cfg)
    lv = np.asarray(levels, dtype=np.float64).reshape(-1)
    delta = float(n) * lv[None, :] - np.asarray(acc, dtype=np.float64).reshape(-1, 1)            # [NT, L]
    gv = (float(cfg.dt) / m) * D[0:3].T                                                          # [NT, 3]
    gw = float(cfg.dt) * np.linalg.solve(J, D[3:6]).T
    return gv[:, None, :] * delta[:, :, None], gw[:, None, :] * delta[:, :, None]


def consist_for(p):
    """The gate `consist` that a residual which fits its hypothesis passes with probability p: the square root of the chi-square(6)
    quantile, the root x of 1 - exp(-x / 2) (1 + x / 2 + x^2 / 8) = p (bisection on a function that rises with x)."""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError("consist_for: p must lie strictly between 0 and 1")
    cdf = lambda x: 1.0 - np.exp(-0.5 * x) * (1.0 + 0.5 * x + 0.125 * x * x)
    lo, hi = 0.0, 16.0
    while cdf(hi) < p:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if cdf(mid) < p else (lo, mid)
    return float(np.sqrt(0.5 * (lo + hi)))


def _isolation(isolation):
    """(consist, persist, revise) of an isolation dict"""
    return float(isolation.get("consist", 0.0)), int(isolation.get("persist", 1)), bool(isolation.get("revise", False))


def test_step(llr, y, xt, n, acc, ub, spec, cfg, isolation=None, lead=None, stuck=None, listed=(), probe=None, pacc=None, health=None):
    """The statistics [NT,L] after the test of one step (after the max(0, .), before a detection's reset).
    isolation = dict(consist, persist, revise): the test under ftmpc_isolation's rule, with lead = (leader, run) as the last test left
    it (None: (-1, 0)), stuck [NT] the controller's levels and listed the thrusters of the vehicle's detection list (both looked at
    with revise only).  It then returns dict(llr [NT,L], q0, q [NT,L] (nan where the hypothesis is not eligible), qmin (nan without an
    eligible hypothesis), void, leader (-1: none), lead (leader, run) after the confirmation and before a decision's reset, decide
    (the leader is decided now), margin (the smallest |q_h - consist^2|, inf without a gate), gap (the leader's statistic minus the
    runner-up's, inf without a leader)).
    probe = dict(reinstate=True, ...) (include/ftmpc.h, ftmpc_probe; csrc/ftmpc_probe.h): the test with the NT further hypotheses
    H + i "listed thruster i is healthy", under isolation's rule (None: the trivial rule).  listed is then ft_mpc_amd.probes.listed
    (off, the newest entry below n_levels), pacc [NT] the applied command summed over the window, health [NT] the statistics; delta
    = pacc_i - n stuck_i, z and q as for a level hypothesis; the gate counts H + i like any other, the leader is the first of equal
    maxima over the H + NT statistics, so a level hypothesis wins a tie.  The dict then also holds health [NT] and qh [NT].  A probe
    without reinstate changes nothing."""
    if probe is not None and probe.get("reinstate") and isolation is None:
        isolation = {}
    if probe is not None and not probe.get("reinstate"):
        probe = None
    lv = np.asarray(spec["levels"], dtype=np.float64).reshape(-1)
    rs = np.asarray(spec["resid_sigma"], dtype=np.float64).reshape(2)
    ds = np.asarray(spec.get("drift_sigma", (0.0, 0.0)), dtype=np.float64).reshape(2)
    xt = np.asarray(xt, dtype=np.float64).reshape(13)
    r = residual(y, xt)
    rho_v = _body_to_inertial(xt[6:10]).T @ r[3:6]
    r_w = r[9:12]
    s_v, s_w = rs[0] ** 2 + n * ds[0] ** 2, rs[1] ** 2 + n * ds[1] ** 2
    a_v, a_w = signature(n, acc, lv, cfg)
    z = (a_v @ rho_v - 0.5 * (a_v * a_v).sum(-1)) / s_v + (a_w @ r_w - 0.5 * (a_w * a_w).sum(-1)) / s_w
    out = np.maximum(0.0, np.asarray(llr, dtype=np.float64).reshape(z.shape) + z)
    live = np.asarray(ub).reshape(-1) > 0
    if isolation is None:
        out[~live] = 0.0
        return out
    consist, persist, revise = _isolation(isolation)
    old = np.asarray(llr, dtype=np.float64).reshape(z.shape)
    NT, L = z.shape
    off = np.zeros(NT, bool)
    if revise:
        off[[i for i in set(int(i) for i in listed) if not live[i]]] = True
        if off.any():      # the signature of a revised level against the model's stuck level: delta = n (levels[l] - stuck_i)
            D, m, J = _cfg_model(cfg)
            delta = float(n) * (lv[None, :] - np.asarray(stuck, dtype=np.float64).reshape(-1, 1))
            b_v = ((float(cfg.dt) / m) * D[0:3].T)[:, None, :] * delta[:, :, None]
            b_w = (float(cfg.dt) * np.linalg.solve(J, D[3:6]).T)[:, None, :] * delta[:, :, None]
            zr = (b_v @ rho_v - 0.5 * (b_v * b_v).sum(-1)) / s_v + (b_w @ r_w - 0.5 * (b_w * b_w).sum(-1)) / s_w
            z = np.where(off[:, None], zr, z)
    if probe is not None:
        # Every hypothesis of an off thruster, revised levels and "healthy" alike, through one elementwise formula: where two of
        # them have the same delta (levels[0] = 0 and no pulse yet: "dead" and "healthy") they tie exactly, as they do on the device
        D, m, J = _cfg_model(cfg)
        u_v, u_w = (float(cfg.dt) / m) * D[0:3].T, float(cfg.dt) * np.linalg.solve(J, D[3:6]).T

        def z_of(delta):      # delta [NT, k]
            a, w = u_v[:, None, :] * delta[:, :, None], u_w[:, None, :] * delta[:, :, None]
            return (((a[..., 0] * rho_v[0] + a[..., 1] * rho_v[1] + a[..., 2] * rho_v[2])
                     - 0.5 * (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2])) / s_v
                    + ((w[..., 0] * r_w[0] + w[..., 1] * r_w[1] + w[..., 2] * r_w[2])
                       - 0.5 * (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1] + w[..., 2] * w[..., 2])) / s_w)
        st = np.asarray(stuck, dtype=np.float64).reshape(-1)
        if off.any():
            z = np.where(off[:, None], z_of(float(n) * lv[None, :] - float(n) * st[:, None]), z)
    eligible = live | off
    q0 = float(rho_v @ rho_v / s_v + r_w @ r_w / s_w)
    q = np.where(eligible[:, None], q0 - 2.0 * z, np.nan)
    counted = eligible[:, None] & ((q <= consist * consist) if consist > 0 else np.ones_like(z, bool))
    new = np.where(counted, np.maximum(0.0, old + z), np.where(eligible[:, None], old, 0.0))
    flat = new.reshape(-1)
    extra = {}
    if probe is not None:      # H + i: the applied command of a listed thruster against the model's stuck level
        lst = np.zeros(NT, bool)
        lst[[i for i in set(int(i) for i in listed) if not live[i]]] = True
        zh = z_of((np.asarray(pacc, dtype=np.float64).reshape(NT) - float(n) * st)[:, None])[:, 0]
        qh = np.where(lst, q0 - 2.0 * zh, np.nan)
        cnth = lst & ((qh <= consist * consist) if consist > 0 else np.ones(NT, bool))
        oldh = np.asarray(health, dtype=np.float64).reshape(NT)
        newh = np.where(cnth, np.maximum(0.0, oldh + zh), np.where(lst, oldh, 0.0))
        flat = np.concatenate([flat, newh])
        extra = dict(health=newh, qh=qh)
        qall = np.concatenate([q[eligible].reshape(-1), qh[lst]])
        any_counted = bool(counted.any() or cnth.any())
    thr = float(spec["threshold"])
    leader = int(np.argmax(flat)) if flat.max() > thr else -1      # (the first of equal maxima)
    gap = np.inf
    if leader >= 0 and flat.size > 1:
        gap = float(flat[leader] - np.delete(flat, leader).max())
    ld, run = (-1, 0) if lead is None else (int(lead[0]), int(lead[1]))
    if leader < 0:
        ld, run = -1, 0
    elif leader == ld:
        run += 1
    else:
        ld, run = leader, 1
    if probe is None:
        qall, any_counted = q[eligible].reshape(-1), bool(counted.any())
    margin = float(np.abs(qall - consist * consist).min()) if consist > 0 and qall.size else np.inf
    return dict(llr=new, q0=q0, q=q, qmin=float(np.min(qall)) if qall.size else np.nan,
                void=bool(consist > 0 and q0 > consist * consist and not any_counted), leader=leader, lead=(ld, run),
                decide=leader >= 0 and run >= persist, margin=margin, gap=gap, **extra)


test_step.__test__ = False      # (not a test of the suite, whatever its name)


def propagate(xt, n, acc, u, ub, stuck, cfg, force=None, torque=None):
    """(xt, n, acc) after the model's step under the applied command u [NT] and the controller's pattern; force / torque [3]: the
    estimated disturbance of the step (ft_mpc_amd.disturbances), None: the model without one."""
    c = np.where(np.asarray(ub).reshape(-1) > 0, np.asarray(u, dtype=np.float64).reshape(-1), 0.0)
    if force is None and torque is None:
        xn = predict(xt, np.asarray(u, dtype=np.float64).reshape(1, -1), ub, stuck, cfg)
    else:
        from .disturbances import predict as predict_dist
        xn = predict_dist(xt, np.zeros(3) if force is None else force, np.zeros(3) if torque is None else torque,
                          np.asarray(u, dtype=np.float64).reshape(1, -1), ub, stuck, cfg)
    return xn, n + 1, np.asarray(acc, dtype=np.float64) + c


def replay(meas, applied_u, ub, stuck, spec, cfg, step0=0, state=None, llr=None, detections=None, force=None, torque=None, avail=None,
           isolation=None, lead=None, voided=0, revised=0, probe=None, pacc=None, health=None, reinstated=0):
    """The loop's diagnosis for ONE vehicle.  meas [T,13]: the y_t; applied_u [T,NT]: the a_t (u_hist); ub, stuck [NT]: the
    controller's pattern at the call's start; spec: dict(every, levels, resid_sigma, drift_sigma, threshold, max_detect); state
    [14+NT] / llr [NT*L] / detections (list of (step, thruster, level)): what a previous call returned; force / torque [T,3]: the
    estimated disturbance of each step (simulate(disturbance=...): force_hist / torque_hist) for the propagation, None: without;
    avail [T] (simulate(outage=...): the avail history; None: always available): on a step where the vehicle is lost there is no test
    and no re-anchor, the statistics carry over and n keeps counting (the first step of a replay without state anchors regardless).
    isolation = dict(consist, persist, revise): ftmpc_isolation's rule (test_step), with lead (leader, run), voided and revised what a
    previous call returned; a lost vehicle's lead and counters do not move.  The result then also holds lead, voided, revised,
    fit_hist [T,2] (q_0 and the smallest q_h of a tested step with an eligible hypothesis, else -1, -1), gate_margin (the smallest
    |q_h - consist^2| met, inf without a gate) and lead_gap (the smallest distance of a leader to its runner-up).
    probe = dict(reinstate=True, restore_ub) (ftmpc_probe): the test with the hypotheses "listed thruster i is healthy" (test_step
    with probe=), under isolation's rule (None: the trivial rule); pacc, health [NT] and reinstated what a previous call returned.
    The decision for H + i appends (c, i, n_levels), sets ub_i = restore_ub, stuck_i = 0 and resets every statistic; pacc sums the
    applied command of the listed thrusters and goes to 0 wherever the diagnosis re-anchors; a level revision looks at
    ft_mpc_amd.probes.listed.  The result then also holds pacc, health, reinstated, health_hist [T,NT] (after each step's test,
    before a decision's reset) and listed [T,NT] (of the pattern each solve saw).  A probe without reinstate changes nothing.
    Returns dict(llr_hist [T,NT*L], detections [(step, thruster, level)], ub [T,NT], stuck [T,NT] (the pattern each solve saw),
    ub_end, stuck_end, state [14+NT], llr [NT*L], peak [T] (the largest statistic of every step that tested, else nan))."""
    meas = np.asarray(meas, dtype=np.float64).reshape(-1, 13)
    T = meas.shape[0]
    u = np.asarray(applied_u, dtype=np.float64).reshape(T, -1)
    NT = u.shape[1]
    ub = np.array(ub, dtype=np.float64).reshape(NT)
    stuck = np.array(stuck, dtype=np.float64).reshape(NT)
    lv = np.asarray(spec["levels"], dtype=np.float64).reshape(-1)
    L = lv.size
    every, K, thr = int(spec.get("every", 1)), int(spec.get("max_detect", 2)), float(spec["threshold"])
    det = [] if detections is None else [tuple(int(v) for v in d) for d in detections]
    if state is None:
        xt, n, acc = None, 0, np.zeros(NT)
    else:
        state = np.asarray(state, dtype=np.float64).reshape(14 + NT)
        xt, n, acc = state[0:13].copy(), float(state[13]), state[14:].copy()
    s = np.zeros((NT, L)) if llr is None else np.array(llr, dtype=np.float64).reshape(NT, L)
    hist, peak = np.empty((T, NT * L)), np.full(T, np.nan)
    ubh, sth = np.empty((T, NT)), np.empty((T, NT))
    ld = (-1, 0) if lead is None else (int(lead[0]), int(lead[1]))
    voided, revised = int(voided), int(revised)
    fit, gate_margin, lead_gap = np.full((T, 2), -1.0), np.inf, np.inf
    rein = probe is not None and bool(probe.get("reinstate"))
    if rein:
        from .probes import listed as probe_listed
        if isolation is None:
            isolation = {}
        pa = np.zeros(NT) if pacc is None else np.array(pacc, dtype=np.float64).reshape(NT)
        hs = np.zeros(NT) if health is None else np.array(health, dtype=np.float64).reshape(NT)
        reinstated = int(reinstated)
        hh, lsh = np.zeros((T, NT)), np.zeros((T, NT), bool)
    for t in range(T):
        c = int(step0) + t
        if xt is None:
            xt, n, acc, s = meas[t].copy(), 0, np.zeros(NT), np.zeros((NT, L))
            hist[t] = 0.0
            if rein:
                pa, hs = np.zeros(NT), np.zeros(NT)
        elif avail is not None and not avail[t]:
            hist[t] = s.reshape(-1)
        else:
            if c % every == 0 and n >= 1 and len(det) < K and isolation is not None:
                if rein:
                    r = test_step(s, meas[t], xt, n, acc, ub, spec, cfg, isolation=isolation, lead=ld, stuck=stuck,
                                  listed=np.flatnonzero(probe_listed(ub, det, L)), probe=probe, pacc=pa, health=hs)
                    hs = r["health"]
                    hh[t] = hs
                else:
                    r = test_step(s, meas[t], xt, n, acc, ub, spec, cfg, isolation=isolation, lead=ld, stuck=stuck,
                                  listed=[d[1] for d in det])
                s, ld = r["llr"], r["lead"]
                hist[t] = s.reshape(-1)
                peak[t] = hist[t].max()
                if not np.isnan(r["qmin"]):
                    fit[t] = r["q0"], r["qmin"]
                voided += int(r["void"])
                gate_margin, lead_gap = min(gate_margin, r["margin"]), min(lead_gap, r["gap"])
                if r["decide"] and r["leader"] >= NT * L:      # "thruster i is healthy": reinstated
                    i = r["leader"] - NT * L
                    det.append((c, i, L))
                    ub[i], stuck[i] = float(probe["restore_ub"]), 0.0
                    reinstated += 1
                    s, ld, hs = np.zeros((NT, L)), (-1, 0), np.zeros(NT)
                elif r["decide"]:
                    i, l = divmod(r["leader"], L)
                    det.append((c, i, l))
                    revised += int(not ub[i] > 0)
                    ub[i], stuck[i] = 0.0, lv[l]
                    s, ld = np.zeros((NT, L)), (-1, 0)
                    if rein:
                        hs = np.zeros(NT)
            elif c % every == 0 and n >= 1 and len(det) < K:
                s = test_step(s, meas[t], xt, n, acc, ub, spec, cfg)
                hist[t] = s.reshape(-1)
                peak[t] = hist[t].max()
                if peak[t] > thr:
                    k = int(np.argmax(hist[t]))      # (the first of equal maxima)
                    det.append((c, k // L, k % L))
                    ub[k // L], stuck[k // L] = 0.0, lv[k % L]
                    s = np.zeros((NT, L))
            else:
                hist[t] = s.reshape(-1)
            if c % every == 0:
                xt, n, acc = meas[t].copy(), 0, np.zeros(NT)
                if rein:
                    pa = np.zeros(NT)
        ubh[t], sth[t] = ub, stuck
        if rein:
            if np.isnan(peak[t]):
                hh[t] = hs
            lsh[t] = probe_listed(ub, det, L)
            pa = pa + np.where(lsh[t], u[t], 0.0)
        xt, n, acc = propagate(xt, n, acc, u[t], ub, stuck, cfg, None if force is None else np.asarray(force)[t],
                               None if torque is None else np.asarray(torque)[t])
    more = dict(pacc=pa, health=hs, reinstated=reinstated, health_hist=hh, listed=lsh) if rein else {}
    return dict(llr_hist=hist, detections=det, ub=ubh, stuck=sth, ub_end=ub, stuck_end=stuck,
                state=np.concatenate([xt, [float(n)], acc]), llr=s.reshape(-1), peak=peak,
                lead=ld, voided=voided, revised=revised, fit_hist=fit, gate_margin=gate_margin, lead_gap=lead_gap, **more)


def pattern(ub, stuck, detections, levels, restore_ub=None):
    """The controller's pattern (ub [NT], stuck [NT]) after the detections [(step, thruster, level)] of one vehicle.  A level equal
    to n_levels is a reinstatement (ftmpc_probe): the thruster is healthy from that step on, with ub = restore_ub."""
    ub = np.array(ub, dtype=np.float64)
    stuck = np.array(stuck, dtype=np.float64)
    lv = np.asarray(levels, dtype=np.float64).reshape(-1)
    for _, i, l in detections:
        if i >= 0 and l == lv.size:
            if restore_ub is None:
                raise ValueError("diagnosis.pattern: a reinstatement (level == n_levels) needs restore_ub")
            ub[i], stuck[i] = float(restore_ub), 0.0
        elif i >= 0:
            ub[i], stuck[i] = 0.0, float(lv[l])
    return ub, stuck


def detections_of(step, thruster, level):
    """[B] lists of (step, thruster, level) from the arrays [B,K] the call returns (-1: unused slot)."""
    step = np.asarray(step)
    return [[(int(step[b, k]), int(thruster[b, k]), int(level[b, k])) for k in range(step.shape[1]) if step[b, k] >= 0]
            for b in range(step.shape[0])]


def score(faults, detections, final=False, n_levels=None):
    """faults: per vehicle a list of (onset, thruster, level) events that happened; detections: per vehicle a list of
    (step, thruster, level).  An event is matched to the first unmatched detection of its thruster at or after its onset; an event
    left over is matched to the first unmatched detection at or after its onset, which then blames the wrong thruster; what is left
    of the events was missed, what is left of the detections are false alarms.
    final=True: an event is matched to the LAST detection of its thruster at or after its onset, so that a revised level counts as
    right; the earlier detections of that thruster from the onset on belong to the same match (they are no false alarms) and the
    delay is taken from the first of them.
    n_levels: the diagnosis' number of levels; an entry (s, i, n_levels) is then a reinstatement (ftmpc_probe): thruster i is
    healthy from step s on, so the vehicle's earlier detections of i are withdrawn: they take no part in the matching, are no false
    alarms and are counted in `withdrawn` (an event whose every detection was withdrawn is missed).
    Returns dict(delay [per event: detect_step - onset, or None when missed], missed, wrong_thruster, wrong_level, false_alarms
    [, withdrawn])."""
    delay, missed, wrong_t, wrong_l, false_alarms, withdrawn = [], 0, 0, 0, 0, 0
    for ev, det in zip(faults, detections):
        if n_levels is not None:
            back = [d for d in det if d[2] == n_levels]
            gone = [d for d in det if d[2] != n_levels and any(r[1] == d[1] and r[0] > d[0] for r in back)]
            withdrawn += len(gone)
            det = [d for d in det if d[2] != n_levels and d not in gone]
        ev, det = sorted(ev), sorted(det)
        used, hit, first = [False] * len(det), [None] * len(ev), [None] * len(ev)
        for same in (True, False):
            for j, (onset, thr, _) in enumerate(ev):
                if hit[j] is None:
                    cand = [k for k, d in enumerate(det) if not used[k] and d[0] >= onset and (d[1] == thr) == same]
                    if cand and final and same:
                        hit[j], first[j] = cand[-1], cand[0]
                        for k in cand:
                            used[k] = True
                    elif cand:
                        hit[j] = first[j] = cand[0]
                        used[hit[j]] = True
        for j, (onset, thr, lvl) in enumerate(ev):
            if hit[j] is None:
                delay.append(None)
                missed += 1
                continue
            delay.append(det[first[j]][0] - onset)
            if det[hit[j]][1] != thr:
                wrong_t += 1
            elif det[hit[j]][2] != lvl:
                wrong_l += 1
        false_alarms += used.count(False)
    out = dict(delay=delay, missed=missed, wrong_thruster=wrong_t, wrong_level=wrong_l, false_alarms=false_alarms)
    if n_levels is not None:
        out["withdrawn"] = withdrawn
    return out


def request(diagnosis, B, T, NT, estimator=None, sensor=None, f_max=None, reinstating=False):
    """The checks BatchedMPC.simulate makes on a diagnosis dict before the call reaches the library (the library's own refusals, raised
    from Python too); returns the dict with defaults filled in: every, levels (L,), resid_sigma (2,), drift_sigma (2,), threshold,
    max_detect, state [B,14+NT] | None, llr [B,NT*L] | None, detect (step, thruster, level) [B,K] | None, fields."""
    spec = dict(diagnosis)
    out = dict(every=spec.pop("every", 1), levels=spec.pop("levels", None), resid_sigma=spec.pop("resid_sigma", None),
               drift_sigma=spec.pop("drift_sigma", (0.0, 0.0)), threshold=spec.pop("threshold", None),
               max_detect=spec.pop("max_detect", 2), state=spec.pop("state", None), llr=spec.pop("llr", None),
               detect=spec.pop("detect", None), fields=tuple(spec.pop("fields", FIELDS)))
    if spec:
        raise ValueError(f"diagnosis: unknown keys {sorted(spec)}")
    if int(out["every"]) != out["every"] or int(out["every"]) < 1:
        raise ValueError(f"diagnosis['every'] must be an integer >= 1, not {out['every']}")
    out["every"] = int(out["every"])
    if estimator is not None and int(estimator.get("every", 1)) != out["every"]:
        raise ValueError(f"diagnosis['every'] = {out['every']} differs from estimator['every'] = {estimator.get('every', 1)}")
    if out["levels"] is None:
        if f_max is None:
            raise ValueError("diagnosis['levels'] is required")
        out["levels"] = (0.0, f_max)
    lv = out["levels"] = np.asarray(out["levels"], dtype=np.float64).reshape(-1)
    if not 1 <= lv.size <= MAX_LEVELS:
        raise ValueError(f"diagnosis['levels'] must hold 1..{MAX_LEVELS} values (n_levels)")
    if not (np.isfinite(lv).all() and (lv >= 0).all() and (np.diff(lv) > 0).all()):
        raise ValueError("diagnosis['levels'] must be finite, >= 0 and strictly increasing")
    if int(out["max_detect"]) != out["max_detect"] or not 1 <= int(out["max_detect"]) <= MAX_DETECT:
        raise ValueError(f"diagnosis['max_detect'] must be an integer in [1, {MAX_DETECT}]")
    K = out["max_detect"] = int(out["max_detect"])
    if out["resid_sigma"] is None:
        raise ValueError("diagnosis['resid_sigma'] is required: 2 values (velocity, rate), e.g. diagnosis.default_sigma")
    out["resid_sigma"] = np.asarray(out["resid_sigma"], dtype=np.float64)
    if out["resid_sigma"].shape != (2,) or not (np.isfinite(out["resid_sigma"]).all() and (out["resid_sigma"] > 0).all()):
        raise ValueError("diagnosis['resid_sigma'] must be 2 finite values > 0")
    out["drift_sigma"] = np.asarray(out["drift_sigma"], dtype=np.float64)
    if out["drift_sigma"].shape != (2,) or not (np.isfinite(out["drift_sigma"]).all() and (out["drift_sigma"] >= 0).all()):
        raise ValueError("diagnosis['drift_sigma'] must be 2 finite values >= 0")
    if out["threshold"] is None or not (np.isfinite(out["threshold"]) and out["threshold"] > 0):
        raise ValueError("diagnosis['threshold'] must be finite and > 0")
    out["threshold"] = float(out["threshold"])
    if any(f not in FIELDS for f in out["fields"]):
        raise ValueError(f"diagnosis['fields'] must be among {list(FIELDS)}")
    if out["state"] is None and (out["llr"] is not None or out["detect"] is not None):
        raise ValueError("diagnosis['llr'] and diagnosis['detect'] require diagnosis['state']")
    H = NT * lv.size
    if out["state"] is not None:
        if out["detect"] is None:
            raise ValueError("diagnosis['state'] requires diagnosis['detect'] = (step, thruster, level)")
        out["state"] = np.array(out["state"], dtype=np.float64)           # copies: the call writes into them
        if out["state"].shape != (B, 14 + NT) or not np.isfinite(out["state"]).all():
            raise ValueError(f"diagnosis['state'] must be finite with shape {(B, 14 + NT)}")
        if (out["state"][:, 13] < 0).any():
            raise ValueError("diagnosis['state'] has n < 0")
        if out["llr"] is not None:
            out["llr"] = np.array(out["llr"], dtype=np.float64)
            if out["llr"].shape != (B, H) or not np.isfinite(out["llr"]).all():
                raise ValueError(f"diagnosis['llr'] must be finite with shape {(B, H)}")
        det = tuple(np.array(a, dtype=np.int32) for a in out["detect"])
        if len(det) != 3 or any(a.shape != (B, K) for a in det):
            raise ValueError(f"diagnosis['detect'] must be (step, thruster, level), each of shape {(B, K)}")
        used = det[0] >= 0
        if (det[0] < -1).any() or (used[:, 1:] & ~used[:, :-1]).any():
            raise ValueError("diagnosis['detect']: a step below -1, or a used slot after an unused one")
        if ((det[1][used] < 0) | (det[1][used] >= NT)).any() or ((det[2][used] < 0) | (det[2][used] >= lv.size + int(bool(reinstating)))).any():
            raise ValueError("diagnosis['detect']: a thruster outside [0, NT) or a level outside [0, n_levels)")
        out["detect"] = det
    if sensor is not None and sensor.get("predict") and estimator is None:
        raise ValueError("diagnosis: a predicting sensor needs an estimator (the sensor alone would predict with the pattern "
                         "before the diagnosis)")
    return out


def isolation_request(isolation, B, NT, diagnosis, reinstating=False):
    """The checks BatchedMPC.simulate makes on an isolation dict before the call reaches the library (the library's own refusals, raised
    from Python too); diagnosis: the call's diagnosis dict or None.  Returns the dict with defaults filled in: consist, persist,
    revise, lead [B,2] | None, voided [B] | None, revised [B] | None (int32 copies: the call writes into them), fields."""
    spec = dict(isolation)
    out = dict(consist=spec.pop("consist", 0.0), persist=spec.pop("persist", 1), revise=spec.pop("revise", False),
               lead=spec.pop("lead", None), voided=spec.pop("voided", None), revised=spec.pop("revised", None),
               fields=spec.pop("fields", None))
    if spec:
        raise ValueError(f"isolation: unknown keys {sorted(spec)}")
    has_state = diagnosis is not None and (diagnosis.get("state") is not None
                                           or any(f in ("detect", "state") for f in diagnosis.get("fields", FIELDS)))
    if out["fields"] is None:
        out["fields"] = tuple(f for f in ISO_FIELDS if f != "lead" or has_state)
    out["fields"] = tuple(out["fields"])
    if any(f not in ISO_FIELDS for f in out["fields"]):
        raise ValueError(f"isolation['fields'] must be among {list(ISO_FIELDS)}")
    try:
        out["consist"] = float(out["consist"])
    except (TypeError, ValueError):
        raise ValueError("isolation['consist'] must be one number") from None
    if not (np.isfinite(out["consist"]) and out["consist"] >= 0):
        raise ValueError("isolation['consist'] must be 0 or finite and positive")
    if isinstance(out["persist"], bool) or int(out["persist"]) != out["persist"] or int(out["persist"]) < 1:
        raise ValueError(f"isolation['persist'] must be an integer >= 1, not {out['persist']}")
    out["persist"] = int(out["persist"])
    if out["revise"] not in (0, 1, False, True):
        raise ValueError(f"isolation['revise'] must be 0 or 1 (False or True), not {out['revise']}")
    out["revise"] = bool(out["revise"])
    trivial = (out["consist"] == 0 and out["persist"] == 1 and not out["revise"] and out["lead"] is None and out["voided"] is None
               and out["revised"] is None and not out["fields"])
    if diagnosis is None and not trivial:
        raise ValueError("isolation: the call has no diagnosis whose rule it could change")
    if out["lead"] is not None or "lead" in out["fields"]:
        if not has_state:
            raise ValueError("isolation['lead'] requires the diagnosis' state (diagnosis['state'], or 'state' or 'detect' among its fields)")
    if out["lead"] is not None:
        lv = diagnosis.get("levels")
        H = NT * (2 if lv is None else np.asarray(lv).size) + (NT if reinstating else 0)      # (a reinstating probe: H + i may lead)
        ld = out["lead"] = np.array(out["lead"], dtype=np.int32)
        if ld.shape != (B, 2):
            raise ValueError(f"isolation['lead'] must have shape {(B, 2)}")
        if ((ld[:, 0] < -1) | (ld[:, 0] >= H)).any():
            raise ValueError(f"isolation['lead']: a leader outside [-1, NT * n_levels) = [-1, {H})")
        if (ld[:, 1] < 0).any():
            raise ValueError("isolation['lead']: a negative run")
    for name in ("voided", "revised"):
        if out[name] is not None:
            a = out[name] = np.array(out[name], dtype=np.int32)
            if a.shape != (B,) or (a < 0).any():
                raise ValueError(f"isolation[{name!r}] must have shape {(B,)} and no negative entry")
    return out
