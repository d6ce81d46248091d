"""Closed-loop campaign throughput with and without a fault schedule (BatchedMPC.simulate(faults=...)): every vehicle gets one
event at a random step in [1, T) that breaks one more healthy thruster (stuck at a random intensity), detected at its onset.

    python scripts/fault_campaign_perf.py [--case thruster|wrench64|wrench32|all] [--reps 3] [--json out.json]
    python scripts/fault_campaign_perf.py --once            # one call per case with the schedule (under rocprofv3)
    python scripts/fault_campaign_perf.py --stats kernel_stats.csv   # the event and outcome kernels' share of the kernel time
    python scripts/fault_campaign_perf.py --outcomes        # also the loop with the schedule and every per-vehicle outcome
    python scripts/fault_campaign_perf.py --slots 2         # every loop on the multi-GPU driver with 2 slots on device 0
    python scripts/fault_campaign_perf.py --dispersion      # also the loops with a dispersed plant (BatchedMPC.simulate(plant=...))
    python scripts/fault_campaign_perf.py --mission         # also the loops under a three-table mission with random phases, and with cost
    python scripts/fault_campaign_perf.py --trace kernel_trace.csv   # per-launch times of the mission kernels and of the linearise kernel
    python scripts/fault_campaign_perf.py --actuator        # also the loops with PWM thrusters (S = 16, min_on 1) and valve lag in the plant
    python scripts/fault_campaign_perf.py --sensor [--latency 0 2 8] [--predict]   # also the loops with navigation errors and latency
    python scripts/fault_campaign_perf.py --sensor --estimator [--every M]   # and each of those once more with the navigation filter
    python scripts/fault_campaign_perf.py --case thruster --diagnosis       # and the sensor loops once more with the fault diagnosis
    python scripts/fault_campaign_perf.py --case wrench64 --diagnosis       # the same on the two-stage form (rebuild_hull=True)

Timed: the whole simulate call with the hull tables built beforehand; also the loop without a schedule but with the after-event
pattern from step 0 on, which brackets what the fault itself does to the QPs.
Cases: thruster form N = 20, NT = 8, B = 65 536, fp32, T = 20; wrench form N = 15, NT = 16, B = 16 384, T = 20 on an fp32 and a
float64 handle (vehicles whose hull would be flat in either pattern are dropped from both runs).
--dispersion: the loops without and with the schedule once more with ft_mpc_amd.dispersion.sample at mass 10 %, inertia 10 %, gain 5 %,
centre of mass 1 cm, force 0.05 N, torque 0.005 N m (ftmpc_plant_step_var_kernel in place of ftmpc_plant_step_kernel); with --once it
makes one call with the dispersed plant and one without, so that a kernel_stats.csv of that run holds both plant kernels, and --stats
reports the time per launch of each.
--mission: the loops without and with the schedule once more under BatchedMPC.simulate(mission=...): three tables (hover, a circle of
radius 0.5 m and period 40 s with its uref, a line at 0.05 m/s), the table number b mod 3 and a start column from
ft_mpc_amd.missions.phase_offsets per vehicle (ftmpc_ref_window_kernel before every solve, per-vehicle windows in the linearise kernel),
and the loop with the schedule, the mission and the cost outcome (ftmpc_outcome_mission_kernel); before them the same two loops under
a mission of the hover table alone, whose QPs are those of the shared loop, so that the difference is the mission's own overhead and
not other work in the solves.  With --once it makes one call with
the mission and the cost and then one with the shared reference; --trace reads the kernel_trace.csv of such a run (rocprofv3
--kernel-trace) and reports the time per launch of the two mission kernels and of the linearise kernel in either call: the launches
of the linearise kernel are split at the first launch of ftmpc_plant_step_kernel that follows the last ftmpc_ref_window_kernel.
--actuator: the loops without and with the schedule once more under BatchedMPC.simulate(actuator=...): PWM on a clock of --substeps
ticks per step (default 16), min_on 1, centred pulses, tau_on 20 ms, tau_off 10 ms, delivered and pulses returned
(ftmpc_plant_step_act_kernel in place of ftmpc_plant_step_kernel).  With --once it makes one call with the actuator and one without,
so that a kernel_stats.csv of that run holds both plant kernels, and --stats reports the time per launch of each and the actuator
kernel's share of the kernel time.
--sensor: the loops without and with the schedule once more under BatchedMPC.simulate(sensor=...): noise on every group (1 cm, 5 mm/s,
0.01 rad, 0.005 rad/s), a bias per vehicle from ft_mpc_amd.sensors.sample_bias, no history returned, once per --latency value (default
2) and, with --predict, once more with the delay-compensating prediction (ftmpc_sense_kernel before every solve, the plant fed from
the command ring).  With --once it makes one call with the sensor (the first --latency, --predict as given) and one without, so that
a kernel_stats.csv of that run holds the sense kernel next to the plant kernel, and --stats reports the time per launch of each.
--estimator (with --sensor): every sensor loop once more under BatchedMPC.simulate(estimator=...): p0 = meas_sigma = the sensor's
sigma, proc_sigma a tenth of it, the update on every --every-th step (default 1), err_sq returned (ftmpc_filter_kernel<0> before
every solve and <1> after every plant step).  With --once the call with the sensor also carries the filter, and --stats reports the
time per launch of either phase and the filter's share of the kernel time.
--diagnosis (without --sensor a sensor of latency 0 is added; on the wrench cases with rebuild_hull=True: ftmpc_hull_offsets_kernel and
ftmpc_hull_switch_kernel follow phase 0 in place of the repair kernel, and the result also counts the vehicles left without a hull): every sensor loop that a diagnosis accepts (no
prediction without the filter) once more under BatchedMPC.simulate(diagnosis=...): levels (0, f_max), resid_sigma =
diagnosis.default_sigma of the sensor and the process noise, threshold 18, the test on every --every-th step, the detections
returned (ftmpc_diagnose_kernel<0> and the repair kernel before every solve, <1> after every plant step).  The loop without a
schedule is the cost of the diagnosis on unchanged solves; with the schedule the controller learns of the fault from the diagnosis
instead of at the onset, and the result holds diagnosis.score.  With --once the call with the sensor also carries the diagnosis, and
--stats reports the time per launch of either phase."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fault-tolerant-mpc_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CASES = {"thruster": dict(N=20, NT=8, B=65536, dtype="f32", formulation="thruster"),
         "wrench32": dict(N=15, NT=16, B=16384, dtype="f32", formulation="wrench"),
         "wrench64": dict(N=15, NT=16, B=16384, dtype="f64", formulation="wrench")}
T = 20


def batch(c, seed=4040):
    import ft_mpc_amd
    from ft_mpc_amd import faults as fl
    from ft_mpc_amd.models.sys_model import allocation_matrix_8, allocation_matrix_16
    N, NT, B = c["N"], c["NT"], c["B"]
    x0, ub, stuck, _ = ft_mpc_amd.make_synthetic_batch(B, N, NT, 1, seed)
    rng = np.random.default_rng(seed)
    eub, est = ub.copy(), stuck.copy()
    for b in range(B):
        i = rng.choice(np.flatnonzero(ub[b] > 0))
        eub[b, i], est[b, i] = 0.0, 3.4 * rng.uniform()
    onset = rng.integers(1, T, (B, 1)).astype(np.int32)
    if c["formulation"] == "wrench":
        D = allocation_matrix_16() if NT == 16 else allocation_matrix_8()
        ok = ~fl.fault_hull_tables(D, ub, stuck, eub[:, None], est[:, None], onset)["degenerate"]
        x0, ub, stuck, eub, est, onset = x0[ok], ub[ok], stuck[ok], eub[ok], est[ok], onset[ok]
    return x0, ub, stuck, dict(onset=onset, ub=eub[:, None], stuck=est[:, None])


PHASES = 200      # start columns of a mission are drawn from [0, PHASES)


def mission(B, N, mass):
    """Three tables of PHASES + T + N columns and a (table, offset) per vehicle; mass: the config's, for the circle's uref."""
    from ft_mpc_amd.missions import mission_tables, phase_offsets
    cols = PHASES + T + N
    t = 0.1 * np.arange(cols)
    hover, circle, line, ucirc = np.zeros((9, cols)), np.zeros((9, cols)), np.zeros((9, cols)), np.zeros((6, cols))
    for x in (hover, circle, line):
        x[8] = 0.6
    R, om = 0.5, 2 * np.pi / 40.0
    circle[0], circle[1], circle[3], circle[4] = R * np.cos(om * t) - R, R * np.sin(om * t), -R * om * np.sin(om * t), R * om * np.cos(om * t)
    ucirc[0], ucirc[1] = -mass * R * om * om * np.cos(om * t), -mass * R * om * om * np.sin(om * t)
    line[0], line[3] = 0.05 * t, 0.05
    return dict(tables=mission_tables([hover, circle, line]), utables=mission_tables([np.zeros((6, 1)), ucirc, np.zeros((6, 1))], rows=6),
                table=(np.arange(B) % 3).astype(np.int32), offset=phase_offsets(B, PHASES, seed=23))


ACTUATOR = dict(mode="pwm", min_on=1, align="centred", tau_on=0.02, tau_off=0.01, fields=("delivered", "pulses"))
SENSOR = dict(sigma=(1e-2, 5e-3, 1e-2, 5e-3), seed=29)
SENSOR_BIAS = (0.05, 0.01, 0.02, 0.005)
ESTIMATOR = dict(p0=SENSOR["sigma"], proc_sigma=tuple(0.1 * s for s in SENSOR["sigma"]), meas_sigma=SENSOR["sigma"], fields=("err_sq",))
DIAGNOSIS = dict(levels=(0.0, 3.4), threshold=18.0, max_detect=2, fields=("detect",))
DISPERSION = dict(mass_rel=0.10, inertia_rel=0.10, gain_rel=0.05, com_offset=0.01, force=0.05, torque=0.005)


def run(name, reps, once=False, outcomes=False, slots=0, dispersion=False, with_mission=False, actuator=False, substeps=16, sensor=False,
        latencies=(2,), predict=False, estimator=False, every=1, diagnosis=False):
    import ft_mpc_amd
    c = CASES[name]
    cfg = ft_mpc_amd.MPCConfig(N=c["N"], NT=c["NT"], dtype=c["dtype"], max_iters=60 if c["formulation"] == "wrench" else 0)
    if slots > 0:
        from ft_mpc_amd.sharding import MultiGPUMPC
        mpc = MultiGPUMPC(cfg, devices=[0] * slots)
    else:
        mpc = ft_mpc_amd.BatchedMPC(cfg)
    x0, ub, stuck, f = batch(c)
    B = x0.shape[0]
    xr = np.zeros((9, T + c["N"]))
    xr[8] = 0.6
    kw = dict(seed=3, formulation=c["formulation"])
    plain, withf = {}, dict(faults=f)
    if c["formulation"] == "wrench":     # the hull tables are host work done once per campaign: built here, outside the timing
        from ft_mpc_amd import faults as fl
        from ft_mpc_amd.controllers.tools.input_bounds import hull_tables
        plain["hull"] = hull_tables(mpc.D, ub, stuck)
        withf["hull"] = fl.fault_hull_tables(mpc.D, ub, stuck, f["ub"], f["stuck"], f["onset"])
    # every outcome, the settle band included: 84 bytes per vehicle instead of x_hist + u_hist
    witho = dict(withf, outcomes=dict(tol_pos=0.5, tol_vel=0.1, tol_rate=0.05))
    plant = None
    if dispersion:
        from ft_mpc_amd.dispersion import sample
        plant = sample(B, c["NT"], mpc.D, cfg.J, cfg.mass, seed=17, **DISPERSION)
    msn = mission(B, c["N"], cfg.mass) if with_mission else None
    act = dict(ACTUATOR, substeps=substeps) if actuator else None
    sensors = []          # (label suffix, sensor dict, reference with the L more columns a predicting sensor needs)
    if sensor:
        from ft_mpc_amd.sensors import sample_bias
        bias = sample_bias(B, SENSOR_BIAS, seed=31)
        for d in latencies:
            for pr in ((False, True) if predict and d > 0 else (False,)):
                xs = np.zeros((9, T + c["N"] + (d if pr else 0)))
                xs[8] = 0.6
                sensors.append((f"sensor_d{d}" + ("_predict" if pr else ""), dict(SENSOR, bias=bias, latency=d, predict=pr), xs))
    est = dict(ESTIMATOR, every=every) if estimator and sensor else None
    diag = None
    if diagnosis:
        from ft_mpc_amd.diagnosis import default_sigma, detections_of, score
        diag = dict(DIAGNOSIS, every=every, resid_sigma=default_sigma(SENSOR["sigma"], (1e-3,) * 4))
        if c["formulation"] == "wrench":
            diag["rebuild_hull"] = True
        if not sensors:
            sensors.append(("sensor_d0", dict(SENSOR, latency=0), xr))
    with_diag = lambda sen: diag is not None and not (sen.get("predict") and est is None)
    if once:
        if sensors:
            label, sen, xs = sensors[-1] if predict else sensors[0]
            mpc.simulate(x0, ub, stuck, xs, T, sensor=sen, estimator=est, diagnosis=diag if with_diag(sen) else None,
                         **(witho if outcomes else withf), **kw)
        if actuator:
            mpc.simulate(x0, ub, stuck, xr, T, actuator=act, **(witho if outcomes else withf), **kw)
        if with_mission:
            mpc.simulate(x0, ub, stuck, None, T, mission=msn, **dict(withf, outcomes=dict(fields=["cost"])), **kw)
        if dispersion:
            mpc.simulate(x0, ub, stuck, xr, T, plant=plant, **(witho if outcomes else withf), **kw)
        mpc.simulate(x0, ub, stuck, xr, T, **(witho if outcomes else withf), **kw)
        mpc.close()
        return None
    res = {}
    after = dict(plain)                  # the after-event pattern from step 0 on (a fault makes some QPs harder or easier)
    if c["formulation"] == "wrench":
        h = withf["hull"]
        after["hull"] = dict(A=h["A"], set=h["ev_set"][:, 0], b=np.ascontiguousarray(h["ev_b"][:, 0]), rows=h["rows"],
                             degenerate=np.zeros(B, bool))
    runs = [("without", plain, ub, stuck), ("with", withf, ub, stuck), ("without_after_pattern", after, f["ub"][:, 0], f["stuck"][:, 0])]
    if outcomes:
        runs.append(("with_outcomes", witho, ub, stuck))
    if dispersion:
        runs += [("without_dispersed", dict(plain, plant=plant), ub, stuck), ("with_dispersed", dict(withf, plant=plant), ub, stuck)]
    if actuator:
        runs += [("without_actuator", dict(plain, actuator=act), ub, stuck), ("with_actuator", dict(withf, actuator=act), ub, stuck)]
    if with_mission:
        # the hover table alone at the same start columns: the QPs of the shared loop bit for bit, so what differs is the gather, the
        # per-vehicle loads of the linearise kernel and the call's staging -- not the work of the solves
        hov = dict(tables=msn["tables"][:1], offset=msn["offset"])
        runs += [("without_mission_hover", dict(plain, mission=hov), ub, stuck), ("with_mission_hover", dict(withf, mission=hov), ub, stuck),
                 ("without_mission", dict(plain, mission=msn), ub, stuck), ("with_mission", dict(withf, mission=msn), ub, stuck),
                 ("with_mission_cost", dict(withf, mission=msn, outcomes=dict(fields=["cost"])), ub, stuck)]
    refs = {}
    for label, sen, xs in sensors:
        runs += [("without_" + label, dict(plain, sensor=sen), ub, stuck), ("with_" + label, dict(withf, sensor=sen), ub, stuck)]
        refs["without_" + label] = refs["with_" + label] = xs
        if est is not None:
            runs += [("without_" + label + "_estimator", dict(plain, sensor=sen, estimator=est), ub, stuck),
                     ("with_" + label + "_estimator", dict(withf, sensor=sen, estimator=est), ub, stuck)]
            refs["without_" + label + "_estimator"] = refs["with_" + label + "_estimator"] = xs
        if with_diag(sen):
            e = "_estimator" if est is not None else ""
            runs += [("without_" + label + e + "_diagnosis", dict(plain, sensor=sen, estimator=est, diagnosis=diag), ub, stuck),
                     ("with_" + label + e + "_diagnosis", dict(withf, sensor=sen, estimator=est, diagnosis=diag), ub, stuck)]
            refs["without_" + label + e + "_diagnosis"] = refs["with_" + label + e + "_diagnosis"] = xs
    for label, extra, u, s in runs:
        u, s = np.ascontiguousarray(u), np.ascontiguousarray(s)
        ref = None if "mission" in extra else refs.get(label, xr)      # a mission's tables are the reference
        mpc.simulate(x0, u, s, ref, T, **extra, **kw)         # warm-up: workspaces, code objects, grid hints
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = mpc.simulate(x0, u, s, ref, T, **extra, **kw)
            ts.append(time.perf_counter() - t0)
        ms = float(np.median(ts)) * 1e3
        res[label] = dict(ms=ms, steps_per_s=B * T / (ms * 1e-3), not_converged=int(out["not_converged"].sum()),
                          alloc_failed=int(out.get("alloc_failed", np.zeros(1)).sum()))
        if "estimator" in out:     # root mean squared position error of the estimates over the call
            res[label]["est_rms_pos_m"] = float(np.sqrt(out["estimator"]["err_sq"][:, 0].mean() / T))
        if "diagnosis" in out:     # what was found: against the schedule's events where the loop has one, else every detection is false
            det = detections_of(*(out["diagnosis"][k] for k in ("step", "thruster", "level")))
            ev = [[] for _ in range(B)]
            if "faults" in extra:
                new = (f["ub"][:, 0] == 0) & (u > 0)
                ev = [[(int(f["onset"][b, 0]), int(i), -1) for i in np.flatnonzero(new[b])] for b in range(B)]
            sc = score(ev, det)
            delays = [d for d in sc.pop("delay") if d is not None]
            sc.pop("wrong_level")      # (the events stick at a random intensity: no level is the right one)
            res[label].update(detections=int(sum(len(d) for d in det)), score=sc,
                              delay_mean=float(np.mean(delays)) if delays else None, delay_max=int(max(delays)) if delays else None)
            if "no_hull" in out["diagnosis"]:
                res[label]["no_hull"] = int((out["diagnosis"]["no_hull"] >= 0).sum())
        if "actuator" in out:      # what the valves delivered and how often they opened, per vehicle and step
            res[label].update(delivered_mean_Ns=float(out["actuator"]["delivered"].mean()),
                              pulses_per_step=float(out["actuator"]["pulses"].mean()) / T)
    mpc.close()
    res["ratio_with_over_without"] = res["with"]["steps_per_s"] / res["without"]["steps_per_s"]
    if outcomes:
        res["ratio_outcomes_over_with"] = res["with_outcomes"]["steps_per_s"] / res["with"]["steps_per_s"]
        res["history_bytes"] = T * B * (13 + c["NT"]) * 8
        res["outcome_bytes"] = B * (8 * 8 + 5 * 4)
    if dispersion:
        res["ratio_dispersed_over_without"] = res["without_dispersed"]["steps_per_s"] / res["without"]["steps_per_s"]
        res["ratio_dispersed_over_with"] = res["with_dispersed"]["steps_per_s"] / res["with"]["steps_per_s"]
        res["plant_model_bytes"] = int(sum(a.nbytes for a in plant.values()))
    for label, _, _ in sensors:
        res[f"ratio_{label}_over_without"] = res["without_" + label]["steps_per_s"] / res["without"]["steps_per_s"]
        res[f"ratio_{label}_over_with"] = res["with_" + label]["steps_per_s"] / res["with"]["steps_per_s"]
        if est is not None:      # the same loop with the filter against without
            for w in ("without_", "with_"):
                res[f"ratio_{label}_estimator_over_{w}{label}"] = res[w + label + "_estimator"]["steps_per_s"] / res[w + label]["steps_per_s"]
                res[f"ms_per_step_estimator_{w}{label}"] = (res[w + label + "_estimator"]["ms"] - res[w + label]["ms"]) / T
            res["every"] = every
        if with_diag(dict(predict="_predict" in label)):      # the same loop with the diagnosis against without
            e = "_estimator" if est is not None else ""
            for w in ("without_", "with_"):
                res[f"ratio_{label}{e}_diagnosis_over_{w}{label}{e}"] = res[w + label + e + "_diagnosis"]["steps_per_s"] / res[w + label + e]["steps_per_s"]
                res[f"ms_per_call_diagnosis_{w}{label}{e}"] = res[w + label + e + "_diagnosis"]["ms"] - res[w + label + e]["ms"]
                res[f"ms_per_step_diagnosis_{w}{label}{e}"] = (res[w + label + e + "_diagnosis"]["ms"] - res[w + label + e]["ms"]) / T
            res["every"] = every
    if actuator:
        res["ratio_actuator_over_without"] = res["without_actuator"]["steps_per_s"] / res["without"]["steps_per_s"]
        res["ratio_actuator_over_with"] = res["with_actuator"]["steps_per_s"] / res["with"]["steps_per_s"]
        res["substeps"] = substeps
    if with_mission:
        res["ratio_mission_hover_over_without"] = res["without_mission_hover"]["steps_per_s"] / res["without"]["steps_per_s"]
        res["ratio_mission_hover_over_with"] = res["with_mission_hover"]["steps_per_s"] / res["with"]["steps_per_s"]
        res["ratio_mission_over_without"] = res["without_mission"]["steps_per_s"] / res["without"]["steps_per_s"]
        res["ratio_mission_over_with"] = res["with_mission"]["steps_per_s"] / res["with"]["steps_per_s"]
        res["ratio_mission_cost_over_with"] = res["with_mission_cost"]["steps_per_s"] / res["with"]["steps_per_s"]
        res["window_bytes"] = B * 15 * (c["N"] + 1) * 8
    res.update(case=name, B=B, T=T, slots=slots, **{k: c[k] for k in ("N", "NT", "dtype", "formulation")})
    return res


def stats(path):
    """Share of ftmpc_fault_event_kernel in the total kernel time of a rocprofv3 --stats kernel_stats.csv."""
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    ev = [r for r in rows if "ftmpc_fault_event_kernel" in r["Name"]]
    evt = sum(float(r["TotalDurationNs"]) for r in ev)
    calls = sum(int(r["Calls"]) for r in ev)
    oc = [r for r in rows if "ftmpc_outcome_kernel" in r["Name"]]
    oct_ = sum(float(r["TotalDurationNs"]) for r in oc)
    ocalls = sum(int(r["Calls"]) for r in oc)
    def per_launch(kernel):      # "name(" so that ftmpc_plant_step_kernel does not also count ftmpc_plant_step_var_kernel
        k = [r for r in rows if kernel + "(" in r["Name"]]
        n = sum(int(r["Calls"]) for r in k)
        return n, (sum(float(r["TotalDurationNs"]) for r in k) / n * 1e-3) if n else 0.0
    pn, pus = per_launch("ftmpc_plant_step_kernel")
    vn, vus = per_launch("ftmpc_plant_step_var_kernel")
    an, aus = per_launch("ftmpc_plant_step_act_kernel")
    sn, sus = per_launch("ftmpc_sense_kernel")
    f0n, f0us = per_launch("ftmpc_filter_kernel<0>")
    f1n, f1us = per_launch("ftmpc_filter_kernel<1>")
    d0n, d0us = per_launch("ftmpc_diagnose_kernel<0>")
    d1n, d1us = per_launch("ftmpc_diagnose_kernel<1>")
    rn, rus = per_launch("ftmpc_diagnose_repair_kernel")
    hon, hous = per_launch("ftmpc_hull_offsets_kernel")
    hsn, hsus = per_launch("ftmpc_hull_switch_kernel")
    return dict(hull_offsets_kernel_calls=hon, hull_offsets_kernel_avg_us=hous, hull_switch_kernel_calls=hsn, hull_switch_kernel_avg_us=hsus,
                hull_kernel_share=(hon * hous + hsn * hsus) * 1e3 / tot if tot else 0.0,
                diagnose_test_kernel_calls=d0n, diagnose_test_kernel_avg_us=d0us, diagnose_model_kernel_calls=d1n, diagnose_model_kernel_avg_us=d1us,
                diagnose_repair_kernel_calls=rn, diagnose_repair_kernel_avg_us=rus,
                diagnose_kernel_share=(d0n * d0us + d1n * d1us + rn * rus) * 1e3 / tot if tot else 0.0,
                filter_update_kernel_calls=f0n, filter_update_kernel_avg_us=f0us, filter_time_kernel_calls=f1n, filter_time_kernel_avg_us=f1us,
                filter_kernel_share=(f0n * f0us + f1n * f1us) * 1e3 / tot if tot else 0.0,
                sense_kernel_calls=sn, sense_kernel_avg_us=sus, sense_kernel_share=sn * sus * 1e3 / tot if tot else 0.0,
                plant_act_kernel_calls=an, plant_act_kernel_avg_us=aus, plant_act_kernel_share=an * aus * 1e3 / tot if tot else 0.0,
                plant_kernel_calls=pn, plant_kernel_avg_us=pus, plant_var_kernel_calls=vn, plant_var_kernel_avg_us=vus,
                total_kernel_ms=tot * 1e-6, event_kernel_ms=evt * 1e-6, event_kernel_calls=calls,
                event_kernel_avg_us=(evt / calls * 1e-3) if calls else 0.0, event_kernel_share=evt / tot if tot else 0.0,
                outcome_kernel_ms=oct_ * 1e-6, outcome_kernel_calls=ocalls, outcome_kernel_avg_us=(oct_ / ocalls * 1e-3) if ocalls else 0.0,
                outcome_kernel_share=oct_ / tot if tot else 0.0)


def trace(path):
    """Time per launch of the mission kernels and of the linearise kernel with and without windows, from the kernel_trace.csv of a
    `--once --mission` run (the call with the mission comes first)."""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
    last_win = max((i for i, r in enumerate(rows) if "ftmpc_ref_window_kernel" in r["Kernel_Name"]), default=-1)
    split = next((i for i in range(last_win + 1, len(rows)) if "ftmpc_plant_step_kernel" in rows[i]["Kernel_Name"]), len(rows))
    out = {}
    for key, name, sel in (("ref_window", "ftmpc_ref_window_kernel", rows), ("outcome_mission", "ftmpc_outcome_mission_kernel", rows),
                           ("linearize_windows", "ftmpc_linearize_kernel", rows[:split + 1]),
                           ("linearize_shared", "ftmpc_linearize_kernel", rows[split + 1:])):
        d = [dur(r) for r in sel if name in r["Kernel_Name"]]
        out[key + "_calls"], out[key + "_avg_us"] = len(d), float(np.mean(d)) if d else 0.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=["all"] + list(CASES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--stats", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--outcomes", action="store_true")
    ap.add_argument("--slots", type=int, default=0)
    ap.add_argument("--dispersion", action="store_true")
    ap.add_argument("--mission", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--actuator", action="store_true")
    ap.add_argument("--substeps", type=int, default=16)
    ap.add_argument("--sensor", action="store_true")
    ap.add_argument("--latency", type=int, nargs="+", default=[2])
    ap.add_argument("--predict", action="store_true")
    ap.add_argument("--estimator", action="store_true")
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--diagnosis", action="store_true")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(stats(a.stats)))
        return
    if a.trace:
        print(json.dumps(trace(a.trace)))
        return
    names = list(CASES) if a.case == "all" else [a.case]
    out = []
    for n in names:
        r = run(n, a.reps, a.once, a.outcomes, a.slots, a.dispersion, a.mission, a.actuator, a.substeps, a.sensor, tuple(a.latency), a.predict,
                a.estimator, a.every, a.diagnosis)
        if r is not None:
            print(json.dumps(r))
            out.append(r)
    if a.json and out:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
