"""GPU: probe pulses for silent faults and the withdrawal of a detection in the on-device closed loop (ftmpc_probe_kernel<0>, <1>,
ftmpc_diagnose_probe_kernel; ftmpc_simulate_probe_batch, ftmpc_simulate_wrench_probe_batch; BatchedMPC.simulate(probe=...)).

The references are ft_mpc_amd/probes.py (step, replay) and ft_mpc_amd/diagnosis.py (replay with probe=); tests/test_probes_host.py
checks both on the CPU against csrc/ftmpc_probe.h, the functions the kernels are made of.

Setting: N = 10, 8 thrusters, B <= 96, T <= 30, a float64 handle, a trivial sensor, no process and no sensor noise; diagnosis every 1,
levels (0, 1.7, 3.4) N, threshold 18, resid_sigma (1e-3, 1e-3), no drift; probe amp 0.5 N, quiet 0.05 N, idle_steps 3.  From
diagnosis.signature (m = 16.8 kg, J = diag(0.2, 0.3, 0.25), dt = 0.1 s): one 0.5 N pulse on a dead thruster adds at least 60.9 to its
statistic on the worst of the eight thrusters, 3.4 x the threshold; the best competing level hypothesis reaches at most 0.6 of it; the
signature's first-order error is 2.7 %.  One pulse decides, and no tolerance is tuned.

A  replay of the probe step, both formulations and latency 2; B  NULL and a probe that never fires give the isolation entry's bits;
C  a silent fault is found; D  a false detection is withdrawn, a true one is not, the wrench form's hull offsets follow;
E  health and llr_hist against the replay; F  a continued run; G  refusals at the ABI."""
import ctypes as C

import numpy as np
import pytest

from ft_mpc_amd import _lib
from ft_mpc_amd import diagnosis as DG
from ft_mpc_amd import probes as PR
from oracle import qp_oracle as qo
from test_gpu_actuators import _entry, _same_bits
from test_gpu_diagnosis import BOUND, F_MAX, LEVELS, ZERO, _meas, _on_orbit, _shift
from test_gpu_outcomes import _hover

pytestmark = pytest.mark.gpu
N, NT = 10, 8
PROBE = dict(amp=0.5, quiet=0.05, idle_steps=3)
PALL = ("thruster_hist", "idle", "pulses", "impulse", "pacc", "health", "reinstated")
DALL = ("detect", "pattern", "llr_hist", "state")
DKEYS = ("step", "thruster", "level", "ub", "stuck", "llr_hist", "state", "llr")
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)


def _dspec(**kw):
    return dict(dict(every=1, levels=LEVELS, resid_sigma=(1e-3, 1e-3), drift_sigma=(0.0, 0.0), threshold=18.0, max_detect=4, fields=DALL),
                **kw)


@pytest.fixture(scope="module")
def probe_mpc(gpu_mpc_factory):
    """one float64 handle (N = 10, 8 thrusters) for the whole file"""
    return gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60)


def _sim(mpc, x0, ub, stuck, T, dg, wrench=False, sensor=None, xr=None, **kw):
    if wrench:
        dg = dict(dg, rebuild_hull=True)
        kw["formulation"] = "wrench"
    return mpc.simulate(x0, ub, stuck, _hover(N, T) if xr is None else xr, T, noise=ZERO, seed=5, return_inputs=True, return_states=True,
                        sensor=sensor, diagnosis=dg, **kw)


def _dets(out):
    do = out["diagnosis"]
    return DG.detections_of(do["step"], do["thruster"], do["level"])


# ---------------------------------------------------------------------------------------------------------------------------
# (A) the probe step, replayed from the run's own commands
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrench,latency", [(False, 0), (True, 0), (False, 2)])
def test_replay_of_the_probe_step(probe_mpc, wrench, latency):
    """65 healthy vehicles, T = 30, max_pulses 2; every third vehicle starts with one thruster off that is in no list (not probeable).
    probes.replay reproduces thruster_hist, idle and pulses exactly from u_hist (with latency 2: u_hist from row 2 on, then the
    sensor's pending commands) and the pattern, which does not move (no detection, asserted).  impulse: each pulse is
    ((u + amp) - u) dt on the device and (a - (a - amp)) dt in the replay, two roundings of relative 2^-53 each on values below
    amp + quiet, and the running sum rounds once per pulse: bound 4 P 2^-53 max(impulse) with P <= T pulses, 6.7e-15 N s at the
    largest impulse of 0.5 N s.  MEASURED on an MI355X, largest |impulse - replay|: 0 N s on the thruster form, on the wrench form
    and with latency 2 (the idle commands are exact zeros, so every pulse is exactly amp dt on both sides); 7.85, 7.60 and 7.97
    pulses per vehicle, every vehicle with a thruster at the cap."""
    B, T = 65, 30
    mpc = probe_mpc
    x0 = _on_orbit(B, 41)
    ub, stuck = np.full((B, NT), F_MAX), np.zeros((B, NT))
    off = np.arange(0, B, 3)
    ub[off, off % NT] = 0.0
    probe = dict(PROBE, max_pulses=2, fields=PALL[:4])
    sen = dict(latency=latency, fields=("pending",)) if latency else None
    out = _sim(mpc, x0, ub, stuck, T, _dspec(), wrench=wrench, sensor=sen, probe=probe)
    po = out["probe"]
    assert sorted(po) == sorted(PALL[:4]) and po["thruster_hist"].shape == (T, B) and po["thruster_hist"].dtype == np.int32
    assert all(not d for d in _dets(out)) and np.array_equal(out["diagnosis"]["ub"], ub)
    cmd = out["u"] if not latency else np.concatenate([out["u"][latency:], out["sensor"]["pending"].transpose(1, 0, 2)])
    worst, npulse = 0.0, 0
    for b in range(B):
        r = PR.replay(cmd[:, b], po["thruster_hist"][:, b], np.tile(ub[b], (T, 1)), None, probe, mpc.cfg.dt)
        assert np.array_equal(r["thruster_hist"], po["thruster_hist"][:, b]), (b, r["thruster_hist"], po["thruster_hist"][:, b])
        assert np.array_equal(r["idle"], po["idle"][b]) and np.array_equal(r["pulses"], po["pulses"][b]), b
        worst = max(worst, abs(r["impulse"] - po["impulse"][b]))
        npulse += int((po["thruster_hist"][:, b] >= 0).sum())
    bound = 4 * T * 2.0 ** -53 * float(po["impulse"].max())
    print(f"probe replay (wrench {wrench}, latency {latency}): {npulse / B:.2f} pulses per vehicle, largest |impulse - replay| "
          f"{worst:.3e} N s, bound {bound:.3e}, largest impulse {po['impulse'].max():.3f} N s")
    assert worst <= bound
    assert po["pulses"].max() == 2 and npulse > B                      # the cap is reached, and it is what ends the pulses
    assert (po["thruster_hist"][:, off] != (off % NT)[None]).all()     # a thruster that is off and in no list is never pulsed
    assert (po["pulses"].sum(axis=1) == (po["thruster_hist"] >= 0).sum(axis=0)).all()
    # the pulse is in the command the plant applied
    t, b = np.argwhere(po["thruster_hist"] >= 0)[0]
    assert cmd[t, b, po["thruster_hist"][t, b]] >= PROBE["amp"]


# ---------------------------------------------------------------------------------------------------------------------------
# (B) NULL and a probe that never fires
# ---------------------------------------------------------------------------------------------------------------------------
def test_null_and_a_probe_that_never_fires_give_the_bits_of_the_isolation_entry(probe_mpc):
    B, T = 96, 8
    mpc = probe_mpc
    x0, ub, stuck = qo.make_batch(B, N, NT, 1, 16)[:3]
    iso = dict(consist=DG.consist_for(0.999), persist=2, revise=True, fields=("lead", "voided", "revised", "fit"))
    dg = _dspec(resid_sigma=(1e-2, 1e-2))
    ref = _sim(mpc, x0, ub, stuck, T, dg, isolation=iso)
    out = _sim(mpc, x0, ub, stuck, T, dg, isolation=iso, probe=dict(PROBE, idle_steps=T + 1, reinstate=False, fields=PALL[:4]))
    for k in ("u", "x_hist", "x"):
        assert np.array_equal(out[k], ref[k]), k
    for k in DKEYS:
        assert np.array_equal(out["diagnosis"][k], ref["diagnosis"][k]), k
    for k in iso["fields"]:
        assert np.array_equal(out["isolation"][k], ref["isolation"][k]), k
    assert (out["probe"]["thruster_hist"] == -1).all() and not out["probe"]["pulses"].any() and not out["probe"]["impulse"].any()
    assert 0 < out["probe"]["idle"].max() <= T
    # through the C entries: NULL against the _isolation_ entry, with a diagnosis and a rule in the call
    dgs = _lib.ftmpc_diagnosis(struct_size=C.sizeof(_lib.ftmpc_diagnosis), every=1, n_levels=2, max_detect=2, threshold=18.0)
    dgs.levels[0], dgs.levels[1] = 0.0, F_MAX
    dgs.resid_sigma[0] = dgs.resid_sigma[1] = 1e-2
    rule = _lib.ftmpc_isolation(struct_size=C.sizeof(_lib.ftmpc_isolation), consist=4.7, persist=2, revise=1)
    tail = (None,) * 5 + (C.byref(dgs),) + (None,) * 4 + (C.byref(rule),)
    rc, err, a = _entry(mpc, "isolation_batch", x0, ub, stuck, N, 4, 7, tail)
    assert rc == 0, err
    rc, err, b = _entry(mpc, "probe_batch", x0, ub, stuck, N, 4, 7, tail + (None,))
    assert rc == 0, err
    _same_bits(b, a)


# ---------------------------------------------------------------------------------------------------------------------------
# (C) a silent fault is found
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_silent_fault_is_found(probe_mpc):
    """96 vehicles on the hover orbit, T = 30.  Per vehicle the thruster with the smallest summed command in a fault-free run of
    the same call dies in the plant at step 2 (the schedule moves the plant only).  With the probe every vehicle whose
    thruster_hist shows a pulse on its dead thruster from step 2 on has that thruster detected at level 0 at the next test; at
    most B / 8 vehicles may go without such a pulse.  Without the probe, on the same seeds, no more of those vehicles find it.
    MEASURED on an MI355X: 96 of 96 vehicles are pulsed on their dead thruster (first at steps 2 to 4) and detect it at the next
    test; without the probe 0 of those 96 detect it within the 30 steps."""
    B, T = 96, 30
    mpc = probe_mpc
    x0 = _on_orbit(B, 43)
    ub, stuck = np.full((B, NT), F_MAX), np.zeros((B, NT))
    dg = _dspec()
    pre = _sim(mpc, x0, ub, stuck, T, dg)
    assert all(not d for d in _dets(pre))
    dead = np.argmin(pre["u"].sum(axis=0), axis=1)
    eub = ub[:, None].copy()
    eub[np.arange(B), 0, dead] = 0.0
    faults = dict(onset=np.full((B, 1), 2, np.int32), ub=eub, stuck=np.zeros((B, 1, NT)))
    out = _sim(mpc, x0, ub, stuck, T, dg, faults=faults, probe=dict(PROBE, fields=PALL[:4]))
    ctl = _sim(mpc, x0, ub, stuck, T, dg, faults=faults)
    th = out["probe"]["thruster_hist"]
    det, cdet = _dets(out), _dets(ctl)
    pulsed, first, found, found_ctl = [], [], 0, 0
    for b in range(B):
        ts = [t for t in range(2, T - 1) if th[t, b] == dead[b]]
        if not ts:
            continue
        pulsed.append(b)
        first.append(ts[0])
        assert (ts[0] + 1, dead[b], 0) in det[b], (b, dead[b], ts[0], det[b])
        found += 1
        found_ctl += int(any(d[1] == dead[b] and d[2] == 0 for d in cdet[b]))
    print(f"silent fault: {len(pulsed)} of {B} vehicles pulsed on their dead thruster (first at steps {min(first)} to {max(first)}), "
          f"{found} detect it at the next test; without the probe {found_ctl} of them detect it within {T} steps")
    assert len(pulsed) >= 1 and B - len(pulsed) <= B // 8
    assert found >= found_ctl


# ---------------------------------------------------------------------------------------------------------------------------
# (D) a false detection is withdrawn, (E) the statistics against the replay
# ---------------------------------------------------------------------------------------------------------------------------
def _listed_three(B, x0):
    """every vehicle starts with thruster 3 listed at level 0 (ub_c,3 = 0, the entry (0, 3, 0), a state anchored on x0); a schedule
    event at step 0 gives the plant of the first half the healthy pattern and leaves thruster 3 of the second half dead"""
    ub, stuck = np.full((B, NT), F_MAX), np.zeros((B, NT))
    ub[:, 3] = 0.0
    eub = np.full((B, 1, NT), F_MAX)
    eub[B // 2:, 0, 3] = 0.0
    faults = dict(onset=np.zeros((B, 1), np.int32), ub=eub, stuck=np.zeros((B, 1, NT)))
    det = tuple(np.full((B, 4), -1, np.int32) for _ in range(3))
    det[0][:, 0], det[1][:, 0], det[2][:, 0] = 0, 3, 0
    state = np.zeros((B, 14 + NT))
    state[:, 0:13] = x0
    return ub, stuck, faults, det, state


def _check_withdrawn(out, B, wrench):
    po, do = out["probe"], out["diagnosis"]
    th, det = po["thruster_hist"], _dets(out)
    steps = []
    for b in range(B // 2):
        t0 = int(np.flatnonzero(th[:, b] == 3)[0])
        assert det[b][:2] == [(0, 3, 0), (t0 + 1, 3, len(LEVELS))], (b, t0, det[b])
        assert do["ub"][b, 3] == F_MAX and do["stuck"][b, 3] == 0.0 and po["reinstated"][b] == 1, b
        steps.append(t0 + 1)
    for b in range(B // 2, B):
        assert po["reinstated"][b] == 0 and po["health"][b, 3] == 0.0 and do["ub"][b, 3] == 0.0, b
        assert all(d[2] < len(LEVELS) for d in det[b]) and (th[:, b] == 3).any(), (b, det[b])
    used = int((out["u"][:, :B // 2, 3] > PROBE["amp"] + PROBE["quiet"]).any(axis=0).sum())
    print(f"withdrawn (wrench {wrench}): reinstated at steps {min(steps)} to {max(steps)} on {B // 2} of {B // 2}; {used} of them "
          f"command thruster 3 above a pulse afterwards; none of the {B - B // 2} dead ones is reinstated")
    return steps


@pytest.mark.parametrize("wrench", [False, True])
def test_a_false_detection_is_withdrawn_and_a_true_one_is_not(probe_mpc, wrench):
    """64 vehicles, T = 20, reinstate with restore_ub = f_max.  First half: the entry (c, 3, n_levels) at the first test after the
    first pulse on thruster 3, ub_c,3 = f_max, reinstated = 1.  Second half: never reinstated, health[3] stays 0.  On the wrench
    form the returned hull offsets of every vehicle are ftmpc_hull_offsets_batch of its final pattern on the healthy layout's
    tables (the call starts from the offsets of the listed pattern on those tables).
    (E) llr_hist and the returned llr, health and pacc against diagnosis.replay(probe=...) of the run's own measurements and
    commands within BOUND = 2.8e-11 of max(1, |value|), the bound tests/test_gpu_isolation.py holds llr_hist to; detections,
    reinstated and the final pattern identical.
    On the thruster form the run is repeated with a threshold out of reach, where nothing is decided and the returned health holds
    every pulse's increment.
    MEASURED on an MI355X: reinstated at step 4 on 32 of 32 (thruster form), at steps 3 to 4 on 32 of 32 (wrench form), none of
    the 32 dead ones; llr_hist within 1.3e-13 of max(1, |value|), health within 9.2e-16 (of values near 2 493: six pulses), pacc
    exact, the returned state within 2.3e-16 (thruster form); llr_hist within 3.2e-14 on the wrench form."""
    from ft_mpc_amd.controllers.tools.input_bounds import hull_tables
    B, T = 64, 20
    mpc = probe_mpc
    x0 = _on_orbit(B, 45)
    ub, stuck, faults, det0, state = _listed_three(B, x0)
    dg = _dspec(state=state, detect=det0)
    probe = dict(PROBE, reinstate=True, restore_ub=F_MAX, fields=PALL)
    kw = {}
    if wrench:
        hull = hull_tables(mpc.D, np.full((B, NT), F_MAX), np.zeros((B, NT)))
        start = mpc.hull_offsets(ub, stuck, hull)
        assert not start["flat"].any()
        dg, kw = dict(dg, hull_b=start["b"]), dict(hull=hull)
    out = _sim(mpc, x0, ub, stuck, T, dg, wrench=wrench, faults=faults, probe=probe, **kw)
    _check_withdrawn(out, B, wrench)
    do, po = out["diagnosis"], out["probe"]
    if wrench:
        assert (do["no_hull"] == -1).all()
        dev = mpc.hull_offsets(do["ub"], do["stuck"], hull)
        assert not dev["flat"].any() and np.array_equal(do["hull_b"], dev["b"])
        assert not np.array_equal(do["hull_b"][:B // 2], start["b"][:B // 2]) and np.array_equal(do["hull_b"][B // 2:], start["b"][B // 2:])
    # (E)
    meas = _meas(out, x0)
    got = _dets(out)
    rel = lambda a, b: float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())
    dev = dict(llr_hist=0.0, llr=0.0, health=0.0, pacc=0.0, state=0.0)
    plain = {k: v for k, v in dg.items() if k not in ("hull_b", "rebuild_hull")}
    for b in range(B):
        r = DG.replay(meas[:, b], out["u"][:, b], ub[b], stuck[b], plain, mpc.cfg, state=state[b], detections=DG.detections_of(*det0)[b],
                      probe=probe)
        assert got[b] == r["detections"], (b, got[b], r["detections"])
        assert po["reinstated"][b] == r["reinstated"] and np.array_equal(do["ub"][b], r["ub_end"]) and np.array_equal(do["stuck"][b], r["stuck_end"])
        dev["llr_hist"] = max(dev["llr_hist"], rel(do["llr_hist"][:, b], r["llr_hist"]))
        dev["llr"] = max(dev["llr"], rel(do["llr"][b], r["llr"]))
        dev["health"] = max(dev["health"], rel(po["health"][b], r["health"]))
        dev["pacc"] = max(dev["pacc"], rel(po["pacc"][b], r["pacc"]))
        dev["state"] = max(dev["state"], float(np.abs(do["state"][b] - r["state"]).max()))
        if b < B // 2:      # the healthy hypothesis was what crossed the threshold, by the margin the module's docstring states
            t1 = r["detections"][1][0]
            assert r["health_hist"][t1, 3] >= 60.9 * (1 - 2 * 0.027) and r["llr_hist"][t1].max() <= 0.6 * r["health_hist"][t1, 3]
    if not wrench:      # with a threshold out of reach nothing is decided and the returned health holds every pulse's increment
        far = dict(plain, threshold=1e6)
        hi = _sim(mpc, x0, ub, stuck, T, far, faults=faults, probe=probe)
        for b in range(B):
            r = DG.replay(_meas(hi, x0)[:, b], hi["u"][:, b], ub[b], stuck[b], far, mpc.cfg, state=state[b],
                          detections=DG.detections_of(*det0)[b], probe=probe)
            dev["health"] = max(dev["health"], rel(hi["probe"]["health"][b], r["health"]))
            dev["llr_hist"] = max(dev["llr_hist"], rel(hi["diagnosis"]["llr_hist"][:, b], r["llr_hist"]))
        hh = hi["probe"]["health"]
        assert (hh[:B // 2, 3] > 60.9).all() and (hh[B // 2:] == 0).all() and (np.delete(hh, 3, axis=1) == 0).all()
        print(f"undecided run: health[3] of the healthy half {hh[:B // 2, 3].min():.1f} to {hh[:B // 2, 3].max():.1f}")
    print(f"probe statistics (wrench {wrench}): max deviation (device - definition): " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    for k, v in dev.items():
        assert v <= BOUND, (k, v)


# ---------------------------------------------------------------------------------------------------------------------------
# (F) a continued run
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_continued_run_is_the_whole_run(probe_mpc):
    """T = 24 against 12 + 12 with the diagnosis' state, llr, detect arrays and returned pattern, the isolation's lead and counters,
    the probe's idle, pulses, impulse, pacc, health and reinstated, step0 = 12 and the shifted schedule handed over: every output
    bit for bit.  persist 2 and max_pulses 4, so that leaders, caps and counters cross the seam; the plant of every fourth vehicle
    turns healthy at step 13 only, so that its reinstatement lies behind the seam."""
    B = 64
    mpc = probe_mpc
    x0 = _on_orbit(B, 47)
    ub, stuck, faults, det0, state = _listed_three(B, x0)
    faults = dict(faults, onset=np.where(np.arange(B)[:, None] % 4 == 1, 13, 0).astype(np.int32))      # (some plants switch after the seam)
    dg = _dspec(state=state, detect=det0)
    iso = dict(persist=2, revise=True, fields=("lead", "voided", "revised", "fit"))
    probe = dict(PROBE, reinstate=True, restore_ub=F_MAX, max_pulses=4, fields=PALL)
    xr = _hover(N, 24)
    sen = dict(fields=("meas",))
    whole = _sim(mpc, x0, ub, stuck, 24, dg, xr=xr, sensor=sen, faults=faults, isolation=iso, probe=probe)
    first = _sim(mpc, x0, ub, stuck, 12, dg, xr=xr[:, :12 + N], sensor=sen, faults=faults, isolation=iso, probe=probe)
    d1, i1, p1 = first["diagnosis"], first["isolation"], first["probe"]
    dg2 = dict(dg, state=d1["state"], llr=d1["llr"], detect=(d1["step"], d1["thruster"], d1["level"]))
    iso2 = dict(iso, lead=i1["lead"], voided=i1["voided"], revised=i1["revised"])
    probe2 = dict(probe, **{k: p1[k] for k in PALL[1:]})
    second = _sim(mpc, first["x"], d1["ub"], d1["stuck"], 12, dg2, xr=xr[:, 12:], sensor=dict(sen, step0=12), faults=_shift(faults, 12),
                  isolation=iso2, probe=probe2)
    d2, dw, p2, pw = second["diagnosis"], whole["diagnosis"], second["probe"], whole["probe"]
    assert np.array_equal(second["x"], whole["x"])
    for k in ("x_hist", "u"):
        assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    assert np.array_equal(np.concatenate([d1["llr_hist"], d2["llr_hist"]]), dw["llr_hist"])
    assert np.array_equal(np.concatenate([p1["thruster_hist"], p2["thruster_hist"]]), pw["thruster_hist"])
    assert np.array_equal(np.concatenate([i1["fit"], second["isolation"]["fit"]]), whole["isolation"]["fit"])
    for k in ("step", "thruster", "level", "state", "llr", "ub", "stuck"):
        assert np.array_equal(d2[k], dw[k]), k
    for k in ("lead", "voided", "revised"):
        assert np.array_equal(second["isolation"][k], whole["isolation"][k]), k
    for k in PALL[1:]:
        assert np.array_equal(p2[k], pw[k]), k
    # both sides of the seam hold reinstatements and pulses, the cap binds, and the handed arrays were not written into
    assert (p1["reinstated"] > 0).any() and (pw["reinstated"] > p1["reinstated"]).any()
    assert (p1["thruster_hist"] >= 0).any() and (p2["thruster_hist"] >= 0).any() and pw["pulses"].max() == 4
    assert np.array_equal(probe2["pulses"], p1["pulses"]) and not np.array_equal(p2["pulses"], p1["pulses"])


# ---------------------------------------------------------------------------------------------------------------------------
# (G) refusals at the ABI
# ---------------------------------------------------------------------------------------------------------------------------
def _bad_probes(B):
    """(field named in the message, offending vehicle or None, the call has a diagnosis, it has a state, the struct, what to keep)"""
    def pb(**kw):
        return _lib.ftmpc_probe(**dict(dict(struct_size=C.sizeof(_lib.ftmpc_probe), amp=0.5, quiet=0.05, idle_steps=3), **kw))
    yield "struct_size", None, True, False, pb(struct_size=96), None
    yield "reserved", None, True, False, pb(reserved=1), None
    yield None, None, False, False, pb(), None
    for amp in (0.0, -1.0, np.inf, np.nan):
        yield "amp", None, True, False, pb(amp=amp), None
    for quiet in (-0.01, 0.5, 0.7, np.nan):
        yield "quiet", None, True, False, pb(quiet=quiet), None
    yield "idle_steps", None, True, False, pb(idle_steps=0), None
    yield "max_pulses", None, True, False, pb(max_pulses=-1), None
    yield "reinstate", None, True, False, pb(reinstate=2), None
    for rub in (0.0, -1.0, np.inf, np.nan):
        yield "restore_ub", None, True, False, pb(reinstate=1, restore_ub=rub), None
    for name, width in (("idle", NT), ("pulses", NT), ("reinstated", 1)):
        a = np.zeros((B, width), np.int32)
        a[7, width - 1] = -1
        yield name, 7, True, False, pb(**{name: a.ctypes.data_as(ip)}), a
    for name, width, state in (("impulse", 1, False), ("pacc", NT, True), ("health", NT, True)):
        for v in (-1.0, np.nan, np.inf):
            a = np.zeros((B, width))
            a[5, 0] = v
            yield name, 5, True, state, pb(**{name: a.ctypes.data_as(dp)}), a
    for name in ("pacc", "health"):
        a = np.zeros((B, NT))
        yield name, None, True, False, pb(**{name: a.ctypes.data_as(dp)}), a


def test_refusals(probe_mpc):
    B, T = 12, 2
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 0, 20)
    mpc = probe_mpc

    def diag(state, level=-1):
        s = _lib.ftmpc_diagnosis(struct_size=C.sizeof(_lib.ftmpc_diagnosis), every=1, n_levels=2, max_detect=2, threshold=18.0)
        s.levels[0], s.levels[1] = 0.0, F_MAX
        s.resid_sigma[0] = s.resid_sigma[1] = 1e-2
        keep = []
        if state:
            st = np.zeros((B, 14 + NT))
            st[:, 0:13] = x0
            det = [np.full((B, 2), -1, np.int32) for _ in range(3)]
            if level >= 0:
                det[0][4, 0], det[1][4, 0], det[2][4, 0] = 0, 3, level
            s.state = st.ctypes.data_as(dp)
            s.detect_step, s.detect_thruster, s.detect_level = (a.ctypes.data_as(ip) for a in det)
            keep = [st] + det
        return s, keep

    def call(name, dref, isoref, pref, wrench):
        tail = (None,) * 5 + (dref,) + (None,) * (6 if wrench else 4) + (isoref, pref)
        return _entry(mpc, name, x0, ub, stuck, N, T, 1, tail, want=False, wrench=wrench)

    n = 0
    for n, (field, v, need, state, pb, keep) in enumerate(_bad_probes(B)):
        dgs, dkeep = diag(state)
        for name, wrench in (("probe_batch", False), ("wrench_probe_batch", True)):      # (every refusal comes before the dummy hull is looked at)
            rc, err, out = call(name, C.byref(dgs) if need else None, None, C.byref(pb), wrench)
            assert rc == -1 and (f"ftmpc_probe.{field}" if field else "no diagnosis").encode() in err, (n, field, name, err)
            assert b"ftmpc_probe" in err
            if v is not None:
                assert f"vehicle {v} ".encode() in err, err
            assert np.array_equal(out["x"], x0)
    assert n >= 30
    # the two checks a reinstating probe widens, and only it: a carried level equal to n_levels, a leader H + i
    good = _lib.ftmpc_probe(struct_size=C.sizeof(_lib.ftmpc_probe), amp=0.5, quiet=0.05, idle_steps=3)
    rein = _lib.ftmpc_probe(struct_size=C.sizeof(_lib.ftmpc_probe), amp=0.5, quiet=0.05, idle_steps=3, reinstate=1, restore_ub=F_MAX)
    dgs, dkeep = diag(True, level=2)
    lead = np.zeros((B, 2), np.int32)
    lead[:, 0] = -1
    lead[9] = (2 * NT + 3, 1)
    rule = _lib.ftmpc_isolation(struct_size=C.sizeof(_lib.ftmpc_isolation), persist=2, lead=lead.ctypes.data_as(ip))
    for pref in (None, C.byref(good)):
        rc, err, out = call("probe_batch", C.byref(dgs), None, pref, False)
        assert rc == -1 and b"ftmpc_diagnosis.detect_level: vehicle 4 " in err and np.array_equal(out["x"], x0), err
    ok, okeep = diag(True)
    for pref in (None, C.byref(good)):
        rc, err, out = call("probe_batch", C.byref(ok), C.byref(rule), pref, False)
        assert rc == -1 and b"ftmpc_isolation.lead: vehicle 9 " in err and np.array_equal(out["x"], x0), err
    keep_lead = lead.copy()
    rc, err, out = call("probe_batch", C.byref(dgs), C.byref(rule), C.byref(rein), False)
    assert rc == 0, err
    assert not np.array_equal(out["x"], x0) and not np.array_equal(lead, keep_lead)      # (no leader after the first test: lead was written)
    lead[:] = keep_lead
    lead[9, 0] = 3 * NT
    rc, err, out = call("probe_batch", C.byref(dgs), C.byref(rule), C.byref(rein), False)
    assert rc == -1 and b"ftmpc_isolation.lead: vehicle 9 " in err, err
    # one good struct is accepted on both forms' front end, and what the front end refuses itself never reaches the library
    rc, err, out = call("probe_batch", C.byref(ok), None, C.byref(good), False)
    assert rc == 0 and not np.array_equal(out["x"], x0), err
    with pytest.raises(ValueError, match="quiet"):
        mpc.simulate(x0, ub, stuck, _hover(N, T), T, diagnosis=_dspec(), probe=dict(PROBE, quiet=0.5))
    with pytest.raises(ValueError, match="no diagnosis"):
        mpc.simulate(x0, ub, stuck, _hover(N, T), T, probe=PROBE)
