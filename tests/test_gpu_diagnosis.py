"""GPU: thruster fault diagnosis in the on-device closed loop (ftmpc_diagnose_kernel; ftmpc_simulate_diagnosis_batch,
ftmpc_multi_simulate_diagnosis_batch; BatchedMPC.simulate(diagnosis=...)).

The reference is ft_mpc_amd/diagnosis.py (tests/test_diagnosis_host.py checks it on the CPU: the signature against differences of RK4
steps, the false-alarm and detection behaviour on an open loop).  Every run is replayed per vehicle from its own histories: llr_hist,
the detections, the returned state, llr, ub and stuck from the device's meas_hist and applied commands and nothing else.

A  replay (every = 1 and 3); B  isolation; C  the switch is the schedule's switch; D  diagnosis = NULL gives the bits of the
_estimator_ entry; E  continued runs; F  slices and device slots; G  noisy closed loop; H  other loops; I  refusals.

BOUND: the deviation of the replay is round-off of a statistic of order one to a few hundred.  Measured on an MI355X, maxima over the
cases of (A) and (H): llr_hist and the returned llr within 2.8e-13 of max(1, |llr|) (the largest on the mission loop with every = 3;
(A) alone 2.1e-13), the returned state within 4.5e-16; BOUND is 100 x the largest of these, 2.8e-11, tighter than the 1e-9 it may in
no case exceed (a wrong sign or column moves a statistic by the order of the threshold).  The decisions are identical, and in no
replay does a test's largest statistic lie within 1e-6 of the threshold.  Also measured: (B) five of the eight dead thrusters are
commanded within the 16 steps and found (four at step 4, one at step 11); (G) every stuck-on vehicle is found one step after the
onset, the healthy third's largest statistic is 0.97, 16 of the 32 dead thrusters are found within 15 steps, no false alarm and no
wrong thruster; (A), B = 96: every = 1 finds 143 faults (3 with the wrong thruster, 4 with the wrong level, 49 not within the run,
no false alarm), every = 3 finds 154 with 30 wrong thrusters, 34 wrong levels and 2 false alarms -- a fault that starts inside a
window shows a part of its signature, and the stuck level 1.7 N lies between two hypotheses of the neighbouring thrusters."""
import ctypes as C

import numpy as np
import pytest

import ft_mpc_amd
from ft_mpc_amd import _lib
from ft_mpc_amd import diagnosis as DG
from ft_mpc_amd.sharding import MultiGPUMPC
from oracle import qp_oracle as qo
from test_diagnosis_host import STUCK_ON_MAX_DELAY
from test_gpu_actuators import _entry, _same_bits
from test_gpu_estimators import _prior, _sensor, _two_faults
from test_gpu_estimators import _spec as _est_spec
from test_gpu_missions import UT, XT
from test_gpu_outcomes import _hover
from test_gpu_plant_dispersion import _plant

pytestmark = pytest.mark.gpu
NOISE = (1e-3,) * 4
ZERO = (0.0,) * 4
SIGMA = (1e-2, 5e-3, 1e-2, 5e-3)
F_MAX = 3.4
BOUND = 2.8e-11
THRESHOLD = 18.0
LEVELS = (0.0, 1.7, F_MAX)
DALL = ("detect", "pattern", "llr_hist", "state")
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)


def _dspec(every=1, **kw):
    return dict(dict(every=every, levels=LEVELS, resid_sigma=DG.default_sigma(SIGMA, NOISE), drift_sigma=(0.0, 0.0), threshold=THRESHOLD,
                     max_detect=2, fields=DALL), **kw)


def _sim(mpc, x0, ub, stuck, N, T, sen, est, dg, seed=5, noise=NOISE, xr=None, **kw):
    L = sen.get("latency", 0) if sen is not None and sen.get("predict") else 0
    xr = _hover(N, T + L) if xr is None else xr
    return mpc.simulate(x0, ub, stuck, xr, T, noise=noise, seed=seed, return_inputs=True, return_states=True, sensor=sen, estimator=est,
                        diagnosis=dg, **kw)


def _on_orbit(B, seed):
    """States within 2 cm, 1 cm/s and 0.01 rad/s of the hover reference's orbit, the attitude random: the controller then holds
    four of the eight thrusters near 1.1 N and the others near 0, far from f_max.  (tests/test_gpu_diagnosis.py first drew the states
    of oracle.qp_oracle.make_batch, up to 2 m off: there one command in eight starts at f_max, and a thruster stuck on at f_max while
    it is commanded f_max has no signature -- the mirror image of the dead thruster that is not commanded.)"""
    from oracle import refmath as rm
    rng = np.random.default_rng(seed)
    r = rm.spiral_r()
    x = np.zeros((B, 13))
    q = rng.standard_normal((B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    for b in range(B):
        w = rm.OMEGA_DES + rng.uniform(-0.01, 0.01, 3)
        Rt = rm.rot(q[b]).T
        x[b, 0:3] = -Rt @ r + rng.uniform(-0.02, 0.02, 3)
        x[b, 3:6] = -Rt @ np.cross(w, r) + rng.uniform(-0.01, 0.01, 3)
        x[b, 6:10], x[b, 10:13] = q[b], w
    return x


def _meas(out, x0):
    so = out.get("sensor") or {}
    return so["meas"] if "meas" in so else np.concatenate([x0[None], out["x_hist"][:-1]])


def _check_replay(out, x0, ub, stuck, dg, cfg, step0=0, bound=BOUND, margin=1e-6):
    """llr_hist, the detections and the returned state, llr, ub, stuck of `out` against diagnosis.replay of its own meas_hist and
    applied commands; returns the deviations and the replays."""
    do = out["diagnosis"]
    T, B, NT = out["u"].shape
    meas = _meas(out, x0)
    dev = dict(llr_hist=0.0, llr=0.0, state=0.0)
    got = DG.detections_of(do["step"], do["thruster"], do["level"])
    reps = []
    for b in range(B):
        st = None if dg.get("state") is None else dg["state"][b]
        r = DG.replay(meas[:, b], out["u"][:, b], ub[b], stuck[b], dg, cfg, step0=step0, state=st,
                      llr=None if dg.get("llr") is None else dg["llr"][b],
                      detections=None if dg.get("detect") is None else DG.detections_of(*dg["detect"])[b])
        reps.append(r)
        tested = ~np.isnan(r["peak"])
        assert (np.abs(r["peak"][tested] - dg["threshold"]) > margin).all(), (b, r["peak"])
        dev["llr_hist"] = max(dev["llr_hist"], (np.abs(do["llr_hist"][:, b] - r["llr_hist"]) / np.maximum(1.0, np.abs(r["llr_hist"]))).max())
        dev["llr"] = max(dev["llr"], (np.abs(do["llr"][b] - r["llr"]) / np.maximum(1.0, np.abs(r["llr"]))).max())
        dev["state"] = max(dev["state"], np.abs(do["state"][b] - r["state"]).max())
        assert got[b] == r["detections"], (b, got[b], r["detections"])
        assert np.array_equal(do["ub"][b], r["ub_end"]) and np.array_equal(do["stuck"][b], r["stuck_end"]), b
    print("diagnosis replay: max deviation (device - definition): " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items())
          + f"; {sum(len(g) for g in got)} detections on {B} vehicles")
    for k, v in dev.items():
        assert v <= bound, (k, v)
    return dev, reps


def _events_of(faults, ub, stuck):
    """per vehicle the list of (onset, thruster, level number in LEVELS) the schedule's events add, in order"""
    B = ub.shape[0]
    out = []
    for b in range(B):
        pu, ev = ub[b], []
        for k in range(faults["onset"].shape[1]):
            if faults["onset"][b, k] < 0:
                continue
            for i in np.nonzero((faults["ub"][b, k] == 0) & (pu > 0))[0]:
                ev.append((int(faults["onset"][b, k]), int(i), LEVELS.index(float(faults["stuck"][b, k, i]))))
            pu = faults["ub"][b, k]
        out.append(ev)
    return out


def _check_switch(mpc, out, x0, ub, stuck, N, T, sen, est, faults, noise, **kw):
    """(C) the _estimator_ entry with the same schedule and detect set to the steps the diagnosis reported gives u, x_hist and est bit
    for bit for every vehicle whose detections are the schedule's events in order (right thruster, right level).  Returns how many."""
    do = out["diagnosis"]
    B = x0.shape[0]
    det = DG.detections_of(do["step"], do["thruster"], do["level"])
    ev = _events_of(faults, ub, stuck)
    E = faults["onset"].shape[1]
    delay = np.zeros((B, E), np.int64)
    right = np.zeros(B, bool)
    for b in range(B):
        ok = len(det[b]) <= len(ev[b]) and all(d[1:] == e[1:] and d[0] >= e[0] for d, e in zip(det[b], ev[b])) and len(ev[b]) <= E
        # one thruster per event here, so event k is detection k; an event never detected gets a detection step beyond the run
        ok = ok and all(sum(1 for e in ev[b] if e[0] == faults["onset"][b, k]) == 1 for k in range(E) if faults["onset"][b, k] >= 0)
        right[b] = ok
        if ok:
            for k in range(E):
                if faults["onset"][b, k] >= 0:
                    delay[b, k] = (det[b][k][0] if k < len(det[b]) else T + 1) - faults["onset"][b, k]
    ref = _sim(mpc, x0, ub, stuck, N, T, sen, est, None, noise=noise, faults=faults, detect_delay=delay, **kw)
    for k in ("u", "x_hist"):
        assert np.array_equal(out[k][:, right], ref[k][:, right]), k
    assert np.array_equal(out["estimator"]["est"][:, right], ref["estimator"]["est"][:, right])
    assert np.array_equal(out["x"][right], ref["x"][right])
    return int(right.sum())


# ---------------------------------------------------------------------------------------------------------------------------
# (A) replay from the run's own histories, and (C) on the vehicles whose isolation was right
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("B", [1, 65, 96])
def test_replay_from_the_runs_own_histories(gpu_mpc_factory, B, every):
    """Noise, a bias, latency 2 with the estimator predicting, a two-fault schedule (which moves the plant only), three levels.
    Measured on an MI355X: see BOUND in the module's docstring."""
    N, NT, T = 10, 8, 20
    bt = _two_faults(B, N)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = _sensor(B, NT)
    xh, cov = _prior(bt["x0"])
    est = _est_spec(every, xhat=xh, cov=cov, fields=("est",))
    dg = _dspec(every)
    out = _sim(mpc, bt["x0"], bt["ub"], bt["stuck"], N, T, sen, est, dg, faults=bt["faults"])
    assert sorted(out["diagnosis"]) == sorted(("step", "thruster", "level", "ub", "stuck", "llr_hist", "state", "llr"))
    _check_replay(out, bt["x0"], bt["ub"], bt["stuck"], dg, mpc.cfg)
    n = _check_switch(mpc, out, bt["x0"], bt["ub"], bt["stuck"], N, T, sen, est, bt["faults"], NOISE)
    sc = DG.score(_events_of(bt["faults"], bt["ub"], bt["stuck"]),
                  DG.detections_of(*(out["diagnosis"][k] for k in ("step", "thruster", "level"))))
    delays = [d for d in sc["delay"] if d is not None]
    print(f"B = {B}, every = {every}: {n} vehicles with the schedule's own switches; score {dict(sc, delay=None)}, "
          f"delay median {np.median(delays):.0f} max {max(delays)}")
    if B > 1:
        assert n > 0


# ---------------------------------------------------------------------------------------------------------------------------
# (B) isolation, and (C) on all of its vehicles
# ---------------------------------------------------------------------------------------------------------------------------
def test_isolation_without_noise(gpu_mpc_factory):
    """Zero noise, trivial sensor, B = 2 NT + 2 NT, the vehicles start on the reference's orbit (_on_orbit): vehicle b < NT has
    thruster b stuck on at f_max, NT <= b < 2 NT has thruster b - NT dead, both from step 3; the other 2 NT are healthy.
    resid_sigma = 1e-6.  Every stuck-on vehicle is detected at step 4 with the right thruster and level; a dead vehicle is detected
    only with the right thruster, and at exactly the step the replay names; the healthy ones have no detection.  Then (C): the
    schedule with detect = the reported steps gives the same bits."""
    N, NT, T = 10, 8, 16
    B = 4 * NT
    x0 = _on_orbit(B, 31)
    ub, stuck = np.full((B, NT), F_MAX), np.zeros((B, NT))
    onset = np.where(np.arange(B) < 2 * NT, 3, -1).astype(np.int32)[:, None]
    eub, est_ = ub[:, None].copy(), np.zeros((B, 1, NT))
    for b in range(2 * NT):
        eub[b, 0, b % NT] = 0.0
        est_[b, 0, b % NT] = F_MAX if b < NT else 0.0
    faults = dict(onset=onset, ub=eub, stuck=est_)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    est = _est_spec(1, fields=("est",))
    dg = _dspec(resid_sigma=(1e-6, 1e-6))
    out = _sim(mpc, x0, ub, stuck, N, T, None, est, dg, noise=ZERO, faults=faults)
    do = out["diagnosis"]
    det = DG.detections_of(do["step"], do["thruster"], do["level"])
    meas = _meas(out, x0)
    for b in range(B):
        r = DG.replay(meas[:, b], out["u"][:, b], ub[b], stuck[b], dg, mpc.cfg)
        assert det[b] == r["detections"], (b, det[b], r["detections"])
        if b < NT:
            assert det[b] == [(4, b, 2)], (b, det[b], "commands of the thruster:", out["u"][:, b, b])
            assert do["ub"][b, b] == 0.0 and do["stuck"][b, b] == F_MAX
        elif b < 2 * NT:
            assert all(d[1] == b - NT and d[2] == 0 for d in det[b]) and len(det[b]) <= 1, (b, det[b])
        else:
            assert det[b] == [] and np.array_equal(do["ub"][b], ub[b]) and np.array_equal(do["stuck"][b], stuck[b])
    found = sum(1 for b in range(NT, 2 * NT) if det[b])
    print(f"isolation: {found} of {NT} dead thrusters were commanded and found, steps {[det[b][0][0] for b in range(NT, 2 * NT) if det[b]]}")
    assert _check_switch(mpc, out, x0, ub, stuck, N, T, None, est, faults, ZERO) == B


# ---------------------------------------------------------------------------------------------------------------------------
# (D) diagnosis = NULL
# ---------------------------------------------------------------------------------------------------------------------------
def test_null_diagnosis_gives_the_bits_of_the_estimator_entry(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 96, 4
    x0, ub, stuck = qo.make_batch(B, N, NT, 1, 16)[:3]
    se = _lib.ftmpc_sensor(struct_size=C.sizeof(_lib.ftmpc_sensor), latency=2, predict=0, seed=9)
    es = _lib.ftmpc_estimator(struct_size=C.sizeof(_lib.ftmpc_estimator), every=1)
    for k in range(4):
        se.sigma[k] = es.p0[k] = es.meas_sigma[k] = SIGMA[k]
        es.proc_sigma[k] = 0.1 * SIGMA[k]
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f32"), devices=[0, 0, 0])
    try:
        for obj in (mpc, m):
            for s, e in ((None, None), (C.byref(se), C.byref(es))):
                rc, err, ref = _entry(obj, "estimator_batch", x0, ub, stuck, N, T, 7, (None, None, None, s, e))
                assert rc == 0, err
                rc, err, out = _entry(obj, "diagnosis_batch", x0, ub, stuck, N, T, 7, (None, None, None, s, e, None))
                assert rc == 0, err
                _same_bits(out, ref)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (E) continued runs
# ---------------------------------------------------------------------------------------------------------------------------
def _shift(faults, k):
    """the schedule as a call that starts k steps later sees it: an event that has fired by then fires at the call's step 0"""
    on = faults["onset"]
    return dict(faults, onset=np.where(on < 0, -1, np.maximum(on - k, 0)).astype(np.int32))


@pytest.mark.parametrize("every", [1, 4])
def test_continued_runs_equal_the_whole(gpu_mpc_factory, every):
    """T = 12 against 6 + 6 with state, llr, the detect arrays, the returned pattern, pending, step0 = 6, xhat, cov and the shifted
    schedule handed over, no process noise: state, u_hist, meas, est, llr_hist, the detect arrays and the returned state, llr and
    pattern bit for bit.  every = 4: step0 matters (the tests run at c = 4, 8)."""
    N, NT, B = 10, 8, 96
    bt = _two_faults(B, N)
    x0, ub, stuck, faults = bt["x0"], bt["ub"], bt["stuck"], bt["faults"]
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = _sensor(B, NT)
    xr = XT[1][:, :12 + N + 2]
    xh, cov = _prior(x0)
    est = _est_spec(every, xhat=xh, cov=cov, fields=("est", "xhat", "cov"))
    dg = _dspec(every)
    whole = _sim(mpc, x0, ub, stuck, N, 12, sen, est, dg, noise=ZERO, xr=xr, faults=faults)
    first = _sim(mpc, x0, ub, stuck, N, 6, sen, est, dg, noise=ZERO, xr=xr[:, :6 + N + 2], faults=faults)
    d1 = first["diagnosis"]
    sen2 = dict(sen, pending=first["sensor"]["pending"], step0=6)
    est2 = dict(est, xhat=first["estimator"]["xhat"], cov=first["estimator"]["cov"])
    dg2 = dict(dg, state=d1["state"], llr=d1["llr"], detect=(d1["step"], d1["thruster"], d1["level"]))
    second = _sim(mpc, first["x"], d1["ub"], d1["stuck"], N, 6, sen2, est2, dg2, noise=ZERO, xr=xr[:, 6:], faults=_shift(faults, 6))
    d2, dw = second["diagnosis"], whole["diagnosis"]
    assert np.array_equal(second["x"], whole["x"])
    for k in ("x_hist", "u"):
        assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    assert np.array_equal(np.concatenate([first["sensor"]["meas"], second["sensor"]["meas"]]), whole["sensor"]["meas"])
    assert np.array_equal(np.concatenate([first["estimator"]["est"], second["estimator"]["est"]]), whole["estimator"]["est"])
    assert np.array_equal(np.concatenate([d1["llr_hist"], d2["llr_hist"]]), dw["llr_hist"])
    for k in ("step", "thruster", "level", "state", "llr", "ub", "stuck"):
        assert np.array_equal(d2[k], dw[k]), k
    assert (dw["step"] >= 6).any() and (d1["step"] >= 0).any()      # detections on both sides of the seam
    # the handed arrays were not written into
    assert np.array_equal(dg2["state"], d1["state"]) and not np.array_equal(d2["state"], d1["state"])


# ---------------------------------------------------------------------------------------------------------------------------
# (F) slices of a campaign and device slots
# ---------------------------------------------------------------------------------------------------------------------------
def test_slices_and_device_slots_equal_the_whole():
    B, N, NT, T = 96, 10, 8, 12
    bt = _two_faults(B, N)
    sen = _sensor(B, NT)
    xh, cov = _prior(bt["x0"])
    est = _est_spec(3, xhat=xh, cov=cov, fields=("est",))
    dg = _dspec(3)

    def run(mpc, lo=0, hi=B, **kw):
        f = {k: v[lo:hi] for k, v in bt["faults"].items()}
        s = dict(sen, bias=sen["bias"][lo:hi], pending=sen["pending"][lo:hi])
        e = dict(est, xhat=xh[lo:hi], cov=cov[lo:hi])
        return mpc.simulate(bt["x0"][lo:hi], bt["ub"][lo:hi], bt["stuck"][lo:hi], _hover(N, T + 2), T, noise=NOISE, seed=5, faults=f,
                            return_inputs=True, return_states=True, sensor=s, estimator=e, diagnosis=dg, **kw)

    def fresh(lo, hi, **kw):
        mpc = ft_mpc_amd.BatchedMPC(N=N, NT=NT, dtype="f32")
        try:
            return run(mpc, lo, hi, **kw)
        finally:
            mpc.close()
    whole = fresh(0, B)
    parts = [fresh(0, 40, index0=0, index_total=B), fresh(40, B, index0=40, index_total=B)]
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f32"), devices=[0, 0, 0])
    try:
        multi = run(m)
    finally:
        m.close()
    assert np.array_equal(np.concatenate([p["x"] for p in parts]), whole["x"]) and np.array_equal(multi["x"], whole["x"])
    for k in ("x_hist", "u"):
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), whole[k]), k
        assert np.array_equal(multi[k], whole[k]), k
    for k in ("step", "thruster", "level", "ub", "stuck", "llr_hist", "state", "llr"):
        assert np.array_equal(np.concatenate([p["diagnosis"][k] for p in parts], axis=1 if k == "llr_hist" else 0), whole["diagnosis"][k]), k
        assert np.array_equal(multi["diagnosis"][k], whole["diagnosis"][k]), k
    assert (whole["diagnosis"]["step"] >= 0).any()


# ---------------------------------------------------------------------------------------------------------------------------
# (G) noisy closed loop
# ---------------------------------------------------------------------------------------------------------------------------
def test_noisy_closed_loop(gpu_mpc_factory):
    """B = 96, sensor sigma as on the CPU, threshold 18, levels (0, f_max), T = 20, onset at step 5, the vehicles start on the
    reference's orbit (_on_orbit: a thruster stuck on at f_max needs a command below f_max to show): vehicles b < 32 are healthy and
    have no detection; 32 <= b < 64 have thruster b % NT stuck on at f_max and are detected with the right thruster (and level) within
    the delay recorded on the CPU (tests/test_diagnosis_host.py, STUCK_ON_MAX_DELAY) plus one test; 64 <= b have thruster b % NT dead,
    whose detection depends on the controller using it: reported with the score."""
    N, NT, B, T, on = 10, 8, 96, 20, 5
    x0 = _on_orbit(B, 33)
    ub, stuck = np.full((B, NT), F_MAX), np.zeros((B, NT))
    onset = np.where(np.arange(B) >= 32, on, -1).astype(np.int32)[:, None]
    eub, est_ = ub[:, None].copy(), np.zeros((B, 1, NT))
    for b in range(32, B):
        eub[b, 0, b % NT] = 0.0
        est_[b, 0, b % NT] = F_MAX if b < 64 else 0.0
    faults = dict(onset=onset, ub=eub, stuck=est_)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = dict(sigma=SIGMA, seed=79, fields=("meas",))
    dg = _dspec(levels=(0.0, F_MAX), resid_sigma=DG.default_sigma(SIGMA, NOISE))
    out = _sim(mpc, x0, ub, stuck, N, T, sen, None, dg, faults=faults)
    do = out["diagnosis"]
    det = DG.detections_of(do["step"], do["thruster"], do["level"])
    ev = [[] if b < 32 else [(on, b % NT, 1 if b < 64 else 0)] for b in range(B)]
    sc = DG.score(ev, det)
    print(f"noisy closed loop: score {dict(sc, delay=None)}; delays of the stuck-on third {[det[b][0][0] - on if det[b] else None for b in range(32, 64)]}; "
          f"dead third found {sum(1 for b in range(64, B) if det[b])} of 32; largest statistic of the healthy third {do['llr_hist'][:, :32].max():.2f}")
    for b in range(32):
        assert det[b] == [], (b, det[b])
    for b in range(32, 64):
        assert det[b] and det[b][0][1:] == (b % NT, 1), (b, det[b])
        assert 1 <= det[b][0][0] - on <= STUCK_ON_MAX_DELAY + 1, (b, det[b])


# ---------------------------------------------------------------------------------------------------------------------------
# (H) other loops: the replay of (A)
# ---------------------------------------------------------------------------------------------------------------------------
def test_with_a_dispersed_plant_and_the_pwm_actuator(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 96, 12
    bt = _two_faults(B, N)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = _sensor(B, NT)
    xh, cov = _prior(bt["x0"])
    est = _est_spec(xhat=xh, cov=cov, fields=("est",))
    dg = _dspec()
    act = dict(mode="pwm", substeps=8, min_on=2, align="centred", tau_on=0.02, tau_off=0.01)
    out = _sim(mpc, bt["x0"], bt["ub"], bt["stuck"], N, T, sen, est, dg, plant=_plant(B, NT, seed=15), actuator=act, faults=bt["faults"])
    _check_replay(out, bt["x0"], bt["ub"], bt["stuck"], dg, mpc.cfg)


def test_with_a_mission(gpu_mpc_factory):
    N, NT, B, T, d = 10, 8, 96, 12, 2
    bt = _two_faults(B, N)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = _sensor(B, NT)
    xh, cov = _prior(bt["x0"])
    est = _est_spec(3, xhat=xh, cov=cov, fields=("est",))
    dg = _dspec(3)
    table, offset = (7 * np.arange(B) % 3).astype(np.int32), (5 * np.arange(B) % 23).astype(np.int32)
    cols = 22 + T + N + d
    ms = dict(tables=XT[:, :, :cols], utables=UT[:, :, :cols], table=table, offset=offset)
    out = mpc.simulate(bt["x0"], bt["ub"], bt["stuck"], None, T, noise=NOISE, seed=5, return_inputs=True, return_states=True, mission=ms,
                       sensor=sen, estimator=est, diagnosis=dg, faults=bt["faults"], outcomes=dict(cost=True))
    _check_replay(out, bt["x0"], bt["ub"], bt["stuck"], dg, mpc.cfg)


def test_with_the_thruster_sqp_loop(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 32, 10
    bt = _two_faults(B, N)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = dict(sigma=SIGMA, seed=80, fields=("meas",))      # a sensor alone: no latency, no filter
    dg = _dspec()
    out = _sim(mpc, bt["x0"], bt["ub"], bt["stuck"], N, T, sen, None, dg, sqp_iters=2, faults=bt["faults"])
    _check_replay(out, bt["x0"], bt["ub"], bt["stuck"], dg, mpc.cfg)
    assert out["u"].any()


# ---------------------------------------------------------------------------------------------------------------------------
# (I) refusals, on a handle and on the driver: FTMPC_ERR_ARG, the message names the field (and the vehicle), x untouched
# ---------------------------------------------------------------------------------------------------------------------------
def _bad_structs(B, NT):
    size = C.sizeof(_lib.ftmpc_diagnosis)
    v = B - 2                                                      # on three slots: in the last shard
    K, L = 2, 2

    def make(every=1, n_levels=L, max_detect=K, levels=(0.0, F_MAX), rs=(1e-2, 1e-2), ds=(0.0, 0.0), threshold=18.0, struct_size=size,
             **ptr):
        s = _lib.ftmpc_diagnosis(struct_size=struct_size, every=every, n_levels=n_levels, max_detect=max_detect, threshold=threshold)
        for k, lv in enumerate(levels):
            s.levels[k] = lv
        for k in range(2):
            s.resid_sigma[k], s.drift_sigma[k] = rs[k], ds[k]
        for name, a in ptr.items():
            setattr(s, name, a.ctypes.data_as(ip if a.dtype == np.int32 else dp))
        return s, list(ptr.values())
    st = np.zeros((B, 14 + NT))
    st[:, 9] = 1.0
    llr = np.zeros((B, NT * L))
    det = dict(detect_step=np.full((B, K), -1, np.int32), detect_thruster=np.full((B, K), -1, np.int32),
               detect_level=np.full((B, K), -1, np.int32))

    def with_det(**kw):
        d = {k: a.copy() for k, a in det.items()}
        for k, (slot, val) in kw.items():
            d[k][v, slot] = val
        return d
    nan_s, neg_n, inf_l = st.copy(), st.copy(), llr.copy()
    nan_s[v, 4], neg_n[v, 13], inf_l[v, 3] = np.nan, -1.0, np.inf
    return [("struct_size", None) + make(struct_size=size - 8), ("every", None) + make(every=0),
            ("n_levels", None) + make(n_levels=0), ("n_levels", None) + make(n_levels=5), ("max_detect", None) + make(max_detect=0),
            ("max_detect", None) + make(max_detect=9), ("levels", None) + make(levels=(-1.0, 1.0)), ("levels", None) + make(levels=(1.0, 1.0)),
            ("levels", None) + make(levels=(0.0, np.inf)), ("resid_sigma", None) + make(rs=(0.0, 1e-2)), ("resid_sigma", None) + make(rs=(1e-2, np.nan)),
            ("drift_sigma", None) + make(ds=(-1e-3, 0.0)), ("drift_sigma", None) + make(ds=(0.0, np.inf)), ("threshold", None) + make(threshold=0.0),
            ("threshold", None) + make(threshold=np.nan), ("llr", None) + make(llr=llr), ("detect_step", None) + make(detect_step=det["detect_step"]),
            ("detect_level", None) + make(detect_level=det["detect_level"]), ("detect_thruster", None) + make(state=st, detect_step=det["detect_step"], detect_level=det["detect_level"]),
            ("state", v) + make(state=nan_s, **det), ("state", v) + make(state=neg_n, **det), ("llr", v) + make(state=st, llr=inf_l, **det),
            ("detect_step", v) + make(state=st, **with_det(detect_step=(1, 4), detect_thruster=(1, 0), detect_level=(1, 0))),
            ("detect_step", v) + make(state=st, **with_det(detect_step=(0, -2))),
            ("detect_thruster", v) + make(state=st, **with_det(detect_step=(0, 4), detect_thruster=(0, NT), detect_level=(0, 0))),
            ("detect_level", v) + make(state=st, **with_det(detect_step=(0, 4), detect_thruster=(0, 0), detect_level=(0, L)))]


def test_refusals(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 12, 2
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 0, 20)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f32"), devices=[0, 0, 0])
    good = _bad_structs(B, NT)[1][2]
    good.every = 2
    es = _lib.ftmpc_estimator(struct_size=C.sizeof(_lib.ftmpc_estimator), every=1)
    for k in range(4):
        es.p0[k] = es.proc_sigma[k] = es.meas_sigma[k] = SIGMA[k]
    se = _lib.ftmpc_sensor(struct_size=C.sizeof(_lib.ftmpc_sensor), latency=0, predict=1)
    on, de = np.full((B, 1), 1, np.int32), np.full((B, 1), 1, np.int32)
    fub, fst = ub[:, None].copy(), stuck[:, None].copy()
    fs = _lib.ftmpc_fault_schedule(struct_size=C.sizeof(_lib.ftmpc_fault_schedule), n_events=1, onset=on.ctypes.data_as(ip),
                                   detect=de.ctypes.data_as(ip), ub=fub.ctypes.data_as(dp), stuck=fst.ctypes.data_as(dp))
    try:
        for obj in (mpc, m):
            for field, v, dg, keep in _bad_structs(B, NT):
                rc, err, out = _entry(obj, "diagnosis_batch", x0, ub, stuck, N, T, 1, (None, None, None, None, None, C.byref(dg)), want=False)
                assert rc == -1 and f"ftmpc_diagnosis.{field}".encode() in err, (field, err)
                if v is not None:
                    assert f"vehicle {v} ".encode() in err, err
                assert np.array_equal(out["x"], x0)
            # every against the estimator's; a predicting sensor without an estimator
            rc, err, out = _entry(obj, "diagnosis_batch", x0, ub, stuck, N, T, 1, (None, None, None, None, C.byref(es), C.byref(good)), want=False)
            assert rc == -1 and b"ftmpc_diagnosis.every" in err and b"estimator" in err and np.array_equal(out["x"], x0), err
            good.every = 1
            rc, err, out = _entry(obj, "diagnosis_batch", x0, ub, stuck, N, T, 1, (None, None, None, C.byref(se), None, C.byref(good)), want=False)
            assert rc == -1 and b"ftmpc_diagnosis" in err and b"predict" in err and np.array_equal(out["x"], x0), err
            good.every = 2
        # a schedule with detect != NULL (through the entry itself: _entry passes no schedule)
        good.every = 1
        x, uh, bad = x0.copy(), np.empty((T, B, NT)), np.zeros(T, np.int32)
        xr, nz = np.ascontiguousarray(_hover(N, T).reshape(-1, order="F")), np.array(NOISE)
        oc = _lib.ftmpc_outcomes(struct_size=C.sizeof(_lib.ftmpc_outcomes))
        for obj, f, last in ((mpc, mpc.lib.ftmpc_simulate_diagnosis_batch, mpc.lib.ftmpc_last_error),
                             (m, m.lib.ftmpc_multi_simulate_diagnosis_batch, m.lib.ftmpc_multi_last_error)):
            rc = f(obj._h, B, T, x.ctypes.data_as(dp), ub.ctypes.data_as(dp), stuck.ctypes.data_as(dp), xr.ctypes.data_as(dp), None,
                   nz.ctypes.data_as(dp), C.c_uint64(1), 0, 8, 1e-9, C.byref(fs), uh.ctypes.data_as(dp), None, bad.ctypes.data_as(ip),
                   C.byref(oc), None, None, None, None, None, C.byref(good))
            assert rc == -1 and b"ftmpc_fault_schedule.detect must be NULL" in last(obj._h) and np.array_equal(x, x0)
        with pytest.raises(ValueError, match="thruster formulation"):
            mpc.simulate(x0, ub, stuck, _hover(N, T), T, formulation="wrench", diagnosis=_dspec())
        with pytest.raises(ValueError, match="every"):      # what the front end refuses itself never reaches the library
            mpc.simulate(x0, ub, stuck, _hover(N, T), T, diagnosis=_dspec(every=0))
        # and a good diagnosis is accepted by both, with the same bits
        a, b = (_sim(o, x0, ub, stuck, N, T, None, None, _dspec()) for o in (mpc, m))
        assert np.array_equal(a["x"], b["x"])
        for k in a["diagnosis"]:
            assert np.array_equal(a["diagnosis"][k], b["diagnosis"][k]), k
    finally:
        m.close()
