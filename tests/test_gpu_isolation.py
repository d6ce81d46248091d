"""GPU: the diagnosis' consistency gate, confirmation and level revision in the on-device closed loop (ftmpc_diagnose_iso_kernel;
ftmpc_simulate_isolation_batch, ftmpc_simulate_wrench_isolation_batch, ftmpc_multi_simulate_isolation_batch;
BatchedMPC.simulate(isolation=...)).

The reference is ft_mpc_amd/diagnosis.py, replay(isolation=...) (tests/test_isolation_host.py checks it on the CPU against
csrc/ftmpc_isolate.h, the functions the kernel is made of).  Every run is replayed per vehicle from its own histories.

A  replay, each rule alone and all three (every = 1 and 3); B  NULL and trivial structs give the bits of the call without the
keyword; C  a wrong level is revised, and the wrench form's hull offsets follow; D  a push is not a fault; E  real faults still get
through; F  continued runs, slices, device slots; G  with an outage; H  refusals.

BOUND is the diagnosis suite's (tests/test_gpu_diagnosis.py: 2.8e-11 of max(1, |value|)) and holds for fit_hist as well: q_0 and
q_h are sums of the same products as the statistics.  In no replay does a statistic lie within 1e-6 of the threshold, a q_h within
1e-6 of consist^2 or a leader within 1e-6 of its runner-up (asserted; another seed would be the remedy).
MEASURED on an MI355X, maxima over every replay of this file: llr_hist within 4.2e-13 of max(1, |llr|), the returned llr 1.1e-13, the
returned state 4.5e-16, fit 8.8e-13 of max(1, |q|) (q_0 reaches a few hundred): BOUND is 30 x the largest.  The decisions, lead,
voided and revised are identical.
Closed loops with and without the rules (measured, not asserted; consist = consist_for(0.999) = 4.74, persist 2; `final`: scored with
diagnosis.score(final=True)):
  tests/test_gpu_diagnosis.py (A), B = 96, every 3, max_detect 2, 192 events, final: plain 154 detections -- 40 missed, 30 wrong thruster,
    34 wrong level, 2 false alarms; gate alone 79 -- 113 / 5 / 1 / 0, 182 void tests; persist alone 114 -- 78 / 8 / 25 / 0; revise
    alone 154 -- 48 / 23 / 25 / 2, 9 revisions; all three 64 -- 128 / 2 / 2 / 0, 185 void tests.  The rules take the wrong names from 64
    to 4 and the false alarms to 0, and pay with the misses: a window that holds a fault's onset partway fits no hypothesis, its test
    is void, and 20 steps at every 3 leave few tests after it.  every 1: plain 143 -- 49 / 3 / 4 / 0, all three 141 -- 51 / 3 / 6 / 0:
    no help, two levels worse.
  tests/test_gpu_outages.py (F), B = 65 (case G here): plain names the opposite thruster first on 65 of 65 and ends on the exact fault
    on 0 (final: 65 wrong levels, 65 false alarms); all three void the first test after the window (65 void tests) and name the dead
    thruster at level 0 first on 65 of 65, the final pattern the exact fault on 65.
  kicks on 64 healthy vehicles on the hover orbit (random directions, steps 8-10, T = 24, max_detect 2; detections / vehicles with one):
    5 N + 0.25 N m, every 1: plain 128 / 64, gate 2 / 1, persist 123 / 64, revise 128 / 64, all three 2 / 1; every 3: plain 107 / 64,
    gate and all three 0.  2 N + 0.1 N m, every 1: plain 68 / 38, gate 44 / 23, persist 40 / 20, revise 68 / 38 (27 revisions), all
    three 44 / 23 (21 of the 44 are revisions); every 3: plain 52 / 41, persist 21 / 21, gate and all three 0.  The 2 N push at every 1
    stays partly unsolved: one step of it is too small to be inconsistent with every hypothesis.
  case D: gate 0 detections and 193 void tests, on 64 of 64 vehicles; control 242 detections on 63 of 64.
  case E: control and rules score alike (no wrong thruster or level, the same 16 dead thrusters not found within the run), the stuck-on
    third is found one test later, 3 void tests."""
import ctypes as C

import numpy as np
import pytest

import ft_mpc_amd
from ft_mpc_amd import _lib
from ft_mpc_amd import diagnosis as DG
from ft_mpc_amd.sharding import MultiGPUMPC
from oracle import qp_oracle as qo
from test_gpu_actuators import _entry, _same_bits
from test_gpu_diagnosis import BOUND, F_MAX, LEVELS, NOISE, SIGMA, ZERO, _dspec, _meas, _on_orbit, _shift, _sim
from test_gpu_estimators import _prior, _sensor, _two_faults
from test_gpu_estimators import _spec as _est_spec
from test_gpu_missions import XT
from test_gpu_outcomes import _hover

pytestmark = pytest.mark.gpu
CONSIST = DG.consist_for(0.999)
RULES = dict(gate=dict(consist=CONSIST), persist=dict(persist=2), revise=dict(revise=True),
             all=dict(consist=CONSIST, persist=2, revise=True))
IALL = ("lead", "voided", "revised", "fit")
DKEYS = ("step", "thruster", "level", "ub", "stuck", "llr_hist", "state", "llr")
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def iso_mpc(gpu_mpc_factory):
    """one fp32 handle (N = 10, 8 thrusters) for the whole file: a handle keeps its work space until the session ends"""
    return gpu_mpc_factory(N=10, NT=8, dtype="f32")


def _check_replay(out, x0, ub, stuck, dg, iso, cfg, step0=0, avail=None, margin=1e-6):
    """llr_hist, fit, the detections and the returned state, llr, lead, voided, revised, ub and stuck of `out` against
    diagnosis.replay(isolation=...) of its own measurements and applied commands; returns the deviations and the replays."""
    do, io = out["diagnosis"], out["isolation"]
    T, B, NT = out["u"].shape
    meas = out["outage"]["meas"] if avail is not None else _meas(out, x0)
    dev = dict(llr_hist=0.0, llr=0.0, state=0.0, fit=0.0)
    got = DG.detections_of(do["step"], do["thruster"], do["level"])
    rel = lambda a, b: float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())
    reps = []
    for b in range(B):
        r = DG.replay(meas[:, b], out["u"][:, b], ub[b], stuck[b], dg, cfg, step0=step0,
                      state=None if dg.get("state") is None else dg["state"][b], llr=None if dg.get("llr") is None else dg["llr"][b],
                      detections=None if dg.get("detect") is None else DG.detections_of(*dg["detect"])[b],
                      avail=None if avail is None else avail[:, b], isolation=iso,
                      lead=None if iso.get("lead") is None else iso["lead"][b],
                      voided=0 if iso.get("voided") is None else iso["voided"][b],
                      revised=0 if iso.get("revised") is None else iso["revised"][b])
        reps.append(r)
        tested = ~np.isnan(r["peak"])
        assert (np.abs(r["peak"][tested] - dg["threshold"]) > margin).all(), (b, r["peak"])
        assert r["gate_margin"] > margin and r["lead_gap"] > margin, (b, r["gate_margin"], r["lead_gap"])
        dev["llr_hist"] = max(dev["llr_hist"], rel(do["llr_hist"][:, b], r["llr_hist"]))
        dev["llr"] = max(dev["llr"], rel(do["llr"][b], r["llr"]))
        dev["state"] = max(dev["state"], float(np.abs(do["state"][b] - r["state"]).max()))
        dev["fit"] = max(dev["fit"], rel(io["fit"][:, b], r["fit_hist"]))
        assert np.array_equal(io["fit"][:, b] < 0, r["fit_hist"] < 0), b
        assert got[b] == r["detections"], (b, got[b], r["detections"])
        assert tuple(io["lead"][b]) == r["lead"] and io["voided"][b] == r["voided"] and io["revised"][b] == r["revised"], \
            (b, io["lead"][b], r["lead"], io["voided"][b], r["voided"], io["revised"][b], r["revised"])
        assert np.array_equal(do["ub"][b], r["ub_end"]) and np.array_equal(do["stuck"][b], r["stuck_end"]), b
    print("isolation replay: max deviation (device - definition): " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items())
          + f"; {sum(len(g) for g in got)} detections, {int(io['voided'].sum())} void tests, {int(io['revised'].sum())} revisions on {B} vehicles")
    for k, v in dev.items():
        assert v <= BOUND, (k, v)
    return dev, reps


# ---------------------------------------------------------------------------------------------------------------------------
# (A) replay from the run's own histories
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("B", [1, 65, 96])
@pytest.mark.parametrize("rule", ["gate", "persist", "revise", "all"])
def test_replay_from_the_runs_own_histories(iso_mpc, rule, every, B):
    """The setting of tests/test_gpu_diagnosis.py (A): noise, a bias, latency 2 with the estimator predicting, the two-fault
    schedule, three levels, max_detect 4."""
    N, NT, T = 10, 8, 20
    bt = _two_faults(B, N)
    mpc = iso_mpc
    sen = _sensor(B, NT)
    xh, cov = _prior(bt["x0"])
    est = _est_spec(every, xhat=xh, cov=cov, fields=("est",))
    dg = _dspec(every, max_detect=4)
    iso = dict(RULES[rule], fields=IALL)
    out = _sim(mpc, bt["x0"], bt["ub"], bt["stuck"], N, T, sen, est, dg, faults=bt["faults"], isolation=iso)
    assert sorted(out["isolation"]) == sorted(IALL) and sorted(out["diagnosis"]) == sorted(DKEYS)
    _check_replay(out, bt["x0"], bt["ub"], bt["stuck"], dg, iso, mpc.cfg)
    assert (out["isolation"]["fit"][..., 0] > 0).any()


# ---------------------------------------------------------------------------------------------------------------------------
# (B) NULL and trivial structs
# ---------------------------------------------------------------------------------------------------------------------------
def test_null_and_trivial_isolation_give_the_bits_of_the_call_without(iso_mpc):
    N, NT, B, T = 10, 8, 96, 8
    bt = _two_faults(B, N)
    mpc = iso_mpc
    sen = _sensor(B, NT)
    xh, cov = _prior(bt["x0"])
    est = _est_spec(1, xhat=xh, cov=cov, fields=("est",))
    dg = _dspec(1)
    ref = _sim(mpc, bt["x0"], bt["ub"], bt["stuck"], N, T, sen, est, dg, faults=bt["faults"])
    out = _sim(mpc, bt["x0"], bt["ub"], bt["stuck"], N, T, sen, est, dg, faults=bt["faults"],
               isolation=dict(consist=0.0, persist=1, revise=False, fields=()))
    assert out["isolation"] == {}
    for k in ("u", "x_hist", "x"):
        assert np.array_equal(out[k], ref[k]), k
    for k in DKEYS:
        assert np.array_equal(out["diagnosis"][k], ref["diagnosis"][k]), k
    assert (ref["diagnosis"]["step"] >= 0).any()
    # through the C entries, on a handle and on the driver: NULL and the trivial struct against the _environment_ entry
    x0, ub, stuck = qo.make_batch(B, N, NT, 1, 16)[:3]
    triv = _lib.ftmpc_isolation(struct_size=C.sizeof(_lib.ftmpc_isolation), persist=1)
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f32"), devices=[0, 0, 0])
    try:
        for obj in (mpc, m):
            rc, err, ref = _entry(obj, "environment_batch", x0, ub, stuck, N, 4, 7, (None,) * 10)
            assert rc == 0, err
            for s in (None, C.byref(triv)):
                rc, err, out = _entry(obj, "isolation_batch", x0, ub, stuck, N, 4, 7, (None,) * 10 + (s,))
                assert rc == 0, err
                _same_bits(out, ref)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (C) revision without noise
# ---------------------------------------------------------------------------------------------------------------------------
def _wrong_level(B, NT, x0, up=None, down=None):
    """thruster i of vehicle b is carried in as detected at 1.7 N (detect = [(0, i, 1)], ub_i = 0, stuck_i = 1.7); the schedule
    puts the plant's thruster at 3.4 N (even b) or at 0 (odd b) from step 0 on.  i = b % NT, or taken in turn from `up` (even b) and
    `down` (odd b)"""
    ub, stuck = np.full((B, NT), F_MAX), np.zeros((B, NT))
    i = np.arange(B) % NT
    if up is not None:
        i = np.array([(up if b % 2 == 0 else down)[(b // 2) % len(up if b % 2 == 0 else down)] for b in range(B)])
    ub[np.arange(B), i], stuck[np.arange(B), i] = 0.0, 1.7
    true = np.where(np.arange(B) % 2 == 0, F_MAX, 0.0)
    est_ = stuck[:, None].copy()
    est_[np.arange(B), 0, i] = true
    faults = dict(onset=np.zeros((B, 1), np.int32), ub=ub[:, None].copy(), stuck=est_)
    det = tuple(np.full((B, 4), -1, np.int32) for _ in range(3))
    det[0][:, 0], det[1][:, 0], det[2][:, 0] = 0, i, 1
    state = np.zeros((B, 14 + NT))
    state[:, 0:13] = x0
    return ub, stuck, i, true, faults, det, state


def _check_revised(out, x0, ub, stuck, i, true, dg, iso, cfg):
    do, io = out["diagnosis"], out["isolation"]
    B, NT = ub.shape
    got = DG.detections_of(do["step"], do["thruster"], do["level"])
    meas = _meas(out, x0)
    for b in range(B):
        r = DG.replay(meas[:, b], out["u"][:, b], ub[b], stuck[b], dg, cfg, state=dg["state"][b],
                      detections=DG.detections_of(*dg["detect"])[b], isolation=iso)
        assert got[b] == r["detections"], (b, got[b], r["detections"])
        assert len(got[b]) == 2 and got[b][1][1:] == (i[b], LEVELS.index(true[b])), (b, got[b])
        assert io["revised"][b] == 1
        assert (do["ub"][b] == 0).sum() == 1 and do["ub"][b, i[b]] == 0 and do["stuck"][b, i[b]] == true[b]
        assert np.array_equal(np.delete(do["stuck"][b], i[b]), np.zeros(NT - 1))
    return sorted({g[1][0] for g in got})


def test_a_wrong_level_is_revised(iso_mpc):
    """MEASURED on an MI355X: every one of the 32 vehicles is revised at step 1, the first test."""
    N, NT, T, B = 10, 8, 8, 32
    x0 = _on_orbit(B, 31)
    ub, stuck, i, true, faults, det, state = _wrong_level(B, NT, x0)
    mpc = iso_mpc
    dg = _dspec(resid_sigma=(1e-6, 1e-6), max_detect=4, state=state, detect=det)
    iso = dict(consist=0.0, persist=1, revise=True, fields=IALL)
    out = _sim(mpc, x0, ub, stuck, N, T, None, _est_spec(1, fields=("est",)), dg, noise=ZERO, faults=faults, isolation=iso)
    steps = _check_revised(out, x0, ub, stuck, i, true, dg, iso, mpc.cfg)
    print(f"revision without noise: revised at steps {steps}")
    # without revise the level stays wrong
    off = _sim(mpc, x0, ub, stuck, N, T, None, _est_spec(1, fields=("est",)), dg, noise=ZERO, faults=faults)
    assert (off["diagnosis"]["stuck"][np.arange(B), i] == 1.7).all()


def test_a_revision_on_the_wrench_form_recomputes_the_hull_offsets(gpu_mpc_factory):
    """The 16 thrusters stand in groups with one signature line: 0 and 1 push exactly along one line, 2 and 3 exactly against it
    (likewise 4, 5 against 6, 7; 8 against 10, 9 against 11, 12 against 13, 14 against 15: oracle.refmath.allocation_matrix_16).
    "Thruster i delivers 1.7 N less than the model says" and "the thruster opposite, commanded 0, is stuck at 1.7 N" are then the same
    signature, statistic for statistic, and the tie goes to the lowest index.  The revised thruster is therefore taken from the ones
    to which that rule resolves: upwards (3.4 N) any thruster that is the first of its parallel pair, downwards (0 N) the ones whose
    opposite thrusters all have higher numbers."""
    from ft_mpc_amd.controllers.tools.input_bounds import hull_tables
    from oracle import refmath as rm
    N, NT, T, B = 10, 16, 6, 32
    x0 = _on_orbit(B, 35)
    ub, stuck, i, true, faults, det, state = _wrong_level(B, NT, x0, up=(0, 2, 4, 6, 8, 9, 10, 11, 12, 13, 14, 15), down=(0, 1, 8, 9, 12, 14))
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f64", max_iters=60)
    hull = hull_tables(rm.allocation_matrix_16(), ub, stuck)
    dg = _dspec(resid_sigma=(1e-6, 1e-6), max_detect=4, state=state, detect=det, rebuild_hull=True)
    iso = dict(consist=0.0, persist=1, revise=True, fields=IALL)
    out = mpc.simulate(x0, ub, stuck, _hover(N, T), T, noise=ZERO, seed=5, return_inputs=True, return_states=True, diagnosis=dg,
                       formulation="wrench", hull=hull, faults=faults, isolation=iso)
    plain = {k: v for k, v in dg.items() if k != "rebuild_hull"}
    _check_revised(out, x0, ub, stuck, i, true, plain, iso, mpc.cfg)
    do = out["diagnosis"]
    assert (do["no_hull"] == -1).all()
    dev = mpc.hull_offsets(do["ub"], do["stuck"], hull)
    assert not dev["flat"].any() and np.array_equal(do["hull_b"], dev["b"]) and not np.array_equal(do["hull_b"], hull["b"])


# ---------------------------------------------------------------------------------------------------------------------------
# (D) a push is not a fault
# ---------------------------------------------------------------------------------------------------------------------------
def _push(cfg, x0, rs, consist, seed=17):
    """A kick [B,6] (force, inertial frame; torque, body frame) per vehicle.  In the whitened residual space of one step,
    w = [dt / m M(q)' f / s_v, dt J^-1 t / s_w], the share of |w|^2 orthogonal to every thruster's signature line is at least 0.6 at
    the attitude the vehicle starts with (directions are drawn until it is), and the size makes share x |w|^2 = 1.5 x 9 consist^2."""
    from ft_mpc_amd.estimators import _body_to_inertial, _cfg_model
    D, m, J = _cfg_model(cfg)
    lines = _lines(cfg, rs)
    rng = np.random.default_rng(seed)
    kick = np.empty((x0.shape[0], 6))
    for b in range(x0.shape[0]):
        while True:
            fb, tb = rng.normal(size=3), 0.05 * rng.normal(size=3)
            w = np.concatenate([(cfg.dt / m) * fb / rs[0], cfg.dt * np.linalg.solve(J, tb) / rs[1]])
            share = 1.0 - ((lines @ w) ** 2).max() / (w @ w)
            if share >= 0.6:
                break
        scale = np.sqrt(1.5 * 9.0 * consist ** 2 / (share * (w @ w)))
        kick[b] = scale * np.r_[_body_to_inertial(x0[b, 6:10]) @ fb, tb]
    return kick


def _lines(cfg, rs):
    """[NT,6] unit vectors: every thruster's signature line in the whitened residual space"""
    from ft_mpc_amd.estimators import _cfg_model
    D, m, J = _cfg_model(cfg)
    lines = np.concatenate([(cfg.dt / m) * D[0:3].T / rs[0], cfg.dt * np.linalg.solve(J, D[3:6]).T / rs[1]], axis=1)
    return lines / np.linalg.norm(lines, axis=1, keepdims=True)


def test_a_push_is_not_a_fault(iso_mpc):
    """64 healthy vehicles on the hover orbit, an environment kick over the steps 1-3.  With the gate at consist_for(0.999): no
    detection, and void tests on every vehicle.  Control, consist = 0: detections.  Measured: the module's docstring."""
    from ft_mpc_amd.estimators import _body_to_inertial, _cfg_model
    N, NT, T, B = 10, 8, 12, 64
    x0 = _on_orbit(B, 37)
    ub, stuck = np.full((B, NT), F_MAX), np.zeros((B, NT))
    mpc = iso_mpc
    cfg = mpc.cfg
    sen = dict(sigma=SIGMA, seed=79, fields=("meas",))
    dg = _dspec(max_detect=4)
    rs = np.asarray(dg["resid_sigma"])
    kick = _push(cfg, x0, rs, CONSIST)
    env = dict(kick=kick, window=np.tile(np.array([[1, 4]], np.int32), (B, 1)), fields=("wrench",))
    arms = {}
    for name, consist in (("gate", CONSIST), ("control", 0.0)):
        out = _sim(mpc, x0, ub, stuck, N, T, sen, None, dg, environment=env, isolation=dict(consist=consist, fields=IALL))
        arms[name] = out
        det = DG.detections_of(*(out["diagnosis"][k] for k in ("step", "thruster", "level")))
        print(f"push, {name}: {sum(len(d) for d in det)} detections on {sum(1 for d in det if d)} of {B} vehicles, "
              f"void tests {int(out['isolation']['voided'].sum())}, vehicles with a void test {int((out['isolation']['voided'] > 0).sum())}")
    # the scenario is what it says, at the attitudes the vehicles had while they were pushed (x_hist[t]: the state after step t)
    D, m, J = _cfg_model(cfg)
    lines = _lines(cfg, rs)
    xh = arms["gate"]["x_hist"]
    for b in range(B):
        for t in (1, 2, 3):
            q = xh[t - 1, b, 6:10]
            w = np.concatenate([(cfg.dt / m) * (_body_to_inertial(q).T @ kick[b, 0:3]) / rs[0], cfg.dt * np.linalg.solve(J, kick[b, 3:6]) / rs[1]])
            share = 1.0 - ((lines @ w) ** 2).max() / (w @ w)
            assert share >= 0.5 and share * (w @ w) >= 9.0 * CONSIST ** 2, (b, t, share, w @ w)
    assert np.array_equal(arms["gate"]["environment"]["wrench"][1:4], np.repeat(kick[None], 3, 0))
    g, c = arms["gate"], arms["control"]
    assert (g["diagnosis"]["step"] < 0).all() and (g["isolation"]["voided"] > 0).all()
    assert (c["diagnosis"]["step"] >= 0).any() and (c["isolation"]["voided"] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# (E) real faults still get through
# ---------------------------------------------------------------------------------------------------------------------------
def test_real_faults_still_get_through(iso_mpc):
    """The scenario of tests/test_gpu_diagnosis.py::test_noisy_closed_loop with all three rules on, against the same call without
    isolation: every stuck-on vehicle the control arm finds on the right thruster is found on the right thruster at most `persist`
    tests later; the healthy third has no detection.  Measured: the module's docstring."""
    N, NT, B, T, on = 10, 8, 96, 20, 5
    x0 = _on_orbit(B, 33)
    ub, stuck = np.full((B, NT), F_MAX), np.zeros((B, NT))
    onset = np.where(np.arange(B) >= 32, on, -1).astype(np.int32)[:, None]
    eub, est_ = ub[:, None].copy(), np.zeros((B, 1, NT))
    for b in range(32, B):
        eub[b, 0, b % NT] = 0.0
        est_[b, 0, b % NT] = F_MAX if b < 64 else 0.0
    faults = dict(onset=onset, ub=eub, stuck=est_)
    mpc = iso_mpc
    sen = dict(sigma=SIGMA, seed=79, fields=("meas",))
    dg = _dspec(levels=(0.0, F_MAX), resid_sigma=DG.default_sigma(SIGMA, NOISE))
    iso = dict(RULES["all"], fields=IALL)
    ctl = _sim(mpc, x0, ub, stuck, N, T, sen, None, dg, faults=faults)
    out = _sim(mpc, x0, ub, stuck, N, T, sen, None, dg, faults=faults, isolation=iso)
    dc = DG.detections_of(*(ctl["diagnosis"][k] for k in ("step", "thruster", "level")))
    do = DG.detections_of(*(out["diagnosis"][k] for k in ("step", "thruster", "level")))
    ev = [[] if b < 32 else [(on, b % NT, 1 if b < 64 else 0)] for b in range(B)]
    print(f"real faults: control {dict(DG.score(ev, dc, final=True), delay=None)}; rules {dict(DG.score(ev, do, final=True), delay=None)}; "
          f"extra delays of the stuck-on third {sorted({do[b][0][0] - dc[b][0][0] for b in range(32, 64) if dc[b] and do[b]})}; "
          f"void tests {int(out['isolation']['voided'].sum())}, revisions {int(out['isolation']['revised'].sum())}")
    for b in range(32):
        assert do[b] == [], (b, do[b])
    n = 0
    for b in range(32, 64):
        if dc[b] and dc[b][0][1] == b % NT:
            n += 1
            assert do[b] and do[b][0][1] == b % NT, (b, dc[b], do[b])
            assert do[b][0][0] - dc[b][0][0] <= iso["persist"], (b, dc[b], do[b])
    assert n > 0


# ---------------------------------------------------------------------------------------------------------------------------
# (F) continued runs, slices and device slots
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 4])
def test_continued_runs_equal_the_whole(iso_mpc, every):
    """T = 12 against 5 + 7 with everything tests/test_gpu_diagnosis.py (E) hands over, and lead, voided and revised."""
    N, NT, B = 10, 8, 96
    bt = _two_faults(B, N)
    x0, ub, stuck, faults = bt["x0"], bt["ub"], bt["stuck"], bt["faults"]
    mpc = iso_mpc
    sen = _sensor(B, NT)
    xr = XT[1][:, :12 + N + 2]
    xh, cov = _prior(x0)
    est = _est_spec(every, xhat=xh, cov=cov, fields=("est", "xhat", "cov"))
    dg = _dspec(every, max_detect=4)
    iso = dict(RULES["all"], fields=IALL)
    whole = _sim(mpc, x0, ub, stuck, N, 12, sen, est, dg, noise=ZERO, xr=xr, faults=faults, isolation=iso)
    first = _sim(mpc, x0, ub, stuck, N, 5, sen, est, dg, noise=ZERO, xr=xr[:, :5 + N + 2], faults=faults, isolation=iso)
    d1, i1 = first["diagnosis"], first["isolation"]
    sen2 = dict(sen, pending=first["sensor"]["pending"], step0=5)
    est2 = dict(est, xhat=first["estimator"]["xhat"], cov=first["estimator"]["cov"])
    dg2 = dict(dg, state=d1["state"], llr=d1["llr"], detect=(d1["step"], d1["thruster"], d1["level"]))
    iso2 = dict(iso, lead=i1["lead"], voided=i1["voided"], revised=i1["revised"])
    second = _sim(mpc, first["x"], d1["ub"], d1["stuck"], N, 7, sen2, est2, dg2, noise=ZERO, xr=xr[:, 5:], faults=_shift(faults, 5),
                  isolation=iso2)
    d2, dw, i2, iw = second["diagnosis"], whole["diagnosis"], second["isolation"], whole["isolation"]
    assert np.array_equal(second["x"], whole["x"])
    for k in ("x_hist", "u"):
        assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    assert np.array_equal(np.concatenate([d1["llr_hist"], d2["llr_hist"]]), dw["llr_hist"])
    assert np.array_equal(np.concatenate([i1["fit"], i2["fit"]]), iw["fit"])
    for k in ("step", "thruster", "level", "state", "llr", "ub", "stuck"):
        assert np.array_equal(d2[k], dw[k]), k
    for k in ("lead", "voided", "revised"):
        assert np.array_equal(i2[k], iw[k]), k
    assert (dw["step"] >= 0).any()
    if every == 1:
        assert (i1["lead"][:, 1] > 0).any()      # a leader was waiting for its confirmation at the seam
    assert np.array_equal(iso2["lead"], i1["lead"])      # the handed arrays were not written into


def test_slices_and_device_slots_equal_the_whole():
    B, N, NT, T = 96, 10, 8, 12
    bt = _two_faults(B, N)
    sen = _sensor(B, NT)
    xh, cov = _prior(bt["x0"])
    est = _est_spec(3, xhat=xh, cov=cov, fields=("est",))
    dg = _dspec(3, max_detect=4)
    iso = dict(RULES["all"], fields=IALL)

    def run(mpc, lo=0, hi=B, **kw):
        f = {k: v[lo:hi] for k, v in bt["faults"].items()}
        s = dict(sen, bias=sen["bias"][lo:hi], pending=sen["pending"][lo:hi])
        e = dict(est, xhat=xh[lo:hi], cov=cov[lo:hi])
        return mpc.simulate(bt["x0"][lo:hi], bt["ub"][lo:hi], bt["stuck"][lo:hi], _hover(N, T + 2), T, noise=NOISE, seed=5, faults=f,
                            return_inputs=True, return_states=True, sensor=s, estimator=e, diagnosis=dg, isolation=iso, **kw)

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
    for grp, keys, hist in (("diagnosis", DKEYS, "llr_hist"), ("isolation", IALL, "fit")):
        for k in keys:
            assert np.array_equal(np.concatenate([p[grp][k] for p in parts], axis=1 if k == hist else 0), whole[grp][k]), k
            assert np.array_equal(multi[grp][k], whole[grp][k]), k
    assert (whole["diagnosis"]["step"] >= 0).any() and (whole["isolation"]["fit"][..., 0] > 0).any()


# ---------------------------------------------------------------------------------------------------------------------------
# (G) with an outage
# ---------------------------------------------------------------------------------------------------------------------------
def test_through_a_scripted_outage(iso_mpc):
    """The scenario of tests/test_gpu_outages.py (F): a thruster dies at step 4 inside a scripted outage [3, 8).  The replay with
    avail matches; while the vehicle is lost its statistics, lead and counters do not move (a run that ends inside the window
    returns what the run that ends at its start returns) and fit holds -1.  Measured: the module's docstring."""
    from test_gpu_estimators import _sim as _esim
    N, NT, B, T = 10, 8, 65, 16
    x0 = _on_orbit(B, 31)
    ub, stuck = np.full((B, NT), F_MAX), np.zeros((B, NT))
    mpc = iso_mpc
    sen = _sensor(B, NT, d=0, predict=False, bias=False)
    healthy = _esim(mpc, x0, ub, stuck, N, 8, sen, _est_spec(fields=("est",)))
    dead = healthy["u"].mean(0).argmax(1)
    eub = ub[:, None].copy()
    eub[np.arange(B), 0, dead] = 0.0
    faults = dict(onset=np.full((B, 1), 4, np.int32), ub=eub, stuck=np.zeros((B, 1, NT)))
    og = dict(p_loss=0.0, p_recover=1.0, window=np.tile(np.array([[3, 8]], np.int32), (B, 1)), fields=("avail", "meas", "state"))
    dg = _dspec(1, max_detect=4)
    iso = dict(RULES["all"], fields=IALL)
    xh, cov = _prior(x0)
    est = _est_spec(xhat=xh, cov=cov, fields=("est",))
    run = lambda Tn, **kw: _sim(mpc, x0, ub, stuck, N, Tn, sen, est, dg, faults=faults, outage=og, **kw)
    out = run(T, isolation=iso)
    _check_replay(out, x0, ub, stuck, dg, iso, mpc.cfg, avail=out["outage"]["avail"])
    assert (out["isolation"]["fit"][3:8] == -1).all()
    a, b = run(3, isolation=iso), run(7, isolation=iso)
    for k in ("lead", "voided", "revised"):
        assert np.array_equal(a["isolation"][k], b["isolation"][k]), k
    assert np.array_equal(a["diagnosis"]["llr"], b["diagnosis"]["llr"])
    ctl = run(T)
    ev = [[(4, int(dead[v]), 0)] for v in range(B)]
    for name, o in (("plain", ctl), ("rules", out)):
        det = DG.detections_of(*(o["diagnosis"][k] for k in ("step", "thruster", "level")))
        first = sum(1 for v in range(B) if det[v] and det[v][0][1] == dead[v])
        print(f"outage, {name}: {dict(DG.score(ev, det, final=True), delay=None)}; the first detection names the dead thruster on {first} of {B}; "
              f"final pattern exactly the fault on {sum(1 for v in range(B) if np.array_equal(o['diagnosis']['ub'][v], eub[v, 0]) and not o['diagnosis']['stuck'][v].any())}")


# ---------------------------------------------------------------------------------------------------------------------------
# (H) refusals, through the three C entries: FTMPC_ERR_ARG, the message names the field (and the vehicle), x untouched
# ---------------------------------------------------------------------------------------------------------------------------
def _bad_structs(B, NT):
    size = C.sizeof(_lib.ftmpc_isolation)
    v = B - 2                                                      # on three slots: in the last shard

    def make(struct_size=size, reserved=0, consist=4.7, persist=2, revise=1, **ptr):
        s = _lib.ftmpc_isolation(struct_size=struct_size, reserved=reserved, consist=consist, persist=persist, revise=revise)
        for name, a in ptr.items():
            setattr(s, name, a.ctypes.data_as(ip))
        return s, list(ptr.values())

    def arr(width, col, value):
        a = np.zeros((B, width) if width > 1 else B, np.int32)
        if width > 1:
            a[:, 0] = -1
            a[v, col] = value
        else:
            a[v] = value
        return a
    # (field, vehicle, needs the diagnosis, with its state)
    return [("struct_size", None, False, False) + make(struct_size=size - 8), ("reserved", None, False, False) + make(reserved=1),
            ("consist", None, True, False) + make(consist=-1.0), ("consist", None, True, False) + make(consist=np.nan),
            ("consist", None, True, False) + make(consist=np.inf), ("persist", None, True, False) + make(persist=0),
            ("revise", None, True, False) + make(revise=2), ("revise", None, True, False) + make(revise=-1),
            ("", None, False, False) + make(),                                                  # not trivial, no diagnosis
            ("lead", None, True, False) + make(lead=arr(2, 0, -1)),                             # lead without diagnosis.state
            ("lead", v, True, True) + make(lead=arr(2, 0, -2)), ("lead", v, True, True) + make(lead=arr(2, 0, NT * 2)),
            ("lead", v, True, True) + make(lead=arr(2, 1, -1)), ("voided", v, True, False) + make(voided=arr(1, 0, -1)),
            ("revised", v, True, False) + make(revised=arr(1, 0, -3))]


def test_refusals(iso_mpc):
    N, NT, B, T = 10, 8, 12, 2
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 0, 20)
    mpc = iso_mpc
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f32"), devices=[0, 0, 0])

    def diag(state):
        s = _lib.ftmpc_diagnosis(struct_size=C.sizeof(_lib.ftmpc_diagnosis), every=1, n_levels=2, max_detect=2, threshold=18.0)
        s.levels[0], s.levels[1] = 0.0, F_MAX
        for k in range(2):
            s.resid_sigma[k] = 1e-2
        keep = []
        if state:
            st = np.zeros((B, 14 + NT))
            st[:, 0:13] = x0
            det = [np.full((B, 2), -1, np.int32) for _ in range(3)]
            s.state = st.ctypes.data_as(dp)
            s.detect_step, s.detect_thruster, s.detect_level = (a.ctypes.data_as(ip) for a in det)
            keep = [st] + det
        return s, keep
    try:
        for n, (field, v, need, state, iso, keep) in enumerate(_bad_structs(B, NT)):
            dgs, dkeep = diag(state)
            dref = C.byref(dgs) if need else None
            for obj in (mpc, m):
                calls = [("isolation_batch", (None,) * 5 + (dref,) + (None,) * 4 + (C.byref(iso),), False)]
                if obj is mpc:     # (the wrench form has no multi-GPU entry; every refusal comes before its dummy hull is looked at)
                    calls.append(("wrench_isolation_batch", (None,) * 5 + (dref,) + (None,) * 6 + (C.byref(iso),), True))
                for name, tail, wrench in calls:
                    rc, err, out = _entry(obj, name, x0, ub, stuck, N, T, 1, tail, want=False, wrench=wrench)
                    assert rc == -1 and (f"ftmpc_isolation.{field}" if field else "no diagnosis").encode() in err, (n, field, name, err)
                    assert b"ftmpc_isolation" in err
                    if v is not None:
                        assert f"vehicle {v} ".encode() in err, err
                    assert np.array_equal(out["x"], x0)
        with pytest.raises(ValueError, match="persist"):      # what the front end refuses itself never reaches the library
            mpc.simulate(x0, ub, stuck, _hover(N, T), T, diagnosis=_dspec(), isolation=dict(persist=0))
        with pytest.raises(ValueError, match="no diagnosis"):
            mpc.simulate(x0, ub, stuck, _hover(N, T), T, isolation=dict(persist=2))
        with pytest.raises(ValueError, match="MultiGPUMPC is not built"):
            m.simulate(x0, ub, stuck, _hover(N, T), T, formulation="wrench", diagnosis=_dspec(rebuild_hull=True), isolation=dict(persist=2))
        # and a good isolation is accepted by both, with the same bits
        iso = dict(RULES["all"], fields=IALL)
        a, b = (_sim(o, x0, ub, stuck, N, T, None, None, _dspec(), isolation=iso) for o in (mpc, m))
        assert np.array_equal(a["x"], b["x"])
        for k in IALL:
            assert np.array_equal(a["isolation"][k], b["isolation"][k]), k
    finally:
        m.close()
