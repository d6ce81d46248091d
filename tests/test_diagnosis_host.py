"""CPU: the host side of the thruster fault diagnosis (include/ftmpc.h, ftmpc_diagnosis; ft_mpc_amd/diagnosis.py): the two entries are
exported, the ctypes struct has the layout gcc gives the header and no earlier struct changed size, the signature is the first-order
effect of a stuck thruster on one and on three RK4 steps of oracle.refmath.plant_dx_dt, an open loop of 64 healthy vehicles raises no
alarm at threshold 18 while the same loop with a thruster stuck on is isolated within two tests, a dead thruster is found once it is
commanded and never blamed on another, max_detect and the tie rule hold, and the refusals Python raises before the library is called."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import qp_oracle as qo
from oracle import refmath as rm

ROOT = Path(__file__).resolve().parents[1]
NEW = ("ftmpc_simulate_diagnosis_batch", "ftmpc_multi_simulate_diagnosis_batch")
FIELDS = ["struct_size", "every", "n_levels", "max_detect", "levels", "resid_sigma", "drift_sigma", "threshold", "state", "llr",
          "detect_step", "detect_thruster", "detect_level", "ub", "stuck", "llr_hist"]
OFFSETS = [0, 4, 8, 12, 16, 48, 64, 80, 88, 96, 104, 112, 120, 128, 136, 144]
SIGMA = (1e-2, 5e-3, 1e-2, 5e-3)
F_MAX = 3.4
NT = 8
# largest delay (steps from onset to detection) of the stuck-on run below, as the restatement shows it; tests/test_gpu_diagnosis.py
# (case G) caps the device's delay at this plus one test
STUCK_ON_MAX_DELAY = 2


def _cfg(**kw):
    from ft_mpc_amd.batch import MPCConfig
    return MPCConfig(NT=NT, **kw)


def _state(rng, wmax=1.0):
    q = rng.normal(size=4)
    w = rng.normal(size=3)
    w *= wmax * rng.uniform() / np.linalg.norm(w)
    return np.concatenate([rng.normal(size=3), rng.normal(size=3), q / np.linalg.norm(q), w])


def _rk4(x, u, ub, stuck, cfg):
    """One RK4 step of oracle.refmath.plant_dx_dt, the quaternion renormalised."""
    from ft_mpc_amd.estimators import _cfg_model
    D, m, J = _cfg_model(cfg)

    def f(z):
        return rm.plant_dx_dt(z, u, D, stuck, ub, m, J)
    h = cfg.dt
    k1 = f(x)
    k2 = f(x + 0.5 * h * k1)
    k3 = f(x + 0.5 * h * k2)
    k4 = f(x + h * k3)
    y = x + h / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    y[6:10] /= np.linalg.norm(y[6:10])
    return y


def test_library_exports_the_diagnosis_entries():
    from ft_mpc_amd import _lib
    _lib.build_library()
    lib = _lib.load_library()
    header = (ROOT / "include" / "ftmpc.h").read_text()
    for n in NEW:
        assert n in _lib.SYMBOLS and getattr(lib, n) is not None
        assert f"int {n}(" in header
    assert lib.ftmpc_simulate_diagnosis_batch.argtypes[:-1] == lib.ftmpc_simulate_estimator_batch.argtypes
    assert lib.ftmpc_multi_simulate_diagnosis_batch.argtypes[:-1] == lib.ftmpc_multi_simulate_estimator_batch.argtypes
    assert lib.ftmpc_version() == 540


def test_diagnosis_struct_layout_matches_the_header(tmp_path):
    from ft_mpc_amd import _lib
    assert [f for f, _ in _lib.ftmpc_diagnosis._fields_] == FIELDS
    src = tmp_path / "layout.c"
    body = "".join(f'printf("{f} %zu\\n", offsetof(ftmpc_diagnosis, {f}));' for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftmpc.h"\nint main(void){printf("sizeof %zu\\n", sizeof(ftmpc_diagnosis));'
                   + body + 'printf("estimator %zu\\nsensor %zu\\nactuator %zu\\noutcomes %zu\\nplant %zu\\nmission %zu\\nschedule %zu\\n", '
                   'sizeof(ftmpc_estimator), sizeof(ftmpc_sensor), sizeof(ftmpc_actuator), sizeof(ftmpc_outcomes), sizeof(ftmpc_plant_model), '
                   'sizeof(ftmpc_mission), sizeof(ftmpc_fault_schedule));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.ftmpc_diagnosis) == 152
    for f, off in zip(FIELDS, OFFSETS):
        assert int(got[f]) == getattr(_lib.ftmpc_diagnosis, f).offset == off, f
    # no existing struct changed
    assert int(got["estimator"]) == C.sizeof(_lib.ftmpc_estimator) == 136
    assert int(got["sensor"]) == C.sizeof(_lib.ftmpc_sensor) == 96
    assert int(got["actuator"]) == C.sizeof(_lib.ftmpc_actuator) == 80
    assert int(got["outcomes"]) == C.sizeof(_lib.ftmpc_outcomes) == 120
    assert int(got["plant"]) == C.sizeof(_lib.ftmpc_plant_model) == 48
    assert int(got["mission"]) == C.sizeof(_lib.ftmpc_mission) == 56
    assert int(got["schedule"]) == C.sizeof(_lib.ftmpc_fault_schedule) == 56


# ---------------------------------------------------------------------------------------------------------------------------
# diagnosis.py
# ---------------------------------------------------------------------------------------------------------------------------
def _signature_error(steps, seed, wmax=0.6):
    """Largest relative error of (a_v, a_w) against the differences of `steps` RK4 steps with thruster i forced to level l and with
    the commanded values, over random states with |w| <= wmax, every thruster and both levels."""
    from ft_mpc_amd.diagnosis import propagate, signature
    from ft_mpc_amd.estimators import _body_to_inertial
    cfg = _cfg()
    rng = np.random.default_rng(seed)
    ub, stuck = np.full(NT, F_MAX), np.zeros(NT)
    levels = (0.0, F_MAX)
    ev = ew = 0.0
    for _ in range(12):
        x0 = _state(rng, wmax)
        u = rng.uniform(0.2 * F_MAX, 0.8 * F_MAX, size=(steps, NT))
        xt, n, acc = x0.copy(), 0, np.zeros(NT)
        for k in range(steps):
            xt, n, acc = propagate(xt, n, acc, u[k], ub, stuck, cfg)
        assert n == steps and np.allclose(acc, u.sum(0))
        a_v, a_w = signature(n, acc, levels, cfg)
        M = _body_to_inertial(xt[6:10])
        for i in range(NT):
            for l, lv in enumerate(levels):
                ubf, stf = ub.copy(), stuck.copy()
                ubf[i], stf[i] = 0.0, lv
                xf = x0.copy()
                for k in range(steps):
                    xf = _rk4(xf, u[k], ubf, stf, cfg)
                dv, dw = M.T @ (xf[3:6] - xt[3:6]), xf[10:13] - xt[10:13]
                if np.linalg.norm(a_v[i, l]) > 0:
                    ev = max(ev, np.linalg.norm(dv - a_v[i, l]) / np.linalg.norm(a_v[i, l]))
                ew = max(ew, np.linalg.norm(dw - a_w[i, l]) / np.linalg.norm(a_w[i, l]))
    return ev, ew


def test_signature_is_the_first_order_effect_of_a_stuck_thruster():
    """One RK4 step of oracle.refmath.plant_dx_dt with thruster i forced to level l (ub_i = 0, stuck_i = level) against one with the
    commanded value, the velocity difference rotated by M(q~)' with q~ the quaternion of the nominal prediction: equal to a_v, a_w to
    first order in dt.  Also checks that diagnosis.propagate is that nominal step.  Measured at |w| up to 0.6 rad/s, every thruster
    of the 8-thruster vehicle, levels 0 and f_max: relative error 2.71e-2 of |a_v|, 1.04e-2 of |a_w|; the bound is 3 times
    that."""
    ev, ew = _signature_error(1, 31)
    print(f"signature, one step: relative error {ev:.3e} (velocity), {ew:.3e} (rate)")
    assert ev <= 3 * SIG1_V and ew <= 3 * SIG1_W


def test_every_three_accumulates_the_three_step_signature():
    """every = 3: the model runs three steps between two tests; n = 3 and acc = the sum of the three effective commands give the
    signature of the three-step difference, to first order in 3 dt.  Measured as above: 1.39e-1 (velocity), 4.07e-2 (rate); bound 3 times
    that.  In a replay with every = 3 only the campaign steps c with c % 3 == 0 test, and each test sees n = 3.  step0 = 2 puts the
    onset (loop step 10, c = 12) on a re-anchor, so the first window after it holds the fault in all three steps: the hypothesis
    assumes the level over the whole window, and a fault that starts inside one shows only a part of its signature there."""
    from ft_mpc_amd.diagnosis import replay
    ev, ew = _signature_error(3, 32)
    print(f"signature, three steps: relative error {ev:.3e} (velocity), {ew:.3e} (rate)")
    assert ev <= 3 * SIG3_V and ew <= 3 * SIG3_W
    cfg = _cfg()
    run = _open_loop("stuck_on")
    spec = dict(_spec(), every=3)
    for b in (0, 5):
        r = replay(run["meas"][:, b], run["u"], run["ub"], run["stuck"], spec, cfg, step0=2)
        tested = ~np.isnan(r["peak"])
        c = 2 + np.arange(run["T"])
        assert not tested[c % 3 != 0].any() and tested[(c % 3 == 0) & (c >= 6)][:2].all()
        assert r["detections"] == [(15, b % NT, 1)]


SIG1_V, SIG1_W, SIG3_V, SIG3_W = 2.712e-2, 1.041e-2, 1.386e-1, 4.072e-2      # the measured relative errors of the two tests above


def _spec(**kw):
    from ft_mpc_amd.diagnosis import default_sigma
    return dict(dict(every=1, levels=(0.0, F_MAX), resid_sigma=default_sigma(SIGMA), drift_sigma=(0.0, 0.0), threshold=18.0,
                     max_detect=2), **kw)


@functools.lru_cache(maxsize=None)
def _open_loop(kind):
    """64 vehicles, 60 steps of an open-loop command sequence uniform in [0, f_max / 2] (the same for every vehicle) through
    dispersion.plant_step, measured with sensors.measure (sigma = SIGMA).  kind "healthy": no fault; "stuck_on": thruster b % NT of
    vehicle b stuck on at f_max from step 10 in the plant, the controller's pattern healthy throughout."""
    from ft_mpc_amd.dispersion import plant_step
    from ft_mpc_amd.sensors import measure
    cfg = _cfg()
    B, T, onset = 64, 60, 10
    rng = np.random.default_rng(14)
    ub, stuck = np.full(NT, F_MAX), np.zeros(NT)
    x = qo.make_batch(B, 10, NT, 0, 23)[0]
    u = rng.uniform(0.0, 0.5 * F_MAX, size=(T, NT))
    meas = np.empty((T, B, 13))
    for t in range(T):
        meas[t] = measure(x, t, SIGMA, seed=78)
        for b in range(B):
            pub, pst = ub.copy(), stuck.copy()
            if kind == "stuck_on" and t >= onset:
                pub[b % NT], pst[b % NT] = 0.0, F_MAX
            x[b] = plant_step(x[b], u[t], pub, pst, {}, cfg)
            x[b, 6:10] /= np.linalg.norm(x[b, 6:10])
    return dict(meas=meas, u=u, ub=ub, stuck=stuck, B=B, T=T, onset=onset)


def test_no_false_alarm_on_64_healthy_vehicles():
    """Open loop, 64 healthy vehicles, 60 steps, NT = 8, L = 2, commands uniform in [0, f_max / 2], sensor sigma (1e-2, 5e-3, 1e-2,
    5e-3), resid_sigma = default_sigma, threshold 18.  By the Wald / Lorden bound a CUSUM with threshold h has a mean time between
    false alarms of at least e^h per hypothesis: 64 x 60 x 16 hypothesis-steps give at most about 1e-3 expected false alarms (the
    residual's noise is negatively correlated from step to step, which only lengthens that time).  Expected: no detection.
    Measured: the largest statistic over the whole run is 5.51."""
    from ft_mpc_amd.diagnosis import replay
    cfg = _cfg()
    run = _open_loop("healthy")
    peak = 0.0
    for b in range(run["B"]):
        r = replay(run["meas"][:, b], run["u"], run["ub"], run["stuck"], _spec(), cfg)
        assert r["detections"] == [], b
        peak = max(peak, np.nanmax(r["peak"]))
        assert np.all(r["ub"] == F_MAX) and np.all(r["stuck"] == 0.0)
    print(f"healthy open loop: largest statistic {peak:.2f} (threshold 18)")
    assert peak < 18.0


def test_stuck_on_thruster_is_isolated_within_two_tests():
    """The same run with thruster b % NT stuck on at f_max from step 10: every vehicle is detected, with the right thruster and the
    right level, no second detection follows, and the pattern the replay returns is the fault's.  The rate signature is about 0.1 rad/s
    per step against a residual sigma of 7e-3, so one or two tests are expected.  Measured: delays of 1 and 2 steps, the largest 2
    (STUCK_ON_MAX_DELAY; the device's noisy closed loop is capped at this plus one test)."""
    from ft_mpc_amd.diagnosis import pattern, replay, score
    cfg = _cfg()
    run = _open_loop("stuck_on")
    dets, faults = [], []
    for b in range(run["B"]):
        r = replay(run["meas"][:, b], run["u"], run["ub"], run["stuck"], _spec(), cfg)
        dets.append(r["detections"])
        faults.append([(run["onset"], b % NT, 1)])
        pu, ps = pattern(run["ub"], run["stuck"], r["detections"], (0.0, F_MAX))
        assert np.array_equal(pu, r["ub_end"]) and np.array_equal(ps, r["stuck_end"])
        assert np.array_equal(r["ub"][-1], r["ub_end"])
    sc = score(faults, dets)
    delays = [d for d in sc["delay"] if d is not None]
    print(f"stuck-on open loop: delays {sorted(set(delays))}, score {dict(sc, delay=None)}")
    assert sc["missed"] == 0 and sc["wrong_thruster"] == 0 and sc["wrong_level"] == 0 and sc["false_alarms"] == 0
    assert min(delays) >= 1 and max(delays) == STUCK_ON_MAX_DELAY


def test_dead_thruster_is_found_once_it_is_commanded():
    """Zero noise.  Thruster i is dead in the plant from the start and commanded 0 until step 6: it has no signature.  From step 6
    on it is commanded c.  With resid_sigma = 1e-3 one test of the exact signature adds z1 = |a_v|^2 / (2 s_v) + |a_w|^2 / (2 s_w);
    c = 0.3 f_max puts z1 far above the threshold and the detection comes at step 7, the first test after the command acted;
    c with z1 = 0.3 x threshold is detected at the fourth test (give or take one: the signature is first order), after the statistic
    has accumulated.  Every thruster in turn: never a wrong thruster, always level 0, and nothing before the command.  (The other
    thrusters are commanded in [0, f_max / 2]: the thruster opposite to i stuck on at f_max would push the same way by at least
    f_max / 2, so c = 0.3 f_max keeps the two hypotheses apart by more than the first-order error; at c = f_max / 2 they can tie.)"""
    from ft_mpc_amd.diagnosis import replay, signature
    from ft_mpc_amd.dispersion import plant_step
    cfg = _cfg()
    T, s0 = 24, 6
    spec = _spec(resid_sigma=(1e-3, 1e-3))
    rng = np.random.default_rng(15)
    x0 = qo.make_batch(1, 10, NT, 0, 24)[0][0]
    ub, stuck = np.full(NT, F_MAX), np.zeros(NT)
    for i in range(NT):
        a_v, a_w = signature(1, np.full(NT, 1.0), (0.0,), cfg)      # per unit of command
        z_unit = (a_v[i, 0] @ a_v[i, 0] + a_w[i, 0] @ a_w[i, 0]) / (2 * 1e-6)
        c_small = np.sqrt(0.3 * 18.0 / z_unit)                     # z1 = 0.3 x threshold
        for c, late in ((0.3 * F_MAX, False), (c_small, True)):
            u = rng.uniform(0.0, 0.5 * F_MAX, size=(T, NT))
            u[:s0, i], u[s0:, i] = 0.0, c
            pub = ub.copy()
            pub[i] = 0.0
            x, meas = x0.copy(), np.empty((T, 13))
            for t in range(T):
                meas[t] = x
                x = plant_step(x, u[t], pub, stuck, {}, cfg)
                x[6:10] /= np.linalg.norm(x[6:10])
            r = replay(meas, u, ub, stuck, spec, cfg)
            assert len(r["detections"]) == 1, (i, c, r["detections"])
            step, thr, lvl = r["detections"][0]
            assert (thr, lvl) == (i, 0), (i, c, r["detections"])
            assert np.nanmax(r["peak"][:s0 + 1]) < 1e-6 * 18.0      # nothing before the command acted
            if late:
                assert s0 + 3 <= step <= s0 + 5, (i, step)      # 0.3 x threshold per test, to first order: the fourth test
            else:
                assert step == s0 + 1, (i, step)


def test_max_detect_and_the_tie_rule():
    """max_detect = 1: after one detection no test runs (the statistics stay 0) although a second thruster fails.  Tie: on a vehicle
    whose thrusters 2 and 5 have the same column of D and get the same command the two hypotheses have bit-identical statistics;
    the detection goes to the lower index."""
    from ft_mpc_amd.diagnosis import replay
    from ft_mpc_amd.dispersion import plant_step
    from ft_mpc_amd.estimators import _cfg_model
    cfg = _cfg()
    run = _open_loop("stuck_on")
    r = replay(run["meas"][:, 3], run["u"], run["ub"], run["stuck"], _spec(max_detect=1), cfg)
    assert len(r["detections"]) == 1
    k = r["detections"][0][0]
    assert np.isnan(r["peak"][k + 1:]).all() and np.all(r["llr_hist"][k + 1:] == 0.0) and r["llr_hist"][k].max() > 18.0
    D = _cfg_model(cfg)[0].copy()
    D[:, 5] = D[:, 2]
    cfg2 = _cfg(D=D)
    T = 12
    rng = np.random.default_rng(16)
    u = rng.uniform(0.0, 0.5 * F_MAX, size=(T, NT))
    u[:, 5] = u[:, 2]
    ub, stuck = np.full(NT, F_MAX), np.zeros(NT)
    pub, pst = ub.copy(), stuck.copy()
    pub[5], pst[5] = 0.0, F_MAX
    x, meas = qo.make_batch(1, 10, NT, 0, 25)[0][0], np.empty((T, 13))
    for t in range(T):
        meas[t] = x
        x = plant_step(x, u[t], pub if t >= 4 else ub, pst if t >= 4 else stuck, {}, cfg2)
        x[6:10] /= np.linalg.norm(x[6:10])
    r = replay(meas, u, ub, stuck, _spec(resid_sigma=(1e-3, 1e-3)), cfg2)
    assert r["detections"][0] == (5, 2, 1)
    h = r["llr_hist"][5].reshape(NT, 2)
    assert h[2, 1] == h[5, 1] == h.max()


def test_replay_continues_bit_for_bit():
    """A replay of 60 steps equals one of 25 and one of 35 with state, llr, the detections and the pattern handed over."""
    from ft_mpc_amd.diagnosis import replay
    cfg = _cfg()
    run = _open_loop("stuck_on")
    for every in (1, 3):
        spec = _spec(every=every)
        whole = replay(run["meas"][:, 9], run["u"], run["ub"], run["stuck"], spec, cfg)
        a = replay(run["meas"][:25, 9], run["u"][:25], run["ub"], run["stuck"], spec, cfg)
        b = replay(run["meas"][25:, 9], run["u"][25:], a["ub_end"], a["stuck_end"], spec, cfg, step0=25, state=a["state"], llr=a["llr"],
                   detections=a["detections"])
        assert np.array_equal(np.concatenate([a["llr_hist"], b["llr_hist"]]), whole["llr_hist"])
        assert b["detections"] == whole["detections"] and np.array_equal(b["state"], whole["state"])


def test_default_sigma_and_score():
    from ft_mpc_amd.diagnosis import default_sigma, detections_of, score
    s = default_sigma(SIGMA, (0, 3e-3, 0, 4e-3))
    assert np.allclose(s, [np.sqrt(2 * 25e-6 + 9e-6), np.sqrt(2 * 25e-6 + 16e-6)])
    det = detections_of(np.array([[12, -1], [-1, -1], [5, 30]]), np.array([[3, -1], [-1, -1], [1, 2]]), np.array([[1, -1], [-1, -1], [0, 1]]))
    assert det == [[(12, 3, 1)], [], [(5, 1, 0), (30, 2, 1)]]
    sc = score([[(10, 3, 1)], [(10, 4, 0)], [(20, 2, 0)]], det)
    assert sc == dict(delay=[2, None, 10], missed=1, wrong_thruster=0, wrong_level=1, false_alarms=1)
    # an event that is missed does not take the detection of a later one; what is left over blames the wrong thruster
    assert score([[(3, 1, 0), (5, 4, 0)]], [[(7, 4, 0)]]) == dict(delay=[None, 2], missed=1, wrong_thruster=0, wrong_level=0, false_alarms=0)
    assert score([[(3, 1, 0)]], [[(2, 1, 0), (6, 5, 1)]]) == dict(delay=[3], missed=0, wrong_thruster=1, wrong_level=0, false_alarms=1)


def test_python_refuses_what_the_library_refuses():
    from ft_mpc_amd.diagnosis import request
    B, T = 4, 3
    ok = dict(every=1, levels=(0.0, F_MAX), resid_sigma=(1e-2, 1e-2), drift_sigma=(0, 0), threshold=18.0, max_detect=2)
    r = request(ok, B, T, NT)
    assert r["every"] == 1 and r["fields"] == ("detect", "pattern", "llr_hist", "state")
    assert np.array_equal(request({k: v for k, v in ok.items() if k != "levels"}, B, T, NT, f_max=F_MAX)["levels"], [0.0, F_MAX])
    st = np.zeros((B, 14 + NT))
    st[:, 9] = 1.0
    det = tuple(np.full((B, 2), -1, np.int32) for _ in range(3))
    llr = np.zeros((B, 2 * NT))

    def dets(step, thr, lvl):
        d = [a.copy() for a in det]
        d[0][1], d[1][1], d[2][1] = step, thr, lvl
        return tuple(d)
    bad_n = st.copy()
    bad_n[2, 13] = -1.0
    for bad, kw, word in [
            (dict(ok, every=0), {}, "every"), (dict(ok, every=2), dict(estimator=dict(every=1)), "differs from estimator"),
            (dict(ok, levels=()), {}, "levels"), (dict(ok, levels=(0, 1, 2, 3, 3.4)), {}, "levels"),
            (dict(ok, levels=(-1.0, 1.0)), {}, "levels"), (dict(ok, levels=(1.0, 1.0)), {}, "strictly increasing"),
            (dict(ok, levels=(0.0, np.inf)), {}, "levels"), (dict(ok, max_detect=0), {}, "max_detect"), (dict(ok, max_detect=9), {}, "max_detect"),
            (dict(ok, resid_sigma=(0, 1e-2)), {}, "resid_sigma"), (dict(ok, resid_sigma=(1e-2, np.nan)), {}, "resid_sigma"),
            (dict(ok, resid_sigma=(1e-2,)), {}, "resid_sigma"), (dict(ok, drift_sigma=(-1e-3, 0)), {}, "drift_sigma"),
            (dict(ok, drift_sigma=(0, np.inf)), {}, "drift_sigma"), (dict(ok, threshold=0.0), {}, "threshold"),
            (dict(ok, threshold=np.inf), {}, "threshold"), ({k: v for k, v in ok.items() if k != "threshold"}, {}, "threshold"),
            ({k: v for k, v in ok.items() if k != "resid_sigma"}, {}, "resid_sigma"),
            (dict(ok, llr=llr), {}, "require"), (dict(ok, detect=det), {}, "require"), (dict(ok, state=st), {}, "requires diagnosis\\['detect'\\]"),
            (dict(ok, state=np.where(np.arange(14 + NT) == 3, np.nan, st), detect=det), {}, "state"), (dict(ok, state=st[:3], detect=det), {}, "state"),
            (dict(ok, state=bad_n, detect=det), {}, "n < 0"), (dict(ok, state=st, detect=det, llr=np.where(np.arange(2 * NT) == 1, np.inf, llr)), {}, "llr"),
            (dict(ok, state=st, detect=det[:2]), {}, "detect"), (dict(ok, state=st, detect=dets([-1, 4], [-1, 0], [-1, 0])), {}, "used slot after"),
            (dict(ok, state=st, detect=dets([-2, -1], [0, 0], [0, 0])), {}, "below -1"),
            (dict(ok, state=st, detect=dets([4, -1], [NT, -1], [0, -1])), {}, "outside"),
            (dict(ok, state=st, detect=dets([4, -1], [0, -1], [2, -1])), {}, "outside"),
            (ok, dict(sensor=dict(predict=True, latency=2)), "predicting sensor"),
            (dict(ok, fields=("detect", "gain")), {}, "fields"), (dict(ok, gain=1), {}, "unknown")]:
        with pytest.raises(ValueError, match=word):
            request(bad, B, T, NT, **kw)
    r = request(dict(ok, state=st, detect=dets([4, -1], [7, -1], [1, -1]), llr=llr), B, T, NT, estimator=dict(every=1),
                sensor=dict(predict=True, latency=2))
    assert r["state"] is not st and r["detect"][0].dtype == np.int32
