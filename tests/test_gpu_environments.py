"""GPU: a disturbance that varies over the run (ftmpc_environment_kernel; ftmpc_simulate_environment_batch,
ftmpc_simulate_wrench_environment_batch, ftmpc_multi_simulate_environment_batch; BatchedMPC.simulate(environment=...)).

Shapes: N = 5, 8 thrusters, T = 12, B = 130 (three blocks of 64 lanes with a partial last one, and [k][B] arrays with B % 64 != 0);
noise = 0 wherever a run is replayed.  The wrench history is held to ft_mpc_amd.environments.replay at rtol 1e-12 + atol 1e-12 (the
bound tests/test_gpu_sensors.py holds the device's Gaussian samples to: the two sides differ by log / cos / sin of the device's
library and the host's); the plant's states replay step by step from the run's own histories through dispersion.plant_step (with an
actuator: actuators.step) with wrench_hist[t] as that step's force and torque, at the bound of tests/test_gpu_plant_dispersion.py
and tests/test_gpu_actuators.py, rtol 1e-12 + atol 1e-12.  Continued runs, slices of a campaign and the multi-GPU driver are compared
bit for bit.

Measured on an MI355X (printed by the tests): wrench_hist within 6.1e-16 of the restatement, x_hist within 4.4e-16 of the plant's
definition (the constant base alone misses step 0 by 6e-2), est_err_sq within 4.4e-16 (relative) of the sum over the histories; the
random-walk disturbance model against the constant one on a sinusoid: 0.047 (force) and 0.015 (torque) of the summed squared error."""
import ctypes as C

import numpy as np
import pytest

import ft_mpc_amd
from ft_mpc_amd import _lib
from ft_mpc_amd import actuators as AC
from ft_mpc_amd import dispersion as DP
from ft_mpc_amd import environments as EV
from ft_mpc_amd.sharding import MultiGPUMPC
from oracle import qp_oracle as qo
from test_gpu_actuators import _entry
from test_gpu_estimators import EALL, SIGMA, _prior, _sensor, _spec, wrench24  # noqa: F401  (a fixture)
from test_gpu_outcomes import _hover, term  # noqa: F401  (term: a fixture)

pytestmark = pytest.mark.gpu
N, NT, T, B = 5, 8, 12, 130
DT = 0.1
ZERO = (0.0,) * 4
EALL_ENV = ("wrench", "state")
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)


def _batch(seed=31, Bv=B, n=N, nt=NT):
    return qo.make_batch(Bv, n, nt, 0, seed)[:3]


def _plant_base(Bv, seed=8):
    rng = np.random.default_rng(seed)
    return dict(force=rng.uniform(-0.05, 0.05, (Bv, 3)), torque=rng.uniform(-0.005, 0.005, (Bv, 3)))


def _parts(Bv, seed=9, step0=0):
    """the four components, each as the keys it needs"""
    rng = np.random.default_rng(seed)
    window = np.stack([step0 + rng.integers(0, 8, Bv), step0 + rng.integers(3, 16, Bv)], axis=1).astype(np.int32)
    return dict(
        markov=dict(sigma=(0.3, 0.02), tau=(1.5, 0.6)),
        periodic=dict(period=2.3, amp_force=rng.normal(size=(Bv, 3)) * 0.2, amp_torque=rng.normal(size=(Bv, 3)) * 0.02,
                      phase=rng.uniform(0, 2 * np.pi, Bv)),
        kick=dict(kick=rng.normal(size=(Bv, 6)) * np.r_[np.full(3, 0.5), np.full(3, 0.05)], window=window),
    )


def _all(Bv, seed=9, step0=0, **kw):
    p = _parts(Bv, seed, step0)
    return dict(seed=1234, step0=step0, **p["markov"], **p["periodic"], **p["kick"], **kw)


def _sim(mpc, x0, ub, stuck, Tn=T, n=N, xr=None, **kw):
    return mpc.simulate(x0, ub, stuck, _hover(n, Tn) if xr is None else xr, Tn, noise=ZERO, seed=5, return_inputs=True, return_states=True,
                        **kw)


def _check_wrench(out, env, plant=None, index0=0, index_total=None):
    Tn, Bv = out["environment"]["wrench"].shape[:2]
    ref = EV.replay(Bv, Tn, DT, env, plant, index0, index_total)
    got = out["environment"]
    worst = np.abs(got["wrench"] - ref["wrench"]).max()
    print(f"wrench_hist against environments.replay: max deviation {worst:.3e}")
    np.testing.assert_allclose(got["wrench"], ref["wrench"], rtol=1e-12, atol=1e-12)
    if "state" in got:
        np.testing.assert_allclose(got["state"], ref["state"], rtol=1e-12, atol=1e-12)
    return ref


def _renorm(x):
    x = x.copy()
    x[6:10] *= 1.0 / np.sqrt((x[6:10] ** 2).sum())
    return x


def _check_plant(out, x0, ub, stuck, cfg, plant=None, actuator=None):
    """x_hist step by step from the run's own commands, with wrench_hist[t] as the step's force and torque (noise = 0)."""
    xh, uh, wh = out["x_hist"], out["u"], out["environment"]["wrench"]
    Tn, Bv = xh.shape[:2]
    rest = {k: v for k, v in (plant or {}).items() if k not in ("force", "torque")}
    valve = np.zeros_like(ub)
    worst, moved = 0.0, 0.0
    for t in range(Tn):
        for b in range(Bv):
            row = dict({k: v[b] for k, v in rest.items()}, force=wh[t, b, 0:3], torque=wh[t, b, 3:6])
            prev = x0[b] if t == 0 else xh[t - 1, b]
            if actuator is None:
                x = DP.plant_step(prev, uh[t, b], ub[b], stuck[b], row, cfg)
            else:
                r = AC.step(prev, uh[t, b], ub[b], stuck[b], actuator, valve[b], row, cfg)
                x, valve[b] = r["x"], r["state"]
            x = _renorm(x)
            worst = max(worst, np.abs(xh[t, b] - x).max())
            np.testing.assert_allclose(xh[t, b], x, rtol=1e-12, atol=1e-12, err_msg=f"step {t}, vehicle {b}")
            if t == 0:      # the constant base alone must not explain the run
                row0 = dict(row, force=(plant or {}).get("force", np.zeros((Bv, 3)))[b], torque=(plant or {}).get("torque", np.zeros((Bv, 3)))[b])
                x_base = DP.plant_step(prev, uh[t, b], ub[b], stuck[b], row0, cfg) if actuator is None else \
                    AC.step(prev, uh[t, b], ub[b], stuck[b], actuator, np.zeros(ub.shape[1]), row0, cfg)["x"]
                moved = max(moved, np.abs(_renorm(x_base) - xh[t, b]).max())
    print(f"plant replay: max |x_hist - definition| = {worst:.3e}; the base alone misses step 0 by up to {moved:.3e}")
    assert moved > 1e-6
    assert np.array_equal(out["x"], xh[-1])


# ---------------------------------------------------------------------------------------------------------------------------
# 1: NULL and trivial
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_plant", [False, True])
def test_null_and_trivial_environment_change_nothing(gpu_mpc_factory, with_plant):
    x0, ub, stuck = _batch()
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    kw = dict(plant=_plant_base(B)) if with_plant else {}
    ref = mpc.simulate(x0, ub, stuck, _hover(N, T), T, noise=(1e-3,) * 4, seed=5, return_inputs=True, return_states=True, **kw)
    for env in (None, {}, dict(seed=9, step0=0, sigma=(0.0, 0.0), tau=(0.0, -1.0), period=0.0)):
        out = mpc.simulate(x0, ub, stuck, _hover(N, T), T, noise=(1e-3,) * 4, seed=5, return_inputs=True, return_states=True,
                           environment=env, **kw)
        for k in ("x", "u", "x_hist"):
            assert np.array_equal(out[k], ref[k]), (env, k)
        assert ("environment" in out) == (env is not None)


# ---------------------------------------------------------------------------------------------------------------------------
# 2, 3: the wrench history against the restatement, the plant against the wrench history
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", ["markov", "periodic", "kick"])
def test_each_component_alone(gpu_mpc_factory, part):
    x0, ub, stuck = _batch()
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    env = dict(_parts(B)[part], seed=77, fields=EALL_ENV if part == "markov" else ("wrench",))
    out = _sim(mpc, x0, ub, stuck, environment=env)
    _check_wrench(out, env)
    w = out["environment"]["wrench"]
    assert np.abs(w).max() > 0.1
    if part == "periodic":      # amp_force alone, amp_torque alone: the other half is exactly zero
        for key, sl in (("amp_force", slice(3, 6)), ("amp_torque", slice(0, 3))):
            e1 = {k: v for k, v in env.items() if k not in ("amp_force", "amp_torque")}
            e1[key] = env[key]
            o1 = _sim(mpc, x0, ub, stuck, environment=e1)
            _check_wrench(o1, e1)
            assert not o1["environment"]["wrench"][:, :, sl].any()


def test_all_components_over_a_plant_base_and_the_plant_replay(gpu_mpc_factory):
    x0, ub, stuck = _batch()
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    plant = dict(_plant_base(B), mass=16.8 * (1 + np.random.default_rng(1).uniform(-0.2, 0.2, B)))
    env = _all(B, fields=("wrench",))                                # (a stationary start drawn on the device)
    out = _sim(mpc, x0, ub, stuck, environment=env, plant=plant)
    _check_wrench(out, env, plant)
    _check_plant(out, x0, ub, stuck, mpc.cfg, plant)
    # without a plant dict the base is zero and the plant is the nominal one
    out0 = _sim(mpc, x0, ub, stuck, environment=env)
    _check_wrench(out0, env)
    _check_plant(out0, x0, ub, stuck, mpc.cfg)


def test_plant_replay_with_an_actuator(gpu_mpc_factory):
    x0, ub, stuck = _batch(seed=32)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    plant = _plant_base(B)
    act = dict(substeps=2, tau_on=0.03, tau_off=0.02)
    env = _all(B, fields=("wrench",))
    out = _sim(mpc, x0, ub, stuck, environment=env, plant=plant, actuator=act)
    _check_wrench(out, env, plant)
    _check_plant(out, x0, ub, stuck, mpc.cfg, plant, actuator=act)


# ---------------------------------------------------------------------------------------------------------------------------
# 4: the kick window
# ---------------------------------------------------------------------------------------------------------------------------
def test_kick_acts_exactly_inside_its_window(gpu_mpc_factory):
    x0, ub, stuck = _batch()
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    step0 = 40
    kick = 1.0 + np.arange(B * 6, dtype=np.float64).reshape(B, 6)
    window = np.zeros((B, 2), np.int32)
    b = np.arange(B)
    window[:, 0] = step0 - 3 + b % 19                               # opens before, at and inside the run, and after it
    window[:, 1] = window[:, 0] + (b % 7) - 1                       # to < from, to == from, and up to five steps
    window[5] = (step0 + 10, step0 + 400)                           # past the run
    window[6] = (0, step0 + 8)                                      # straddles the continuation below
    env = dict(step0=step0, kick=kick, window=window, fields=("wrench",))
    first = _sim(mpc, x0, ub, stuck, 5, environment=env)
    second = _sim(mpc, first["x"], ub, stuck, 7, environment=dict(env, step0=step0 + 5))
    w = np.concatenate([first["environment"]["wrench"], second["environment"]["wrench"]])
    c = step0 + np.arange(T)
    inside = (window[None, :, 0] <= c[:, None]) & (c[:, None] < window[None, :, 1])
    assert np.array_equal(w, np.where(inside[:, :, None], kick[None], 0.0))
    assert inside.any(axis=0).sum() > B // 4 and (~inside.any(axis=0)).sum() > B // 4 and inside[4:6, 6].all() and not inside[8:, 6].any()


# ---------------------------------------------------------------------------------------------------------------------------
# 5: continuation
# ---------------------------------------------------------------------------------------------------------------------------
def test_continued_wrench_and_state_are_the_whole_runs(gpu_mpc_factory):
    x0, ub, stuck = _batch()
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    env = _all(B, fields=EALL_ENV)
    plant = _plant_base(B)
    whole = _sim(mpc, x0, ub, stuck, environment=env, plant=plant)
    first = _sim(mpc, x0, ub, stuck, 5, environment=env, plant=plant)
    second = _sim(mpc, first["x"], ub, stuck, 7, environment=dict(env, step0=5, state=first["environment"]["state"]), plant=plant)
    assert np.array_equal(np.concatenate([first["environment"]["wrench"], second["environment"]["wrench"]]), whole["environment"]["wrench"])
    assert np.array_equal(second["environment"]["state"], whole["environment"]["state"])
    # and from a stationary start drawn on the device (no state asked back), the first five steps are the whole run's first five
    dev = _sim(mpc, x0, ub, stuck, 5, environment=dict(env, fields=("wrench",)), plant=plant)
    np.testing.assert_allclose(dev["environment"]["wrench"], whole["environment"]["wrench"][:5], rtol=1e-12, atol=1e-12)


def test_continued_run_with_the_estimator_is_the_whole_run(gpu_mpc_factory):
    x0, ub, stuck = _batch()
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = _sensor(B, NT)
    xh, cov = _prior(x0)
    est = _spec(3, xhat=xh, cov=cov, fields=EALL)
    env = _all(B, fields=EALL_ENV)
    plant = _plant_base(B)
    xr = _hover(N, T + 2)
    whole = _sim(mpc, x0, ub, stuck, xr=xr, environment=env, plant=plant, sensor=sen, estimator=est)
    first = _sim(mpc, x0, ub, stuck, 5, xr=xr[:, :5 + N + 2], environment=env, plant=plant, sensor=sen, estimator=est)
    sen2 = dict(sen, pending=first["sensor"]["pending"], step0=5)
    est2 = dict(est, xhat=first["estimator"]["xhat"], cov=first["estimator"]["cov"])
    env2 = dict(env, step0=5, state=first["environment"]["state"])
    second = _sim(mpc, first["x"], ub, stuck, 7, xr=xr[:, 5:], environment=env2, plant=plant, sensor=sen2, estimator=est2)
    assert np.array_equal(second["x"], whole["x"])
    for k in ("x_hist", "u"):
        assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    assert np.array_equal(np.concatenate([first["environment"]["wrench"], second["environment"]["wrench"]]), whole["environment"]["wrench"])
    assert np.array_equal(second["environment"]["state"], whole["environment"]["state"])
    assert np.array_equal(second["estimator"]["xhat"], whole["estimator"]["xhat"])


# ---------------------------------------------------------------------------------------------------------------------------
# 6, 7: slices of a campaign, the multi-GPU driver on one device
# ---------------------------------------------------------------------------------------------------------------------------
PER_VEHICLE = ("amp_force", "amp_torque", "phase", "kick", "window", "state")


def test_slices_and_device_slots_equal_the_whole():
    x0, ub, stuck = _batch()
    plant = _plant_base(B)
    env = _all(B, fields=EALL_ENV, state=np.random.default_rng(4).normal(size=(B, 6)) * 0.1)

    def run(mpc, lo, hi, **kw):
        e = dict(env, **{k: env[k][lo:hi] for k in PER_VEHICLE})
        return _sim(mpc, x0[lo:hi], ub[lo:hi], stuck[lo:hi], environment=e, plant={k: v[lo:hi] for k, v in plant.items()}, **kw)

    def fresh(lo, hi, **kw):
        mpc = ft_mpc_amd.BatchedMPC(N=N, NT=NT, dtype="f32")
        try:
            return run(mpc, lo, hi, **kw)
        finally:
            mpc.close()
    whole = fresh(0, B)
    parts = [fresh(0, 70, index0=0, index_total=B), fresh(70, B, index0=70, index_total=B)]
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f32"), devices=[0] * 3)
    try:
        multi = run(m, 0, B)
    finally:
        m.close()
    assert np.array_equal(np.concatenate([p["x"] for p in parts]), whole["x"]) and np.array_equal(multi["x"], whole["x"])
    for k in ("x_hist", "u"):
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), whole[k]), k
        assert np.array_equal(multi[k], whole[k]), k
    for k, axis in (("wrench", 1), ("state", 0)):
        assert np.array_equal(np.concatenate([p["environment"][k] for p in parts], axis=axis), whole["environment"][k]), k
        assert np.array_equal(multi["environment"][k], whole["environment"][k]), k
    _check_wrench(whole, env, plant)


# ---------------------------------------------------------------------------------------------------------------------------
# 8: the two-stage wrench form, float64
# ---------------------------------------------------------------------------------------------------------------------------
def test_on_the_wrench_form(gpu_mpc_factory, wrench24):  # noqa: F811
    w, n, Tn = wrench24, 10, 8
    mpc = gpu_mpc_factory(N=n, NT=16, dtype="f64", max_iters=60, terminal_set=w["term"])
    plant = _plant_base(24)
    env = _all(24, fields=("wrench",))
    out = mpc.simulate(w["x0"], w["ub"], w["stuck"], w["xr"][:, :Tn + n], Tn, noise=ZERO, seed=w["seed"], formulation="wrench",
                       sqp_iters=0, return_inputs=True, return_states=True, plant=plant, environment=env)
    _check_wrench(out, env, plant)
    _check_plant(out, w["x0"], w["ub"], w["stuck"], mpc.cfg, plant)
    assert out["u"].any()


# ---------------------------------------------------------------------------------------------------------------------------
# 9, 10: the estimate's error against the wrench
# ---------------------------------------------------------------------------------------------------------------------------
def _dist(**kw):
    return dict(dict(p0=(0.5, 0.05), proc_sigma=(1e-2, 1e-3), compensate=True, fields=("force_hist", "torque_hist", "state")), **kw)


def test_estimate_error_is_the_sum_over_the_histories(gpu_mpc_factory):
    x0, ub, stuck = _batch()
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = _sensor(B, NT)
    xh, cov = _prior(x0)
    est = _spec(1, xhat=xh, cov=cov, fields=EALL)
    env = _all(B, fields=("wrench", "state", "est_err_sq"))
    plant = _plant_base(B)
    xr = _hover(N, T + 2)
    whole = _sim(mpc, x0, ub, stuck, xr=xr, environment=env, plant=plant, sensor=sen, estimator=est, disturbance=_dist())
    d, e = whole["disturbance"], whole["environment"]
    ref = np.stack([((d["force_hist"] - e["wrench"][:, :, 0:3]) ** 2).sum(axis=(0, 2)),
                    ((d["torque_hist"] - e["wrench"][:, :, 3:6]) ** 2).sum(axis=(0, 2))], axis=1)
    print(f"est_err_sq against the histories: max relative deviation {np.abs(e['est_err_sq'] / ref - 1).max():.3e}")
    np.testing.assert_allclose(e["est_err_sq"], ref, rtol=1e-12, atol=0)
    assert (ref > 0).all()
    first = _sim(mpc, x0, ub, stuck, 5, xr=xr[:, :5 + N + 2], environment=env, plant=plant, sensor=sen, estimator=est, disturbance=_dist())
    fd, fe = first["disturbance"], first["environment"]
    sen2 = dict(sen, pending=first["sensor"]["pending"], step0=5)
    est2 = dict(est, xhat=first["estimator"]["xhat"], cov=first["estimator"]["cov"])
    dist2 = _dist(force=fd["force"], torque=fd["torque"], cross=fd["cross"], cov=fd["cov"])
    env2 = dict(env, step0=5, state=fe["state"], est_err_sq=fe["est_err_sq"])
    second = _sim(mpc, first["x"], ub, stuck, 7, xr=xr[:, 5:], environment=env2, plant=plant, sensor=sen2, estimator=est2, disturbance=dist2)
    assert np.array_equal(second["x"], whole["x"])
    assert np.array_equal(second["environment"]["est_err_sq"], e["est_err_sq"])
    assert np.array_equal(second["environment"]["state"], e["state"])


def test_a_random_walk_model_follows_a_disturbance_that_moves(gpu_mpc_factory):
    """Periodic term only, period 100 steps, T = 200, B = 64.  Amplitudes 0.5 N and 0.02 N m: per step they change the velocity by
    F dt / m = 3e-3 m/s and the rate by about t dt / J = 8e-3 rad/s, 30 and 80 times meas_sigma = 1e-4.  The same campaign with
    proc_sigma = (0, 0), a constant model, and with proc_sigma = amplitude 2 pi / 100, the disturbance's largest step-to-step change:
    the random-walk model's summed squared error is below the constant model's, for force and for torque.  (The ratios are in
    CHANGELOG.md; only < 1 is asserted.)"""
    Bv, Tn, period_steps = 64, 200, 100
    x0, ub, stuck = _batch(Bv=Bv)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    amp = (0.5, 0.02)
    rng = np.random.default_rng(6)
    unit = rng.normal(size=(Bv, 2, 3))
    unit /= np.linalg.norm(unit, axis=2, keepdims=True)
    env = dict(period=period_steps * DT, amp_force=amp[0] * unit[:, 0], amp_torque=amp[1] * unit[:, 1], phase=rng.uniform(0, 2 * np.pi, Bv),
               fields=("est_err_sq",))
    ms = (1e-4,) * 4
    sen = dict(sigma=ms, seed=77)
    est = dict(every=1, p0=SIGMA, proc_sigma=tuple(0.1 * s for s in SIGMA), meas_sigma=ms)
    step = tuple(a * 2 * np.pi / period_steps for a in amp)
    sums = []
    for q in ((0.0, 0.0), step):
        out = mpc.simulate(x0, ub, stuck, _hover(N, Tn), Tn, noise=ZERO, seed=5, sensor=sen, estimator=est, environment=env,
                           disturbance=dict(p0=(0.5, 0.05), proc_sigma=q, compensate=True))
        assert np.isfinite(out["x"]).all()
        sums.append(out["environment"]["est_err_sq"].sum(axis=0))
    ratio = sums[1] / sums[0]
    print(f"summed est_err_sq, constant model {sums[0]}, random walk {sums[1]}: ratio force {ratio[0]:.4f}, torque {ratio[1]:.4f}")
    assert ratio[0] < 1 and ratio[1] < 1


# ---------------------------------------------------------------------------------------------------------------------------
# 11: refusals through the C entries: FTMPC_ERR_ARG, the message names the field (and the vehicle), x untouched
# ---------------------------------------------------------------------------------------------------------------------------
def _bad_structs(Bv):
    size = C.sizeof(_lib.ftmpc_environment)
    v = Bv - 2                                                      # on three slots: in the last shard

    def make(struct_size=size, reserved=0, step0=0, sigma=(0.1, 0.01), tau=(1.0, 1.0), period=1.0, **ptr):
        s = _lib.ftmpc_environment(struct_size=struct_size, reserved=reserved, step0=step0, period=period)
        for a in range(2):
            s.sigma[a], s.tau[a] = sigma[a], tau[a]
        for name, arr in ptr.items():
            setattr(s, name, arr.ctypes.data_as(ip if name == "window" else dp))
        return s, list(ptr.values())

    def bad(width, value=np.nan):
        a = np.zeros((Bv, width))
        a[v, width - 1] = value
        return a
    win = np.zeros((Bv, 2), np.int32)
    return [("struct_size", None, False) + make(struct_size=size - 8), ("reserved", None, False) + make(reserved=1),
            ("step0", None, False) + make(step0=-1), ("step0", None, "sensor") + make(step0=3),
            ("sigma", None, False) + make(sigma=(-1e-9, 0)), ("sigma", None, False) + make(sigma=(0, np.inf)),
            ("tau", None, False) + make(tau=(0.0, 1.0)), ("tau", None, False) + make(tau=(1.0, np.nan)),
            ("period", None, False) + make(period=0.0, amp_force=np.ones((Bv, 3))),
            ("period", None, False) + make(period=np.inf, amp_torque=np.ones((Bv, 3))),
            ("amp_force", v, False) + make(amp_force=bad(3)), ("amp_torque", v, False) + make(amp_torque=bad(3, np.inf)),
            ("phase", v, False) + make(phase=bad(1)), ("kick", v, False) + make(kick=bad(6), window=win),
            ("kick", None, False) + make(kick=np.ones((Bv, 6))), ("state", v, False) + make(state=bad(6, -np.inf)),
            ("est_err_sq", None, False) + make(est_err_sq=np.zeros((Bv, 2))),
            ("est_err_sq", v, "dist") + make(est_err_sq=bad(2, -1.0)), ("est_err_sq", v, "dist") + make(est_err_sq=bad(2))]


def test_refusals(gpu_mpc_factory):
    Bv, Tn = 12, 2
    x0, ub, stuck = _batch(Bv=Bv, seed=20)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f32"), devices=[0, 0, 0])
    es = _lib.ftmpc_estimator(struct_size=C.sizeof(_lib.ftmpc_estimator), every=1)
    for k in range(4):
        es.p0[k], es.proc_sigma[k], es.meas_sigma[k] = SIGMA[k], SIGMA[k], SIGMA[k]
    db = _lib.ftmpc_disturbance(struct_size=C.sizeof(_lib.ftmpc_disturbance), compensate=1)
    for k in range(2):
        db.p0[k], db.proc_sigma[k] = (0.5, 0.05)[k], 0.0
    se = _lib.ftmpc_sensor(struct_size=C.sizeof(_lib.ftmpc_sensor), step0=2)

    def call(obj, ev, with_=False, wrench=False):
        sensor = C.byref(se) if with_ == "sensor" else None
        est, dist = (C.byref(es), C.byref(db)) if with_ == "dist" else (None, None)
        if wrench:
            tail = (None, None, None, sensor, est, None, None, None, dist, None, None, ev)
            return _entry(obj, "wrench_environment_batch", x0, ub, stuck, N, Tn, 1, tail, want=False, wrench=True)
        return _entry(obj, "environment_batch", x0, ub, stuck, N, Tn, 1, (None, None, None, sensor, est, None, dist, None, None, ev), want=False)
    try:
        for n, (field, v, with_, ev, keep) in enumerate(_bad_structs(Bv)):
            for obj in (mpc, m):
                for wrench in ((False, True) if n in (0, 10) and obj is mpc else (False,)):
                    rc, err, out = call(obj, C.byref(ev), with_, wrench)
                    assert rc == -1 and f"ftmpc_environment.{field}".encode() in err, (field, err)
                    if v is not None:
                        assert f"vehicle {v} ".encode() in err, err
                    assert np.array_equal(out["x"], x0)
        with pytest.raises(ValueError, match="sigma"):      # what the front end refuses itself never reaches the library
            mpc.simulate(x0, ub, stuck, _hover(N, Tn), Tn, environment=dict(sigma=-1.0))
        with pytest.raises(ValueError, match="MultiGPUMPC is not built"):
            m.simulate(x0, ub, stuck, _hover(N, Tn), Tn, formulation="wrench", environment=dict(sigma=0.1))
        # and a good environment is accepted by both, with the same bits
        env = _all(Bv, fields=EALL_ENV)
        a, b = _sim(mpc, x0, ub, stuck, Tn, environment=env), _sim(m, x0, ub, stuck, Tn, environment=env)
        assert np.array_equal(a["x"], b["x"]) and a["environment"]["wrench"].any()
        for k in EALL_ENV:
            assert np.array_equal(a["environment"][k], b["environment"][k]), k
    finally:
        m.close()
