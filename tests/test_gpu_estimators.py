"""GPU: the navigation filter in the on-device closed loops (ftmpc_filter_kernel; ftmpc_simulate_estimator_batch,
ftmpc_simulate_wrench_estimator_batch, ftmpc_multi_simulate_*_estimator_batch; BatchedMPC.simulate(estimator=...)).

The reference is ft_mpc_amd/estimators.py (tests/test_estimators_host.py checks it on the CPU: the Jacobian against differences, the
update against the batch form).  Every run is replayed per vehicle from its own histories: est, pred and the returned xhat / cov from
the device's meas_hist, u_hist and the controller's pattern of each step, whatever the solver returned.

A  replay (every = 1 and 3); B  what the solve reads; C  zero gain; D  estimator = NULL gives the bits of the _sensor_ entry;
E  continued runs; F  slices and device slots; G  the filter filters; H  other features; I  refusals.

BOUND: the deviation of the replay is round-off.  Measured on an MI355X over the cases of (A) and (H): est within 4.4e-16, pred
within 8.9e-16, xhat within 4.4e-16 of the state's units, cov within 2.7e-16 of p0_i p0_j, an estimate held between two updates within
2.2e-16 of the propagation of the one before; BOUND is 100 x the largest of these (and may in no case be looser than 1e-9: a wrong
block of A moves P by about dt |F/m| p0^2 = 1e-2 p0^2).  err_sq is a sum of squares of differences of nearby numbers, which loses
digits to cancellation: it deviates from the same sum formed on the host from est_hist by 9.2e-15 of its value, BOUND_SQ is 100 x that."""
import ctypes as C

import numpy as np
import pytest

import ft_mpc_amd
from ft_mpc_amd import _lib
from ft_mpc_amd import estimators as E
from ft_mpc_amd.sharding import MultiGPUMPC
from oracle import qp_oracle as qo
from test_gpu_actuators import _entry, _same_bits
from test_gpu_missions import UT, XT
from test_gpu_outcomes import _hover, _wrench_batch, term  # noqa: F401  (term: a fixture)
from test_gpu_plant_dispersion import _plant
from test_gpu_sensors import _bias, _ctrl_patterns

pytestmark = pytest.mark.gpu
NOISE = (1e-3,) * 4
ZERO = (0.0,) * 4
SIGMA = (1e-2, 5e-3, 1e-2, 5e-3)
BOUND = 8.9e-14
BOUND_SQ = 9.2e-13
EALL = ("est", "err_sq", "xhat", "cov")
SALL = ("meas", "pred", "pending")
dp = C.POINTER(C.c_double)
_G = np.repeat(np.arange(4), 3)


def _spec(every=1, **kw):
    return dict(dict(every=every, p0=SIGMA, proc_sigma=tuple(0.1 * s for s in SIGMA), meas_sigma=SIGMA), **kw)


def _sensor(B, NT, d=2, predict=True, bias=True, seed=41, **kw):
    pend = np.random.default_rng(seed).uniform(0, 1.0, (B, d, NT)) if d else None
    return dict(dict(sigma=SIGMA, bias=_bias(B) if bias else None, seed=77, latency=d, predict=predict, pending=pend,
                     fields=tuple(f for f in SALL if (f != "pred" or predict) and (f != "pending" or d))), **kw)


def _prior(x0, seed=3):
    """a prior mean a few sigma off the truth, and the packed diag(p0^2) it is handed with"""
    B = x0.shape[0]
    d = np.random.default_rng(seed).normal(size=(B, 12)) * np.asarray(SIGMA)[_G]
    xh = np.stack([E.retract(x0[b], d[b]) for b in range(B)])
    return xh, E.pack(np.repeat(np.diag(np.asarray(SIGMA)[_G] ** 2)[None], B, 0))


def _two_faults(B, N, seed=11):
    """two events per vehicle (steps 3..8 and two steps later), each detected two steps late on every second vehicle, the first
    broken thruster stuck on every third"""
    NT = 8
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 0, seed)
    on = 3 + np.arange(B) % 6
    onset = np.stack([on, on + 2], axis=1).astype(np.int32)
    eub, est = np.repeat(ub[:, None], 2, 1).copy(), np.zeros((B, 2, NT))
    for b in range(B):
        eub[b, :, b % NT] = 0.0
        est[b, :, b % NT] = 1.7 if b % 3 == 0 else 0.0
        eub[b, 1, (b + 3) % NT] = 0.0
    return dict(x0=x0, ub=ub, stuck=stuck, faults=dict(onset=onset, ub=eub, stuck=est), delay=np.where(np.arange(B) % 2 == 0, 2, 0))


def _sim(mpc, x0, ub, stuck, N, T, sen, est, seed=5, noise=NOISE, xr=None, **kw):
    L = sen.get("latency", 0) if sen is not None and sen.get("predict") else 0
    xr = _hover(N, T + L) if xr is None else xr
    return mpc.simulate(x0, ub, stuck, xr, T, noise=noise, seed=seed, return_inputs=True, return_states=True, sensor=sen, estimator=est,
                        **kw)


def _check_filter(out, x0, ub, stuck, sen, est, cfg, faults=None, delay=0, bound=BOUND):
    """est, pred, xhat, cov and err_sq of `out` against estimators.replay of its own histories; returns the deviations."""
    eo, so = out["estimator"], out.get("sensor") or {}
    T, B, NT = out["u"].shape
    d = sen.get("latency", 0) if sen else 0
    predict = bool(sen and sen.get("predict"))
    cu, cs = (np.repeat(ub[None], T, 0), np.repeat(stuck[None], T, 0)) if faults is None else _ctrl_patterns(ub, stuck, faults, delay, T)
    truth = np.concatenate([x0[None], out["x_hist"][:-1]])
    meas = so["meas"] if "meas" in so else truth
    p0 = np.asarray(est["p0"], float)[_G]
    unit = E.pack(np.outer(p0, p0))
    every, step0 = est.get("every", 1), (sen or {}).get("step0", 0)
    dev = dict(est=0.0, pred=0.0, xhat=0.0, cov=0.0, hold=0.0, err_sq=0.0)
    esq = np.zeros((B, 4))
    for b in range(B):
        r = E.replay(meas[:, b], out["u"][:, b], cu[:, b], cs[:, b], est, cfg, xhat=None if est.get("xhat") is None else est["xhat"][b],
                     cov=None if est.get("cov") is None else est["cov"][b], step0=step0, latency=d if predict else 0,
                     tail=so["pending"][b] if predict and d else None)
        dev["est"] = max(dev["est"], np.abs(eo["est"][:, b] - r["est"]).max())
        if predict and d:
            dev["pred"] = max(dev["pred"], np.abs(so["pred"][:, b] - r["pred"]).max())
        if "xhat" in eo:
            dev["xhat"] = max(dev["xhat"], np.abs(eo["xhat"][b] - r["xhat"]).max())
            dev["cov"] = max(dev["cov"], (np.abs(eo["cov"][b] - r["cov"]) / unit).max())
        for t in range(T):
            if t > 0 and (step0 + t) % every != 0:      # no update: the pure propagation of the step before
                z = E.predict(eo["est"][t - 1, b], out["u"][t - 1:t, b], cu[t - 1, b], cs[t - 1, b], cfg)
                dev["hold"] = max(dev["hold"], np.abs(eo["est"][t, b] - z).max())
            esq[b] += (E.residual(truth[t, b], eo["est"][t, b]) ** 2).reshape(4, 3).sum(1)
    if "err_sq" in eo:
        dev["err_sq"] = (np.abs(eo["err_sq"] - esq) / np.maximum(esq, 1e-300)).max()
    print("filter replay: max |device - definition|: " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    for k, v in dev.items():
        assert v <= (BOUND_SQ if k == "err_sq" else bound), (k, v)
    return dev


# ---------------------------------------------------------------------------------------------------------------------------
# (A) replay from the run's own histories
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("B", [1, 65, 96])
def test_replay_from_the_runs_own_histories(gpu_mpc_factory, B, every):
    N, NT, T = 10, 8, 12
    bt = _two_faults(B, N)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = _sensor(B, NT)
    xh, cov = _prior(bt["x0"])
    est = _spec(every, xhat=xh, cov=cov, fields=EALL)
    out = _sim(mpc, bt["x0"], bt["ub"], bt["stuck"], N, T, sen, est, faults=bt["faults"], detect_delay=bt["delay"])
    assert sorted(out["estimator"]) == sorted(EALL) and sorted(out["sensor"]) == sorted(SALL)
    _check_filter(out, bt["x0"], bt["ub"], bt["stuck"], sen, est, mpc.cfg, faults=bt["faults"], delay=bt["delay"])
    # the handed priors were not written into, the returned ones moved on
    assert np.array_equal(est["xhat"], xh) and not np.array_equal(out["estimator"]["xhat"], xh)
    # the first estimate of a call without xhat is the first measurement, bit for bit
    est0 = _spec(every, fields=("est",))
    out0 = _sim(mpc, bt["x0"], bt["ub"], bt["stuck"], N, 3, sen, est0, faults=bt["faults"], detect_delay=bt["delay"])
    assert np.array_equal(out0["estimator"]["est"][0], out0["sensor"]["meas"][0])
    _check_filter(out0, bt["x0"], bt["ub"], bt["stuck"], sen, est0, mpc.cfg, faults=bt["faults"], delay=bt["delay"])


# ---------------------------------------------------------------------------------------------------------------------------
# (B) what the solve reads
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [0, 2])
def test_the_solve_starts_from_the_estimate(gpu_mpc_factory, d):
    N, NT, B, T = 10, 8, 96, 4
    x0, ub, stuck = qo.make_batch(B, N, NT, 1, 13)[:3]
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    xr = XT[1][:, :T + N + d]                                      # a circle: every window differs from its neighbour
    sen = _sensor(B, NT, d=d, predict=d > 0, fields=("meas", "pred") if d else ("meas",))
    xh, cov = _prior(x0)
    out = _sim(mpc, x0, ub, stuck, N, T, sen, _spec(xhat=xh, cov=cov, fields=("est",)), xr=xr)
    seen = out["sensor"]["pred"][0] if d else out["estimator"]["est"][0]
    win = np.ascontiguousarray(xr[:, d:d + N + 1].reshape(-1, order="F"))
    u0 = mpc.solve(seen, ub, stuck, win)["u0"]
    assert np.array_equal(out["u"][d], u0)                         # the command of step 0 (no warm start) acts in step d
    for other in (out["sensor"]["meas"][0], x0, out["estimator"]["est"][0] if d else None):
        if other is not None:
            assert not np.array_equal(mpc.solve(other, ub, stuck, win)["u0"], u0)


# ---------------------------------------------------------------------------------------------------------------------------
# (C) zero gain
# ---------------------------------------------------------------------------------------------------------------------------
def test_zero_gain_follows_the_truth(gpu_mpc_factory):
    """p0 = proc_sigma = 0, xhat = the truth, no sensor errors, no process noise, d = 0: the filter is a chained RK4 of the truth's
    own model, est[t] = x_hist[t-1] within 1e-12 (the sensor test's bound for a chained RK4)."""
    N, NT, B, T = 10, 8, 96, 12
    x0, ub, stuck = qo.make_batch(B, N, NT, 1, 12)[:3]
    est = dict(every=1, p0=ZERO, proc_sigma=ZERO, meas_sigma=SIGMA, xhat=x0, fields=EALL)
    for sen in (None, dict(fields=("meas",))):                     # no sensor at all, and a sensor without errors
        out = _sim(gpu_mpc_factory(N=N, NT=NT, dtype="f32"), x0, ub, stuck, N, T, sen, est, noise=ZERO)
        eo = out["estimator"]
        worst = np.abs(eo["est"][1:] - out["x_hist"][:-1]).max()
        print(f"zero gain: max |est[t] - x_hist[t-1]| = {worst:.3e}")
        np.testing.assert_allclose(eo["est"][0], x0, rtol=0, atol=1e-15)
        np.testing.assert_allclose(eo["est"][1:], out["x_hist"][:-1], rtol=0, atol=1e-12)
        np.testing.assert_allclose(eo["xhat"], out["x"], rtol=0, atol=1e-12)
        assert np.all(eo["cov"] == 0.0) and eo["err_sq"].max() <= 1e-22
        assert out["u"].any()


# ---------------------------------------------------------------------------------------------------------------------------
# (D) estimator = NULL
# ---------------------------------------------------------------------------------------------------------------------------
def test_null_estimator_gives_the_bits_of_the_sensor_entry(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 96, 4
    x0, ub, stuck = qo.make_batch(B, N, NT, 1, 16)[:3]
    bias = _bias(B)
    se = _lib.ftmpc_sensor(struct_size=C.sizeof(_lib.ftmpc_sensor), latency=2, predict=0, seed=9, bias=bias.ctypes.data_as(dp))
    for k in range(4):
        se.sigma[k] = SIGMA[k]
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f32"), devices=[0, 0, 0])
    try:
        for obj in (mpc, m):
            for s in (None, C.byref(se)):
                rc, err, ref = _entry(obj, "sensor_batch", x0, ub, stuck, N, T, 7, (None, None, None, s))
                assert rc == 0, err
                rc, err, out = _entry(obj, "estimator_batch", x0, ub, stuck, N, T, 7, (None, None, None, s, None))
                assert rc == 0, err
                _same_bits(out, ref)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (E) continued runs
# ---------------------------------------------------------------------------------------------------------------------------
def test_continued_runs_equal_the_whole(gpu_mpc_factory):
    """T = 12 against 6 + 6 with xhat, cov, pending and step0 = 6 handed over, no process noise, every = 3 (steps 0, 3 | 6, 9: the
    phase crosses the seam, and every = 3 with step0 = 0 in the second call would update at its steps 0 and 3 too, so the test adds
    every = 4, where step0 matters).  State, u_hist, meas, est, pred, the returned xhat, cov and pending: bit for bit.  err_sq is a
    sum formed on the device step by step; the halves added differ from the whole by the rounding of one addition in another order,
    so it is compared within 4 T eps."""
    N, NT, B = 10, 8, 96
    x0, ub, stuck = qo.make_batch(B, N, NT, 1, 17)[:3]
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = _sensor(B, NT)
    xr = XT[1][:, :12 + N + 2]
    xh, cov = _prior(x0)
    for every in (3, 4):
        est = _spec(every, xhat=xh, cov=cov, fields=EALL)
        whole = _sim(mpc, x0, ub, stuck, N, 12, sen, est, noise=ZERO, xr=xr)
        first = _sim(mpc, x0, ub, stuck, N, 6, sen, est, noise=ZERO, xr=xr[:, :6 + N + 2])
        sen2 = dict(sen, pending=first["sensor"]["pending"], step0=6)
        est2 = dict(est, xhat=first["estimator"]["xhat"], cov=first["estimator"]["cov"])
        second = _sim(mpc, first["x"], ub, stuck, N, 6, sen2, est2, noise=ZERO, xr=xr[:, 6:])
        assert np.array_equal(second["x"], whole["x"])
        for k in ("x_hist", "u"):
            assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k]), k
        for k in ("meas", "pred"):
            assert np.array_equal(np.concatenate([first["sensor"][k], second["sensor"][k]]), whole["sensor"][k]), k
        assert np.array_equal(np.concatenate([first["estimator"]["est"], second["estimator"]["est"]]), whole["estimator"]["est"])
        for k in ("xhat", "cov"):
            assert np.array_equal(second["estimator"][k], whole["estimator"][k]), k
        assert np.array_equal(second["sensor"]["pending"], whole["sensor"]["pending"])
        halves = first["estimator"]["err_sq"] + second["estimator"]["err_sq"]
        assert np.abs(halves - whole["estimator"]["err_sq"]).max() <= 4 * 12 * 2.0 ** -53 * whole["estimator"]["err_sq"].max()
        assert whole["estimator"]["err_sq"].min() > 0
    # without step0 the second call updates on other steps
    off = _sim(mpc, first["x"], ub, stuck, N, 6, dict(sen2, step0=0), est2, noise=ZERO, xr=xr[:, 6:])
    assert not np.array_equal(off["estimator"]["est"], second["estimator"]["est"])


# ---------------------------------------------------------------------------------------------------------------------------
# (F) slices of a campaign and device slots
# ---------------------------------------------------------------------------------------------------------------------------
def _run(mpc, bt, sen, est, lo=0, hi=None, T=12, **kw):
    hi = bt["x0"].shape[0] if hi is None else hi
    f = {k: v[lo:hi] for k, v in bt["faults"].items()}
    s = dict(sen, bias=sen["bias"][lo:hi], pending=sen["pending"][lo:hi])
    e = dict(est, xhat=est["xhat"][lo:hi], cov=est["cov"][lo:hi])
    return mpc.simulate(bt["x0"][lo:hi], bt["ub"][lo:hi], bt["stuck"][lo:hi], _hover(10, T + 2), T, noise=NOISE, seed=5, faults=f,
                        detect_delay=bt["delay"][lo:hi], return_inputs=True, return_states=True, sensor=s, estimator=e, **kw)


def test_slices_and_device_slots_equal_the_whole(gpu_mpc_factory):
    B = 96
    bt = _two_faults(B, 10)
    sen = _sensor(B, 8)
    xh, cov = _prior(bt["x0"])
    est = _spec(3, xhat=xh, cov=cov, fields=EALL)

    def fresh(lo, hi, **kw):
        mpc = ft_mpc_amd.BatchedMPC(N=10, NT=8, dtype="f32")
        try:
            return _run(mpc, bt, sen, est, lo, hi, **kw)
        finally:
            mpc.close()
    whole = fresh(0, B)
    parts = [fresh(0, 40, index0=0, index_total=B), fresh(40, B, index0=40, index_total=B)]
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=10, NT=8, dtype="f32"), devices=[0, 0, 0])
    try:
        multi = _run(m, bt, sen, est)
    finally:
        m.close()
    assert np.array_equal(np.concatenate([p["x"] for p in parts]), whole["x"]) and np.array_equal(multi["x"], whole["x"])
    for k in ("x_hist", "u"):
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), whole[k]), k
        assert np.array_equal(multi[k], whole[k]), k
    for k in SALL:
        assert np.array_equal(np.concatenate([p["sensor"][k] for p in parts], axis=0 if k == "pending" else 1), whole["sensor"][k]), k
        assert np.array_equal(multi["sensor"][k], whole["sensor"][k]), k
    for k in EALL:
        assert np.array_equal(np.concatenate([p["estimator"][k] for p in parts], axis=1 if k == "est" else 0), whole["estimator"][k]), k
        assert np.array_equal(multi["estimator"][k], whole["estimator"][k]), k


# ---------------------------------------------------------------------------------------------------------------------------
# (G) the filter filters
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_filter_filters(gpu_mpc_factory):
    """B = 96, T = 40, no bias: err_sq summed over the vehicles is below the same sum of the raw measurements in every group, and
    equals that sum formed from est_hist within the bound of (A) for such sums (BOUND_SQ)."""
    N, NT, B, T = 10, 8, 96, 40
    x0, ub, stuck = qo.make_batch(B, N, NT, 1, 19)[:3]
    sen = _sensor(B, NT, d=0, predict=False, bias=False)
    est = _spec(fields=("est", "err_sq"))
    out = _sim(gpu_mpc_factory(N=N, NT=NT, dtype="f32"), x0, ub, stuck, N, T, sen, est)
    truth = np.concatenate([x0[None], out["x_hist"][:-1]])
    e_est, e_meas = np.zeros((B, 4)), np.zeros((B, 4))
    for t in range(T):
        for b in range(B):
            e_est[b] += (E.residual(truth[t, b], out["estimator"]["est"][t, b]) ** 2).reshape(4, 3).sum(1)
            e_meas[b] += (E.residual(truth[t, b], out["sensor"]["meas"][t, b]) ** 2).reshape(4, 3).sum(1)
    got = out["estimator"]["err_sq"]
    print("sum err_sq / sum of the raw measurements' (position, velocity, attitude, rate):", np.round(got.sum(0) / e_meas.sum(0), 3))
    assert (got.sum(0) < e_meas.sum(0)).all()
    assert (np.abs(got - e_est) / e_est).max() <= BOUND_SQ


# ---------------------------------------------------------------------------------------------------------------------------
# (H) other features
# ---------------------------------------------------------------------------------------------------------------------------
def test_with_a_dispersed_plant_and_the_pwm_actuator(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 96, 6
    x0, ub, stuck = qo.make_batch(B, N, NT, 1, 14)[:3]
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = _sensor(B, NT)
    xh, cov = _prior(x0)
    est = _spec(xhat=xh, cov=cov, fields=EALL)
    act = dict(mode="pwm", substeps=8, min_on=2, align="centred", tau_on=0.02, tau_off=0.01)
    out = _sim(mpc, x0, ub, stuck, N, T, sen, est, plant=_plant(B, NT, seed=15), actuator=act)
    _check_filter(out, x0, ub, stuck, sen, est, mpc.cfg)


def test_with_a_mission(gpu_mpc_factory):
    N, NT, B, T, d = 10, 8, 96, 8, 2
    x0, ub, stuck = qo.make_batch(B, N, NT, 1, 15)[:3]
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = _sensor(B, NT)
    xh, cov = _prior(x0)
    est = _spec(3, xhat=xh, cov=cov, fields=EALL)
    table, offset = (7 * np.arange(B) % 3).astype(np.int32), (5 * np.arange(B) % 23).astype(np.int32)
    cols = 22 + T + N + d
    ms = dict(tables=XT[:, :, :cols], utables=UT[:, :, :cols], table=table, offset=offset)
    out = mpc.simulate(x0, ub, stuck, None, T, noise=NOISE, seed=5, return_inputs=True, return_states=True, mission=ms, sensor=sen,
                       estimator=est, outcomes=dict(cost=True))
    _check_filter(out, x0, ub, stuck, sen, est, mpc.cfg)


def test_with_the_thruster_sqp_loop(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 32, 4
    x0, ub, stuck = qo.make_batch(B, N, NT, 1, 13)[:3]
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = _sensor(B, NT)
    xh, cov = _prior(x0)
    est = _spec(xhat=xh, cov=cov, fields=EALL)
    out = _sim(mpc, x0, ub, stuck, N, T, sen, est, sqp_iters=2)
    _check_filter(out, x0, ub, stuck, sen, est, mpc.cfg)
    assert out["u"][2:].any()


@pytest.fixture(scope="module")
def wrench24(term):  # noqa: F811
    bt = _wrench_batch(term)
    sel = np.r_[0:12, 20:32]
    return dict(x0=bt["x0"][sel], ub=bt["ub"][sel], stuck=bt["stuck"][sel], xr=bt["xr"], seed=bt["seed"], term=term[0])


@pytest.mark.parametrize("sqp_iters", [0, 2])
def test_on_the_wrench_form(gpu_mpc_factory, wrench24, sqp_iters):
    w, T, d = wrench24, 6 if sqp_iters == 0 else 4, 2
    mpc = gpu_mpc_factory(N=15, NT=16, dtype="f64", max_iters=60, terminal_set=w["term"])
    sen = _sensor(24, 16, d=d)
    xh, cov = _prior(w["x0"])
    est = _spec(xhat=xh, cov=cov, fields=EALL)
    out = mpc.simulate(w["x0"], w["ub"], w["stuck"], w["xr"][:, :T + 15 + d], T, noise=(1e-4,) * 4, seed=w["seed"], formulation="wrench",
                       sqp_iters=sqp_iters, return_inputs=True, return_states=True, sensor=sen, estimator=est)
    _check_filter(out, w["x0"], w["ub"], w["stuck"], sen, est, mpc.cfg)
    assert out["u"][d:].any()


# ---------------------------------------------------------------------------------------------------------------------------
# (I) refusals, on a handle and on the driver: FTMPC_ERR_ARG, the message names the field (and the vehicle), x untouched
# ---------------------------------------------------------------------------------------------------------------------------
def _bad_structs(B):
    size = C.sizeof(_lib.ftmpc_estimator)
    v = B - 2                                                      # on three slots: in the last shard
    S = _lib.ftmpc_estimator

    def make(every=1, p0=SIGMA, proc=SIGMA, meas=SIGMA, struct_size=size, **ptr):
        s = S(struct_size=struct_size, every=every)
        for k in range(4):
            s.p0[k], s.proc_sigma[k], s.meas_sigma[k] = p0[k], proc[k], meas[k]
        for name, a in ptr.items():
            setattr(s, name, a.ctypes.data_as(dp))
        return s, list(ptr.values())
    xh = np.tile(np.r_[np.zeros(9), 1.0, np.zeros(3)], (B, 1))
    nan_x, cov, inf_c, neg_c = xh.copy(), np.zeros((B, 78)), np.zeros((B, 78)), np.zeros((B, 78))
    nan_x[v, 4], inf_c[v, 30], neg_c[v, 12] = np.nan, np.inf, -1e-12
    return [("struct_size", None) + make(struct_size=size - 8), ("every", None) + make(every=0), ("every", None) + make(every=-3),
            ("p0", None) + make(p0=(1, -1e-9, 1, 1)), ("p0", None) + make(p0=(1, 1, np.nan, 1)),
            ("proc_sigma", None) + make(proc=(0, 0, 0, -1.0)), ("proc_sigma", None) + make(proc=(np.inf, 0, 0, 0)),
            ("meas_sigma", None) + make(meas=(1, 0.0, 1, 1)), ("meas_sigma", None) + make(meas=(1, 1, 1, np.nan)),
            ("meas_sigma", None) + make(meas=(-1.0, 1, 1, 1)),
            ("cov", None) + make(cov=cov), ("xhat", v) + make(xhat=nan_x), ("cov", v) + make(xhat=xh, cov=inf_c),
            ("cov", v) + make(xhat=xh, cov=neg_c)]


def test_refusals(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 12, 2
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 0, 20)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f32"), devices=[0, 0, 0])
    try:
        for n, (field, v, es, keep) in enumerate(_bad_structs(B)):
            for obj in (mpc, m):
                for wrench in ((False, True) if n in (0, 11) else (False,)):
                    name = "wrench_estimator_batch" if wrench else "estimator_batch"
                    rc, err, out = _entry(obj, name, x0, ub, stuck, N, T, 1, (None, None, None, None, C.byref(es)), want=False, wrench=wrench)
                    assert rc == -1 and f"ftmpc_estimator.{field}".encode() in err, (field, err)
                    if v is not None:
                        assert f"vehicle {v} ".encode() in err, err
                    assert np.array_equal(out["x"], x0)
        with pytest.raises(ValueError):      # what the front end refuses itself never reaches the library
            mpc.simulate(x0, ub, stuck, _hover(N, T), T, estimator=_spec(every=0))
        # and a good estimator is accepted by both, with the same bits
        sen = _sensor(B, NT)
        xh, cov = _prior(x0)
        est = _spec(xhat=xh, cov=cov, fields=EALL)
        a, b = _sim(mpc, x0, ub, stuck, N, T, sen, est), _sim(m, x0, ub, stuck, N, T, sen, est)
        assert np.array_equal(a["x"], b["x"])
        for k in EALL:
            assert np.array_equal(a["estimator"][k], b["estimator"][k]), k
    finally:
        m.close()
