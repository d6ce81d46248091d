"""GPU: navigation errors and command latency in the on-device closed loops (ftmpc_sense_kernel; ftmpc_simulate_sensor_batch,
ftmpc_simulate_wrench_sensor_batch, ftmpc_multi_simulate_*_sensor_batch; BatchedMPC.simulate(sensor=...)).

The references are written here from oracle.refmath and oracle.closed_loop.u01 and do not use ft_mpc_amd/sensors.py: the definition of
include/ftmpc.h (Box-Muller draws at counter ((step0 + t) index_total + index0 + b) 12 + j, the bias, the attitude error as a
body-frame rotation vector, the prediction as RK4 steps of oracle.refmath.plant_dx_dt with renormalisation) in NumPy.  Every run is
replayed step by step from its own histories: meas[t] from the truth x_t, pred[t] from meas[t] and the commands the plant applied in
steps t .. t+d-1, x_hist[t] from x_hist[t-1] under u_hist[t] -- which checks the sense kernel and the command queue whatever the
solver returned.  Bound: rtol 1e-12 + atol 1e-12, that of tests/test_gpu_plant_dispersion.py for the plant step; the measurement adds
one log, one sqrt and one cos per channel (a few ulp each) scaled by sigma <= 1e-2, the prediction d <= 3 more steps of the same
arithmetic.

A  replay with noise, bias, latency 2 and prediction; B  the prediction is exact when nothing is unknown (thruster and wrench form);
C  the solve sees what the histories say; D  the trivial struct gives the bits of the _actuator_ entry; E  split runs;
F  slices of a campaign and device slots; G  composition with a fault schedule, a dispersed plant and PWM, a mission, the SQP loop;
H  refusals."""
import ctypes as C

import numpy as np
import pytest

import ft_mpc_amd
from ft_mpc_amd import _lib
from ft_mpc_amd._lib import FtmpcError
from ft_mpc_amd.faults import normalize_schedule
from ft_mpc_amd.sharding import MultiGPUMPC
from oracle import closed_loop as cl
from oracle import qp_oracle as qo
from oracle import refmath as rm
from test_gpu_actuators import _act_step, _entry, _same_bits
from test_gpu_missions import UT, XT
from test_gpu_outcomes import _hover, _plant_patterns, _thruster_batch, _wrench_batch, term  # noqa: F401  (term: a fixture)
from test_gpu_plant_dispersion import _plant

pytestmark = pytest.mark.gpu
NOISE = (1e-3,) * 4
ZERO = (0.0,) * 4
DT = 0.1
SIGMA = (1e-2, 5e-3, 1e-2, 5e-3)
ALL = ("meas", "pred", "pending")
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


# ---------------------------------------------------------------------------------------------------------------------------
# the definition, in NumPy
# ---------------------------------------------------------------------------------------------------------------------------
def _gauss(seed, c):
    c = np.asarray(c, dtype=np.uint64)
    u1, u2 = cl.u01(seed, np.uint64(2) * c), cl.u01(seed, np.uint64(2) * c + np.uint64(1))
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)


def _bias(B, seed=31):
    """position +-5 cm, velocity +-1 cm/s, attitude +-0.02 rad, rate +-0.005 rad/s"""
    return np.random.default_rng(seed).uniform(-1, 1, (B, 12)) * np.repeat([0.05, 0.01, 0.02, 0.005], 3)


def _measure(x, t, sen, index0=0, index_total=None):
    """y [B,13] of the truths x [B,13] at loop step t by the definition."""
    B = x.shape[0]
    total = B if index_total is None else index_total
    sigma = np.asarray(sen.get("sigma", ZERO), float)
    e = np.zeros((B, 12)) if sen.get("bias") is None else np.array(sen["bias"], float)
    c = ((np.uint64(sen.get("step0", 0) + t) * np.uint64(total) + np.uint64(index0) + np.arange(B, dtype=np.uint64))[:, None] * np.uint64(12)
         + np.arange(12, dtype=np.uint64)[None, :])
    z = _gauss(sen.get("seed", 0), c)
    for k in range(4):
        if sigma[k] > 0:
            e[:, 3 * k:3 * k + 3] += sigma[k] * z[:, 3 * k:3 * k + 3]
    y = x.copy()
    y[:, 0:3] += e[:, 0:3]
    y[:, 3:6] += e[:, 3:6]
    y[:, 10:13] += e[:, 9:12]
    for b in range(B):
        th = e[b, 6:9]
        n = np.linalg.norm(th)
        s = 0.5 if n < 1e-8 else np.sin(0.5 * n) / n
        q = np.cos(0.5 * n) * x[b, 6:10] + s * (rm.omega_op(th) @ x[b, 6:10])
        y[b, 6:10] = q / np.linalg.norm(q)
    return y


def _predict(y, cmds, cu, cs, D):
    """x^ [B,13] from y [B,13] over the commands cmds [d,B,NT] under the controller's pattern cu / cs [B,NT] and the nominal model."""
    out = y.copy()
    for b in range(y.shape[0]):
        for u in cmds[:, b]:
            out[b] = rm.normalize_quaternion_plant(rm.rk4(lambda x: rm.plant_dx_dt(x, u, D, cs[b], cu[b]), out[b], DT))
    return out


def _ctrl_patterns(ub, stuck, faults, delay, T):
    """the controller's pattern at every step: it switches at the detection step"""
    B, NT = ub.shape
    _, detect, eub, est = normalize_schedule(faults, B, NT, T, delay)
    cu, cs = np.repeat(ub[None], T, 0), np.repeat(stuck[None], T, 0)
    for b in range(B):
        for k in range(detect.shape[1]):
            if detect[b, k] >= 0:
                cu[detect[b, k]:, b], cs[detect[b, k]:, b] = eub[b, k], est[b, k]
    return cu, cs


def _applied(out, d):
    """a [T+d,B,NT]: what the plant applied in the run's T steps, then the d commands still waiting at its end."""
    return np.concatenate([out["u"], out["sensor"]["pending"].transpose(1, 0, 2)]) if d else out["u"]


def _check_replay(out, x0, ub, stuck, sen, noise, seed, plant=None, act=None, faults=None, delay=0, state0=None, index0=0, index_total=None,
                  truth_must_miss=False):
    """meas, pred, x_hist and the head of u_hist of `out` against the definition; returns the worst deviation."""
    xh, uh, so = out["x_hist"], out["u"], out["sensor"]
    T, B, NT = uh.shape
    D = rm.allocation_matrix_16() if NT == 16 else rm.allocation_matrix_8()
    d = sen.get("latency", 0)
    pend = np.zeros((B, d, NT)) if sen.get("pending") is None else np.asarray(sen["pending"], float)
    assert np.array_equal(uh[:d], pend.transpose(1, 0, 2)[:T]), "the first d steps apply the pending commands, bit for bit"
    a_full = _applied(out, d)
    pu, ps = (np.repeat(ub[None], T, 0), np.repeat(stuck[None], T, 0)) if faults is None else _plant_patterns(ub, stuck, faults, T)
    cu, cs = (pu, ps) if faults is None else _ctrl_patterns(ub, stuck, faults, delay, T)
    a = np.zeros((B, NT)) if state0 is None else np.array(state0, float)
    worst = dict(meas=0.0, pred=0.0, x=0.0)
    for t in range(T):
        xt = x0 if t == 0 else xh[t - 1]
        y = _measure(xt, t, sen, index0, index_total)
        worst["meas"] = max(worst["meas"], np.abs(so["meas"][t] - y).max())
        np.testing.assert_allclose(so["meas"][t], y, rtol=1e-12, atol=1e-12, err_msg=f"meas, step {t}")
        if sen.get("predict"):
            p = _predict(so["meas"][t], a_full[t:t + d], cu[t], cs[t], D)
            worst["pred"] = max(worst["pred"], np.abs(so["pred"][t] - p).max())
            np.testing.assert_allclose(so["pred"][t], p, rtol=1e-12, atol=1e-12, err_msg=f"pred, step {t}")
        x, a, *_ = _act_step(xt, uh[t], pu[t], ps[t], a, act or {}, plant or {}, t, noise, seed, index0, index_total)
        worst["x"] = max(worst["x"], np.abs(xh[t] - x).max())
        np.testing.assert_allclose(xh[t], x, rtol=1e-12, atol=1e-12, err_msg=f"x_hist, step {t}")
    assert np.array_equal(out["x"], xh[-1])
    print("replay: max |device - definition|: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    if truth_must_miss:      # a replay that takes the truth for the measurement must not explain the run
        miss = np.abs(so["meas"][0] - x0).max(axis=1)
        print(f"meas[0] = x_0 misses by min {miss.min():.3e}, median {np.median(miss):.3e}")
        assert (miss > 1e-4).all()
    return max(worst.values())


def _sim(mpc, x0, ub, stuck, N, T, sen, seed=5, noise=NOISE, xr=None, **kw):
    L = sen.get("latency", 0) if sen is not None and sen.get("predict") else 0
    xr = _hover(N, T + L) if xr is None else xr
    return mpc.simulate(x0, ub, stuck, xr, T, noise=noise, seed=seed, return_inputs=True, return_states=True, sensor=sen, **kw)


def _one_fault(B, N, NT, seed):
    return qo.make_batch(B, N, NT, 1, seed)[:3]


def _sensor(B, NT, d=2, predict=True, seed=41, **kw):
    """noise and bias on every group, d pending commands of 0 .. 1 N, every output"""
    pend = np.random.default_rng(seed).uniform(0, 1.0, (B, d, NT)) if d else None
    return dict(dict(sigma=SIGMA, bias=_bias(B), seed=77, latency=d, predict=predict, pending=pend,
                     fields=tuple(f for f in ALL if (f != "pred" or predict) and (f != "pending" or d))), **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# (A) replay from the run's own histories
# ---------------------------------------------------------------------------------------------------------------------------
def test_replay_from_the_runs_own_histories(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 96, 12                                    # B = 96: a partial last wave
    x0, ub, stuck = _one_fault(B, N, NT, 11)
    sen = _sensor(B, NT)
    out = _sim(gpu_mpc_factory(N=N, NT=NT, dtype="f32"), x0, ub, stuck, N, T, sen)
    assert sorted(out["sensor"]) == sorted(ALL)
    _check_replay(out, x0, ub, stuck, sen, NOISE, 5, truth_must_miss=True)
    assert not np.array_equal(out["sensor"]["pending"], sen["pending"])          # the queue moved on


# ---------------------------------------------------------------------------------------------------------------------------
# (B) the prediction is exact when nothing is unknown
# ---------------------------------------------------------------------------------------------------------------------------
def _exact(out, T, d):
    pred, xh = out["sensor"]["pred"], out["x_hist"]
    worst = max(np.abs(pred[t] - xh[t + d - 1]).max() for t in range(T - d + 1))
    print(f"prediction against the truth d = {d} steps later: max {worst:.3e}")
    for t in range(T - d + 1):
        np.testing.assert_allclose(pred[t], xh[t + d - 1], rtol=0, atol=1e-10, err_msg=f"step {t}")


def test_prediction_is_exact_without_unknowns(gpu_mpc_factory):
    N, NT, B, T, d = 10, 8, 96, 12, 3
    x0, ub, stuck = _one_fault(B, N, NT, 12)
    sen = dict(latency=d, predict=True, fields=ALL)
    out = _sim(gpu_mpc_factory(N=N, NT=NT, dtype="f32"), x0, ub, stuck, N, T, sen, noise=ZERO)
    assert np.array_equal(out["u"][:d], np.zeros((d, B, NT))) and out["u"][d:].any()
    _exact(out, T, d)
    # without errors the measurement is the truth (renormalised)
    np.testing.assert_allclose(out["sensor"]["meas"][1:], out["x_hist"][:-1], rtol=0, atol=1e-15)


@pytest.fixture(scope="module")
def wrench24(term):  # noqa: F811
    bt = _wrench_batch(term)
    sel = np.r_[0:12, 20:32]
    return dict(x0=bt["x0"][sel], ub=bt["ub"][sel], stuck=bt["stuck"][sel], xr=bt["xr"], N=bt["N"], seed=bt["seed"], term=term[0])


def test_prediction_is_exact_without_unknowns_wrench_form(gpu_mpc_factory, wrench24):
    w, T, d = wrench24, 6, 3
    mpc = gpu_mpc_factory(N=15, NT=16, dtype="f64", max_iters=60, terminal_set=w["term"])
    sen = dict(latency=d, predict=True, fields=ALL)
    out = mpc.simulate(w["x0"], w["ub"], w["stuck"], w["xr"][:, :T + 15 + d], T, noise=ZERO, seed=w["seed"], formulation="wrench",
                       return_inputs=True, return_states=True, sensor=sen)
    assert out["alloc_failed"].shape == (T,) and out["u"][d:].any()
    _exact(out, T, d)
    _check_replay(out, w["x0"], w["ub"], w["stuck"], sen, ZERO, w["seed"])


# ---------------------------------------------------------------------------------------------------------------------------
# (C) the solve sees what the histories say
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("predict", [True, False])
def test_the_solve_takes_the_history_entry_and_its_window(gpu_mpc_factory, predict):
    N, NT, B, T, d = 10, 8, 96, 4, 2
    x0, ub, stuck = _one_fault(B, N, NT, 13)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    xr = XT[1][:, :T + N + (d if predict else 0)]                  # a circle: every window differs from its neighbour
    sen = _sensor(B, NT, d=d, predict=predict)
    out = _sim(mpc, x0, ub, stuck, N, T, sen, xr=xr)
    col = d if predict else 0
    seen = out["sensor"]["pred" if predict else "meas"][0]
    win = np.ascontiguousarray(xr[:, col:col + N + 1].reshape(-1, order="F"))
    sol = mpc.solve(seen, ub, stuck, win)
    assert np.array_equal(out["u"][d], sol["u0"])                  # the command of step 0 (no warm start) acts in step d
    # ... and neither the truth nor the neighbouring window gives it
    assert not np.array_equal(mpc.solve(x0, ub, stuck, win)["u0"], sol["u0"])
    other = np.ascontiguousarray(xr[:, col + 1:col + N + 2].reshape(-1, order="F")) if predict else None
    if predict:
        assert not np.array_equal(mpc.solve(seen, ub, stuck, other)["u0"], sol["u0"])


# ---------------------------------------------------------------------------------------------------------------------------
# (D) the trivial struct
# ---------------------------------------------------------------------------------------------------------------------------
def test_trivial_sensor_gives_the_bits_of_the_actuator_entry(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 96, 4
    x0, ub, stuck = _one_fault(B, N, NT, 16)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    rc, err, ref = _entry(mpc, "actuator_batch", x0, ub, stuck, N, T, 7, (None, None, None))
    assert rc == 0, err
    rc, err, out = _entry(mpc, "sensor_batch", x0, ub, stuck, N, T, 7, (None, None, None, None))
    assert rc == 0, err
    _same_bits(out, ref)
    se = _lib.ftmpc_sensor(struct_size=C.sizeof(_lib.ftmpc_sensor), seed=99, step0=3)      # seed and step0 alone draw nothing
    rc, err, out = _entry(mpc, "sensor_batch", x0, ub, stuck, N, T, 7, (None, None, None, C.byref(se)))
    assert rc == 0, err
    _same_bits(out, ref)
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f32"), devices=[0, 0, 0])
    try:
        rc, err, mref = _entry(m, "actuator_batch", x0, ub, stuck, N, T, 7, (None, None, None))
        assert rc == 0, err
        rc, err, mout = _entry(m, "sensor_batch", x0, ub, stuck, N, T, 7, (None, None, None, C.byref(se)))
        assert rc == 0, err
        _same_bits(mout, mref)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (E) split runs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def split(gpu_mpc_factory):
    N, NT, B = 10, 8, 96
    x0, ub, stuck = _one_fault(B, N, NT, 17)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = _sensor(B, NT)
    xr = XT[1][:, :12 + N + 2]
    whole = _sim(mpc, x0, ub, stuck, N, 12, sen, noise=ZERO, xr=xr)
    first = _sim(mpc, x0, ub, stuck, N, 6, sen, noise=ZERO, xr=xr[:, :6 + N + 2])
    sen2 = dict(sen, pending=first["sensor"]["pending"], step0=6)
    second = _sim(mpc, first["x"], ub, stuck, N, 6, sen2, noise=ZERO, xr=xr[:, 6:])
    return x0, ub, stuck, sen, sen2, whole, first, second


def test_split_runs_hand_over_the_queue_and_the_counters(split):
    """What the sensor forms is handed over whole: the first half is the whole run's, bit for bit; the second call applies the handed
    pending commands in its first d steps, and its first measurement and prediction are the whole run's of step 6, bit for bit (the
    same truth, the same counters through step0, the same queue); from there it replays by the definition with step0 = 6."""
    x0, ub, stuck, sen, sen2, whole, first, second = split
    for k in ("x_hist", "u"):
        assert np.array_equal(first[k], whole[k][:6]), k
    for k in ("meas", "pred"):
        assert np.array_equal(first["sensor"][k], whole["sensor"][k][:6]), k
    assert np.array_equal(first["sensor"]["pending"].transpose(1, 0, 2), whole["u"][6:8])
    assert np.array_equal(second["u"][:2], whole["u"][6:8])
    for k in ("meas", "pred"):
        assert np.array_equal(second["sensor"][k][0], whole["sensor"][k][6]), k
    assert np.array_equal(second["x_hist"][:2], whole["x_hist"][6:8])          # the plant under the handed commands
    _check_replay(second, first["x"], ub, stuck, sen2, ZERO, 5)
    # without step0 the second call draws the first call's noise again
    again = _measure(first["x"], 0, dict(sen2, step0=0))
    assert not np.allclose(again, second["sensor"]["meas"][0], rtol=0, atol=1e-6)


def test_a_continuation_the_handle_did_not_see_starts_cold(split, gpu_mpc_factory):
    """The warm start is kept per handle and only for the exact continuation: on another handle, or from another x, the second call's
    first solve starts cold -- its first command is that of `solve` without a warm start, and differs from the whole run's."""
    x0, ub, stuck, sen, sen2, whole, first, second = split
    N, d = 10, 2
    xr = XT[1][:, 6:12 + N + 2]
    other = gpu_mpc_factory(N=N, NT=8, dtype="f32")
    cold = _sim(other, first["x"], ub, stuck, N, 6, sen2, noise=ZERO, xr=xr)
    win = np.ascontiguousarray(xr[:, d:d + N + 1].reshape(-1, order="F"))
    assert np.array_equal(cold["u"][d], other.solve(cold["sensor"]["pred"][0], ub, stuck, win)["u0"])
    assert not np.array_equal(cold["u"][d], whole["u"][6 + d])
    assert np.array_equal(cold["sensor"]["meas"][0], whole["sensor"]["meas"][6])      # what the struct hands over still holds
    # the same handle that ran `first`, but the run is continued twice: the second continuation is not the one it kept
    mpc = gpu_mpc_factory(N=N, NT=8, dtype="f32")
    a = _sim(mpc, x0, ub, stuck, N, 6, sen, noise=ZERO, xr=XT[1][:, :6 + N + 2])
    b1 = _sim(mpc, a["x"], ub, stuck, N, 6, sen2, noise=ZERO, xr=xr)
    b2 = _sim(mpc, a["x"], ub, stuck, N, 6, sen2, noise=ZERO, xr=xr)             # the handle now holds step 12, not step 6
    assert np.array_equal(b1["u"], whole["u"][6:]) and np.array_equal(b2["u"], cold["u"])


def test_split_runs_equal_the_whole(split):
    """T = 12 against 6 + 6 with pending and step0 = 6 handed over and no process noise: the state, u_hist, meas and pred bit for
    bit.  The queue and the counters travel in the struct; the warm start of the second call's first solve is the one the handle
    kept from the first call (step0, B, form and x match), so the second call must run on the handle of the first."""
    x0, ub, stuck, sen, sen2, whole, first, second = split
    got = {k: np.concatenate([first[k], second[k]]) for k in ("x_hist", "u")}
    got.update({k: np.concatenate([first["sensor"][k], second["sensor"][k]]) for k in ("meas", "pred")})
    ref = dict(x_hist=whole["x_hist"], u=whole["u"], meas=whole["sensor"]["meas"], pred=whole["sensor"]["pred"])
    for k in ref:
        dev = np.abs(got[k] - ref[k]).reshape(12, -1).max(axis=1)
        print(f"{k}: first step that differs {next((t for t in range(12) if dev[t] > 0), None)}, max |difference| {dev.max():.3e}")
    assert np.array_equal(second["x"], whole["x"])
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(second["sensor"]["pending"], whole["sensor"]["pending"])


# ---------------------------------------------------------------------------------------------------------------------------
# (F) slices of a campaign and device slots
# ---------------------------------------------------------------------------------------------------------------------------
def _run(mpc, bt, sen, lo=0, hi=None, **kw):
    hi = bt["B"] if hi is None else hi
    f = {k: v[lo:hi] for k, v in bt["faults"].items()}
    s = dict(sen, bias=sen["bias"][lo:hi], pending=sen["pending"][lo:hi])
    L = sen["latency"] if sen["predict"] else 0
    return mpc.simulate(bt["x0"][lo:hi], bt["ub"][lo:hi], bt["stuck"][lo:hi], _hover(bt["N"], bt["T"] + L), bt["T"], noise=NOISE,
                        seed=bt["seed"], faults=f, detect_delay=bt["delay"][lo:hi], return_inputs=True, return_states=True, sensor=s, **kw)


def _same_sensor(a, b):
    assert sorted(a["sensor"]) == sorted(b["sensor"]) == sorted(ALL)
    for k in ALL:
        assert np.array_equal(a["sensor"][k], b["sensor"][k]), k


def test_slices_with_bias_and_pending_sliced_equal_the_whole():
    bt = _thruster_batch(96, 10)
    B = bt["B"]
    sen = _sensor(B, 8)

    def fresh(lo, hi, **kw):
        mpc = ft_mpc_amd.BatchedMPC(N=10, NT=8, dtype="f32")
        try:
            return _run(mpc, bt, sen, lo, hi, outcomes=True, return_status=True, **kw)
        finally:
            mpc.close()
    whole = fresh(0, B)
    parts = [fresh(0, 40, index0=0, index_total=B), fresh(40, B, index0=40, index_total=B)]
    assert np.array_equal(np.concatenate([p["x"] for p in parts]), whole["x"])
    for k in ("x_hist", "u", "status_hist"):
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), whole[k]), k
    for k in whole["outcomes"]:
        assert np.array_equal(np.concatenate([p["outcomes"][k] for p in parts]), whole["outcomes"][k]), k
    for k in ALL:
        assert np.array_equal(np.concatenate([p["sensor"][k] for p in parts], axis=0 if k == "pending" else 1), whole["sensor"][k]), k
    # the second slice by the definition, with its campaign numbers
    _check_replay(parts[1], bt["x0"][40:], bt["ub"][40:], bt["stuck"][40:], dict(sen, bias=sen["bias"][40:], pending=sen["pending"][40:]),
                  NOISE, bt["seed"], faults={k: v[40:] for k, v in bt["faults"].items()}, delay=bt["delay"][40:], index0=40, index_total=B)


def test_three_slots_on_one_device_equal_one_handle(gpu_mpc_factory):
    bt = _thruster_batch(100, 20)
    bt["T"] = 8
    bt["faults"]["onset"] = np.minimum(bt["faults"]["onset"], 6)
    sen = _sensor(100, 8)
    kw = dict(outcomes=dict(tol_pos=1.0, tol_vel=0.3, tol_rate=0.1), return_status=True)
    serial = _run(gpu_mpc_factory(N=20, NT=8, dtype="f32"), bt, sen, **kw)
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=20, NT=8, dtype="f32"), devices=[0, 0, 0])
    try:
        multi = _run(m, bt, sen, **kw)
    finally:
        m.close()
    _same_bits(multi, serial)
    _same_sensor(multi, serial)


# ---------------------------------------------------------------------------------------------------------------------------
# (G) composition
# ---------------------------------------------------------------------------------------------------------------------------
def test_with_a_fault_schedule_the_prediction_uses_the_controllers_pattern(gpu_mpc_factory):
    bt = _thruster_batch(96, 10)
    B, T, d = 96, bt["T"], 2
    sen = _sensor(B, 8)
    mpc = gpu_mpc_factory(N=10, NT=8, dtype="f32")
    out = _run(mpc, bt, sen)
    _check_replay(out, bt["x0"], bt["ub"], bt["stuck"], sen, NOISE, bt["seed"], faults=bt["faults"], delay=bt["delay"])
    # nothing unknown but the undetected fault: before the onset the prediction is the truth d steps later; a prediction made at the
    # onset step of a vehicle that detects late integrates the old pattern while the plant has the new one
    clean = dict(latency=d, predict=True, fields=ALL)
    f = bt["faults"]
    out = mpc.simulate(bt["x0"], bt["ub"], bt["stuck"], _hover(10, T + d), T, noise=ZERO, seed=bt["seed"], faults=f,
                       detect_delay=bt["delay"], return_inputs=True, return_states=True, sensor=clean)
    _check_replay(out, bt["x0"], bt["ub"], bt["stuck"], clean, ZERO, bt["seed"], faults=f, delay=bt["delay"])
    pred, xh, a = out["sensor"]["pred"], out["x_hist"], _applied(out, d)
    seen = 0
    for b in range(B):
        on, k = int(f["onset"][b, 0]), b % 8
        for t in range(on - d + 1):
            assert np.abs(pred[t, b] - xh[t + d - 1, b]).max() <= 1e-10, (b, t)
        if bt["delay"][b] >= d and on + d <= T:
            lost = np.abs(a[on:on + d, b, k]).max()                # what the controller believes the dead thruster delivers
            if lost > 1e-3 or f["stuck"][b, 0, k] > 0:
                assert np.abs(pred[on, b] - xh[on + d - 1, b]).max() > 1e-8, (b, lost)
                seen += 1
    assert seen >= 8


def test_with_a_dispersed_plant_and_the_pwm_actuator(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 96, 6
    x0, ub, stuck = _one_fault(B, N, NT, 14)
    plant = _plant(B, NT, seed=15)
    act = dict(mode="pwm", substeps=8, min_on=2, align="centred", tau_on=0.02, tau_off=0.01, fields=("applied", "ticks", "state"))
    sen = _sensor(B, NT)
    out = _sim(gpu_mpc_factory(N=N, NT=NT, dtype="f32"), x0, ub, stuck, N, T, sen, plant=plant, actuator=act)
    _check_replay(out, x0, ub, stuck, sen, NOISE, 5, plant=plant, act=act)
    # the actuator sees the command the plant applied in the step: in the first d steps the pending ones
    from test_gpu_actuators import _targets
    _, k = _targets(sen["pending"][:, 0], ub, act)
    assert np.array_equal(out["actuator"]["ticks"][0], k)


def test_with_a_mission(gpu_mpc_factory):
    N, NT, B, T, d = 10, 8, 96, 8, 2
    x0, ub, stuck = _one_fault(B, N, NT, 15)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    sen = _sensor(B, NT)
    table, offset = (7 * np.arange(B) % 3).astype(np.int32), (5 * np.arange(B) % 23).astype(np.int32)
    cols = 22 + T + N + d                                          # the largest offset just fits
    ms = dict(tables=XT[:, :, :cols], utables=UT[:, :, :cols], table=table, offset=offset)
    kw = dict(outcomes=dict(tol_pos=1.0, tol_vel=0.3, tol_rate=0.1, cost=True), return_status=True)
    out = mpc.simulate(x0, ub, stuck, None, T, noise=NOISE, seed=5, return_inputs=True, return_states=True, mission=ms, sensor=sen, **kw)
    _check_replay(out, x0, ub, stuck, sen, NOISE, 5)
    # one table without offsets is the shared trajectory of T + N + L columns: the same windows for the solve (at + L columns), the
    # same columns for the outcomes and the cost (at t + 1 and t), bit for bit
    one = dict(tables=XT[1:2, :, :T + N + d], utables=UT[1:2, :, :T + N + d])
    a = mpc.simulate(x0, ub, stuck, None, T, noise=NOISE, seed=5, return_inputs=True, return_states=True, mission=one, sensor=sen, **kw)
    b = mpc.simulate(x0, ub, stuck, XT[1][:, :T + N + d], T, uref_traj=UT[1][:, :T + N + d], noise=NOISE, seed=5, return_inputs=True,
                     return_states=True, sensor=sen, **kw)
    _same_bits(a, b)
    _same_sensor(a, b)
    assert not np.array_equal(a["u"][d:], out["u"][d:])
    # the tables must hold offset + T + N + L columns: refused by Python, and by the library when called past Python's check
    short = dict(ms, tables=XT[:, :, :cols - 1], utables=UT[:, :, :cols - 1])
    with pytest.raises(ValueError, match="L"):
        mpc.simulate(x0, ub, stuck, None, T, mission=short, sensor=sen)
    v = int(np.argmax(offset))
    xt = np.ascontiguousarray(XT[:, :, :cols - 1].transpose(0, 2, 1))
    msc = _lib.ftmpc_mission(struct_size=C.sizeof(_lib.ftmpc_mission), n_tables=3, n_cols=cols - 1, xref=xt.ctypes.data_as(dp),
                             table=table.ctypes.data_as(ip), offset=offset.ctypes.data_as(ip))
    sec = _lib.ftmpc_sensor(struct_size=C.sizeof(_lib.ftmpc_sensor), latency=d, predict=1)
    oc = _lib.ftmpc_outcomes(struct_size=C.sizeof(_lib.ftmpc_outcomes))
    x, nz = x0.copy(), np.array(NOISE)
    rc = mpc.lib.ftmpc_simulate_sensor_batch(mpc._h, B, T, x.ctypes.data_as(dp), ub.ctypes.data_as(dp), stuck.ctypes.data_as(dp), None, None,
                                             nz.ctypes.data_as(dp), C.c_uint64(5), 0, 8, 1e-9, None, None, None, None, C.byref(oc), None,
                                             C.byref(msc), None, C.byref(sec))
    err = mpc.lib.ftmpc_last_error(mpc._h).decode()
    assert rc == -1 and "ftmpc_mission.offset" in err and f"vehicle {v} " in err and "T + N + L" in err, err
    assert np.array_equal(x, x0)
    sec.predict = 0                                                # without the prediction the same tables are long enough
    rc = mpc.lib.ftmpc_simulate_sensor_batch(mpc._h, B, T, x.ctypes.data_as(dp), ub.ctypes.data_as(dp), stuck.ctypes.data_as(dp), None, None,
                                             nz.ctypes.data_as(dp), C.c_uint64(5), 0, 8, 1e-9, None, None, None, None, C.byref(oc), None,
                                             C.byref(msc), None, C.byref(sec))
    assert rc == 0, mpc.lib.ftmpc_last_error(mpc._h)


def test_with_the_thruster_sqp_loop(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 32, 4
    x0, ub, stuck = _one_fault(B, N, NT, 13)
    sen = _sensor(B, NT)
    out = _sim(gpu_mpc_factory(N=N, NT=NT, dtype="f32"), x0, ub, stuck, N, T, sen, sqp_iters=2)
    _check_replay(out, x0, ub, stuck, sen, NOISE, 5)
    assert out["u"][2:].any()


def test_with_the_wrench_sqp_loop(gpu_mpc_factory, wrench24):
    w, T, d = wrench24, 4, 2
    mpc = gpu_mpc_factory(N=15, NT=16, dtype="f64", max_iters=60, terminal_set=w["term"])
    sen = _sensor(24, 16, d=d)
    out = mpc.simulate(w["x0"], w["ub"], w["stuck"], w["xr"][:, :T + 15 + d], T, noise=(1e-4,) * 4, seed=w["seed"], formulation="wrench",
                       sqp_iters=2, return_inputs=True, return_states=True, sensor=sen)
    _check_replay(out, w["x0"], w["ub"], w["stuck"], sen, (1e-4,) * 4, w["seed"])
    assert out["u"][d:].any()


# ---------------------------------------------------------------------------------------------------------------------------
# (H) refusals, on a handle and on the driver: FTMPC_ERR_ARG, the message names the field (and the vehicle), x untouched
# ---------------------------------------------------------------------------------------------------------------------------
def _bad_structs(B, NT):
    """(field, vehicle | None, struct, what it points into) for every refusal of include/ftmpc.h."""
    size = C.sizeof(_lib.ftmpc_sensor)
    v = B - 2                                                      # on three slots: in the last shard
    S = _lib.ftmpc_sensor
    nan_b, inf_p, pend, hist = np.zeros((B, 12)), np.zeros((B, 2, NT)), np.zeros((B, 1, NT)), np.zeros((2, B, 13))
    nan_b[v, 7], inf_p[v, 1, 3] = np.nan, np.inf

    def sig(k, val):
        s = S(struct_size=size)
        s.sigma[k] = val
        return s
    return [("struct_size", None, S(struct_size=size - 8, latency=2), None),
            ("latency", None, S(struct_size=size, latency=9), None), ("latency", None, S(struct_size=size, latency=-1), None),
            ("predict", None, S(struct_size=size, latency=2, predict=2), None),
            ("predict", None, S(struct_size=size, latency=2, predict=-1), None),
            ("sigma", None, sig(0, -1e-3), None), ("sigma", None, sig(2, np.nan), None), ("sigma", None, sig(3, np.inf), None),
            ("bias", v, S(struct_size=size, bias=nan_b.ctypes.data_as(dp)), nan_b),
            ("pending", v, S(struct_size=size, latency=2, pending=inf_p.ctypes.data_as(dp)), inf_p),
            ("pending", None, S(struct_size=size, latency=0, pending=pend.ctypes.data_as(dp)), pend),
            ("pred_hist", None, S(struct_size=size, latency=2, predict=0, pred_hist=hist.ctypes.data_as(dp)), hist),
            ("step0", None, S(struct_size=size, step0=-1), None)]


def test_refusals(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 12, 2
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 0, 20)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f32"), devices=[0, 0, 0])
    try:
        for n, (field, v, se, keep) in enumerate(_bad_structs(B, NT)):
            for obj in (mpc, m):
                for wrench in ((False, True) if n in (0, 8, 9) else (False,)):
                    name = "wrench_sensor_batch" if wrench else "sensor_batch"
                    rc, err, out = _entry(obj, name, x0, ub, stuck, N, T, 1, (None, None, None, C.byref(se)), want=False, wrench=wrench)
                    assert rc == -1 and f"ftmpc_sensor.{field}".encode() in err, (field, err)
                    if v is not None:
                        assert f"vehicle {v} ".encode() in err, err
                    assert np.array_equal(out["x"], x0)
        # what the front end refuses itself never reaches the library
        with pytest.raises(ValueError):
            mpc.simulate(x0, ub, stuck, _hover(N, T), T, sensor=dict(latency=9))
        with pytest.raises(ValueError):
            mpc.simulate(x0, ub, stuck, _hover(N, T), T, sensor=dict(latency=2, predict=True))      # T + N + L columns
        # and a good sensor is accepted by both
        sen = _sensor(B, NT)
        a = _sim(mpc, x0, ub, stuck, N, T, sen)
        b = _sim(m, x0, ub, stuck, N, T, sen)
        assert np.array_equal(a["x"], b["x"])
        _same_sensor(a, b)
    finally:
        m.close()
