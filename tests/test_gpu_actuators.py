"""GPU: pulsed (PWM) thrusters and valve lag in the on-device closed loops (ftmpc_plant_step_act_kernel; ftmpc_simulate_actuator_batch,
ftmpc_simulate_wrench_actuator_batch, ftmpc_multi_simulate_*_actuator_batch; BatchedMPC.simulate(actuator=...)).

The reference is written here from oracle pieces and does not use ft_mpc_amd/actuators.py: the definition of include/ftmpc.h
(ticks, dead band, alignment window, the valve recurrence with the four lag constants) in NumPy, oracle.refmath.plant_dx_dt under the
thrust m_j + stuck of each sub-step, integrated by oracle.refmath.rk4 with dt = h, then the noise of oracle.closed_loop.u01 at
counter (t * index_total + index0 + b) * 13 + i and the renormalisation, once per step.  Every run is replayed step by step from its
own histories (x_hist[t-1] under u_hist[t] and the carried valve state must give x_hist[t]), which checks the plant kernel alone
whatever the solver returned.  Bound: rtol 1e-12 + atol 1e-12, that of tests/test_gpu_plant_dispersion.py: the same arithmetic, S
times as many steps of 1 / S the length.  ticks are compared exactly; before that the test asserts that no d_i S of the run lies
within 1e-9 of a half-integer, so that an FMA contraction in floor(d S + 0.5) cannot flip a tick."""
import ctypes as C

import numpy as np
import pytest

import ft_mpc_amd
from ft_mpc_amd import _lib
from ft_mpc_amd._lib import FtmpcError
from ft_mpc_amd.batch import _outcome_request
from ft_mpc_amd.controllers.tools.terminal_ingredients import load_terminal
from ft_mpc_amd.sharding import MultiGPUMPC
from oracle import closed_loop as cl
from oracle import qp_oracle as qo
from oracle import refmath as rm
from test_gpu_outcomes import _hover, _plant_patterns, _thruster_batch, _wrench_batch
from test_gpu_plant_dispersion import _nominal, _plant

pytestmark = pytest.mark.gpu
NOISE = (1e-3,) * 4
DT = 0.1
ALL = ("delivered", "pulses", "applied", "ticks", "state")
PWM_A = dict(mode="pwm", substeps=8, min_on=2, align="centred", tau_on=0.02, tau_off=0.01, fields=ALL)


# ---------------------------------------------------------------------------------------------------------------------------
# the definition, in NumPy
# ---------------------------------------------------------------------------------------------------------------------------
def _lag(h, tau):
    return (np.exp(-h / tau), -np.expm1(-h / tau) * tau / h) if tau > 0 else (0.0, 0.0)


def _targets(u, pu, act):
    """g [S,B,NT] and k [B,NT] | None of one step; asserts that no d S is within 1e-9 of a half-integer."""
    S = act.get("substeps", 1)
    if act.get("mode", "proportional") != "pwm":
        return np.repeat(np.where(pu > 0, u, 0.0)[None], S, 0), None
    live = pu > 0
    d = np.where(live, np.clip(u / np.where(live, pu, 1.0), 0.0, 1.0), 0.0)
    dS = d * S
    assert np.abs(dS - np.floor(dS) - 0.5).min() > 1e-9, "a duty within 1e-9 of a half tick: take another seed"
    k = np.floor(dS + 0.5).astype(np.int32)
    k[k < act.get("min_on", 0)] = 0
    s = {"leading": np.zeros_like(k), "centred": (S - k) // 2, "trailing": S - k}[act.get("align", "leading")]
    j = np.arange(S)[:, None, None]
    return np.where((j >= s[None]) & (j < (s + k)[None]), np.where(live, pu, 0.0)[None], 0.0), k


def _act_step(x_prev, u, pu, ps, a, act, plant, t, noise, seed, index0=0, index_total=None):
    """One loop step by the definition: (x [B,13], valve state [B,NT], applied [B,NT], ticks [B,NT] | None, delivered increment [B])."""
    B, NT = u.shape
    S = act.get("substeps", 1)
    h = DT / S
    (E_on, K_on), (E_off, K_off) = _lag(h, act.get("tau_on", 0.0)), _lag(h, act.get("tau_off", 0.0))
    g, k = _targets(u, pu, act)
    p = dict(_nominal(B, NT), **plant)
    a = a.copy()
    x = x_prev.copy()
    applied, deliv = np.zeros((B, NT)), np.zeros(B)
    ones = np.ones(NT)
    add = [np.concatenate([np.zeros(3), p["force"][b] / p["mass"][b], np.zeros(4), np.linalg.solve(p["J"][b], p["torque"][b])]) for b in range(B)]
    for j in range(S):
        on = g[j] > a
        m = g[j] + (a - g[j]) * np.where(on, K_on, K_off)
        a = g[j] + (a - g[j]) * np.where(on, E_on, E_off)
        thrust = m + ps
        applied += thrust
        deliv += h * thrust.sum(axis=1)
        for b in range(B):
            x[b] = rm.rk4(lambda y: rm.plant_dx_dt(y, m[b], p["D"][b], ps[b], ones, p["mass"][b], p["J"][b]) + add[b], x[b], h)
    amp = np.repeat(np.asarray(noise, float), [3, 3, 4, 3])
    total = B if index_total is None else index_total
    idx = (np.uint64(t) * np.uint64(total) + np.uint64(index0) + np.arange(B, dtype=np.uint64))[:, None] * np.uint64(13) \
        + np.arange(13, dtype=np.uint64)[None, :]
    x = x + amp[None, :] * cl.u01(seed, idx) * (amp[None, :] > 0)
    x[:, 6:10] /= np.linalg.norm(x[:, 6:10], axis=1, keepdims=True)
    return x, a, applied / S, k, deliv


def _check_replay(out, x0, ub, stuck, act, plant, noise, seed, faults=None, state0=None, nominal_must_miss=False):
    """Every x_hist[t] and every actuator output of `out` against the definition; returns the valve state the replay carries."""
    xh, uh, ao = out["x_hist"], out["u"], out["actuator"]
    T, B, NT = uh.shape
    pu, ps = (np.repeat(ub[None], T, 0), np.repeat(stuck[None], T, 0)) if faults is None else _plant_patterns(ub, stuck, faults, T)
    a = np.zeros((B, NT)) if state0 is None else np.array(state0, float)
    deliv, pulses, worst = np.zeros(B), np.zeros(B, np.int32), 0.0
    for t in range(T):
        x, a, applied, k, dl = _act_step(x0 if t == 0 else xh[t - 1], uh[t], pu[t], ps[t], a, act, plant, t, noise, seed)
        worst = max(worst, np.abs(xh[t] - x).max())
        np.testing.assert_allclose(xh[t], x, rtol=1e-12, atol=1e-12, err_msg=f"step {t}")
        deliv += dl
        if "applied" in ao:
            np.testing.assert_allclose(ao["applied"][t], applied, rtol=1e-12, atol=1e-12, err_msg=f"applied, step {t}")
        if k is not None:
            pulses += (k > 0).sum(axis=1).astype(np.int32)
            if "ticks" in ao:
                assert np.array_equal(ao["ticks"][t], k), f"ticks, step {t}"
    assert np.array_equal(out["x"], xh[-1])
    if "delivered" in ao:
        np.testing.assert_allclose(ao["delivered"], deliv, rtol=1e-12, atol=1e-12)
    if "applied" in ao and "delivered" in ao:        # the histories add up to the sum
        np.testing.assert_allclose(DT * ao["applied"].sum(axis=(0, 2)), ao["delivered"], rtol=1e-12, atol=1e-12)
    if "pulses" in ao:
        assert np.array_equal(ao["pulses"], pulses)
    if "state" in ao:
        np.testing.assert_allclose(ao["state"], a, rtol=1e-12, atol=1e-12)
    print(f"replay: max |x_hist - definition| = {worst:.3e}")
    if nominal_must_miss:      # the plant kernels' step (no actuator) must not explain the run
        x, *_ = _act_step(x0, uh[0], pu[0], ps[0], np.zeros((B, NT)), {}, plant, 0, noise, seed)
        miss = np.abs(xh[0] - x).max(axis=1)
        print(f"nominal replay of step 0 misses by median {np.median(miss):.3e}, {(miss > 1e-6).sum()} of {B} vehicles above 1e-6")
        assert (miss > 1e-6).sum() >= (B + 1) // 2
    return a


def _sim(mpc, x0, ub, stuck, N, T, act, seed=5, noise=NOISE, **kw):
    return mpc.simulate(x0, ub, stuck, _hover(N, T), T, noise=noise, seed=seed, return_inputs=True, return_states=True, actuator=act, **kw)


def _one_fault(B, N, NT, seed):
    return qo.make_batch(B, N, NT, 1, seed)[:3]


# ---------------------------------------------------------------------------------------------------------------------------
# (A) replay from the run's own histories
# ---------------------------------------------------------------------------------------------------------------------------
def test_pwm_with_lag_replay_from_the_runs_own_histories(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 96, 12                                    # B = 96: a partial last wave
    x0, ub, stuck = _one_fault(B, N, NT, 11)
    out = _sim(gpu_mpc_factory(N=N, NT=NT, dtype="f32"), x0, ub, stuck, N, T, PWM_A)
    assert sorted(out["actuator"]) == sorted(ALL)
    _check_replay(out, x0, ub, stuck, PWM_A, {}, NOISE, 5, nominal_must_miss=True)


# ---------------------------------------------------------------------------------------------------------------------------
# (B) each alone
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [dict(mode="pwm", substeps=5, align="leading"), dict(mode="pwm", substeps=5, align="trailing"),
                                 dict(mode="proportional", substeps=4, tau_on=0.02, tau_off=0.01), dict(mode="pwm", substeps=64)],
                         ids=["leading-S5", "trailing-S5", "proportional-lag", "S64"])
def test_each_alone(gpu_mpc_factory, act):
    N, NT, B, T = 10, 8, 70, 3
    x0, ub, stuck = _one_fault(B, N, NT, 12)
    act = dict(act, fields=ALL if act["mode"] == "pwm" else ("delivered", "applied", "state"))
    out = _sim(gpu_mpc_factory(N=N, NT=NT, dtype="f32"), x0, ub, stuck, N, T, act)
    _check_replay(out, x0, ub, stuck, act, {}, NOISE, 5)


def test_dead_band(gpu_mpc_factory):
    N, NT, B, T, S = 10, 8, 70, 3, 8
    x0, ub, stuck = _one_fault(B, N, NT, 12)
    act = dict(mode="pwm", substeps=S, min_on=3, fields=ALL)
    out = _sim(gpu_mpc_factory(N=N, NT=NT, dtype="f32"), x0, ub, stuck, N, T, act)
    _check_replay(out, x0, ub, stuck, act, {}, NOISE, 5)
    _, raw = _targets(out["u"].reshape(T * B, NT), np.tile(ub, (T, 1)), dict(mode="pwm", substeps=S))
    short = (raw.reshape(T, B, NT) == 1) | (raw.reshape(T, B, NT) == 2)
    assert short.sum() > 0
    assert np.array_equal(out["actuator"]["ticks"][short], np.zeros(short.sum(), np.int32))
    assert np.array_equal(out["actuator"]["applied"][short], np.broadcast_to(stuck, (T, B, NT))[short])      # stuck only


# ---------------------------------------------------------------------------------------------------------------------------
# (C) every plant-model field dispersed at once
# ---------------------------------------------------------------------------------------------------------------------------
def test_dispersed_with_a_fault_schedule_whose_onset_precedes_detection(gpu_mpc_factory):
    bt = _thruster_batch(96, 10)
    plant = _plant(96, 8, seed=15)
    assert (bt["delay"] > 0).any()
    f = bt["faults"]
    out = gpu_mpc_factory(N=10, NT=8, dtype="f32").simulate(bt["x0"], bt["ub"], bt["stuck"], bt["xr"], bt["T"], noise=NOISE, seed=bt["seed"],
                                                           faults=f, detect_delay=bt["delay"], return_inputs=True, return_states=True,
                                                           plant=plant, actuator=PWM_A)
    _check_replay(out, bt["x0"], bt["ub"], bt["stuck"], PWM_A, plant, NOISE, bt["seed"], faults=f)
    # a thruster that dies mid-run (no jam): from its onset on no ticks, and what it delivers only falls, towards nothing
    ap, tk = out["actuator"]["applied"], out["actuator"]["ticks"]
    seen = 0
    for b in range(96):
        i, on = b % 8, int(f["onset"][b, 0])
        if f["stuck"][b, 0, i] == 0.0:
            assert (tk[on:, b, i] == 0).all()
            tail = ap[on:, b, i]
            assert (np.diff(tail) <= 0).all() and (tail >= 0).all() and tail[-1] <= 1e-3 * 3.4
            seen += tail[0] > 0
    assert seen > 0        # some valve was open when its thruster died: the decay was exercised


def test_dispersed_wrench_form(gpu_mpc_factory):
    t = load_terminal().term_set
    term = (t, np.asarray(t.A, float).reshape(-1, 9), np.asarray(t.b, float).reshape(-1))
    bt = _wrench_batch(term)
    T, B = 6, 24
    sel = np.r_[0:12, 20:32]
    f = {k: v[sel] for k, v in bt["faults"].items()}
    f["onset"] = np.minimum(f["onset"], 4)
    x0, ub, stuck = bt["x0"][sel], bt["ub"][sel], bt["stuck"][sel]
    xr = bt["xr"][:, :T + bt["N"]]
    plant = _plant(B, 16, seed=8)
    act = dict(mode="pwm", substeps=16, min_on=1, align="centred", tau_on=0.02, tau_off=0.01, fields=ALL)
    mpc = gpu_mpc_factory(N=15, NT=16, dtype="f64", max_iters=60, terminal_set=term[0])
    noise = (1e-4,) * 4
    out = mpc.simulate(x0, ub, stuck, xr, T, noise=noise, seed=bt["seed"], faults=f, formulation="wrench", return_inputs=True,
                       return_states=True, plant=plant, actuator=act)
    assert out["alloc_failed"].shape == (T,)
    _check_replay(out, x0, ub, stuck, act, plant, noise, bt["seed"], faults=f)


def test_dispersed_thruster_sqp_loop(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 32, 4
    x0, ub, stuck = _one_fault(B, N, NT, 13)
    plant = _plant(B, NT, seed=9)
    out = _sim(gpu_mpc_factory(N=N, NT=NT, dtype="f32"), x0, ub, stuck, N, T, PWM_A, sqp_iters=2, plant=plant)
    _check_replay(out, x0, ub, stuck, PWM_A, plant, NOISE, 5)


# ---------------------------------------------------------------------------------------------------------------------------
# (D) the trivial actuator
# ---------------------------------------------------------------------------------------------------------------------------
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _entry(obj, name, x0, ub, stuck, N, T, seed, tail, want=True, wrench=False):
    """A thruster (or, with dummy hull arguments, wrench) loop entry called through ctypes with the structs `tail` after the outcomes."""
    B, NT = ub.shape
    multi = isinstance(obj, MultiGPUMPC)
    oc, orec, sh = _outcome_request(obj, B, T, False, True, True, 0, None) if want else (_lib.ftmpc_outcomes(struct_size=C.sizeof(_lib.ftmpc_outcomes)), None, None)
    x, uh, xh, bad = x0.copy(), np.empty((T, B, NT)), np.empty((T, B, 13)), np.zeros(T, np.int32)
    xr, nz = np.ascontiguousarray(_hover(N, T).reshape(-1, order="F")), np.array(NOISE)
    f = getattr(obj.lib, ("ftmpc_multi_simulate_" if multi else "ftmpc_simulate_") + name)
    head = (obj._h, B, T, x.ctypes.data_as(dp), ub.ctypes.data_as(dp), stuck.ctypes.data_as(dp))
    mid = (xr.ctypes.data_as(dp), None, nz.ctypes.data_as(dp), C.c_uint64(seed), 0, 8, 1e-9)
    if wrench:
        hA, hb, abad = np.zeros(6), np.zeros(B), np.zeros(T, np.int32)
        rc = f(*head, hA.ctypes.data_as(dp), 1, None, hb.ctypes.data_as(dp), 1, *mid, 0.0, None, uh.ctypes.data_as(dp), xh.ctypes.data_as(dp),
               bad.ctypes.data_as(ip), abad.ctypes.data_as(ip), C.byref(oc), *tail)
    else:
        rc = f(*head, *mid, None, uh.ctypes.data_as(dp), xh.ctypes.data_as(dp), bad.ctypes.data_as(ip), C.byref(oc), *tail)
    err = (obj.lib.ftmpc_multi_last_error if multi else obj.lib.ftmpc_last_error)(obj._h)
    return rc, err, dict(x=x, u=uh, x_hist=xh, not_converged=bad, status_hist=sh, outcomes=orec)


def _same_bits(a, b, actuator=False):
    for k in ("x", "u", "x_hist", "not_converged", "status_hist"):
        assert np.array_equal(a[k], b[k]), k
    assert sorted(a["outcomes"]) == sorted(b["outcomes"])
    for k in b["outcomes"]:
        assert np.array_equal(a["outcomes"][k], b["outcomes"][k]), k
    if actuator:
        assert sorted(a["actuator"]) == sorted(b["actuator"])
        for k in b["actuator"]:
            assert np.array_equal(a["actuator"][k], b["actuator"][k]), k


def test_trivial_actuator_gives_the_bits_of_the_mission_entry(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 96, 4
    x0, ub, stuck = _one_fault(B, N, NT, 16)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    rc, err, ref = _entry(mpc, "mission_batch", x0, ub, stuck, N, T, 7, (None, None))
    assert rc == 0, err
    rc, err, out = _entry(mpc, "actuator_batch", x0, ub, stuck, N, T, 7, (None, None, None))
    assert rc == 0, err
    _same_bits(out, ref)
    for substeps in (0, 1):
        ac = _lib.ftmpc_actuator(struct_size=C.sizeof(_lib.ftmpc_actuator), substeps=substeps)
        rc, err, out = _entry(mpc, "actuator_batch", x0, ub, stuck, N, T, 7, (None, None, C.byref(ac)))
        assert rc == 0, err
        _same_bits(out, ref)


def test_proportional_one_substep_without_lag_is_the_plant_kernels_step(gpu_mpc_factory):
    N, NT, B = 10, 8, 96
    x0, ub, stuck = _one_fault(B, N, NT, 16)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    base = _sim(mpc, x0, ub, stuck, N, 1, None)
    act = dict(mode="proportional", substeps=1, fields=("delivered",))          # an output: the new kernel runs
    out = _sim(mpc, x0, ub, stuck, N, 1, act)
    assert np.array_equal(out["u"], base["u"])
    print("trivial parameters through the actuator kernel against the plant kernel: max |x - x| =", np.abs(out["x"] - base["x"]).max())
    assert np.abs(out["x"] - base["x"]).max() <= 1e-13
    cmd = np.where(ub > 0, out["u"][0], 0.0) + stuck
    np.testing.assert_allclose(out["actuator"]["delivered"], DT * cmd.sum(axis=1), rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------------
# (E) continuation across calls
# ---------------------------------------------------------------------------------------------------------------------------
def test_two_calls_with_the_state_handed_over_continue_one(gpu_mpc_factory):
    N, NT, B = 10, 8, 70
    x0, ub, stuck = _one_fault(B, N, NT, 17)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    zero = (0.0,) * 4
    whole = _sim(mpc, x0, ub, stuck, N, 12, PWM_A, noise=zero)
    first = _sim(mpc, x0, ub, stuck, N, 6, PWM_A, noise=zero)
    second = _sim(mpc, first["x"], ub, stuck, N, 6, dict(PWM_A, state=first["actuator"]["state"]), noise=zero)
    # the first six steps are the same computation; step 6's state to the replay bound
    np.testing.assert_allclose(first["x"], whole["x_hist"][5], rtol=1e-12, atol=1e-12)
    a_whole = _check_replay(whole, x0, ub, stuck, PWM_A, {}, zero, 5)
    a6 = _check_replay(first, x0, ub, stuck, PWM_A, {}, zero, 5)
    assert (a6 > 0).any()                                          # there is a state to hand over
    # the second call (no warm start of its own: other commands) follows the definition from the state handed over, and returns
    # the valve state the replay carries
    a12 = _check_replay(second, first["x"], ub, stuck, PWM_A, {}, zero, 5, state0=first["actuator"]["state"])
    np.testing.assert_allclose(second["actuator"]["state"], a12, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(whole["actuator"]["state"], a_whole, rtol=1e-12, atol=1e-12)
    # without the state the second call starts from closed valves: another first step
    cold = _sim(mpc, first["x"], ub, stuck, N, 1, PWM_A, noise=zero)
    assert np.array_equal(cold["u"][0], second["u"][0]) and not np.array_equal(cold["x_hist"][0], second["x_hist"][0])


# ---------------------------------------------------------------------------------------------------------------------------
# (F) slices of a campaign and device slots
# ---------------------------------------------------------------------------------------------------------------------------
def _run(mpc, bt, state, lo=0, hi=None, **kw):
    hi = bt["B"] if hi is None else hi
    f = {k: v[lo:hi] for k, v in bt["faults"].items()}
    return mpc.simulate(bt["x0"][lo:hi], bt["ub"][lo:hi], bt["stuck"][lo:hi], bt["xr"], bt["T"], noise=NOISE, seed=bt["seed"],
                        faults=f, detect_delay=bt["delay"][lo:hi], return_inputs=True, return_states=True,
                        actuator=dict(PWM_A, state=state[lo:hi]), **kw)


def test_slices_with_the_state_sliced_equal_the_whole():
    bt = _thruster_batch(96, 10)
    B = bt["B"]
    state = np.random.default_rng(21).uniform(0, 3.4, (B, 8))

    def fresh(lo, hi, **kw):
        mpc = ft_mpc_amd.BatchedMPC(N=10, NT=8, dtype="f32")
        try:
            return _run(mpc, bt, state, lo, hi, outcomes=True, return_status=True, **kw)
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
        axis = 1 if k in ("applied", "ticks") else 0
        assert np.array_equal(np.concatenate([p["actuator"][k] for p in parts], axis=axis), whole["actuator"][k]), k


def test_three_slots_on_one_device_equal_one_handle(gpu_mpc_factory):
    bt = _thruster_batch(100, 20)
    bt["T"] = 8
    bt["xr"] = _hover(20, 8)
    bt["faults"]["onset"] = np.minimum(bt["faults"]["onset"], 6)
    state = np.random.default_rng(22).uniform(0, 3.4, (100, 8))
    kw = dict(outcomes=dict(tol_pos=1.0, tol_vel=0.3, tol_rate=0.1), return_status=True)
    serial = _run(gpu_mpc_factory(N=20, NT=8, dtype="f32"), bt, state, **kw)
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=20, NT=8, dtype="f32"), devices=[0, 0, 0])
    try:
        multi = _run(m, bt, state, **kw)
    finally:
        m.close()
    _same_bits(multi, serial, actuator=True)


# ---------------------------------------------------------------------------------------------------------------------------
# (G) refusals, on a handle and on the driver: FTMPC_ERR_ARG, the message names the field (and the vehicle), x untouched
# ---------------------------------------------------------------------------------------------------------------------------
def _bad_structs(B, NT):
    """(field, vehicle | None, struct, what it points into) for every refusal of include/ftmpc.h."""
    size = C.sizeof(_lib.ftmpc_actuator)
    v = B - 2                                                      # on three slots: in the last shard
    pul, tick = np.zeros(B, np.int32), np.zeros((2, B, NT), np.int32)
    neg, nan = np.zeros((B, NT)), np.zeros((B, NT))
    neg[v, 3], nan[v, NT - 1] = -1e-3, np.nan
    A = _lib.ftmpc_actuator
    return [("struct_size", None, A(struct_size=size - 8, mode=1, substeps=8), None),
            ("mode", None, A(struct_size=size, mode=2, substeps=8), None), ("mode", None, A(struct_size=size, mode=-1), None),
            ("substeps", None, A(struct_size=size, mode=1, substeps=65), None),
            ("substeps", None, A(struct_size=size, mode=1, substeps=-1), None),
            ("min_on", None, A(struct_size=size, mode=1, substeps=8, min_on=-1), None),
            ("min_on", None, A(struct_size=size, mode=1, substeps=8, min_on=9), None),
            ("min_on", None, A(struct_size=size, mode=1, substeps=0, min_on=2), None),      # substeps 0 is read as 1
            ("align", None, A(struct_size=size, mode=1, substeps=8, align=3), None),
            ("align", None, A(struct_size=size, mode=1, substeps=8, align=-1), None),
            ("tau_on", None, A(struct_size=size, mode=1, substeps=8, tau_on=-0.01), None),
            ("tau_on", None, A(struct_size=size, mode=1, substeps=8, tau_on=np.nan), None),
            ("tau_off", None, A(struct_size=size, mode=1, substeps=8, tau_off=np.inf), None),
            ("min_on", None, A(struct_size=size, mode=0, substeps=8, min_on=1), None),
            ("align", None, A(struct_size=size, mode=0, substeps=8, align=1), None),
            ("pulses", None, A(struct_size=size, mode=0, substeps=8, pulses=pul.ctypes.data_as(ip)), pul),
            ("ticks_hist", None, A(struct_size=size, mode=0, substeps=8, ticks_hist=tick.ctypes.data_as(ip)), tick),
            ("state", v, A(struct_size=size, mode=1, substeps=8, state=neg.ctypes.data_as(dp)), neg),
            ("state", v, A(struct_size=size, mode=0, substeps=2, state=nan.ctypes.data_as(dp)), nan)]


def test_refusals(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 12, 2
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 0, 20)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f32"), devices=[0, 0, 0])
    try:
        bad = _bad_structs(B, NT)
        for n, (field, v, ac, keep) in enumerate(bad):
            for obj in (mpc, m):
                for wrench in ((False, True) if n in (0, 6, 17) else (False,)):
                    name = "wrench_actuator_batch" if wrench else "actuator_batch"
                    rc, err, out = _entry(obj, name, x0, ub, stuck, N, T, 1, (None, None, C.byref(ac)), want=False, wrench=wrench)
                    assert rc == -1 and f"ftmpc_actuator.{field}".encode() in err, (field, err)
                    if v is not None:
                        assert f"vehicle {v} ".encode() in err, err
                    assert np.array_equal(out["x"], x0)
        # what the front end refuses itself never reaches the library
        with pytest.raises(ValueError):
            mpc.simulate(x0, ub, stuck, _hover(N, T), T, actuator=dict(mode="pwm", substeps=65))
        with pytest.raises(ValueError):
            mpc.simulate(x0, ub, stuck, _hover(N, T), T, actuator=dict(mode="proportional", fields=("pulses",)))
        # and a good actuator is accepted by both
        a = mpc.simulate(x0, ub, stuck, _hover(N, T), T, actuator=PWM_A)
        b = m.simulate(x0, ub, stuck, _hover(N, T), T, actuator=PWM_A)
        assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["actuator"]["delivered"], b["actuator"]["delivered"])
    finally:
        m.close()
