"""GPU: plant dispersion in the on-device closed loops (ftmpc_plant_step_var_kernel; ftmpc_simulate_plant_batch,
ftmpc_simulate_wrench_plant_batch, ftmpc_multi_simulate_*_plant_batch; BatchedMPC.simulate(plant=...)).

The reference is written here from oracle pieces and does not use ft_mpc_amd/dispersion.py: oracle.refmath.plant_dx_dt with the
vehicle's D_b, m_b, J_b, plus f_b / m_b on rows 3..5 and solve(J_b, t_b) on rows 10..12, integrated by oracle.refmath.rk4, then the
noise of oracle.closed_loop.u01 at counter (t * index_total + index0 + b) * 13 + i, then the renormalisation.  Every run is replayed
step by step from its own histories (x_hist[t-1] under u_hist[t] must give x_hist[t]), which checks the plant kernel alone whatever
the solver returned.  Bound: rtol 1e-12 + atol 1e-12, that of tests/test_gpu_outcomes.py for the same reason -- a step is a few
hundred float64 operations, cond(J_b) <= 3.4, and FMA contraction and inverse-versus-solve are the only sources of difference.  So
that the parity cannot hold vacuously, the same replay with the NOMINAL plant must miss x_hist[0] by more than 1e-6 on at least half
of the vehicles (checked on the CPU with random commands: each field alone moves one step by at least 2.6e-5 on every vehicle of
make_batch(96, 10, 8, 0, 11), medians mass 1.3e-3, inertia 2.7e-2, D 2.1e-2, force 2.4e-4, torque 1.6e-3; with the controller's own
commands the margin is unmeasured, hence half and not all)."""
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

pytestmark = pytest.mark.gpu
FIELDS = ("mass", "J", "D", "force", "torque")
J0 = rm.INERTIA + 0.02 * np.array([[0, 1, -1], [1, 0, 0.5], [-1, 0.5, 0]])


def _plant(B, NT, seed=3, fields=FIELDS):
    """mass and inertia scale by +-20 %, gain +-10 %, centre of mass +-2 cm, force +-0.05 N, torque +-0.005 N m."""
    rng = np.random.default_rng(seed)
    D = rm.allocation_matrix_16() if NT == 16 else rm.allocation_matrix_8()
    s = 1 + rng.uniform(-0.2, 0.2, (B, 3))
    gain = 1 + rng.uniform(-0.1, 0.1, (B, NT))
    d = rng.uniform(-0.02, 0.02, (B, 3))
    Db = np.empty((B, 6, NT))
    for b in range(B):
        for i in range(NT):
            f, t = D[0:3, i] * gain[b, i], D[3:6, i] * gain[b, i]
            Db[b, 0:3, i], Db[b, 3:6, i] = f, t - np.cross(d[b], f)
    p = dict(mass=rm.MASS * (1 + rng.uniform(-0.2, 0.2, B)), J=J0[None] * (s[:, :, None] * s[:, None, :]), D=Db,
             force=rng.uniform(-0.05, 0.05, (B, 3)), torque=rng.uniform(-0.005, 0.005, (B, 3)))
    assert np.linalg.cond(p["J"]).max() <= 3.4
    return {k: p[k] for k in fields}


def _nominal(B, NT):
    D = rm.allocation_matrix_16() if NT == 16 else rm.allocation_matrix_8()
    return dict(mass=np.full(B, rm.MASS), J=np.repeat(rm.INERTIA[None], B, 0), D=np.repeat(D[None], B, 0), force=np.zeros((B, 3)),
                torque=np.zeros((B, 3)))


def _step(x, u, ub, stuck, m, J, D, f, t):
    def rhs(y):
        dx = rm.plant_dx_dt(y, u, D, stuck, ub, m, J)
        dx[3:6] += f / m
        dx[10:13] += np.linalg.solve(J, t)
        return dx
    return rm.rk4(rhs, x)


def _replay(x_prev, u, pu, ps, plant, t, noise, seed, index0=0, index_total=None):
    """x_hist[t] [B,13] that the definition gives from x_prev [B,13] under the commands u [B,NT] and the plant's pattern of step t."""
    B, NT = u.shape
    p = dict(_nominal(B, NT), **plant)
    x = np.stack([_step(x_prev[b], u[b], pu[b], ps[b], p["mass"][b], p["J"][b], p["D"][b], p["force"][b], p["torque"][b])
                  for b in range(B)])
    amp = np.repeat(np.asarray(noise, float), [3, 3, 4, 3])
    total = B if index_total is None else index_total
    idx = (np.uint64(t) * np.uint64(total) + np.uint64(index0) + np.arange(B, dtype=np.uint64))[:, None] * np.uint64(13) \
        + np.arange(13, dtype=np.uint64)[None, :]
    x = x + amp[None, :] * cl.u01(seed, idx) * (amp[None, :] > 0)
    x[:, 6:10] /= np.linalg.norm(x[:, 6:10], axis=1, keepdims=True)
    return x


def _check_replay(out, x0, ub, stuck, plant, noise, seed, faults=None, half_must_differ=True):
    xh, uh = out["x_hist"], out["u"]
    T, B = xh.shape[:2]
    pu, ps = (np.repeat(ub[None], T, 0), np.repeat(stuck[None], T, 0)) if faults is None else _plant_patterns(ub, stuck, faults, T)
    worst = 0.0
    for t in range(T):
        ref = _replay(x0 if t == 0 else xh[t - 1], uh[t], pu[t], ps[t], plant, t, noise, seed)
        worst = max(worst, np.abs(xh[t] - ref).max())
        np.testing.assert_allclose(xh[t], ref, rtol=1e-12, atol=1e-12, err_msg=f"step {t}")
    assert np.array_equal(out["x"], xh[-1])
    miss = np.abs(xh[0] - _replay(x0, uh[0], pu[0], ps[0], {}, 0, noise, seed)).max(axis=1)
    print(f"replay: max |x_hist - reference| = {worst:.3e}; nominal replay of step 0 misses by median {np.median(miss):.3e}, "
          f"{(miss > 1e-6).sum()} of {B} vehicles above 1e-6")
    if half_must_differ:
        assert (miss > 1e-6).sum() >= (B + 1) // 2


NOISE = (1e-3,) * 4


def _sim(mpc, x0, ub, stuck, N, T, plant, seed=5, **kw):
    return mpc.simulate(x0, ub, stuck, _hover(N, T), T, noise=NOISE, seed=seed, return_inputs=True, return_states=True, plant=plant, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# 1, 2: the thruster form, all fields and each field alone
# ---------------------------------------------------------------------------------------------------------------------------
def test_all_fields_dispersed_replay_from_the_runs_own_histories(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 96, 12                                    # B = 96: a partial last wave
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 0, 11)
    plant = _plant(B, NT)
    out = _sim(gpu_mpc_factory(N=N, NT=NT, dtype="f32"), x0, ub, stuck, N, T, plant)
    _check_replay(out, x0, ub, stuck, plant, NOISE, 5)


@pytest.mark.parametrize("field", FIELDS)
def test_each_field_alone(gpu_mpc_factory, field):
    N, NT, B, T = 10, 8, 70, 3
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 1, 12)
    plant = _plant(B, NT, seed=4, fields=(field,))
    assert list(plant) == [field]
    out = _sim(gpu_mpc_factory(N=N, NT=NT, dtype="f32"), x0, ub, stuck, N, T, plant)
    _check_replay(out, x0, ub, stuck, plant, NOISE, 5)


# ---------------------------------------------------------------------------------------------------------------------------
# 3: the other loop kinds
# ---------------------------------------------------------------------------------------------------------------------------
def test_wrench_form(gpu_mpc_factory):
    t = load_terminal().term_set
    term = (t, np.asarray(t.A, float).reshape(-1, 9), np.asarray(t.b, float).reshape(-1))
    bt = _wrench_batch(term)
    T = 6
    bt["faults"]["onset"] = np.minimum(bt["faults"]["onset"], 4)
    xr = bt["xr"][:, :T + bt["N"]]
    plant = _plant(bt["B"], 16, seed=8)
    mpc = gpu_mpc_factory(N=15, NT=16, dtype="f64", max_iters=60, terminal_set=term[0])
    noise = (1e-4,) * 4
    out = mpc.simulate(bt["x0"], bt["ub"], bt["stuck"], xr, T, noise=noise, seed=bt["seed"], faults=bt["faults"], formulation="wrench",
                       return_inputs=True, return_states=True, plant=plant)
    assert out["alloc_failed"].shape == (T,)
    _check_replay(out, bt["x0"], bt["ub"], bt["stuck"], plant, noise, bt["seed"], faults=bt["faults"], half_must_differ=False)


def test_thruster_sqp_loop(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 32, 4
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 1, 13)
    plant = _plant(B, NT, seed=9)
    out = _sim(gpu_mpc_factory(N=N, NT=NT, dtype="f32"), x0, ub, stuck, N, T, plant, sqp_iters=2)
    _check_replay(out, x0, ub, stuck, plant, NOISE, 5, half_must_differ=False)


def test_float64_handle(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 70, 3
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 1, 14)
    plant = _plant(B, NT, seed=10)
    out = _sim(gpu_mpc_factory(N=N, NT=NT, dtype="f64"), x0, ub, stuck, N, T, plant)
    _check_replay(out, x0, ub, stuck, plant, NOISE, 5, half_must_differ=False)


# ---------------------------------------------------------------------------------------------------------------------------
# 4: with a fault schedule -- the replay uses the plant's pattern of each step (the last event with onset <= t)
# ---------------------------------------------------------------------------------------------------------------------------
def _run(mpc, bt, plant, lo=0, hi=None, **kw):
    hi = bt["B"] if hi is None else hi
    f = {k: v[lo:hi] for k, v in bt["faults"].items()}
    p = None if plant is None else {k: v[lo:hi] for k, v in plant.items()}
    return mpc.simulate(bt["x0"][lo:hi], bt["ub"][lo:hi], bt["stuck"][lo:hi], bt["xr"], bt["T"], noise=NOISE, seed=bt["seed"],
                        faults=f, detect_delay=bt["delay"][lo:hi], return_inputs=True, return_states=True, plant=p, **kw)


def test_with_a_fault_schedule(gpu_mpc_factory):
    bt = _thruster_batch(96, 10)
    plant = _plant(96, 8, seed=15)
    out = _run(gpu_mpc_factory(N=10, NT=8, dtype="f32"), bt, plant, outcomes=True)
    pu, _ = _plant_patterns(bt["ub"], bt["stuck"], bt["faults"], bt["T"])
    assert (pu != bt["ub"]).any()
    _check_replay(out, bt["x0"], bt["ub"], bt["stuck"], plant, NOISE, bt["seed"], faults=bt["faults"], half_must_differ=False)
    # impulse keeps its meaning of thruster force: the plant's pattern and the commands, no D_b
    cmd = np.where(pu > 0.0, out["u"], 0.0)
    np.testing.assert_allclose(out["outcomes"]["impulse"][:, 1], 0.1 * cmd.sum(axis=(0, 2)), rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------------
# 5, 6: nothing given changes nothing; the nominal values given explicitly change the arithmetic only
# ---------------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    for k in ("x", "u", "x_hist", "not_converged", "status_hist"):
        assert np.array_equal(a[k], b[k]), k
    assert sorted(a["outcomes"]) == sorted(b["outcomes"])
    for k in b["outcomes"]:
        assert np.array_equal(a["outcomes"][k], b["outcomes"][k]), k


def test_nothing_given_changes_nothing(gpu_mpc_factory):
    bt = _thruster_batch(96, 10)
    mpc = gpu_mpc_factory(N=10, NT=8, dtype="f32")
    base = _run(mpc, bt, None, outcomes=True, return_status=True)                 # the _outcomes_ entry
    _same_bits(_run(mpc, bt, {}, outcomes=True, return_status=True), base)        # the _plant_ entry, five NULL arrays
    # the same through ctypes, without a schedule
    B, T, NT = bt["B"], bt["T"], 8
    ref = mpc.simulate(bt["x0"], bt["ub"], bt["stuck"], bt["xr"], T, noise=NOISE, seed=7, return_inputs=True, return_states=True,
                       outcomes=True, return_status=True)
    oc, orec, sh = _outcome_request(mpc, B, T, False, True, True, 0, None)
    pm = _lib.ftmpc_plant_model(struct_size=C.sizeof(_lib.ftmpc_plant_model))
    assert not (pm.mass or pm.J or pm.D or pm.force or pm.torque)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    x, uh, xh, bad = bt["x0"].copy(), np.empty((T, B, NT)), np.empty((T, B, 13)), np.zeros(T, np.int32)
    xr, nz = np.ascontiguousarray(bt["xr"].reshape(-1, order="F")), np.array(NOISE)
    rc = mpc.lib.ftmpc_simulate_plant_batch(mpc._h, B, T, x.ctypes.data_as(dp), bt["ub"].ctypes.data_as(dp), bt["stuck"].ctypes.data_as(dp),
                                            xr.ctypes.data_as(dp), None, nz.ctypes.data_as(dp), C.c_uint64(7), 0, 8, 1e-9, None,
                                            uh.ctypes.data_as(dp), xh.ctypes.data_as(dp), bad.ctypes.data_as(ip), C.byref(oc), C.byref(pm))
    assert rc == 0, mpc.lib.ftmpc_last_error(mpc._h)
    _same_bits(dict(x=x, u=uh, x_hist=xh, not_converged=bad, status_hist=sh, outcomes=orec), ref)


def test_nominal_values_given_explicitly(gpu_mpc_factory):
    N, NT, B = 10, 8, 96
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 1, 16)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    base = _sim(mpc, x0, ub, stuck, N, 1, None)
    out = _sim(mpc, x0, ub, stuck, N, 1, _nominal(B, NT))
    assert np.array_equal(out["u"], base["u"])                     # the solve of step 0 is the same
    print("nominal plant model against no plant model: max |x - x| =", np.abs(out["x"] - base["x"]).max())
    assert np.abs(out["x"] - base["x"]).max() <= 1e-13


# ---------------------------------------------------------------------------------------------------------------------------
# 7: slices of a campaign and device slots
# ---------------------------------------------------------------------------------------------------------------------------
def test_slices_with_the_plant_arrays_sliced_equal_the_whole():
    bt = _thruster_batch(96, 10)
    B = bt["B"]
    plant = _plant(B, 8, seed=17)

    def fresh(lo, hi, **kw):
        mpc = ft_mpc_amd.BatchedMPC(N=10, NT=8, dtype="f32")
        try:
            return _run(mpc, bt, plant, lo, hi, outcomes=True, return_status=True, **kw)
        finally:
            mpc.close()
    whole = fresh(0, B)
    parts = [fresh(0, 40, index0=0, index_total=B), fresh(40, B, index0=40, index_total=B)]
    assert np.array_equal(np.concatenate([p["x"] for p in parts]), whole["x"])
    for k in ("x_hist", "u", "status_hist"):
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), whole[k]), k
    for k in whole["outcomes"]:
        assert np.array_equal(np.concatenate([p["outcomes"][k] for p in parts]), whole["outcomes"][k]), k


def test_three_slots_on_one_device_equal_one_handle(gpu_mpc_factory):
    bt = _thruster_batch(100, 20)
    bt["T"] = 8
    bt["xr"] = _hover(20, 8)
    bt["faults"]["onset"] = np.minimum(bt["faults"]["onset"], 6)
    plant = _plant(100, 8, seed=18)
    kw = dict(outcomes=dict(tol_pos=1.0, tol_vel=0.3, tol_rate=0.1), return_status=True)
    serial = _run(gpu_mpc_factory(N=20, NT=8, dtype="f32"), bt, plant, **kw)
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=20, NT=8, dtype="f32"), devices=[0, 0, 0])
    try:
        multi = _run(m, bt, plant, **kw)
    finally:
        m.close()
    _same_bits(multi, serial)
    nominal = _run(gpu_mpc_factory(N=20, NT=8, dtype="f32"), bt, None, **kw)
    assert not np.array_equal(nominal["x"], serial["x"])


# ---------------------------------------------------------------------------------------------------------------------------
# 8: refusals, on the single handle and on the multi driver: FTMPC_ERR_ARG, the message names the field and the vehicle
# ---------------------------------------------------------------------------------------------------------------------------
def _bad_models(B, NT):
    """(field, offending vehicle, plant dict) for every refusal of include/ftmpc.h."""
    good = _plant(B, NT, seed=19)
    v = B - 2                                                      # on three slots: in the last shard

    def with_(field, idx, value):
        a = good[field].copy()
        a[(v,) + idx] = value
        return field, v, {field: a}
    asym = good["J"].copy()
    asym[v, 0, 1] += 1e-9
    indef = good["J"].copy()
    indef[v] = np.diag([0.2, -0.3, 0.25])
    semi = good["J"].copy()
    semi[v] = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    return [with_("mass", (), np.nan), with_("mass", (), np.inf), with_("mass", (), 0.0), with_("mass", (), -16.8),
            with_("J", (1, 1), np.nan), ("J", v, dict(J=asym)), ("J", v, dict(J=indef)), ("J", v, dict(J=semi)),
            with_("D", (4, NT - 1), np.inf), with_("force", (2,), np.nan), with_("torque", (0,), -np.inf)]


def test_refusals(gpu_mpc_factory):
    N, NT, B, T = 10, 8, 12, 2
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, 0, 20)
    mpc = gpu_mpc_factory(N=N, NT=NT, dtype="f32")
    m = MultiGPUMPC(ft_mpc_amd.MPCConfig(N=N, NT=NT, dtype="f32"), devices=[0, 0, 0])
    try:
        for field, v, plant in _bad_models(B, NT):
            for obj in (mpc, m):
                with pytest.raises(FtmpcError) as e:
                    obj.simulate(x0, ub, stuck, _hover(N, T), T, plant=plant)
                assert e.value.code == -1 and f"ftmpc_plant_model.{field}" in str(e.value) and f"vehicle {v} " in str(e.value), str(e.value)
        # a struct of another size, straight at the C entries
        dp = C.POINTER(C.c_double)
        xr, nz = np.ascontiguousarray(_hover(N, T).reshape(-1, order="F")), np.array(NOISE)
        pm = _lib.ftmpc_plant_model(struct_size=C.sizeof(_lib.ftmpc_plant_model) - 8)
        for lib_f, h, err in ((mpc.lib.ftmpc_simulate_plant_batch, mpc._h, mpc.lib.ftmpc_last_error),
                              (m.lib.ftmpc_multi_simulate_plant_batch, m._h, m.lib.ftmpc_multi_last_error)):
            x = x0.copy()
            rc = lib_f(h, B, T, x.ctypes.data_as(dp), ub.ctypes.data_as(dp), stuck.ctypes.data_as(dp), xr.ctypes.data_as(dp), None,
                       nz.ctypes.data_as(dp), C.c_uint64(1), 0, 8, 1e-9, None, None, None, None, None, C.byref(pm))
            assert rc == -1 and b"ftmpc_plant_model.struct_size" in err(h)
            assert np.array_equal(x, x0)
        # shapes are the front end's business
        with pytest.raises(ValueError):
            mpc.simulate(x0, ub, stuck, _hover(N, T), T, plant=dict(mass=np.ones(B + 1)))
        with pytest.raises(ValueError):
            mpc.simulate(x0, ub, stuck, _hover(N, T), T, plant=dict(inertia=np.ones((B, 3, 3))))
        # and a good model is accepted by both
        good = _plant(B, NT, seed=19)
        a = mpc.simulate(x0, ub, stuck, _hover(N, T), T, plant=good)
        b = m.simulate(x0, ub, stuck, _hover(N, T), T, plant=good)
        assert np.array_equal(a["x"], b["x"])
    finally:
        m.close()
