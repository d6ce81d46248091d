"""CPU: the host side of the disturbance estimate on the two-stage wrench form (include/ftmpc.h, ftmpc_simulate_wrench_disturbance_batch
and the three *_wrench_disturbance_batch entries of the cost, the QP step and the SQP; ft_mpc_amd/disturbances.py, request with the
opt-in key `wrench` and rollout_centre): the five entries are exported with the argument lists of their plain entries plus the
estimate, no struct changed size, every new acceptance and refusal of `request`, the old refusals word for word without the key, and
rollout_centre against centre_step stage by stage and against central differences of model_step-consistent dynamics."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from test_disturbances_host import FORCE, SIGMA, TORQUE, _cfg, _state

ROOT = Path(__file__).resolve().parents[1]
NEW = ("ftmpc_simulate_wrench_disturbance_batch", "ftmpc_multi_simulate_wrench_disturbance_batch",
       "ftmpc_eval_cost_wrench_disturbance_batch", "ftmpc_solve_wrench_disturbance_batch", "ftmpc_solve_sqp_wrench_disturbance_batch")


def test_library_exports_the_wrench_disturbance_entries():
    from ft_mpc_amd import _lib
    _lib.build_library()
    lib = _lib.load_library()
    header = (ROOT / "include" / "ftmpc.h").read_text()
    for n in NEW:
        assert n in _lib.SYMBOLS and getattr(lib, n) is not None
        assert f"int {n}(" in header
    dp = C.POINTER(C.c_double)
    dbp = C.POINTER(_lib.ftmpc_disturbance)
    assert lib.ftmpc_simulate_wrench_disturbance_batch.argtypes == lib.ftmpc_simulate_wrench_diagnosis_batch.argtypes + [dbp]
    assert lib.ftmpc_multi_simulate_wrench_disturbance_batch.argtypes == lib.ftmpc_multi_simulate_wrench_diagnosis_batch.argtypes + [dbp]
    # dist [B*6] follows G (the cost) and warmG (the QP step, the SQP)
    for name, at in (("eval_cost_wrench", 10), ("solve_wrench", 15), ("solve_sqp_wrench", 15)):
        plain, new = getattr(lib, f"ftmpc_{name}_batch").argtypes, getattr(lib, f"ftmpc_{name}_disturbance_batch").argtypes
        assert new == plain[:at] + [dp] + plain[at:], name
    assert C.sizeof(_lib.ftmpc_disturbance) == 88 and C.sizeof(_lib.ftmpc_estimator) == 136


def test_request_accepts_the_wrench_form_only_with_the_key():
    from ft_mpc_amd.disturbances import request
    B, T = 4, 3
    est = dict(every=1, p0=SIGMA, proc_sigma=SIGMA, meas_sigma=SIGMA)
    ok = dict(p0=(1.0, 0.1), proc_sigma=(1e-3, 1e-4))
    # new acceptances
    for k in (0, 2, 10):
        r = request(dict(ok, wrench=True), B, T, est, sqp_iters=k, formulation="wrench")
        assert r["wrench"] is True and r["compensate"] is True
    assert request(dict(ok, wrench=1, compensate=0), B, T, est, formulation="wrench")["compensate"] is False
    # without the key (or with wrench=False) the call is the thruster form's, and says so in the result
    assert request(ok, B, T, est)["wrench"] is False and request(dict(ok, wrench=False), B, T, est)["wrench"] is False
    # new refusals: the key on the thruster formulation, a value that is no flag, a negative count
    for spec, kw in ((dict(ok, wrench=True), {}), (dict(ok, wrench=True), dict(formulation="thruster")),
                     (dict(ok, wrench=True), dict(formulation="thruster", sqp_iters=2)),
                     (dict(ok, wrench=2), dict(formulation="wrench")), (dict(ok, wrench="yes"), dict(formulation="wrench")),
                     (dict(ok, wrench=True), dict(formulation="wrench", sqp_iters=-1))):
        with pytest.raises(ValueError):
            request(spec, B, T, est, **kw)
    with pytest.raises(ValueError, match="formulation must be 'wrench'"):
        request(dict(ok, wrench=True), B, T, est)
    # every other refusal holds with the key as without it
    f3, c72 = np.zeros((B, 3)), np.zeros((B, 72))
    for spec, e in ((dict(ok, wrench=True), None), (dict(ok, wrench=True, compensate=2), est), (dict(ok, wrench=True, p0=(1.0, -1.0)), est),
                    (dict(ok, wrench=True, gain=1), est), (dict(ok, wrench=True, force=f3, torque=f3, cross=c72), est),
                    (dict(ok, wrench=True, force=np.full((B, 3), np.nan)), est), (dict(ok, wrench=True, fields=("force",)), est)):
        with pytest.raises(ValueError):
            request(spec, B, T, e, formulation="wrench", sqp_iters=2)


def test_the_opt_in_leaves_the_old_refusals_in_place():
    """Without the key: the wrench formulation and sqp_iters > 0 raise ValueError with the messages they had."""
    from ft_mpc_amd.disturbances import request
    B, T = 4, 3
    est = dict(every=1, p0=SIGMA, proc_sigma=SIGMA, meas_sigma=SIGMA)
    ok = dict(p0=(1.0, 0.1), proc_sigma=(1e-3, 1e-4))
    for spec in (ok, dict(ok, wrench=False)):
        with pytest.raises(ValueError) as e:
            request(spec, B, T, est, formulation="wrench")
        assert str(e.value) == "disturbance: thruster formulation only (the two-stage wrench form has no disturbance entry)"
        with pytest.raises(ValueError) as e:
            request(spec, B, T, est, sqp_iters=2)
        assert str(e.value) == "disturbance: sqp_iters must be 0 (the cost kernels of the SQP do not know the estimate)"
        with pytest.raises(ValueError) as e:
            request(spec, B, T, est, sqp_iters=2, formulation="wrench")
        assert "thruster formulation only" in str(e.value)


def test_rollout_centre_is_centre_step_stage_by_stage():
    from ft_mpc_amd import disturbances as ds
    cfg = _cfg(NT=16, N=15)
    rng = np.random.default_rng(41)
    r = np.array([0.0, 0.5787037037037037, 0.0])
    x = _state(rng, 0.5)
    c0 = ds.to_centre(x, cfg, r)
    G = rng.normal(size=(cfg.N, 6)) * np.r_[2.0, 2.0, 2.0, 0.2, 0.2, 0.2]
    f, t = np.asarray(FORCE), np.asarray(TORQUE)
    X = ds.rollout_centre(c0, G, f, t, cfg, r)
    assert X.shape == (cfg.N + 1, 13) and np.array_equal(X[0], c0)
    c = c0
    for k in range(cfg.N):
        c = ds.centre_step(c, G[k], f, t, cfg, r)
        assert np.array_equal(X[k + 1], c), k
    # the estimate moves the rollout, and a zero estimate is the nominal rollout
    X0 = ds.rollout_centre(c0, G, 0 * f, 0 * t, cfg, r)
    assert np.abs(X - X0)[-1, 0:3].max() > 1e-3
    c = c0
    for k in range(cfg.N):
        c = ds.centre_step(c, G[k], np.zeros(3), np.zeros(3), cfg, r)
    assert np.array_equal(X0[-1], c)


def test_rollout_centre_is_the_vehicle_models_rollout_seen_from_the_centre():
    """The centre of the vehicle that model_step moves (without its renormalisation: a unit quaternion stays one to 1e-9 over a step
    of dt = 0.1 at these rates) follows rollout_centre: c_k = to_centre(x_k) within the RK4 truncation, which both rollouts share
    only in order -- the bound 1e-6 is dt^5 |w|^5 = 3e-7 with head room, against a movement by the estimate of 1e-3 and more.  And the
    sensitivity of c_N to the torque estimate by central differences is dt^2-sized and non-zero in the rate rows."""
    from ft_mpc_amd import disturbances as ds
    from ft_mpc_amd.estimators import _cfg_model
    cfg = _cfg(NT=16, N=5)
    rng = np.random.default_rng(43)
    r = np.array([0.0, 0.5787037037037037, 0.0])
    x = _state(rng, 0.3)
    G = rng.normal(size=(cfg.N, 6)) * np.r_[1.0, 1.0, 1.0, 0.05, 0.05, 0.05]
    f, t = np.asarray(FORCE), np.asarray(TORQUE)
    X = ds.rollout_centre(ds.to_centre(x, cfg, r), G, f, t, cfg, r)
    worst = 0.0
    for k in range(cfg.N):
        x = ds.model_step(x, G[k], f, t, cfg)
        worst = max(worst, np.abs(ds.to_centre(x, cfg, r) - X[k + 1]).max())
    assert worst <= 1e-6, worst
    # d c_N / d t^ by central differences: rate rows ~ N dt J^-1
    _, m, J = _cfg_model(cfg)
    h = 1e-6
    c0 = X[0]
    S = np.zeros((13, 3))
    for i in range(3):
        d = np.zeros(3)
        d[i] = h
        S[:, i] = (ds.rollout_centre(c0, G, f, t + d, cfg, r)[-1] - ds.rollout_centre(c0, G, f, t - d, cfg, r)[-1]) / (2 * h)
    lead = cfg.N * float(cfg.dt) * np.linalg.inv(J)
    assert np.abs(S[6:9] - lead).max() <= 0.2 * np.abs(lead).max()
    # d c_N / d f^: the velocity rows are exactly N dt / m I (the force is inertial and enters v' additively)
    Sf = np.zeros((13, 3))
    for i in range(3):
        d = np.zeros(3)
        d[i] = h
        Sf[:, i] = (ds.rollout_centre(c0, G, f + d, t, cfg, r)[-1] - ds.rollout_centre(c0, G, f - d, t, cfg, r)[-1]) / (2 * h)
    assert np.abs(Sf[3:6] - cfg.N * float(cfg.dt) / m * np.eye(3)).max() <= 1e-8
    assert np.abs(Sf[6:13]).max() <= 1e-8
