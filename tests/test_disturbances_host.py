"""CPU: the host side of the disturbance estimate (include/ftmpc.h, ftmpc_disturbance; ft_mpc_amd/disturbances.py): the three entries
are exported, the ctypes struct has the layout gcc gives the header (88 bytes) and no earlier struct changed size, the Jacobian is the
derivative of model_step under the retraction, the sequential update is the batch Kalman update, the split P_xx / P_xd / P_dd
propagation is the dense 18 x 18 product, pack / unpack are inverse, with a zero disturbance covariance the augmented filter is the
estimator's, the filter finds a constant force and torque from noiseless measurements, diagnosis.replay takes the estimate, and the
refusals Python raises before any call reaches the library."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NEW = ("ftmpc_simulate_disturbance_batch", "ftmpc_multi_simulate_disturbance_batch", "ftmpc_debug_records_disturbance")
FIELDS = ["struct_size", "compensate", "p0", "proc_sigma", "force", "torque", "cross", "cov", "force_hist", "torque_hist"]
OFFSETS = [0, 4, 8, 24, 40, 48, 56, 64, 72, 80]
SIGMA = (1e-2, 5e-3, 1e-2, 5e-3)
F_MAX = 3.4
# what tests/test_gpu_disturbances.py (G) runs the closed loop with: chosen in test_filter_converges_on_synthetic_data below
FORCE = (0.90, -0.60, 0.75)           # N, inertial frame
TORQUE = (0.060, -0.045, 0.030)       # N m, body frame
EST_G = dict(every=1, p0=(1e-3,) * 4, proc_sigma=(1e-5,) * 4, meas_sigma=(1e-3,) * 4)
DIST_G = dict(p0=(1.0, 0.1), proc_sigma=(1e-3, 1e-4))
T_CONV = 59


def _cfg(NT=8, **kw):
    from ft_mpc_amd.batch import MPCConfig
    return MPCConfig(NT=NT, **kw)


def _state(rng, wmax=1.0):
    q = rng.normal(size=4)
    w = rng.normal(size=3)
    w *= wmax * rng.uniform() / np.linalg.norm(w)
    return np.concatenate([rng.normal(size=3), rng.normal(size=3), q / np.linalg.norm(q), w])


def _spd(rng, n, scale):
    A = rng.normal(size=(n, n))
    s = np.asarray(scale, float)
    return (A @ A.T / n + np.eye(n)) * np.outer(s, s)


def test_library_exports_the_disturbance_entries():
    from ft_mpc_amd import _lib
    _lib.build_library()
    lib = _lib.load_library()
    header = (ROOT / "include" / "ftmpc.h").read_text()
    for n in NEW:
        assert n in _lib.SYMBOLS and getattr(lib, n) is not None
        assert f"int {n}(" in header
    assert lib.ftmpc_simulate_disturbance_batch.argtypes[:-1] == lib.ftmpc_simulate_diagnosis_batch.argtypes
    assert lib.ftmpc_multi_simulate_disturbance_batch.argtypes[:-1] == lib.ftmpc_multi_simulate_diagnosis_batch.argtypes
    assert lib.ftmpc_debug_records_disturbance.argtypes[:-2] == lib.ftmpc_debug_records.argtypes[:-1]


def test_disturbance_struct_layout_matches_the_header(tmp_path):
    from ft_mpc_amd import _lib
    assert [f for f, _ in _lib.ftmpc_disturbance._fields_] == FIELDS
    src = tmp_path / "layout.c"
    body = "".join(f'printf("{f} %zu\\n", offsetof(ftmpc_disturbance, {f}));' for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftmpc.h"\nint main(void){printf("sizeof %zu\\n", sizeof(ftmpc_disturbance));'
                   + body + 'printf("estimator %zu\\ndiagnosis %zu\\nsensor %zu\\nplant %zu\\n", sizeof(ftmpc_estimator), '
                   'sizeof(ftmpc_diagnosis), sizeof(ftmpc_sensor), sizeof(ftmpc_plant_model));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.ftmpc_disturbance) == 88
    for f, off in zip(FIELDS, OFFSETS):
        assert int(got[f]) == getattr(_lib.ftmpc_disturbance, f).offset == off, f
    # no existing struct changed
    assert int(got["estimator"]) == C.sizeof(_lib.ftmpc_estimator) == 136
    assert int(got["diagnosis"]) == C.sizeof(_lib.ftmpc_diagnosis)
    assert int(got["sensor"]) == C.sizeof(_lib.ftmpc_sensor) == 96
    assert int(got["plant"]) == C.sizeof(_lib.ftmpc_plant_model) == 48


def test_model_step_is_the_plant_step_with_the_nominal_model():
    """model_step under gen = D a is dispersion.plant_step with plant = dict(force, torque) (the plant's own equation with the
    config's m, J, D), renormalised; with a zero estimate it is sensors.predict."""
    from ft_mpc_amd import disturbances as ds
    from ft_mpc_amd.dispersion import plant_step
    from ft_mpc_amd.estimators import generalized_force
    from ft_mpc_amd.sensors import predict
    cfg = _cfg()
    rng = np.random.default_rng(2)
    ub, stuck = np.full(8, F_MAX), np.zeros(8)
    ub[3], stuck[3] = 0.0, 1.7
    for _ in range(5):
        x, u = _state(rng), F_MAX * rng.uniform(size=8)
        f, t = rng.normal(size=3), 0.1 * rng.normal(size=3)
        ref = plant_step(x, u, ub, stuck, dict(force=f, torque=t), cfg)
        ref[6:10] /= np.linalg.norm(ref[6:10])
        gen = generalized_force(u, ub, stuck, cfg)
        assert np.abs(ds.model_step(x, gen, f, t, cfg) - ref).max() <= 1e-14
        assert np.abs(ds.model_step(x, gen, np.zeros(3), np.zeros(3), cfg) - predict(x, u[None], ub, stuck, cfg)).max() <= 1e-14


def test_centre_step_follows_the_vehicle():
    """The orbit-centre model with the estimate is the vehicle's model seen from the centre: to_centre(vehicle RK4 step without
    renormalisation) and centre_step(to_centre(x)) are two RK4 discretisations of one flow, so they agree to the local error of RK4
    at dt = 1e-2, (|w| dt)^5 ~ 1e-10; a disturbance force or torque left out of either side would leave dt^2 f / (2 m) ~ 3e-6."""
    from ft_mpc_amd import disturbances as ds
    from ft_mpc_amd.dispersion import plant_step
    from ft_mpc_amd.estimators import generalized_force
    cfg = _cfg(dt=1e-2)
    rng = np.random.default_rng(4)
    ub, stuck = np.full(8, F_MAX), np.zeros(8)
    for _ in range(5):
        x, u = _state(rng), F_MAX * rng.uniform(size=8)
        f, t = rng.normal(size=3), 0.1 * rng.normal(size=3)
        nxt = plant_step(x, u, ub, stuck, dict(force=f, torque=t), cfg)
        c = ds.centre_step(ds.to_centre(x, cfg), generalized_force(u, ub, stuck, cfg), f, t, cfg)
        assert np.abs(c - ds.to_centre(nxt, cfg)).max() <= 1e-8
        c0 = ds.centre_step(ds.to_centre(x, cfg), generalized_force(u, ub, stuck, cfg), 0 * f, 0 * t, cfg)
        assert np.abs(c0 - ds.to_centre(nxt, cfg)).max() >= 1e-7


def test_jacobian_against_central_differences_of_model_step():
    """Phi_h = d (F_h(z [+] d) [-] F_h(z)) / dd at d = 0 for the augmented map F_h(x, f, t) = (model_step over h, f, t), by central
    differences of step 1e-6.  (Phi_h - I) / h = A + h A^2 / 2 + O(h^2), so 2 L(h / 2) - L(h) = A + O(h^2 |A|^3 / 6): with h = 1e-3
    and |A| <= 5 (the block J^-1) that is 2e-5, the differences' own rounding 1e-16 / 1e-6 / h = 1e-7.  Bound: 1e-4 of
    max(1, the block's scale); a wrong sign or a missing block is of order one.  The disturbance rows of A are zero."""
    from ft_mpc_amd import disturbances as ds
    from ft_mpc_amd.estimators import generalized_force, residual
    rng = np.random.default_rng(3)
    ub, stuck = np.full(8, F_MAX), np.zeros(8)

    def phi(h, x, f, t, gen):
        cfg = _cfg(dt=h)
        base = ds.model_step(x, gen, f, t, cfg)
        out = np.zeros((18, 18))
        for i in range(18):
            col = []
            for s in (1e-6, -1e-6):
                e = np.zeros(18)
                e[i] = s
                xe, fe, te = ds.retract18(x, f, t, e)
                col.append(np.concatenate([residual(ds.model_step(xe, gen, fe, te, cfg), base), fe - f, te - t]))
            out[:, i] = (col[0] - col[1]) / 2e-6
        return out

    worst = 0.0
    for _ in range(4):
        x = _state(rng, 1.0)
        f, t = rng.normal(size=3), 0.1 * rng.normal(size=3)
        gen = generalized_force(F_MAX * (rng.uniform(size=8) > 0.5), ub, stuck, _cfg())
        A = ds.jacobian(x, gen, _cfg())
        h = 1e-3
        An = 2 * (phi(h / 2, x, f, t, gen) - np.eye(18)) / (h / 2) - (phi(h, x, f, t, gen) - np.eye(18)) / h
        for a in range(6):
            for b in range(6):
                blk = np.s_[3 * a:3 * a + 3, 3 * b:3 * b + 3]
                worst = max(worst, np.abs(An[blk] - A[blk]).max() / max(1.0, np.abs(A[blk]).max()))
        assert not A[12:18].any()
        assert np.array_equal(A[3:6, 12:15], np.eye(3) / _cfg().mass) and np.allclose(A[9:12, 15:18] @ _cfg().J, np.eye(3), atol=1e-15)
    print(f"jacobian against differences: worst block deviation {worst:.2e} of its scale")
    assert worst <= 1e-4


def test_sequential_update_is_the_batch_update():
    """Twelve scalar updates over all 18 coordinates against P - P H' (H P H' + R)^-1 H P and delta = P H' (H P H' + R)^-1 r with
    H = [I 0]: the same posterior for a diagonal R, within round-off of the conditioning (1e-10 of the entries' scale)."""
    from ft_mpc_amd import disturbances as ds
    from ft_mpc_amd.estimators import residual, retract
    rng = np.random.default_rng(7)
    G = np.repeat(np.arange(4), 3)
    scale = np.r_[np.asarray(SIGMA)[G], [0.5] * 3, [0.05] * 3]
    for _ in range(5):
        x = _state(rng)
        f, t = rng.normal(size=3), 0.1 * rng.normal(size=3)
        P = _spd(rng, 18, scale)
        y = retract(x, rng.normal(size=12) * np.asarray(SIGMA)[G])
        xn, fn, tn, Pn = ds.update(x, f, t, P, y, SIGMA)
        H = np.eye(12, 18)
        S = H @ P @ H.T + np.diag(np.asarray(SIGMA)[G] ** 2)
        K = P @ H.T @ np.linalg.inv(S)
        d = K @ residual(y, x)
        Pb = P - K @ H @ P
        assert (np.abs(Pn - Pb) / np.outer(scale, scale)).max() <= 1e-10
        assert np.abs(xn - retract(x, d[:12])).max() <= 1e-12
        assert np.abs(fn - f - d[12:15]).max() <= 1e-10 and np.abs(tn - t - d[15:18]).max() <= 1e-11
        assert np.abs(Pn - Pn.T).max() <= 1e-18 and np.linalg.eigvalsh(Pn / np.outer(scale, scale)).min() > 0


def test_split_propagation_is_the_dense_product():
    """propagate (the three pieces, as the device forms them) against Phi P Phi' + Q with the dense 18 x 18 Phi = I + dt A."""
    from ft_mpc_amd import disturbances as ds
    from ft_mpc_amd.estimators import generalized_force
    cfg = _cfg()
    rng = np.random.default_rng(9)
    G = np.repeat(np.arange(4), 3)
    scale = np.r_[np.asarray(SIGMA)[G], [0.5] * 3, [0.05] * 3]
    ub, stuck = np.full(8, F_MAX), np.zeros(8)
    qx, qd = tuple(0.1 * s for s in SIGMA), (1e-2, 1e-3)
    for _ in range(5):
        x, u = _state(rng), F_MAX * rng.uniform(size=8)
        f, t = rng.normal(size=3), 0.1 * rng.normal(size=3)
        P = _spd(rng, 18, scale)
        xn, Pn = ds.propagate(x, f, t, P, u, ub, stuck, qx, qd, cfg)
        gen = generalized_force(u, ub, stuck, cfg)
        Phi = np.eye(18) + cfg.dt * ds.jacobian(x, gen, cfg)
        Q = np.diag(np.r_[np.asarray(qx)[G] ** 2, [qd[0] ** 2] * 3, [qd[1] ** 2] * 3])
        assert (np.abs(Pn - (Phi @ P @ Phi.T + Q)) / np.outer(scale, scale)).max() <= 1e-13
        assert np.array_equal(Pn, Pn.T) or np.abs(Pn - Pn.T).max() <= 1e-18
        assert np.array_equal(xn, ds.model_step(x, gen, f, t, cfg))
        # a wrong block of Phi_xd is orders above the bound: it moves P_xd by dt / m p0_d^2
        wrong = Phi.copy()
        wrong[3:6, 12:15] = 0.0
        assert (np.abs(Pn - (wrong @ P @ wrong.T + Q)) / np.outer(scale, scale)).max() > 1e-3


def test_pack_and_unpack_are_inverse():
    from ft_mpc_amd import disturbances as ds
    rng = np.random.default_rng(5)
    P = np.stack([_spd(rng, 18, np.ones(18)) for _ in range(3)])
    c78, c72, c21 = ds.pack(P)
    assert c78.shape == (3, 78) and c72.shape == (3, 72) and c21.shape == (3, 21)
    assert np.array_equal(ds.unpack(c78, c72, c21), P)
    assert np.array_equal(c72[1].reshape(12, 6), P[1, 0:12, 12:18]) and c21[2, 6] == P[2, 13, 13]


def test_zero_disturbance_covariance_is_the_estimators_filter():
    """p0 = proc_sigma = 0 for the disturbance and no handed estimate: P_xd and P_dd stay zero, (f^, t^) stay zero, and est / xhat / cov
    are estimators.replay's within round-off."""
    from ft_mpc_amd import disturbances as ds
    from ft_mpc_amd import estimators as es
    cfg = _cfg()
    rng = np.random.default_rng(12)
    T = 10
    ub, stuck = np.full(8, F_MAX), np.zeros(8)
    G = np.repeat(np.arange(4), 3)
    x = _state(rng, 0.3)
    meas, us = [], []
    for _ in range(T):
        meas.append(es.retract(x, rng.normal(size=12) * np.asarray(SIGMA)[G]))
        us.append(F_MAX * rng.uniform(size=8))
        x = es.predict(x, us[-1][None], ub, stuck, cfg)
    spec = dict(every=2, p0=SIGMA, proc_sigma=tuple(0.1 * s for s in SIGMA), meas_sigma=SIGMA)
    a = es.replay(meas, us, ub, stuck, spec, cfg, latency=2, tail=np.ones((2, 8)))
    b = ds.replay(meas, us, ub, stuck, spec, dict(p0=(0, 0), proc_sigma=(0, 0)), cfg, latency=2, tail=np.ones((2, 8)))
    assert not b["force"].any() and not b["torque"].any() and not b["cross"].any() and not b["cov_d"].any()
    for k in ("est", "pred", "xhat"):
        assert np.abs(a[k] - b[k]).max() <= 1e-13, k
    assert (np.abs(a["cov"] - b["cov"]) / es.pack(np.outer(np.asarray(SIGMA)[G], np.asarray(SIGMA)[G]))).max() <= 1e-12


def test_filter_converges_on_synthetic_data():
    """No QP here: model_step integrated with the fixed FORCE / TORQUE under random commands (up to 0.3 f_max per thruster), noiseless
    measurements fed to replay.  Chosen for tests/test_gpu_disturbances.py (G): FORCE = (0.9, -0.6, 0.75) N (|f| = 1.32 N), TORQUE =
    (0.06, -0.045, 0.03) N m; estimator p0 = 1e-3, proc_sigma = 1e-5, meas_sigma = 1e-3 in every group; disturbance p0 = (1 N,
    0.1 N m), proc_sigma = (1e-3, 1e-4) per step; T_conv = 59 (why: the docstring of that test).  Reached: |f^ - f| / |f| = 2.4e-3
    at step 5, 4.0e-4 at step 15, 1.7e-5 at step 58; |t^ - t| / |t| = 8.7e-4, 2.5e-4, 5.0e-6 (the bound is 2 % at T_conv)."""
    from ft_mpc_amd import disturbances as ds
    from ft_mpc_amd.estimators import generalized_force
    cfg = _cfg()
    rng = np.random.default_rng(5)
    ub, stuck = np.full(8, F_MAX), np.zeros(8)
    F, Tq = np.asarray(FORCE), np.asarray(TORQUE)
    q = rng.normal(size=4)
    x = np.concatenate([rng.normal(size=3), 0.1 * rng.normal(size=3), q / np.linalg.norm(q), 0.2 * rng.normal(size=3)])
    meas, us = [], []
    for _ in range(T_CONV):
        meas.append(x.copy())
        us.append(0.3 * F_MAX * rng.uniform(size=8))
        x = ds.model_step(x, generalized_force(us[-1], ub, stuck, cfg), F, Tq, cfg)
    r = ds.replay(np.array(meas), np.array(us), ub, stuck, EST_G, DIST_G, cfg)
    ef = np.linalg.norm(r["force"] - F, axis=1) / np.linalg.norm(F)
    et = np.linalg.norm(r["torque"] - Tq, axis=1) / np.linalg.norm(Tq)
    print("force error at steps 5, 15, T_conv - 1:", ef[[5, 15, -1]], "torque error:", et[[5, 15, -1]])
    assert ef[-1] <= 0.02 and et[-1] <= 0.02
    assert np.array_equal(r["force_end"], r["force"][-1]) and np.array_equal(r["torque_end"], r["torque"][-1])
    # the estimator alone, told nothing, keeps a bias in its prediction: the augmented filter's one-step prediction error is smaller
    from ft_mpc_amd import estimators as es
    plain = es.replay(np.array(meas), np.array(us), ub, stuck, EST_G, cfg)
    assert np.abs(r["est"][-5:, 3:6] - np.array(meas)[-5:, 3:6]).max() < np.abs(plain["est"][-5:, 3:6] - np.array(meas)[-5:, 3:6]).max()


def test_diagnosis_replay_takes_the_estimate():
    """force / torque None is the present behaviour bit for bit; with the plant's own disturbance as the estimate a noiseless open loop
    has a zero residual, so every statistic stays exactly 0, while without it the drift shows."""
    from ft_mpc_amd import diagnosis as dg
    from ft_mpc_amd import disturbances as ds
    from ft_mpc_amd.estimators import generalized_force
    cfg = _cfg()
    rng = np.random.default_rng(8)
    T = 12
    ub, stuck = np.full(8, F_MAX), np.zeros(8)
    F, Tq = np.asarray(FORCE), np.asarray(TORQUE)
    x = _state(rng, 0.3)
    meas, us = [], []
    for _ in range(T):
        meas.append(x.copy())
        us.append(F_MAX * rng.uniform(size=8))
        x = ds.model_step(x, generalized_force(us[-1], ub, stuck, cfg), F, Tq, cfg)
    spec = dict(every=1, levels=(0.0, F_MAX), resid_sigma=(1e-3, 1e-3), threshold=1e9, max_detect=2)
    base = dg.replay(meas, us, ub, stuck, spec, cfg)
    same = dg.replay(meas, us, ub, stuck, spec, cfg, force=None, torque=None)
    assert np.array_equal(base["llr_hist"], same["llr_hist"]) and np.array_equal(base["state"], same["state"])
    told = dg.replay(meas, us, ub, stuck, spec, cfg, force=np.tile(F, (T, 1)), torque=np.tile(Tq, (T, 1)))
    assert not told["llr_hist"].any() and base["llr_hist"].max() > 1.0


def test_request_refusals():
    from ft_mpc_amd.disturbances import request
    B, T = 4, 3
    est = dict(every=1, p0=SIGMA, proc_sigma=SIGMA, meas_sigma=SIGMA)
    estx = dict(est, xhat=np.zeros((B, 13)))
    ok = dict(p0=(1.0, 0.1), proc_sigma=(1e-3, 1e-4))
    r = request(ok, B, T, est)
    assert r["compensate"] is True and r["force"] is None and r["fields"] == ("force_hist", "torque_hist", "state")
    f3, c72, c21 = np.zeros((B, 3)), np.zeros((B, 72)), np.zeros((B, 21))
    full = request(dict(ok, compensate=0, force=f3, torque=f3, cross=c72.reshape(B, 12, 6), cov=np.zeros((B, 6, 6))), B, T, estx)
    assert full["compensate"] is False and full["cross"].shape == (B, 72) and full["cov"].shape == (B, 21)
    assert full["force"] is not f3                                      # a copy: the call writes into it
    nan3, inf72, neg21 = f3.copy(), c72.copy(), c21.copy()
    nan3[2, 1], inf72[1, 40], neg21[3, 11] = np.nan, np.inf, -1e-12
    bad = [
        (dict(ok, gain=1), est, {}), (ok, None, {}), (ok, est, dict(sqp_iters=2)), (ok, est, dict(formulation="wrench")),
        (dict(ok, compensate=2), est, {}), (dict(ok, compensate=-1), est, {}),
        (dict(proc_sigma=(0, 0)), est, {}), (dict(p0=(1, 1)), est, {}),
        (dict(ok, p0=(1.0, -1e-9)), est, {}), (dict(ok, p0=(np.nan, 1.0)), est, {}), (dict(ok, p0=(1.0, 1.0, 1.0)), est, {}),
        (dict(ok, proc_sigma=(-1.0, 0)), est, {}), (dict(ok, proc_sigma=(0, np.inf)), est, {}),
        (dict(ok, fields=("force",)), est, {}),
        (dict(ok, torque=f3, cross=c72), estx, {}), (dict(ok, force=f3, cross=c72), estx, {}),
        (dict(ok, force=f3, torque=f3, cross=c72), est, {}),
        (dict(ok, force=f3, torque=f3, cov=c21), estx, {}),
        (dict(ok, force=nan3), est, {}), (dict(ok, torque=nan3), est, {}), (dict(ok, force=np.zeros((B, 4))), est, {}),
        (dict(ok, force=f3, torque=f3, cross=inf72), estx, {}), (dict(ok, force=f3, torque=f3, cross=c72, cov=neg21), estx, {}),
        (dict(ok, force=f3, torque=f3, cross=c72, cov=np.full((B, 21), np.nan)), estx, {}),
    ]
    for spec, e, kw in bad:
        with pytest.raises(ValueError):
            request(spec, B, T, e, **kw)
