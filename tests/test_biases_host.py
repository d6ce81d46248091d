"""CPU: the NumPy restatement of the bias filter (ft_mpc_amd/biases.py; include/ftmpc.h, ftmpc_bias_estimate) against itself.

The device form (measured coordinates m = (dp, dv + db_v, dtheta, dw + db_w), H = [I 0]) against the textbook form (H = [I, HB],
Phi = diag(Phi_xx, I)) over a synthetic run, the split propagation against the dense product, E against (I - Phi_xx) HB, the
sequential update against the batch form, the convergence, the refusals Python raises before any call reaches the library, and the
one refusal of the library that needs no device.

The synthetic run (RUN): 120 open-loop steps of the controller's model (sensors.predict) under random commands, N = 5, NT = 8, the
measurements with the Gaussian noise of MEAS and the constant bias BIAS on velocity and rate.
Measured here: device form against textbook form over 60 steps, means within 1.5e-16 (bound 1e-12), covariances within 2.0e-14
relative after applying T (bound 1e-10); |b^ - b| / |b| at step 120: 5.5 % (velocity), 12.8 % (rate) (bound 15 %); rms errors over
steps 20..120 against the plain filter's: velocity 4.1e-3 against 2.4e-2 m/s (0.172), rate 2.7e-3 against 2.0e-2 rad/s (0.137) (bound
1/4)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from ft_mpc_amd import biases as BS
from ft_mpc_amd import estimators as ES
from ft_mpc_amd import sensors as SN

ROOT = Path(__file__).resolve().parents[1]
F_MAX = 3.4
MEAS = (0.01, 0.01, 0.005, 0.005)
EST = dict(every=1, p0=(0.05, 0.05, 0.02, 0.02), proc_sigma=(1e-4, 1e-3, 1e-4, 1e-3), meas_sigma=MEAS)
BSPEC = dict(p0=(0.05, 0.02), proc_sigma=(1e-4, 1e-3))       # the estimator's p0[0], p0[1] and proc_sigma[0], proc_sigma[1]
BIAS = np.array((0.03, -0.02, 0.025, 0.02, 0.015, -0.01))
NEW = ("ftmpc_simulate_bias_batch", "ftmpc_simulate_wrench_bias_batch", "ftmpc_multi_simulate_bias_batch")
FIELDS = ["struct_size", "reserved", "p0", "proc_sigma", "bias", "cross", "cov", "bias_hist"]
OFFSETS = [0, 4, 8, 24, 40, 48, 56, 64]
_G = np.repeat(np.arange(4), 3)


def _cfg(NT=8, **kw):
    from ft_mpc_amd.batch import MPCConfig
    return MPCConfig(N=5, NT=NT, **kw)


def _spd(rng, n, scale):
    A = rng.normal(size=(n, n))
    s = np.asarray(scale, float)
    return (A @ A.T / n + np.eye(n)) * np.outer(s, s)


def _run(T=120, seed=7):
    """truth [T,13], meas [T,13], u [T,8]"""
    cfg = _cfg()
    rng = np.random.default_rng(seed)
    ub, stuck = np.full(8, F_MAX), np.zeros(8)
    q = rng.normal(size=4)
    x = np.concatenate([rng.normal(size=3), 0.1 * rng.normal(size=3), q / np.linalg.norm(q), 0.2 * rng.normal(size=3)])
    truth, meas, us = [], [], []
    sig = np.asarray(MEAS)[_G]
    for _ in range(T):
        truth.append(x.copy())
        meas.append(BS.with_bias(ES.retract(x, rng.normal(size=12) * sig), BIAS))
        us.append(0.3 * F_MAX * rng.uniform(size=8))
        x = SN.predict(x, us[-1].reshape(1, -1), ub, stuck, cfg)
    return cfg, ub, stuck, np.array(truth), np.array(meas), np.array(us)


RUN = _run()


def test_device_form_is_the_textbook_form():
    """60 steps of RUN, both forms from the same prior: the means within 1e-12 and T P T' within 1e-10 relative at every step."""
    cfg, ub, stuck, _, meas, us = RUN
    P = np.diag(np.r_[np.asarray(EST["p0"])[_G] ** 2, np.repeat(np.asarray(BSPEC["p0"]) ** 2, 3)])
    Pm = BS.prior(EST, BSPEC)
    np.testing.assert_allclose(Pm, BS.to_measured_dense(P), rtol=0, atol=1e-18)
    xd = xn = meas[0].copy()
    bd = bn = np.zeros(6)
    dmean, dcov = 0.0, 0.0
    for t in range(1, 61):
        xd, Pm = BS.propagate(xd, bd, Pm, us[t - 1], ub, stuck, EST["proc_sigma"], BSPEC["proc_sigma"], cfg)
        xn, P = BS.propagate_natural(xn, bn, P, us[t - 1], ub, stuck, EST["proc_sigma"], BSPEC["proc_sigma"], cfg)
        xd, bd, Pm = BS.update(xd, bd, Pm, meas[t], MEAS)
        xn, bn, P = BS.update_natural(xn, bn, P, meas[t], MEAS)
        dmean = max(dmean, np.abs(xd - xn).max(), np.abs(bd - bn).max())
        TP = BS.to_measured_dense(P)
        dcov = max(dcov, (np.abs(Pm - TP) / np.sqrt(np.outer(np.diag(TP), np.diag(TP)))).max())
    print(f"device form against textbook form: means within {dmean:.3e}, covariances within {dcov:.3e} relative")
    assert dmean <= 1e-12 and dcov <= 1e-10
    assert np.abs(bd).max() > 1e-3      # (the run moved the estimate)


def test_pieces_change_coordinates_and_back():
    rng = np.random.default_rng(2)
    P = _spd(rng, 18, np.r_[np.asarray(EST["p0"])[_G], np.repeat(BSPEC["p0"], 3)])
    pieces = BS.pack(P)
    m = BS.to_measured(*pieces)
    np.testing.assert_allclose(BS.unpack(*m), BS.T18 @ P @ BS.T18.T, rtol=1e-14, atol=0)
    back = BS.from_measured(*m)
    for a, b in zip(back, pieces):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-18)
    assert (BS.HB.sum(axis=0) == 1).all() and BS.HB[3, 0] == BS.HB[5, 2] == BS.HB[9, 3] == BS.HB[11, 5] == 1


def test_split_propagation_is_the_dense_product_and_e_is_i_minus_phi_hb():
    cfg, ub, stuck, truth, _, us = RUN
    rng = np.random.default_rng(3)
    scale = np.r_[np.asarray(EST["p0"])[_G], np.repeat(BSPEC["p0"], 3)]
    for t in (0, 17, 63):
        Pm = _spd(rng, 18, scale)
        gen = ES.generalized_force(us[t], ub, stuck, cfg)
        Phi_xx = np.eye(12) + cfg.dt * ES.jacobian(truth[t], gen, cfg)
        E = BS.e_block(Phi_xx)
        ref = np.zeros((12, 6))
        ref[0:3, 0:3] = ref[6:9, 3:6] = -cfg.dt * np.eye(3)
        ref[9:12, 3:6] = np.eye(3) - Phi_xx[9:12, 9:12]
        np.testing.assert_allclose(E, ref, rtol=0, atol=1e-17)
        assert not E[3:6].any()
        Phi = np.block([[Phi_xx, E], [np.zeros((6, 12)), np.eye(6)]])
        Qx, Qb = BS._q(EST["proc_sigma"], BSPEC["proc_sigma"])
        dense = Phi @ Pm @ Phi.T + BS.T18 @ np.diag(np.r_[Qx, Qb]) @ BS.T18.T
        a, b, c = BS.propagate_split(Pm[:12, :12], Pm[:12, 12:], Pm[12:, 12:], Phi_xx, Qx, Qb)
        got = np.block([[a, b], [b.T, c]])
        np.testing.assert_allclose(got, dense, rtol=0, atol=1e-15 * np.abs(dense).max())
        # and it is the textbook propagation in the other coordinates
        P = BS.from_measured_dense(Pm)
        _, Pn = BS.propagate_natural(truth[t], np.zeros(6), P, us[t], ub, stuck, EST["proc_sigma"], BSPEC["proc_sigma"], cfg)
        np.testing.assert_allclose(got, BS.to_measured_dense(Pn), rtol=0, atol=1e-14 * np.abs(dense).max())


def test_sequential_update_is_the_batch_update():
    cfg, ub, stuck, truth, meas, _ = RUN
    rng = np.random.default_rng(4)
    scale = np.r_[np.asarray(EST["p0"])[_G], np.repeat(BSPEC["p0"], 3)]
    R = np.diag(np.asarray(MEAS)[_G] ** 2)
    for t in (1, 30):
        Pm = _spd(rng, 18, scale)
        b = 0.01 * rng.normal(size=6)
        x = ES.retract(truth[t], rng.normal(size=12) * scale[:12])
        H = np.hstack([np.eye(12), np.zeros((12, 6))])
        K = Pm @ H.T @ np.linalg.inv(H @ Pm @ H.T + R)
        d = K @ ES.residual(meas[t], BS.with_bias(x, b))
        xn, bn, Pn = BS.update(x, b, Pm, meas[t], MEAS)
        np.testing.assert_allclose(Pn, (np.eye(18) - K @ H) @ Pm, rtol=0, atol=1e-12 * np.abs(Pm).max())
        np.testing.assert_allclose(bn, b + d[12:], rtol=0, atol=1e-13)
        ref = ES.retract(x, d[:12])
        ref[3:6] -= d[12:15]
        ref[10:13] -= d[15:18]
        np.testing.assert_allclose(xn, ref, rtol=0, atol=1e-13)
        # the textbook form with H = [I, HB] likewise
        P = BS.from_measured_dense(Pm)
        Hn = np.hstack([np.eye(12), BS.HB])
        Kn = P @ Hn.T @ np.linalg.inv(Hn @ P @ Hn.T + R)
        _, b2, P2 = BS.update_natural(x, b, P, meas[t], MEAS)
        np.testing.assert_allclose(P2, (np.eye(18) - Kn @ Hn) @ P, rtol=0, atol=1e-12 * np.abs(P).max())
        np.testing.assert_allclose(b2, bn, rtol=0, atol=1e-13)


def test_filter_finds_the_bias_and_beats_the_plain_filter():
    """|b^ - b| below 15 % of |b| per group at step 120; the rms velocity and rate errors over steps 20 to 120 at most 1/4 of the
    plain estimators.replay's on the same measurements."""
    cfg, ub, stuck, truth, meas, us = RUN
    r = BS.replay(meas, us, ub, stuck, EST, BSPEC, cfg)
    plain = ES.replay(meas, us, ub, stuck, EST, cfg)
    ev = np.linalg.norm(r["bias"][-1, 0:3] - BIAS[0:3]) / np.linalg.norm(BIAS[0:3])
    ew = np.linalg.norm(r["bias"][-1, 3:6] - BIAS[3:6]) / np.linalg.norm(BIAS[3:6])

    def rms(est, sl):
        return np.sqrt(((est[20:, sl] - truth[20:, sl]) ** 2).sum(axis=1).mean())
    rv, rw = rms(r["est"], slice(3, 6)), rms(r["est"], slice(10, 13))
    pv, pw = rms(plain["est"], slice(3, 6)), rms(plain["est"], slice(10, 13))
    print(f"|b^ - b| / |b| at step 120: velocity {ev:.3f}, rate {ew:.3f}; rms errors over steps 20..120: velocity {rv:.3e} m/s against "
          f"{pv:.3e} plain (ratio {rv / pv:.3f}), rate {rw:.3e} rad/s against {pw:.3e} plain (ratio {rw / pw:.3f})")
    assert ev < 0.15 and ew < 0.15
    assert rv <= pv / 4 and rw <= pw / 4
    assert np.array_equal(r["bias_end"], r["bias"][-1])
    # a run of 120 is two continued runs of 60 (to round-off: the dense P of the restatement is symmetric only up to that, and the
    # pieces carry its upper triangle)
    a = BS.replay(meas[:60], us[:60], ub, stuck, EST, BSPEC, cfg)
    b = BS.replay(meas[60:], us[60:], ub, stuck, EST, BSPEC, cfg, xhat=a["xhat"], cov=a["cov"], bias=a["bias_end"], cross=a["cross"],
                  cov_b=a["cov_b"], step0=60)
    np.testing.assert_allclose(np.concatenate([a["est"], b["est"]]), r["est"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(b["cov_b"], r["cov_b"], rtol=1e-9, atol=0)
    # with p0 = proc_sigma = 0 the bias stays 0 and the filter is the estimator's
    z = BS.replay(meas[:30], us[:30], ub, stuck, EST, dict(p0=(0, 0), proc_sigma=(0, 0)), cfg)
    assert not z["bias"].any() and not z["cross"].any()
    np.testing.assert_allclose(z["est"], plain["est"][:30], rtol=0, atol=1e-13)


def test_request_refusals():
    B, T = 4, 3
    est = dict(EST)
    ok = dict(p0=(0.05, 0.02), proc_sigma=(1e-4, 1e-3))
    r = BS.request(ok, B, T, est)
    assert r["fields"] == BS.FIELDS and r["bias"] is None and r["p0"].shape == (2,)
    xh = dict(est, xhat=np.zeros((B, 13)))
    b6, c72, c21 = np.zeros((B, 6)), np.zeros((B, 72)), np.zeros((B, 21))
    neg = c21.copy()
    neg[2, 11] = -1e-12
    nan6 = b6.copy()
    nan6[1, 2] = np.nan
    for spec, e, kw, msg in [
            (dict(ok, gain=1), est, {}, "unknown keys"),
            (ok, None, {}, "needs an estimator"),
            (ok, est, dict(disturbance=dict(p0=(1, 1))), "24 filter states"),
            (dict(proc_sigma=(0, 0)), est, {}, r"\['p0'\] is required"),
            (dict(ok, p0=(1.0, -1e-9)), est, {}, r"\['p0'\] must be 2 finite values >= 0"),
            (dict(ok, proc_sigma=(np.nan, 0)), est, {}, r"\['proc_sigma'\] must be 2 finite values >= 0"),
            (dict(ok, fields=("force_hist",)), est, {}, r"\['fields'\] must be among"),
            (dict(ok, cross=c72), xh, {}, r"\['cross'\] requires bias_estimate\['bias'\]"),
            (dict(ok, bias=b6, cross=c72), est, {}, r"\['cross'\] requires estimator\['xhat'\]"),
            (dict(ok, bias=b6, cov=c21), xh, {}, r"\['cov'\] requires bias_estimate\['cross'\]"),
            (dict(ok, bias=nan6), est, {}, r"\['bias'\] must be finite with shape"),
            (dict(ok, bias=np.zeros((B, 5))), est, {}, r"\['bias'\] must be finite with shape"),
            (dict(ok, bias=b6, cross=c72, cov=neg), xh, {}, "negative diagonal entry")]:
        with pytest.raises(ValueError, match=msg):
            BS.request(spec, B, T, e, **kw)
    r = BS.request(dict(ok, bias=b6, cross=c72.reshape(B, 12, 6), cov=np.zeros((B, 6, 6))), B, T, xh)
    assert r["cross"].shape == (B, 72) and r["cov"].shape == (B, 21) and r["bias"] is not b6


def test_library_exports_the_bias_entries_and_the_struct_layout(tmp_path):
    from ft_mpc_amd import _lib
    _lib.build_library()
    lib = _lib.load_library()
    header = (ROOT / "include" / "ftmpc.h").read_text()
    for n in NEW:
        assert n in _lib.SYMBOLS and getattr(lib, n) is not None
        assert f"int {n}(" in header
    assert lib.ftmpc_simulate_bias_batch.argtypes[:-1] == lib.ftmpc_simulate_disturbance_batch.argtypes
    assert lib.ftmpc_simulate_wrench_bias_batch.argtypes[:-1] == lib.ftmpc_simulate_wrench_disturbance_batch.argtypes
    assert lib.ftmpc_multi_simulate_bias_batch.argtypes[:-1] == lib.ftmpc_multi_simulate_disturbance_batch.argtypes
    assert lib.ftmpc_version() == 540
    assert [f for f, _ in _lib.ftmpc_bias_estimate._fields_] == FIELDS
    src = tmp_path / "layout.c"
    body = "".join(f'printf("%zu\\n", offsetof(ftmpc_bias_estimate, {f}));' for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftmpc.h"\nint main(void){printf("%zu\\n", sizeof(ftmpc_bias_estimate));'
                   + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(_lib.ftmpc_bias_estimate) == 72
    assert got[1:] == OFFSETS == [getattr(_lib.ftmpc_bias_estimate, f).offset for f in FIELDS]


def test_library_refuses_a_wrong_struct_size_before_any_device_work():
    """The ABI guard stands before the handle is looked at: no handle (there is none without a GPU), a struct_size of 0, and both
    single-handle entries return FTMPC_ERR_ARG with the message that names the field."""
    from ft_mpc_amd import _lib
    _lib.build_library()
    lib = _lib.load_library()
    be = _lib.ftmpc_bias_estimate(struct_size=0)
    n_thr = len(lib.ftmpc_simulate_bias_batch.argtypes)
    n_wr = len(lib.ftmpc_simulate_wrench_bias_batch.argtypes)
    scalars = {C.c_int64: 0, C.c_int32: 0, C.c_uint64: 0, C.c_double: 0.0}
    for f, n in ((lib.ftmpc_simulate_bias_batch, n_thr), (lib.ftmpc_simulate_wrench_bias_batch, n_wr)):
        args = [scalars.get(t) for t in f.argtypes[:-1]]
        assert len(args) == n - 1
        assert f(*args, C.byref(be)) == -1
        err = lib.ftmpc_last_error(None)
        assert b"ftmpc_bias_estimate.struct_size is 0" in err and str(C.sizeof(_lib.ftmpc_bias_estimate)).encode() in err, err
    good = _lib.ftmpc_bias_estimate(struct_size=C.sizeof(_lib.ftmpc_bias_estimate))
    args = [scalars.get(t) for t in lib.ftmpc_simulate_bias_batch.argtypes[:-1]]
    assert lib.ftmpc_simulate_bias_batch(*args, C.byref(good)) == -1      # (no handle: refused, without that message)
