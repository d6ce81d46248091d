"""CPU: the host side of measurement dropouts, outliers and the gated filter (include/ftmpc.h, ftmpc_outage; ft_mpc_amd/outages.py).

1  the availability chain of outages.draw meets its stationary loss fraction and its mean outage length, and the window forces
   exactly [from, to);  2  gated_update / replay without gate and with everything available are estimators.update / replay bit for
   bit;  3  a rejected channel leaves the batch-form update with that row of H removed;  4  the refusals of outages.request, the
   three symbols and the layout gcc gives the struct;  5  which entry BatchedMPC.simulate(outage=...) reaches.

Chain statistics (1): 2000 vehicles x 100 steps = 2e5 chain steps behind a burn-in of 40 steps (the chain's second eigenvalue is
1 - p_loss - p_recover = 0.4, so the start is forgotten to 1e-16).  The loss fraction is held to four binomial standard deviations
of 2e5 draws, 4 sqrt(f (1 - f) / 2e5) = 4.2e-3; the draws of one vehicle are correlated, which makes the true deviation 1.53 times the
binomial one, so the bound is 2.6 true standard deviations: measured |fraction - 1/3| = 1.46e-3.  An outage that starts inside the
100 steps is followed to its end (60 more steps), so the lengths are complete geometric draws: their mean is held to four geometric
standard deviations of the mean, 4 sqrt(1 - p_recover) / p_recover / sqrt(m) with m the number of outages; measured |mean - 2.5| =
1.68e-2 over 26 615 outages (bound 4.7e-2)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from ft_mpc_amd import _lib
from ft_mpc_amd import diagnosis as DG
from ft_mpc_amd import estimators as ES
from ft_mpc_amd import outages as OG
from ft_mpc_amd.batch import _simulate
from test_simulate_dispatch_host import B, DIAG, EST, F_MAX, FULL, N, NT, T, _pointee, _stand_in

ROOT = Path(__file__).resolve().parents[1]
NEW = ("ftmpc_simulate_outage_batch", "ftmpc_simulate_wrench_outage_batch", "ftmpc_multi_simulate_outage_batch")
FIELDS = ["struct_size", "reserved", "seed", "p_loss", "p_recover", "p_outlier", "outlier_sigma", "gate", "window", "state", "rejected",
          "outliers", "avail_hist", "outlier_hist", "gate_hist", "meas_hist"]
OFFSETS = [0, 4, 8, 16, 24, 32, 64, 96, 104, 112, 120, 128, 136, 144, 152, 160]
SIGMA = (1e-2, 5e-3, 1e-2, 5e-3)
_G = np.repeat(np.arange(4), 3)


def _y(nb):
    y = np.zeros((nb, 13))
    y[:, 9] = 1.0
    return y


# ---------------------------------------------------------------------------------------------------------------------------
# 1  the chain and the window
# ---------------------------------------------------------------------------------------------------------------------------
def test_chain_meets_its_stationary_loss_fraction_and_mean_outage_length():
    nb, burn, span, tail = 2000, 40, 100, 60
    p_loss, p_recover = 0.2, 0.4
    frac, mean_len = OG.chain_stats(p_loss, p_recover)
    assert frac == pytest.approx(1 / 3) and mean_len == pytest.approx(2.5)
    pl, pr = OG.chain_params(frac, mean_len)
    assert pl == pytest.approx(p_loss, rel=1e-14) and pr == pytest.approx(p_recover, rel=1e-14)
    y, run = _y(nb), np.zeros(nb, np.int32)
    avail = np.empty((burn + span + tail, nb), bool)
    for t in range(avail.shape[0]):
        r = OG.draw(y, t, run, p_loss=p_loss, p_recover=p_recover, seed=2024)
        assert np.array_equal(r["y"], y) and not r["outlier"].any()                 # no outlier asked for: y untouched
        assert np.array_equal(r["run"] == 0, r["avail"] == 1) and np.array_equal(r["run"], np.where(r["avail"] == 1, 0, run + 1))
        run, avail[t] = r["run"], r["avail"] == 1
    lost = ~avail[burn:burn + span]
    n = lost.size
    assert n == 200000
    dev_f = abs(lost.mean() - frac)
    # complete outages that start inside the span
    lengths = []
    for b in range(nb):
        a = avail[:, b]
        for t in range(burn, burn + span):
            if not a[t] and a[t - 1]:
                e = t
                while not a[e]:
                    e += 1
                lengths.append(e - t)
    lengths = np.array(lengths)
    dev_l = abs(lengths.mean() - mean_len)
    print(f"chain: |loss fraction - {frac:.4f}| = {dev_f:.2e} over {n} steps, |mean length - {mean_len}| = {dev_l:.2e} over {lengths.size} outages")
    assert dev_f <= 4 * np.sqrt(frac * (1 - frac) / n)
    assert dev_l <= 4 * np.sqrt(1 - p_recover) / p_recover / np.sqrt(lengths.size)
    # the draws are keyed by (seed, campaign step, vehicle number) alone: a slice of the campaign draws what the whole draws
    whole = OG.draw(y, 7, run, p_loss=p_loss, p_recover=p_recover, seed=5, step0=3)
    part = OG.draw(y[500:800], 4, run[500:800], p_loss=p_loss, p_recover=p_recover, seed=5, step0=6, index0=500, index_total=nb)
    assert np.array_equal(whole["avail"][500:800], part["avail"])


def test_window_forces_exactly_its_steps_and_the_init_step_is_available():
    nb, steps, step0 = 7, 12, 5
    window = np.array([[0, 0], [6, 9], [5, 6], [9, 9], [10, 8], [16, 40], [0, 100]], np.int32)
    y, run = _y(nb), np.zeros(nb, np.int32)
    longest = np.zeros(nb, np.int32)
    for t in range(steps):
        r = OG.draw(y, t, run, p_loss=0.0, p_recover=1.0, window=window, step0=step0)
        c = step0 + t
        assert np.array_equal(r["avail"] == 0, (window[:, 0] <= c) & (c < window[:, 1])), t
        run = r["run"]
        longest = np.maximum(longest, run)
    assert longest.tolist() == [0, 3, 1, 0, 0, 1, 12]
    r = OG.draw(y, 0, np.full(nb, 3), p_loss=0.9, p_recover=0.1, p_outlier=1.0, outlier_sigma=1.0, window=window, step0=7, init=True)
    assert r["avail"].all() and not r["run"].any() and not r["outlier"].any() and np.array_equal(r["y"], y)


def test_outliers_hit_their_group_alone():
    nb = 400
    rng = np.random.default_rng(1)
    y = rng.normal(size=(nb, 13))
    y[:, 6:10] /= np.linalg.norm(y[:, 6:10], axis=1, keepdims=True)
    r = OG.draw(y, 3, np.zeros(nb), p_outlier=(0.1, 0.0, 0.3, 1.0), outlier_sigma=(0.5, 0.5, 0.2, 0.0), seed=9)
    bits = r["outlier"]
    assert r["avail"].all() and not (bits & 2).any() and (bits & 8).all()
    assert 0 < ((bits & 1) > 0).sum() < nb and 0 < ((bits & 4) > 0).sum() < nb
    moved = np.stack([(r["y"][:, 0:3] != y[:, 0:3]).any(1), (r["y"][:, 3:6] != y[:, 3:6]).any(1),
                      (r["y"][:, 6:10] != y[:, 6:10]).any(1), (r["y"][:, 10:13] != y[:, 10:13]).any(1)], axis=1)
    assert np.array_equal(moved[:, 0], (bits & 1) > 0) and not moved[:, 1].any() and np.array_equal(moved[:, 2], (bits & 4) > 0)
    assert not moved[:, 3].any()                                                     # a sigma of zero moves nothing
    np.testing.assert_allclose(np.linalg.norm(r["y"][:, 6:10], axis=1), 1.0, rtol=0, atol=1e-15)
    # a lost vehicle draws no outlier
    r = OG.draw(y, 3, np.zeros(nb), p_loss=0.5, p_outlier=1.0, outlier_sigma=0.1, seed=9)
    assert 0 < (r["avail"] == 0).sum() < nb and np.array_equal(r["outlier"] == 0, r["avail"] == 0)
    assert np.array_equal(r["y"][r["avail"] == 0], y[r["avail"] == 0])


# ---------------------------------------------------------------------------------------------------------------------------
# 2, 3  the gated update
# ---------------------------------------------------------------------------------------------------------------------------
def _prior(rng):
    p0 = np.asarray(SIGMA)[_G]
    m = rng.normal(size=(12, 12))
    c = m @ m.T / 12 + np.eye(12)
    s = 1 / np.sqrt(np.diag(c))
    P = (c * np.outer(s, s)) * np.outer(p0, p0)
    q = rng.normal(size=4)
    x = np.concatenate([rng.normal(size=6), q / np.linalg.norm(q), 0.3 * rng.normal(size=3)])
    return x, 0.5 * (P + P.T), p0


def test_without_gate_and_all_available_it_is_the_estimators_update_bit_for_bit():
    rng = np.random.default_rng(3)
    for _ in range(20):
        x, P, p0 = _prior(rng)
        y = ES.retract(x, rng.normal(size=12) * p0)
        xa, Pa = ES.update(x, P, y, SIGMA)
        xb, Pb, mask = OG.gated_update(x, P, y, SIGMA)
        assert mask == 0 and np.array_equal(xa, xb) and np.array_equal(Pa, Pb)
        xc, Pc, mask = OG.gated_update(x, P, y, SIGMA, avail=False, gate=3.0)
        assert mask == 0 and np.array_equal(xc, x) and np.array_equal(Pc, P)
        xd, Pd, mask = OG.gated_update(x, P, y, SIGMA, gate=1e3)                     # a gate nothing reaches
        assert mask == 0 and np.array_equal(xa, xd) and np.array_equal(Pa, Pd)


def test_replay_without_gate_is_the_estimators_replay_bit_for_bit():
    from ft_mpc_amd.batch import MPCConfig
    cfg = MPCConfig(N=5, NT=8)
    rng = np.random.default_rng(4)
    steps = 9
    x, P, p0 = _prior(rng)
    meas = np.stack([ES.retract(x, rng.normal(size=12) * p0) for _ in range(steps)])
    u = rng.uniform(0, F_MAX, (steps, 8))
    ub, stuck = np.full(8, F_MAX), np.zeros(8)
    spec = dict(every=2, p0=SIGMA, proc_sigma=tuple(0.1 * s for s in SIGMA), meas_sigma=SIGMA)
    for kw in (dict(), dict(xhat=x, cov=ES.pack(P), step0=3)):
        a = ES.replay(meas, u, ub, stuck, spec, cfg, **kw)
        b = OG.replay(meas, None, u, ub, stuck, spec, cfg, **kw)
        for k in ("est", "xhat", "cov"):
            assert np.array_equal(a[k], b[k]), k
        assert not b["gate"].any() and not b["rejected"].any()
    # a lost step holds the propagated estimate
    avail = np.ones(steps, bool)
    avail[[2, 4]] = False
    c = OG.replay(meas, avail, u, ub, stuck, spec, cfg, xhat=x, cov=ES.pack(P))
    for t in (2, 4):
        assert np.array_equal(c["est"][t], ES.predict(c["est"][t - 1], u[t - 1:t], ub, stuck, cfg))


@pytest.mark.parametrize("j", [1, 4, 10])
def test_a_rejected_channel_leaves_the_batch_update_without_its_row(j):
    rng = np.random.default_rng(5 + j)
    x, P, p0 = _prior(rng)
    R = np.asarray(SIGMA)[_G] ** 2
    r = rng.normal(size=12) * 0.5 * np.sqrt(np.diag(P) + R)
    r[j] = 50.0 * np.sqrt(P[j, j] + R[j])
    r[6:9] = 0.0                                                                     # (keeps the residual of y exactly linear in r)
    y = ES.retract(x, r)
    xn, Pn, mask = OG.gated_update(x, P, y, SIGMA, gate=5.0)
    assert mask == 1 << j
    keep = [i for i in range(12) if i != j]
    H = np.eye(12)[keep]
    S = H @ P @ H.T + np.diag(R[keep])
    K = P @ H.T @ np.linalg.inv(S)
    d_ref = K @ ES.residual(y, x)[keep]
    P_ref = P - K @ H @ P
    dev_P = (np.abs(Pn - P_ref) / np.outer(p0, p0)).max()
    dev_d = (np.abs(ES.residual(xn, x) - d_ref) / p0).max()
    print(f"rejected channel {j}: max |P - batch| / p0_i p0_j = {dev_P:.2e}, max |d - batch| / p0_i = {dev_d:.2e}")
    assert dev_P <= 1e-12 and dev_d <= 1e-12
    # and without the gate the wild sample moves the estimate by many p0
    x0, _, m0 = OG.gated_update(x, P, y, SIGMA, gate=0.0)
    assert m0 == 0 and (np.abs(ES.residual(x0, x)) / p0).max() > 10


# ---------------------------------------------------------------------------------------------------------------------------
# 4  request, the symbols, the layout
# ---------------------------------------------------------------------------------------------------------------------------
def test_request_refusals():
    nb, steps = 4, 3
    ok = dict(p_loss=0.2, p_recover=0.4, p_outlier=0.1, outlier_sigma=(0.5, 0.2, 0.5, 0.2), gate=5.0)
    r = OG.request(ok, nb, steps, EST)
    assert r["p_outlier"].tolist() == [0.1] * 4 and r["outlier_sigma"].shape == (4,) and r["fields"] == () and r["window"] is None
    neg3, neg4 = np.zeros((nb, 3), np.int32), np.zeros((nb, 4), np.int32)
    neg3[2, 1], neg4[1, 3] = -1, -2
    for spec, e, kw, msg in [
            (dict(ok, every=2), EST, {}, "unknown keys"),
            (ok, None, {}, "needs an estimator"),
            (ok, EST, dict(disturbance=dict(p0=(1, 1))), "disturbance filter has no gated form"),
            (ok, EST, dict(bias_estimate=dict(p0=(1, 1))), "bias filter has no gated form"),
            (dict(ok, p_loss=1.0), EST, {}, r"\['p_loss'\] must be in \[0, 1\)"),
            (dict(ok, p_loss=-0.1), EST, {}, r"\['p_loss'\] must be in \[0, 1\)"),
            (dict(ok, p_loss=np.nan), EST, {}, r"\['p_loss'\] must be in \[0, 1\)"),
            (dict(ok, p_recover=0.0), EST, {}, r"\['p_recover'\] must be in \(0, 1\]"),
            (dict(ok, p_recover=1.5), EST, {}, r"\['p_recover'\] must be in \(0, 1\]"),
            (dict(ok, p_outlier=(0, 0, 1.1, 0)), EST, {}, r"\['p_outlier'\] must be in \[0, 1\]"),
            (dict(ok, p_outlier=(0, 0, np.nan, 0)), EST, {}, r"\['p_outlier'\] must be in \[0, 1\]"),
            (dict(ok, p_outlier=(0, 0, 0)), EST, {}, r"\['p_outlier'\] must be one value or 4"),
            (dict(ok, outlier_sigma=(1, -1e-9, 1, 1)), EST, {}, r"\['outlier_sigma'\] must be finite and >= 0"),
            (dict(ok, outlier_sigma=np.inf), EST, {}, r"\['outlier_sigma'\] must be finite and >= 0"),
            (dict(ok, gate=-1.0), EST, {}, r"\['gate'\] must be finite and >= 0"),
            (dict(ok, gate=np.nan), EST, {}, r"\['gate'\] must be finite and >= 0"),
            (dict(ok, fields=("est",)), EST, {}, r"\['fields'\] must be among"),
            (dict(ok, window=np.zeros((nb, 3), np.int32)), EST, {}, r"\['window'\] must have shape"),
            (dict(ok, state=neg3), EST, {}, r"\['state'\] must have shape"),
            (dict(ok, state=np.zeros((nb, 4), np.int32)), EST, {}, r"\['state'\] must have shape"),
            (dict(ok, rejected=neg4), EST, {}, r"\['rejected'\] must have shape"),
            (dict(ok, outliers=neg4), EST, {}, r"\['outliers'\] must have shape")]:
        with pytest.raises(ValueError, match=msg):
            OG.request(spec, nb, steps, e, **kw)
    st = np.ones((nb, 3), np.int32)
    r = OG.request(dict(ok, state=st, window=[[0, 2]] * nb), nb, steps, EST)
    assert r["state"] is not st and r["state"].dtype == np.int32 and r["window"].dtype == np.int32
    with pytest.raises(ValueError, match="mean_length >= 1"):
        OG.chain_params(0.2, 0.5)
    with pytest.raises(ValueError, match="no chain"):
        OG.chain_params(0.9, 1.0)


def test_library_exports_the_outage_entries_and_the_struct_layout(tmp_path):
    _lib.build_library()
    lib = _lib.load_library()
    header = (ROOT / "include" / "ftmpc.h").read_text()
    for n in NEW:
        assert n in _lib.SYMBOLS and getattr(lib, n) is not None
        assert f"int {n}(" in header
    assert lib.ftmpc_simulate_outage_batch.argtypes[:-1] == lib.ftmpc_simulate_bias_batch.argtypes
    assert lib.ftmpc_simulate_wrench_outage_batch.argtypes[:-1] == lib.ftmpc_simulate_wrench_bias_batch.argtypes
    assert lib.ftmpc_multi_simulate_outage_batch.argtypes[:-1] == lib.ftmpc_multi_simulate_bias_batch.argtypes
    assert [f for f, _ in _lib.ftmpc_outage._fields_] == FIELDS
    src = tmp_path / "layout.c"
    body = "".join(f'printf("%zu\\n", offsetof(ftmpc_outage, {f}));' for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftmpc.h"\nint main(void){printf("%zu\\n", sizeof(ftmpc_outage));'
                   + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(_lib.ftmpc_outage) == 168
    assert got[1:] == OFFSETS == [getattr(_lib.ftmpc_outage, f).offset for f in FIELDS]
    # no earlier struct changed size
    assert [C.sizeof(s) for s in (_lib.ftmpc_sensor, _lib.ftmpc_estimator, _lib.ftmpc_diagnosis, _lib.ftmpc_disturbance,
                                  _lib.ftmpc_bias_estimate)] == [96, 136, 152, 88, 72]


def test_diagnosis_replay_skips_a_lost_step():
    from ft_mpc_amd.batch import MPCConfig
    cfg = MPCConfig(N=5, NT=8)
    rng = np.random.default_rng(8)
    steps = 8
    x = np.r_[np.zeros(9), 1.0, np.zeros(3)]
    meas = x[None] + 1e-3 * rng.normal(size=(steps, 13))
    u = rng.uniform(0, F_MAX, (steps, 8))
    ub, stuck = np.full(8, F_MAX), np.zeros(8)
    spec = dict(DIAG, threshold=1e9)
    a = DG.replay(meas, u, ub, stuck, spec, cfg)
    b = DG.replay(meas, u, ub, stuck, spec, cfg, avail=np.ones(steps, bool))
    assert np.array_equal(a["llr_hist"], b["llr_hist"]) and np.array_equal(a["state"], b["state"])
    avail = np.ones(steps, bool)
    avail[[3, 4]] = False
    c = DG.replay(meas, u, ub, stuck, spec, cfg, avail=avail)
    assert np.array_equal(c["llr_hist"][:3], a["llr_hist"][:3])
    assert np.array_equal(c["llr_hist"][3], c["llr_hist"][2]) and np.array_equal(c["llr_hist"][4], c["llr_hist"][2])
    assert np.isnan(c["peak"][3:5]).all() and not np.isnan(c["peak"][5])            # the first test afterwards covers n = 3 steps
    assert not np.array_equal(c["llr_hist"][5], a["llr_hist"][5])


# ---------------------------------------------------------------------------------------------------------------------------
# 5  dispatch
# ---------------------------------------------------------------------------------------------------------------------------
OUTAGE = dict(p_loss=0.2, p_recover=0.4, gate=5.0, fields=("avail", "gate", "state"))


def _call(obj, multi, wrench, **kw):
    x0 = np.zeros((B, 13))
    x0[:, 6] = 1.0
    args = dict(uref_traj=None, noise=(0, 0, 0, 0), seed=3, return_inputs=True, sqp_iters=0, backtracks=8, tol=1e-9,
                formulation="wrench" if wrench else "thruster", hull=None, penalty=0.0, faults=None, detect_delay=0, return_states=False,
                outcomes=None, return_status=False, index0=0, index_total=None)
    args.update(kw)
    return _simulate(obj, multi, x0, np.full((B, NT), F_MAX), np.zeros((B, NT)), np.zeros((9, T + N)), T, **args)


@pytest.mark.parametrize("wrench,multi", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("full", [False, True])
def test_outage_reaches_its_entry_with_the_struct_last(wrench, multi, full):
    kw = dict(FULL) if full else dict(estimator=EST)
    if wrench and "diagnosis" in kw:
        kw["diagnosis"] = dict(kw["diagnosis"], rebuild_hull=True)
    obj, rec, real = _stand_in()
    out = _call(obj, multi, wrench, outage=OUTAGE, **kw)
    assert len(rec.calls) == 1
    name, got = rec.calls[0]
    assert name == ("ftmpc_multi_simulate_outage_batch" if multi else
                    "ftmpc_simulate_wrench_outage_batch" if wrench else "ftmpc_simulate_outage_batch")
    assert len(got) == len(getattr(real, name).argtypes)
    og = _pointee(got[-1])
    assert isinstance(og, _lib.ftmpc_outage) and og.struct_size == 168 and og.p_loss == 0.2 and og.gate == 5.0
    assert got[-2] is None and got[-3] is None                                       # no bias estimate, no disturbance
    assert bool(og.avail_hist) and bool(og.gate_hist) and bool(og.state) and not og.meas_hist and not og.rejected and not og.window
    assert sorted(out["outage"]) == ["avail", "gate", "state"] and out["outage"]["avail"].shape == (T, B)
    assert out["outage"]["state"].shape == (B, 3)


def test_without_outage_the_entry_is_the_narrower_one_and_the_wrench_driver_request_is_refused():
    obj, rec, _ = _stand_in()
    out = _call(obj, False, False, estimator=EST)
    assert rec.calls[0][0] == "ftmpc_simulate_estimator_batch" and "outage" not in out
    obj, rec, _ = _stand_in()
    with pytest.raises(ValueError, match="MultiGPUMPC is not built"):
        _call(obj, True, True, estimator=EST, outage=OUTAGE)
    with pytest.raises(ValueError, match="needs an estimator"):
        _call(obj, False, False, outage=OUTAGE)
    assert rec.calls == []
