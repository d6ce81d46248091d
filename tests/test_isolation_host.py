"""CPU: the diagnosis' consistency gate, confirmation and level revision (include/ftmpc.h, ftmpc_isolation; csrc/ftmpc_isolate.h, the
host / device functions ftmpc_diagnose_iso_kernel is made of; ft_mpc_amd/diagnosis.py, test_step / replay with isolation=).

The header runs in a stand-alone C++ program with its own main, built with -fsanitize=address,undefined where the toolchain links
them (a plain executable: nothing is preloaded and nothing is loaded into python), else without, and is compared with
diagnosis.test_step(..., isolation=...) plus the decision over 40 tests of 7 vehicles with every rule on.  The bound on the
statistics and on fit_hist is rtol 1e-12 + atol 1e-12: the two sides differ by the order of their sums and by 1 / s against a
division, on values of order 1 to 1e3.  The decisions are identical.

The open loops are the ones of tests/test_diagnosis_host.py::_open_loop with 48 vehicles and 45 steps, levels (0, 1.7, 3.4),
threshold 18, max_detect 4, consist = consist_for(0.999) = 4.74 and persist 2; every assertion is against the plain arm of the same
data, the counts are printed.  Measured here (plain -> all three rules; "wrong": the final pattern is not exactly the fault):
  every 3, stuck 3.4 N, onset 11 (inside a window)   183 detections, 47 of 48 wrong -> 47 detections, 1 wrong
  every 1, stuck 3.4 N, onset 10                      48 detections, 0 wrong        -> 48 detections, 0 wrong, at most 1 test later, 1 void
  healthy, kick 5 N + 0.25 N m over 3 steps           192 false detections          -> 0, 144 void tests (the gate alone)
  healthy, no kick                                    0                             -> 0, no void test"""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from ft_mpc_amd import diagnosis as DG
from test_diagnosis_host import F_MAX, NT, SIGMA, _cfg

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "fault-tolerant-mpc_amd" / "csrc"
LEVELS = (0.0, 1.7, F_MAX)
CONSIST = DG.consist_for(0.999)
ALL = dict(consist=CONSIST, persist=2, revise=True)
FIELDS = ["struct_size", "reserved", "consist", "persist", "revise", "lead", "voided", "revised", "fit_hist"]
OFFSETS = [0, 4, 8, 16, 20, 24, 32, 40, 48]


def _spec(**kw):
    return dict(dict(every=1, levels=LEVELS, resid_sigma=DG.default_sigma(SIGMA), drift_sigma=(0.0, 0.0), threshold=18.0, max_detect=4),
                **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# the header against test_step plus the decision
# ---------------------------------------------------------------------------------------------------------------------------
HB, HT, HL, HK = 7, 40, 3, 4
HH = NT * HL
N_HEAD, N_VEH, N_IN, N_OUT = 71, 2 * NT + 1 + 3 * HK, 13 + 13 + 1 + NT + 1, HH + 2 + 5

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ftmpc_isolate.h"
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int B = 7, T = 40, NT = 8, L = 3, H = 24, K = 4;
    const int NHEAD = 71, NVEH = 29, NIN = 36, NOUT = 31;
    std::vector<double> in((size_t)NHEAD + (size_t)B * NVEH + (size_t)T * B * NIN), out((size_t)T * B * NOUT + (size_t)B * NOUT);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
    std::fclose(f);
    const double* hd = in.data();
    const double dt = hd[0], inv_mass = hd[1];
    const double* Jinv = hd + 2;
    const double* D = hd + 11;      // [6][NT]
    ftmpc_iso::Rule R;
    for (int l = 0; l < 4; ++l) R.levels[l] = hd[59 + l];
    const double* rsq = hd + 63;
    const double* dsq = hd + 65;
    R.threshold = hd[67];
    R.consist_sq = hd[68];
    R.L = L, R.persist = (int)hd[69], R.revise = (int)hd[70], R.pad0 = 0;
    std::vector<double> ub((size_t)B * NT), stuck((size_t)B * NT), llr((size_t)B * H, 0.0);
    std::vector<int> cnt(B), det((size_t)B * 3 * K), lead(B, -1), run(B, 0), voided(B, 0), revised(B, 0);
    for (int b = 0; b < B; ++b) {
        const double* v = in.data() + NHEAD + (size_t)b * NVEH;
        for (int i = 0; i < NT; ++i) ub[(size_t)b * NT + i] = v[i], stuck[(size_t)b * NT + i] = v[NT + i];
        cnt[b] = (int)v[2 * NT];
        for (int k = 0; k < 3 * K; ++k) det[(size_t)b * 3 * K + k] = (int)v[2 * NT + 1 + k];
    }
    for (int t = 0; t < T; ++t)
        for (int b = 0; b < B; ++b) {
            const double* v = in.data() + NHEAD + (size_t)B * NVEH + ((size_t)t * B + b) * NIN;
            const double* y = v;
            const double* xt = v + 13;
            const double n = v[26];
            const double* acc = v + 27;
            const int c = (int)v[27 + NT];
            double* o = out.data() + ((size_t)t * B + b) * NOUT;
            double* s = llr.data() + (size_t)b * H;
            int* dstep = det.data() + (size_t)b * 3 * K;
            o[H] = o[H + 1] = -1.0;
            for (int k = 0; k < 5; ++k) o[H + 2 + k] = 0.0;
            if (cnt[b] < K) {
                ftmpc_iso::Resid r;
                ftmpc_iso::residual(xt, y, n, rsq, dsq, r);
                ftmpc_iso::Scan sc;
                ftmpc_iso::scan_start(R, sc);
                for (int i = 0; i < NT; ++i) {
                    const bool live = ub[(size_t)b * NT + i] > 0.0;
                    bool listed = false;
                    for (int k = 0; k < cnt[b]; ++k) listed = listed || dstep[K + k] == i;
                    const double d[6] = {D[i], D[NT + i], D[2 * NT + i], D[3 * NT + i], D[4 * NT + i], D[5 * NT + i]};
                    double gh[6];
                    ftmpc_iso::unit_signature(dt, inv_mass, Jinv, d, gh);
                    ftmpc_iso::thruster(R, r, n, i, live, listed, acc[i], stuck[(size_t)b * NT + i], gh, s + i * L, 1, o + i * L, sc);
                }
                if (sc.eligible > 0) o[H] = r.q0, o[H + 1] = sc.qmin;
                const bool vd = ftmpc_iso::is_void(R, r, sc);
                voided[b] += vd ? 1 : 0;
                o[H + 2] = vd ? 1.0 : 0.0;
                o[H + 3] = sc.besth;
                if (ftmpc_iso::confirm(R, sc, lead[b], run[b])) {
                    revised[b] += ftmpc_iso::decide(R, sc.besth, c, cnt[b], H, ub.data() + (size_t)b * NT, stuck.data() + (size_t)b * NT,
                                                    dstep, dstep + K, dstep + 2 * K, s, 1, lead[b], run[b]);
                    cnt[b] += 1;
                    o[H + 6] = 1.0;
                }
                o[H + 4] = lead[b];
                o[H + 5] = run[b];
            } else {
                for (int k = 0; k < H; ++k) o[k] = s[k];
                o[H + 3] = -1.0, o[H + 4] = lead[b], o[H + 5] = run[b];
            }
        }
    for (int b = 0; b < B; ++b) {
        double* o = out.data() + (size_t)T * B * NOUT + (size_t)b * NOUT;
        for (int i = 0; i < NT; ++i) o[i] = ub[(size_t)b * NT + i], o[NT + i] = stuck[(size_t)b * NT + i];
        for (int k = 0; k < 3 * K; ++k) o[2 * NT + k] = det[(size_t)b * 3 * K + k];
        o[2 * NT + 3 * K] = cnt[b], o[2 * NT + 3 * K + 1] = voided[b], o[2 * NT + 3 * K + 2] = revised[b];
    }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
    std::fclose(f);
    return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "isolate_main.cpp"
    src.write_text(MAIN)
    exe = tmp_path / "isolate"
    base = ["g++", "-std=c++17", "-O1", "-g", "-I", str(CSRC), str(src), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:
        subprocess.run(base, check=True)
    return exe


def _decide(r, c, det, ub, stuck, lv):
    """the decision of replay on test_step's result; returns (llr, lead, revision)"""
    if not r["decide"]:
        return r["llr"], r["lead"], 0
    i, l = divmod(r["leader"], len(lv))
    det.append((c, i, l))
    rev = int(not ub[i] > 0)
    ub[i], stuck[i] = 0.0, lv[l]
    return np.zeros_like(r["llr"]), (-1, 0), rev


def test_header_step_is_test_step_plus_the_decision(tmp_path):
    """7 vehicles, 40 tests, every rule on (consist 4.74, persist 2, revise), three levels, max_detect 4.  Vehicles 0-2: thruster b
    stuck at 3.4 N from test 8; vehicles 3-4 start with (b, 1.7 N) in their list and pattern while the plant is at 3.4 N (a
    revision); vehicles 5-6 are healthy and are pushed over the tests 20-22 (void tests).  The residual of every test is the
    signature of what the plant delivers beyond the model's pattern as it stands on the Python side, plus noise, so both sides walk
    through detections, confirmations and revisions on the same inputs."""
    from ft_mpc_amd.estimators import _body_to_inertial, _cfg_model
    cfg = _cfg()
    D, m, J = _cfg_model(cfg)
    spec = _spec(max_detect=HK)
    lv = np.array(LEVELS)
    rs = np.asarray(spec["resid_sigma"])
    rng = np.random.default_rng(41)
    gv, gw = (cfg.dt / m) * D[0:3].T, cfg.dt * np.linalg.solve(J, D[3:6]).T
    head = np.concatenate([[cfg.dt, 1.0 / m], np.linalg.inv(J).reshape(-1), D.reshape(-1), np.r_[lv, 0.0], rs ** 2, [0.0, 0.0],
                           [spec["threshold"], CONSIST ** 2, ALL["persist"], 1.0]])
    assert head.size == N_HEAD and N_VEH == 29 and N_IN == 36 and N_OUT == 31
    ub, stuck = np.full((HB, NT), F_MAX), np.zeros((HB, NT))
    det = [[] for _ in range(HB)]
    for b in (3, 4):
        ub[b, b], stuck[b, b] = 0.0, 1.7
        det[b].append((0, b, 1))
    veh = np.full((HB, N_VEH), -1.0)
    for b in range(HB):
        veh[b, :2 * NT + 1] = np.r_[ub[b], stuck[b], len(det[b])]
        for k, d in enumerate(det[b]):
            veh[b, 2 * NT + 1 + k], veh[b, 2 * NT + 1 + HK + k], veh[b, 2 * NT + 1 + 2 * HK + k] = d
    llr = np.zeros((HB, NT, HL))
    lead = [(-1, 0)] * HB
    voided, revised = np.zeros(HB, int), np.zeros(HB, int)
    rows, ref = np.empty((HT, HB, N_IN)), np.zeros((HT, HB, N_OUT))
    for t in range(HT):
        for b in range(HB):
            xt = np.concatenate([rng.normal(size=6), rng.normal(size=4), 0.3 * rng.normal(size=3)])
            xt[6:10] /= np.linalg.norm(xt[6:10])
            n = float(1 + (t + b) % 3)
            acc = n * rng.uniform(0.0, 0.4 * F_MAX, size=NT)
            true = np.where(ub[b] > 0, acc, n * stuck[b])          # what the plant delivers: the model's, but for the fault
            if b < 5 and t >= 8:
                true[b] = n * F_MAX
            extra = true - np.where(ub[b] > 0, acc, n * stuck[b])
            dv, dw = gv.T @ extra + rs[0] * rng.normal(size=3), gw.T @ extra + rs[1] * rng.normal(size=3)
            if b >= 5 and 20 <= t < 23:
                dv, dw = dv + 12 * rs[0] * rng.normal(size=3), dw + 12 * rs[1] * rng.normal(size=3)
            y = xt.copy()
            y[3:6] += _body_to_inertial(xt[6:10]) @ dv
            y[10:13] += dw
            rows[t, b] = np.r_[y, xt, n, acc, 100 + t]
            o = ref[t, b]
            o[HH:HH + 2] = -1.0
            if len(det[b]) < HK:
                r = DG.test_step(llr[b], y, xt, n, acc, ub[b], spec, cfg, isolation=ALL, lead=lead[b], stuck=stuck[b],
                                 listed=[d[1] for d in det[b]])
                o[:HH] = r["llr"].reshape(-1)
                if not np.isnan(r["qmin"]):
                    o[HH:HH + 2] = r["q0"], r["qmin"]
                    # q_h = q_0 - 2 z_h against the energy of the residual with the signature subtracted
                    a_v, a_w = DG.signature(n, acc, lv, cfg)
                    direct = (((dv - a_v) ** 2).sum(-1) / rs[0] ** 2 + ((dw - a_w) ** 2).sum(-1) / rs[1] ** 2)[ub[b] > 0]
                    assert np.allclose(r["q"][ub[b] > 0], direct, rtol=1e-9, atol=1e-9 * r["q0"])
                voided[b] += r["void"]
                llr[b], lead[b], rev = _decide(r, 100 + t, det[b], ub[b], stuck[b], lv)
                revised[b] += rev
                o[HH + 2:] = r["void"], r["leader"], lead[b][0], lead[b][1], r["decide"]
            else:
                o[:HH] = llr[b].reshape(-1)
                o[HH + 3:HH + 6] = -1, lead[b][0], lead[b][1]
    (tmp_path / "in.bin").write_bytes(np.concatenate([head, veh.reshape(-1), rows.reshape(-1)]).tobytes())
    exe = _build(tmp_path)
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.float64)
    steps, fin = got[:HT * HB * N_OUT].reshape(HT, HB, N_OUT), got[HT * HB * N_OUT:].reshape(HB, N_OUT)
    np.testing.assert_allclose(steps[:, :, :HH + 2], ref[:, :, :HH + 2], rtol=1e-12, atol=1e-12)
    assert np.array_equal(steps[:, :, HH + 2:], ref[:, :, HH + 2:])
    for b in range(HB):
        assert np.array_equal(fin[b, :NT], ub[b]) and np.array_equal(fin[b, NT:2 * NT], stuck[b]), b
        K0 = 2 * NT
        got_det = [(int(fin[b, K0 + k]), int(fin[b, K0 + HK + k]), int(fin[b, K0 + 2 * HK + k])) for k in range(int(fin[b, K0 + 3 * HK]))]
        assert got_det == det[b], (b, got_det, det[b])
        assert (fin[b, K0 + 3 * HK + 1], fin[b, K0 + 3 * HK + 2]) == (voided[b], revised[b])
    print(f"header: detections {det}, voided {voided}, revised {revised}")
    # the case exercises what it says: detections after a confirmation, revisions to the right level, void tests on the pushed ones
    for b in range(3):
        assert det[b] and det[b][0][1] == b and det[b][0][0] >= 100 + 9, det[b]
        assert ub[b, b] == 0.0 and stuck[b, b] == F_MAX
    for b in (3, 4):
        assert revised[b] >= 1 and stuck[b, b] == F_MAX
    assert voided[5] > 0 and voided[6] > 0 and det[5] == [] and det[6] == []
    assert (ref[:, :, HH + 5] == 1).any()      # a leader that waited for its confirmation


def test_fit_identity_against_the_direct_energy():
    """q_h = q_0 - 2 z_h against |rho_v - a_v|^2 / s_v + |r_w - a_w|^2 / s_w, to 1e-12 relative (of q_0, the larger of the two)."""
    from ft_mpc_amd.estimators import _body_to_inertial, residual
    cfg = _cfg()
    spec = _spec()
    rng = np.random.default_rng(7)
    lv, rs = np.array(LEVELS), np.asarray(spec["resid_sigma"])
    worst = 0.0
    for _ in range(50):
        xt = np.concatenate([rng.normal(size=6), rng.normal(size=4), 0.3 * rng.normal(size=3)])
        xt[6:10] /= np.linalg.norm(xt[6:10])
        y = xt + np.concatenate([np.zeros(3), 3 * rs[0] * rng.normal(size=3), np.zeros(4), 3 * rs[1] * rng.normal(size=3)])
        n = float(rng.integers(1, 4))
        acc = n * rng.uniform(0, F_MAX, NT)
        r = DG.test_step(np.zeros((NT, 3)), y, xt, n, acc, np.full(NT, F_MAX), spec, cfg, isolation=dict(consist=CONSIST))
        res = residual(y, xt)
        rho_v, r_w = _body_to_inertial(xt[6:10]).T @ res[3:6], res[9:12]
        a_v, a_w = DG.signature(n, acc, lv, cfg)
        direct = ((rho_v - a_v) ** 2).sum(-1) / rs[0] ** 2 + ((r_w - a_w) ** 2).sum(-1) / rs[1] ** 2
        worst = max(worst, (np.abs(r["q"] - direct) / np.maximum(r["q0"], direct)).max())
    print(f"fit identity: largest relative deviation {worst:.2e}")
    assert worst <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# replay
# ---------------------------------------------------------------------------------------------------------------------------
def test_trivial_isolation_is_the_plain_replay_bit_for_bit():
    from test_diagnosis_host import _open_loop
    from test_diagnosis_host import _spec as spec2
    cfg = _cfg()
    run = _open_loop("stuck_on")
    for b in range(0, run["B"], 7):
        a = DG.replay(run["meas"][:, b], run["u"], run["ub"], run["stuck"], spec2(), cfg)
        r = DG.replay(run["meas"][:, b], run["u"], run["ub"], run["stuck"], spec2(), cfg, isolation=dict(consist=0, persist=1, revise=False))
        for k in ("llr_hist", "ub", "stuck", "ub_end", "stuck_end", "state", "llr"):
            assert np.array_equal(a[k], r[k]), (b, k)
        assert np.array_equal(a["peak"], r["peak"], equal_nan=True) and a["detections"] == r["detections"] and a["detections"]
        assert r["voided"] == 0 and r["revised"] == 0 and r["lead"] == (-1, 0)


@functools.lru_cache(maxsize=None)
def _loop(level, onset, kick):
    """tests/test_diagnosis_host.py::_open_loop with 48 vehicles and 45 steps: thruster b % NT stuck at `level` from `onset` on
    (level < 0: healthy), a push of kick N and kick / 20 N m over the steps 20-22.  The push's directions are drawn per vehicle (the
    force in the body frame of step 20) until, in the whitened residual space, at least half of its energy is orthogonal to every
    thruster's signature line: a push along such a line IS that thruster's signature for as long as it lasts, and no test on this
    residual can tell the two apart (the first draws, seed 15, put 90 % of vehicle 25's push on thruster 6's line)."""
    from oracle import qp_oracle as qo
    from ft_mpc_amd.dispersion import plant_step
    from ft_mpc_amd.sensors import measure
    cfg = _cfg()
    B, T = 48, 45
    rng = np.random.default_rng(14)
    ub, stuck = np.full(NT, F_MAX), np.zeros(NT)
    x = qo.make_batch(B, 10, NT, 0, 23)[0]
    u = rng.uniform(0.0, 0.5 * F_MAX, size=(T, NT))
    from ft_mpc_amd.estimators import _body_to_inertial, _cfg_model
    D, m, J = _cfg_model(cfg)
    rs = DG.default_sigma(SIGMA)
    lines = np.concatenate([(cfg.dt / m) * D[0:3].T / rs[0], cfg.dt * np.linalg.solve(J, D[3:6]).T / rs[1]], axis=1)      # [NT, 6]
    lines /= np.linalg.norm(lines, axis=1, keepdims=True)
    drng, dirs = np.random.default_rng(15), np.empty((B, 2, 3))
    for b in range(B):
        while True:
            d = drng.normal(size=(2, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            w = np.concatenate([(cfg.dt / m) * d[0] / rs[0], cfg.dt * np.linalg.solve(J, 0.05 * d[1]) / rs[1]])
            if 1.0 - ((lines @ w) ** 2).max() / (w @ w) >= 0.5:
                break
        dirs[b] = d
    meas = np.empty((T, B, 13))
    for t in range(T):
        meas[t] = measure(x, t, SIGMA, seed=78)
        for b in range(B):
            pub, pst = ub.copy(), stuck.copy()
            if level >= 0 and t >= onset:
                pub[b % NT], pst[b % NT] = 0.0, level
            if t == 20:
                dirs[b, 0] = _body_to_inertial(x[b, 6:10]) @ dirs[b, 0]
            pl = dict(force=kick * dirs[b, 0], torque=0.05 * kick * dirs[b, 1]) if kick and 20 <= t < 23 else {}
            x[b] = plant_step(x[b], u[t], pub, pst, pl, cfg)
            x[b, 6:10] /= np.linalg.norm(x[b, 6:10])
    return dict(meas=meas, u=u, ub=ub, stuck=stuck, B=B, T=T)


def _arm(run, every, isolation):
    cfg = _cfg()
    return [DG.replay(run["meas"][:, b], run["u"], run["ub"], run["stuck"], _spec(every=every), cfg, isolation=isolation)
            for b in range(run["B"])]


def _wrong(reps, level):
    """vehicles whose final pattern is not exactly the fault"""
    n = 0
    for b, r in enumerate(reps):
        ub, st = np.full(NT, F_MAX), np.zeros(NT)
        if level >= 0:
            ub[b % NT], st[b % NT] = 0.0, level
        n += int(not (np.array_equal(r["ub_end"], ub) and np.array_equal(r["stuck_end"], st)))
    return n


def _ndet(reps):
    return sum(len(r["detections"]) for r in reps)


def test_a_push_is_not_a_fault_and_a_healthy_run_has_no_void_test():
    run = _loop(-1.0, 0, 5.0)
    plain, gate = _arm(run, 1, None), _arm(run, 1, dict(consist=CONSIST))
    print(f"5 N kick: plain {_ndet(plain)} detections, gate {_ndet(gate)} detections, {sum(r['voided'] for r in gate)} void tests")
    assert all(len(r["detections"]) >= 1 for r in plain)
    assert _ndet(gate) == 0 and all(r["voided"] > 0 for r in gate)
    run = _loop(-1.0, 0, 0.0)
    rules = _arm(run, 1, ALL)
    print(f"healthy: {_ndet(rules)} detections, {sum(r['voided'] for r in rules)} void tests")
    assert _ndet(rules) == 0 and sum(r["voided"] for r in rules) == 0


def test_onset_inside_a_window_is_named_better_with_the_rules():
    run = _loop(F_MAX, 11, 0.0)
    plain, rules = _arm(run, 3, None), _arm(run, 3, ALL)
    wp, wr = _wrong(plain, F_MAX), _wrong(rules, F_MAX)
    print(f"every 3, 3.4 N from step 11: plain {_ndet(plain)} detections, {wp} of {run['B']} wrong; rules {_ndet(rules)} detections, {wr} wrong, "
          f"{sum(r['revised'] for r in rules)} revisions")
    assert wr < wp


def test_a_clear_fault_is_found_at_most_one_test_later():
    run = _loop(F_MAX, 10, 0.0)
    plain, rules = _arm(run, 1, None), _arm(run, 1, ALL)
    late = 0
    for b in range(run["B"]):
        dp, dr = plain[b]["detections"], rules[b]["detections"]
        assert dp and dp[0][1] == b % NT and dr and dr[0][1] == b % NT, (b, dp, dr)
        assert dr[0][0] - dp[0][0] <= ALL["persist"] - 1 + 1, (b, dp, dr)      # the confirmation's test, and one the gate may take
        late = max(late, dr[0][0] - dp[0][0])
    print(f"every 1, 3.4 N from step 10: plain {_ndet(plain)} detections, {_wrong(plain, F_MAX)} wrong; rules {_ndet(rules)}, "
          f"{_wrong(rules, F_MAX)} wrong, largest extra delay {late}, {sum(r['voided'] for r in rules)} void tests")


def test_a_wrong_level_is_revised():
    """The controller's pattern and list say (i, 1.7 N), the plant is stuck at 3.4 N, no noise: one more entry (i, 3.4 N), no other
    thruster touched, revised == 1; without revise nothing happens (the thruster is off: no hypothesis is eligible for it)."""
    from ft_mpc_amd.dispersion import plant_step
    cfg = _cfg()
    i, T = 2, 12
    rng = np.random.default_rng(3)
    from oracle import qp_oracle as qo
    x = qo.make_batch(1, 10, NT, 0, 5)[0][0]
    ub, stuck = np.full(NT, F_MAX), np.zeros(NT)
    ub[i], stuck[i] = 0.0, 1.7
    pst = stuck.copy()
    pst[i] = F_MAX
    u = rng.uniform(0.0, 0.5 * F_MAX, size=(T, NT))
    meas = np.empty((T, 13))
    for t in range(T):
        meas[t] = x
        x = plant_step(x, u[t], ub, pst, {}, cfg)
        x[6:10] /= np.linalg.norm(x[6:10])
    spec = _spec(resid_sigma=(1e-3, 1e-3))
    state = np.concatenate([meas[0], [0.0], np.zeros(NT)])
    kw = dict(state=state, detections=[(0, i, 1)])
    r = DG.replay(meas, u, ub, stuck, spec, cfg, isolation=dict(consist=0, persist=1, revise=True), **kw)
    assert r["detections"] == [(0, i, 1), (1, i, 2)], r["detections"]      # step 0 anchors, step 1 is the first test, persist 1 decides
    assert r["revised"] == 1 and r["stuck_end"][i] == F_MAX and r["ub_end"][i] == 0.0
    assert np.array_equal(np.delete(r["ub_end"], i), np.delete(ub, i)) and np.array_equal(np.delete(r["stuck_end"], i), np.delete(stuck, i))
    off = DG.replay(meas, u, ub, stuck, spec, cfg, isolation=dict(consist=0, persist=2, revise=False), **kw)
    assert off["revised"] == 0 and off["stuck_end"][i] == 1.7


def test_continued_replay_through_lead_is_bit_for_bit():
    run = _loop(F_MAX, 11, 0.0)
    cfg = _cfg()
    spec = _spec(every=1)
    seam = False
    for b in range(0, run["B"], 5):
        m, u = run["meas"][8:20, b], run["u"][8:20]
        whole = DG.replay(m, u, run["ub"], run["stuck"], spec, cfg, step0=8, isolation=ALL)
        a = DG.replay(m[:5], u[:5], run["ub"], run["stuck"], spec, cfg, step0=8, isolation=ALL)
        seam = seam or a["lead"][1] > 0
        c = DG.replay(m[5:], u[5:], a["ub_end"], a["stuck_end"], spec, cfg, step0=13, state=a["state"], llr=a["llr"],
                      detections=a["detections"], isolation=ALL, lead=a["lead"], voided=a["voided"], revised=a["revised"])
        assert np.array_equal(np.concatenate([a["llr_hist"], c["llr_hist"]]), whole["llr_hist"]), b
        assert np.array_equal(np.concatenate([a["fit_hist"], c["fit_hist"]]), whole["fit_hist"]), b
        for k in ("detections", "lead", "voided", "revised"):
            assert c[k] == whole[k], (b, k)
        for k in ("state", "llr", "ub_end", "stuck_end"):
            assert np.array_equal(c[k], whole[k]), (b, k)
    assert seam      # on some vehicle a leader was waiting for its confirmation at the seam


# ---------------------------------------------------------------------------------------------------------------------------
# the struct, the entries, the refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_isolation_struct_layout_matches_the_header(tmp_path):
    from ft_mpc_amd import _lib
    assert [f for f, _ in _lib.ftmpc_isolation._fields_] == FIELDS
    src = tmp_path / "layout.c"
    body = "".join(f'printf("{f} %zu\\n", offsetof(ftmpc_isolation, {f}));' for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftmpc.h"\nint main(void){printf("sizeof %zu\\n", sizeof(ftmpc_isolation));'
                   + body + 'printf("diagnosis %zu\\nenvironment %zu\\noutage %zu\\n", sizeof(ftmpc_diagnosis), sizeof(ftmpc_environment), '
                   'sizeof(ftmpc_outage));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.ftmpc_isolation) == 56
    for f, off in zip(FIELDS, OFFSETS):
        assert int(got[f]) == getattr(_lib.ftmpc_isolation, f).offset == off, f
    # no existing struct changed
    assert int(got["diagnosis"]) == C.sizeof(_lib.ftmpc_diagnosis) == 152
    assert int(got["environment"]) == C.sizeof(_lib.ftmpc_environment)
    assert int(got["outage"]) == C.sizeof(_lib.ftmpc_outage)


def test_library_exports_the_isolation_entries():
    from ft_mpc_amd import _lib
    _lib.build_library()
    lib = _lib.load_library()
    header = (ROOT / "include" / "ftmpc.h").read_text()
    for n in ("ftmpc_simulate_isolation_batch", "ftmpc_simulate_wrench_isolation_batch", "ftmpc_multi_simulate_isolation_batch"):
        assert n in _lib.SYMBOLS and getattr(lib, n) is not None
        assert f"int {n}(" in header
    assert lib.ftmpc_simulate_isolation_batch.argtypes[:-1] == lib.ftmpc_simulate_environment_batch.argtypes
    assert lib.ftmpc_simulate_wrench_isolation_batch.argtypes[:-1] == lib.ftmpc_simulate_wrench_environment_batch.argtypes
    assert lib.ftmpc_version() == 540


def test_consist_for_is_the_chi_square_6_quantile():
    for p, x in ((0.5, 5.348120627447116), (0.95, 12.591587243743977), (0.999, 22.457744484825323)):      # (published tables)
        assert abs(DG.consist_for(p) ** 2 - x) < 1e-9 * x
    assert round(CONSIST, 2) == 4.74
    with pytest.raises(ValueError):
        DG.consist_for(1.0)


def test_score_final_matches_the_last_detection_of_the_thruster():
    ev = [[(5, 2, 2)], [(5, 1, 0)]]
    det = [[(6, 2, 1), (8, 2, 2)], [(7, 3, 0)]]
    a, f = DG.score(ev, det), DG.score(ev, det, final=True)
    assert (a["wrong_level"], a["false_alarms"], a["wrong_thruster"]) == (1, 1, 1)
    assert (f["wrong_level"], f["false_alarms"], f["wrong_thruster"], f["delay"]) == (0, 0, 1, [1, 2])


def test_python_refuses_what_the_library_refuses():
    B = 5
    dg = dict(levels=LEVELS, fields=DG.FIELDS)
    ok = DG.isolation_request(dict(consist=4.7, persist=2, revise=True), B, NT, dg)
    assert ok["fields"] == DG.ISO_FIELDS and ok["revise"] is True and ok["lead"] is None
    assert DG.isolation_request(dict(), B, NT, dict(levels=LEVELS, fields=("pattern",)))["fields"] == ("voided", "revised", "fit")
    assert DG.isolation_request(dict(fields=()), B, NT, None)["persist"] == 1      # a trivial one needs no diagnosis
    lead = np.zeros((B, 2), np.int32)
    bad = [(dict(consist=-1.0), dg, "consist"), (dict(consist=np.inf), dg, "consist"), (dict(consist=np.nan), dg, "consist"),
           (dict(persist=0), dg, "persist"), (dict(persist=1.5), dg, "persist"), (dict(revise=2), dg, "revise"),
           (dict(persist=2), None, "no diagnosis"), (dict(lead=lead), dict(levels=LEVELS, fields=("pattern",)), "state"),
           (dict(fields=("lead",)), dict(levels=LEVELS, fields=("pattern",)), "state"),
           (dict(lead=lead[:3]), dg, "shape"), (dict(lead=lead - 2), dg, "leader"), (dict(lead=lead + NT * 3), dg, "leader"),
           (dict(lead=np.stack([lead[:, 0], lead[:, 1] - 1], 1)), dg, "run"), (dict(voided=np.full(B, -1)), dg, "voided"),
           (dict(revised=np.full(B, -1)), dg, "revised"), (dict(voided=np.zeros(B + 1)), dg, "voided"),
           (dict(fields=("llr",)), dg, "fields"), (dict(gate=3.0), dg, "unknown")]
    for iso, d, word in bad:
        with pytest.raises(ValueError, match=word):
            DG.isolation_request(iso, B, NT, d)
