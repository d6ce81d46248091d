"""CPU: probe pulses for silent faults and the withdrawal of a detection (include/ftmpc.h, ftmpc_probe; csrc/ftmpc_probe.h, the host /
device functions ftmpc_probe_kernel and ftmpc_diagnose_probe_kernel are made of; ft_mpc_amd/probes.py and ft_mpc_amd/diagnosis.py,
test_step / replay with probe=).

The header runs in stand-alone C++ programs with their own main, built with -fsanitize=address,undefined where the toolchain links
them (plain executables: nothing is preloaded and nothing is loaded into python), else without.
  the probe step     480 random cases (u, ub, idle, pulses, detection list, rule) with ties, capped thrusters, listed thrusters, NaN
                     commands, max_pulses reached and clipped pulses, against probes.step and probes.listed: integers exactly, the
                     command bit for bit, the impulse bit for bit
  the healthy test   7 vehicles over 36 tests with gate, confirmation and revision on, against diagnosis.test_step(probe=...) plus
                     the decision: decisions exactly, statistics and the fit to rtol 1e-12 + atol 1e-12 (the two sides differ by the
                     order of their sums and by 1 / s against a division, on values of order 1 to 1e3; the bound of
                     tests/test_isolation_host.py)
Then the refusals of probes.request, the struct's layout against gcc, the two symbols and the entry simulate(probe=...) reaches."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from ft_mpc_amd import _lib
from ft_mpc_amd import diagnosis as DG
from ft_mpc_amd import probes as PR
from test_diagnosis_host import F_MAX, NT, SIGMA, _cfg
from test_simulate_dispatch_host import DIAG, EST, _pointee, _stand_in
from test_simulate_dispatch_host import B as SB
from test_simulate_dispatch_host import T as ST
from test_outages_host import _call

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "fault-tolerant-mpc_amd" / "csrc"
LEVELS = (0.0, 1.7, F_MAX)
CONSIST = DG.consist_for(0.999)
FIELDS = ["struct_size", "reserved", "amp", "quiet", "idle_steps", "max_pulses", "reinstate", "restore_ub", "idle", "pulses", "impulse",
          "pacc", "health", "reinstated", "thruster_hist"]
OFFSETS = [0, 4, 8, 16, 24, 28, 32, 40, 48, 56, 64, 72, 80, 88, 96]
NEW = ("ftmpc_simulate_probe_batch", "ftmpc_simulate_wrench_probe_batch")


def _build(tmp_path, name, text):
    src = tmp_path / f"{name}.cpp"
    src.write_text(text)
    exe = tmp_path / name
    base = ["g++", "-std=c++17", "-O1", "-g", "-I", str(CSRC), str(src), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:
        subprocess.run(base, check=True)
    return exe


def _run(tmp_path, exe, data):
    (tmp_path / "in.bin").write_bytes(np.ascontiguousarray(data, dtype=np.float64).tobytes())
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    return np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# the probe step against probes.step
# ---------------------------------------------------------------------------------------------------------------------------
SC, SK, SL = 480, 4, 3
S_IN, S_OUT = 7 + 4 * NT + 1 + 2 * SK, 3 * NT + 2

STEP_MAIN = r"""
#include <cstdio>
#include <vector>
#include "ftmpc_probe.h"
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int C = 480, NT = 8, K = 4, NIN = 48, NOUT = 26;
    std::vector<double> in((size_t)C * NIN), out((size_t)C * NOUT);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
    std::fclose(f);
    for (int c = 0; c < C; ++c) {
        const double* v = in.data() + (size_t)c * NIN;
        ftmpc_prb::Rule R;
        R.amp = v[0], R.quiet = v[1], R.restore_ub = 0.0, R.dt = v[2];
        R.idle_steps = (int)v[3], R.max_pulses = (int)v[4], R.reinstate = (int)v[5], R.n_levels = (int)v[6];
        double u[8], ub[8];
        int idle[8], pulses[8], dth[4], dlv[4];
        for (int i = 0; i < NT; ++i) u[i] = v[7 + i], ub[i] = v[7 + NT + i], idle[i] = (int)v[7 + 2 * NT + i], pulses[i] = (int)v[7 + 3 * NT + i];
        const int cnt = (int)v[7 + 4 * NT];
        for (int k = 0; k < K; ++k) dth[k] = (int)v[8 + 4 * NT + k], dlv[k] = (int)v[8 + 4 * NT + K + k];
        ftmpc_prb::Pick p;
        ftmpc_prb::pick_start(p);
        for (int i = 0; i < NT; ++i) {
            const bool live = ub[i] > 0.0;
            const bool lst = R.reinstate != 0 && ftmpc_prb::listed(i, live, cnt, dth, dlv, R.n_levels);
            ftmpc_prb::thruster(R, i, live, lst, u[i], pulses[i], idle[i], p);
        }
        double impulse = 0.0;
        if (p.cand >= 0) {
            int id = p.idle;
            impulse = ftmpc_prb::pulse(R, ub[p.cand] > 0.0, ub[p.cand], u[p.cand], pulses[p.cand], id);
            idle[p.cand] = id;
        }
        double* o = out.data() + (size_t)c * NOUT;
        for (int i = 0; i < NT; ++i) o[i] = u[i], o[NT + i] = idle[i], o[2 * NT + i] = pulses[i];
        o[3 * NT] = p.cand, o[3 * NT + 1] = impulse;
    }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
    std::fclose(f);
    return 0;
}
"""


def _step_cases():
    rng = np.random.default_rng(2024)
    rows, refs = np.zeros((SC, S_IN)), []
    kinds = dict(pulsed=0, listed_pulse=0, capped=0, nan=0, clipped=0, none=0)
    for c in range(SC):
        amp = float(rng.choice([0.5, 0.25, 1.0]))
        quiet = float(rng.choice([0.0, 0.05, 0.2]))
        need, cap, rein = int(rng.integers(1, 5)), int(rng.choice([0, 0, 1, 2, 3])), int(rng.integers(0, 2))
        dt = float(rng.choice([0.1, 0.05]))
        ub = np.where(rng.random(NT) < 0.75, rng.choice([F_MAX, 0.3]), 0.0)
        u = np.where(rng.random(NT) < 0.6, rng.uniform(0.0, 0.06, NT), rng.uniform(0.0, F_MAX, NT))
        u = np.where(rng.random(NT) < 0.25, 0.0, u)
        if c % 9 == 0:
            u[rng.integers(0, NT)] = np.nan
        if c % 31 == 0:
            u[rng.integers(0, NT)] = np.inf
        idle = rng.integers(0, 6, NT)
        if c % 4 == 0:      # ties at the top
            idle[rng.choice(NT, 3, replace=False)] = 7
        pulses = rng.integers(0, 4, NT)
        cnt = int(rng.integers(0, SK + 1))
        dth, dlv = rng.integers(0, NT, SK), rng.integers(0, SL + 1, SK)      # (level SL: a reinstatement)
        if cnt and c % 3 == 0:      # an off thruster that is listed, and an entry that a newer one overrides
            off = np.flatnonzero(ub == 0)
            if off.size:
                dth[cnt - 1], dlv[cnt - 1] = off[0], rng.integers(0, SL)
        det = [(k, int(dth[k]), int(dlv[k])) for k in range(cnt)]
        rows[c] = np.r_[amp, quiet, dt, need, cap, rein, SL, u, ub, idle, pulses, cnt, dth, dlv]
        lst = PR.listed(ub, det, SL)
        spec = dict(amp=amp, quiet=quiet, idle_steps=need, max_pulses=cap, reinstate=bool(rein))
        r = PR.step(u, ub, idle, pulses, lst, spec, dt)
        refs.append(r)
        j = r["thruster"]
        kinds["none" if j < 0 else "pulsed"] += 1
        if j >= 0:
            kinds["listed_pulse"] += int(not ub[j] > 0)
            kinds["clipped"] += int(ub[j] > 0 and r["u"][j] == ub[j])
        kinds["nan"] += int(np.isnan(u).any())
        kinds["capped"] += int(cap > 0 and (pulses >= cap).any())
    return rows, refs, kinds


def test_header_probe_step_is_probes_step(tmp_path):
    """480 random cases; integers exactly, the command and the impulse bit for bit."""
    rows, refs, kinds = _step_cases()
    assert rows.shape[1] == 48 and S_OUT == 26
    got = _run(tmp_path, _build(tmp_path, "probe_step", STEP_MAIN), rows).reshape(SC, S_OUT)
    ties = 0
    for c, r in enumerate(refs):
        o = got[c]
        assert np.array_equal(o[:NT].view(np.uint64), r["u"].view(np.uint64)), (c, o[:NT], r["u"])
        assert np.array_equal(o[NT:2 * NT], r["idle"]) and np.array_equal(o[2 * NT:3 * NT], r["pulses"]), c
        assert int(o[3 * NT]) == r["thruster"], (c, o[3 * NT], r["thruster"])
        assert np.float64(o[3 * NT + 1]).view(np.uint64) == np.float64(r["impulse"]).view(np.uint64), c
        # a tie at the top among the candidates went to the lowest index
        j = r["thruster"]
        if j >= 0:
            idle_before = rows[c, 7 + 2 * NT:7 + 3 * NT] + 1
            cap, need = rows[c, 4], rows[c, 3]
            ub, u = rows[c, 7 + NT:7 + 2 * NT], rows[c, 7:7 + NT]
            same = [i for i in range(NT) if i != j and r["idle"][i] == idle_before[j] and r["idle"][i] >= need
                    and (cap == 0 or rows[c, 7 + 3 * NT + i] < cap)]
            if same:
                ties += 1
                assert min(same) > j, (c, j, same)
    print(f"probe step: {kinds}, ties at the top {ties}")
    assert kinds["pulsed"] > 100 and kinds["none"] > 20 and kinds["listed_pulse"] > 5 and kinds["nan"] > 20 and kinds["capped"] > 50
    assert kinds["clipped"] > 0 and ties > 5


def test_step_rules_one_by_one():
    spec = dict(amp=0.5, quiet=0.05, idle_steps=3)
    ub = np.array([F_MAX, F_MAX, 0.0, 0.0, F_MAX, 0.2, F_MAX, F_MAX])
    lst = np.array([0, 0, 1, 0, 0, 0, 0, 0], bool)
    u = np.array([0.0, 1.0, 0.7, 0.0, np.nan, 0.01, 0.049, 0.05])
    idle = np.array([2, 9, 2, 9, 9, 1, 2, 9])
    r = PR.step(u, ub, idle, np.zeros(NT, int), lst, spec, 0.1)
    # live and quiet counts; commanded, NaN and exactly `quiet` reset; off thrusters reset without reinstate; the lowest index of 0 and 6
    assert r["idle"].tolist() == [0, 0, 0, 0, 0, 2, 3, 0] and r["thruster"] == 0 and r["u"][0] == 0.5 and r["pulses"][0] == 1
    assert r["impulse"] == 0.5 * 0.1 and np.isnan(r["u"][4]) and np.array_equal(np.delete(r["u"], [0, 4]), np.delete(u, [0, 4]))
    # with reinstate the listed thruster counts whatever the solve commands on it (e = 0), wins with the largest counter, gets amp
    r = PR.step(u, ub, np.array([2, 9, 5, 9, 9, 1, 2, 9]), np.zeros(NT, int), lst, dict(spec, reinstate=True), 0.1)
    assert r["thruster"] == 2 and r["u"][2] == 0.5 and r["impulse"] == 0.5 * 0.1 and r["idle"][2] == 0 and r["idle"][3] == 0
    # the cap counts what is carried in; a pulse on a degraded thruster is clipped to its bound
    r = PR.step(u, ub, idle, np.array([1, 0, 0, 0, 0, 0, 0, 0]), lst, dict(spec, max_pulses=1), 0.1)
    assert r["thruster"] == 6 and r["idle"][0] == 3
    r = PR.step(u, ub, np.array([0, 0, 0, 0, 0, 8, 0, 0]), np.zeros(NT, int), lst, spec, 0.1)
    assert r["thruster"] == 5 and r["u"][5] == 0.2 and r["impulse"] == (0.2 - 0.01) * 0.1
    # listed: off, and the newest entry below n_levels
    assert PR.listed(ub, [(1, 2, 0), (4, 3, 1), (6, 3, 3), (7, 0, 1)], 3).tolist() == [False, False, True, False, False, False, False, False]


def test_replay_follows_step_and_refuses_a_clipped_pulse():
    rng = np.random.default_rng(5)
    steps = 40
    spec = dict(amp=0.5, quiet=0.05, idle_steps=3, max_pulses=4, reinstate=True)
    ub = np.array([F_MAX, F_MAX, 0.0, F_MAX, 0.0, F_MAX, F_MAX, F_MAX])
    lst = np.array([0, 0, 1, 0, 0, 0, 0, 0], bool)
    solved = np.where(rng.random((steps, NT)) < 0.5, 0.0, rng.uniform(0, 2.0, (steps, NT)))
    idle, pulses, imp = np.zeros(NT, int), np.zeros(NT, int), 0.0
    cmd, th = np.empty((steps, NT)), np.empty(steps, int)
    for t in range(steps):
        r = PR.step(solved[t], ub, idle, pulses, lst, spec, 0.1)
        idle, pulses, imp, cmd[t], th[t] = r["idle"], r["pulses"], imp + r["impulse"], r["u"], r["thruster"]
    ubh, lh = np.tile(ub, (steps, 1)), np.tile(lst, (steps, 1))
    for kw in (dict(), dict(solved=solved)):
        rp = PR.replay(cmd, th, ubh, lh, spec, 0.1, **kw)
        assert np.array_equal(rp["thruster_hist"], th) and np.array_equal(rp["idle"], idle) and np.array_equal(rp["pulses"], pulses)
        assert abs(rp["impulse"] - imp) <= 1e-12 * imp
    assert (th >= 0).sum() >= 8 and (th == 2).sum() == 4 and pulses.max() == 4
    a = PR.replay(cmd[:17], th[:17], ubh[:17], lh[:17], spec, 0.1)
    b = PR.replay(cmd[17:], th[17:], ubh[17:], lh[17:], spec, 0.1, idle=a["idle"], pulses=a["pulses"], impulse=a["impulse"])
    assert np.array_equal(b["idle"], idle) and np.array_equal(b["pulses"], pulses) and abs(b["impulse"] - imp) <= 1e-12 * imp
    wrong = th.copy()
    wrong[np.flatnonzero(th < 0)[0]] = 1      # a pulse the rule did not make shows as a mismatch
    assert not np.array_equal(PR.replay(cmd, wrong, ubh, lh, spec, 0.1)["thruster_hist"], wrong)
    low = np.full(NT, 0.2)
    r = PR.step(np.zeros(NT), low, np.full(NT, 5), np.zeros(NT, int), np.zeros(NT, bool), spec, 0.1)
    with pytest.raises(ValueError, match="clipped"):
        PR.replay(r["u"][None], [r["thruster"]], low[None], None, spec, 0.1)


# ---------------------------------------------------------------------------------------------------------------------------
# the healthy hypothesis against test_step(probe=...) plus the decision
# ---------------------------------------------------------------------------------------------------------------------------
HB, HT, HL, HK = 7, 36, 3, 4
HH = NT * HL
N_HEAD, N_VEH, N_IN, N_OUT = 71, 2 * NT + 1 + 3 * HK, 13 + 13 + 1 + 2 * NT + 1, HH + NT + 2 + 5
RESTORE = 2.9

TEST_MAIN = r"""
#include <cstdio>
#include <vector>
#include "ftmpc_probe.h"
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int B = 7, T = 36, NT = 8, L = 3, H = 24, K = 4;
    const int NHEAD = 71, NVEH = 29, NIN = 44, NOUT = 39;
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
    R.L = L, R.persist = (int)hd[69], R.revise = 1, R.pad0 = 0;
    ftmpc_prb::Rule PRB;
    PRB.amp = 0.5, PRB.quiet = 0.05, PRB.restore_ub = hd[70], PRB.dt = dt;
    PRB.idle_steps = 3, PRB.max_pulses = 0, PRB.reinstate = 1, PRB.n_levels = L;
    std::vector<double> ub((size_t)B * NT), stuck((size_t)B * NT), llr((size_t)B * H, 0.0), health((size_t)B * NT, 0.0);
    std::vector<int> cnt(B), det((size_t)B * 3 * K), lead(B, -1), run(B, 0), voided(B, 0), revised(B, 0), reinstated(B, 0);
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
            const double* pacc = v + 27 + NT;
            const int c = (int)v[27 + 2 * NT];
            double* o = out.data() + ((size_t)t * B + b) * NOUT;
            double* s = llr.data() + (size_t)b * H;
            double* hs = health.data() + (size_t)b * NT;
            double* vub = ub.data() + (size_t)b * NT;
            double* vst = stuck.data() + (size_t)b * NT;
            int* dstep = det.data() + (size_t)b * 3 * K;
            o[H + NT] = o[H + NT + 1] = -1.0;
            for (int k = 0; k < 5; ++k) o[H + NT + 2 + k] = 0.0;
            if (cnt[b] < K) {
                ftmpc_iso::Resid r;
                ftmpc_iso::residual(xt, y, n, rsq, dsq, r);
                ftmpc_iso::Scan sc;
                ftmpc_iso::scan_start(R, sc);
                ftmpc_prb::Lead hl;
                ftmpc_prb::lead_start(R, hl);
                for (int i = 0; i < NT; ++i) {
                    const bool live = vub[i] > 0.0;
                    const bool lst = ftmpc_prb::listed(i, live, cnt[b], dstep + K, dstep + 2 * K, L);
                    const double d[6] = {D[i], D[NT + i], D[2 * NT + i], D[3 * NT + i], D[4 * NT + i], D[5 * NT + i]};
                    double gh[6];
                    ftmpc_iso::unit_signature(dt, inv_mass, Jinv, d, gh);
                    ftmpc_iso::thruster(R, r, n, i, live, lst, acc[i], vst[i], gh, s + i * L, 1, o + i * L, sc);
                    ftmpc_prb::healthy(R, r, n, i, lst, pacc[i], vst[i], gh, hs + i, sc, hl);
                    o[H + i] = hs[i];
                }
                ftmpc_prb::merge(hl, H, sc);
                if (sc.eligible > 0) o[H + NT] = r.q0, o[H + NT + 1] = sc.qmin;
                const bool vd = ftmpc_iso::is_void(R, r, sc);
                voided[b] += vd ? 1 : 0;
                o[H + NT + 2] = vd ? 1.0 : 0.0;
                o[H + NT + 3] = sc.besth;
                if (ftmpc_iso::confirm(R, sc, lead[b], run[b])) {
                    if (sc.besth >= H) {
                        ftmpc_prb::reinstate(PRB, sc.besth - H, c, cnt[b], vub, vst, dstep, dstep + K, dstep + 2 * K);
                        for (int k = 0; k < H; ++k) s[k] = 0.0;
                        lead[b] = -1, run[b] = 0;
                        reinstated[b] += 1;
                    } else {
                        revised[b] += ftmpc_iso::decide(R, sc.besth, c, cnt[b], H, vub, vst, dstep, dstep + K, dstep + 2 * K, s, 1, lead[b], run[b]);
                    }
                    for (int i = 0; i < NT; ++i) hs[i] = 0.0;
                    cnt[b] += 1;
                    o[H + NT + 6] = 1.0;
                }
                o[H + NT + 4] = lead[b];
                o[H + NT + 5] = run[b];
            } else {
                for (int k = 0; k < H; ++k) o[k] = s[k];
                for (int i = 0; i < NT; ++i) o[H + i] = hs[i];
                o[H + NT + 3] = -1.0, o[H + NT + 4] = lead[b], o[H + NT + 5] = run[b];
            }
        }
    for (int b = 0; b < B; ++b) {
        double* o = out.data() + (size_t)T * B * NOUT + (size_t)b * NOUT;
        for (int i = 0; i < NT; ++i) o[i] = ub[(size_t)b * NT + i], o[NT + i] = stuck[(size_t)b * NT + i];
        for (int k = 0; k < 3 * K; ++k) o[2 * NT + k] = det[(size_t)b * 3 * K + k];
        o[2 * NT + 3 * K] = cnt[b], o[2 * NT + 3 * K + 1] = voided[b], o[2 * NT + 3 * K + 2] = revised[b], o[2 * NT + 3 * K + 3] = reinstated[b];
    }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
    std::fclose(f);
    return 0;
}
"""


def _spec(**kw):
    return dict(dict(every=1, levels=LEVELS, resid_sigma=DG.default_sigma(SIGMA), drift_sigma=(0.0, 0.0), threshold=18.0, max_detect=HK),
                **kw)


def test_header_healthy_test_is_test_step_with_probe_plus_the_decision(tmp_path):
    """7 vehicles, 36 tests, gate 4.74, persist 2, revise, three levels, max_detect 4, restore_ub 2.9.  A listed thruster gets a 0.5 N
    pulse in every third test's window.  Vehicles 0-2: thruster b listed as dead, the plant healthy (it delivers the pulses):
    reinstated.  Vehicles 3-4: listed as dead and dead: nothing is withdrawn, the health statistic stays 0.  Vehicle 5: thruster 5
    listed at 1.7 N and never pulsed while the plant delivers nothing: "dead" (level 0) and "healthy" tie exactly, the level wins and
    the thruster is revised, not reinstated.  Vehicle 6: thruster 6 sticks at 3.4 N from test 8 on: detected, then pulsed, not
    withdrawn.  The residual of every test is the signature of what the plant delivers beyond the model's pattern as it stands on
    the Python side, plus noise, so both sides walk through the same decisions."""
    from ft_mpc_amd.estimators import _body_to_inertial, _cfg_model
    cfg = _cfg()
    D, m, J = _cfg_model(cfg)
    spec = _spec(resid_sigma=(2e-3, 2e-3))      # (one pulse on the weakest thruster, 0 or 7, then adds 15 to its statistic)
    iso = dict(consist=CONSIST, persist=2, revise=True)
    probe = dict(reinstate=True, restore_ub=RESTORE)
    lv = np.array(LEVELS)
    rs = np.asarray(spec["resid_sigma"])
    rng = np.random.default_rng(43)
    gv, gw = (cfg.dt / m) * D[0:3].T, cfg.dt * np.linalg.solve(J, D[3:6]).T
    head = np.concatenate([[cfg.dt, 1.0 / m], np.linalg.inv(J).reshape(-1), D.reshape(-1), np.r_[lv, 0.0], rs ** 2, [0.0, 0.0],
                           [spec["threshold"], CONSIST ** 2, iso["persist"], RESTORE]])
    assert head.size == N_HEAD and N_VEH == 29 and N_IN == 44 and N_OUT == 39
    ub, stuck = np.full((HB, NT), F_MAX), np.zeros((HB, NT))
    det = [[] for _ in range(HB)]
    for b in range(5):
        ub[b, b] = 0.0
        det[b].append((0, b, 0))
    ub[5, 5], stuck[5, 5] = 0.0, 1.7
    det[5].append((0, 5, 1))
    dead = {3: 3, 4: 4, 5: 5}                                # vehicle: the thruster that delivers nothing, whatever is commanded
    veh = np.full((HB, N_VEH), -1.0)
    for b in range(HB):
        veh[b, :2 * NT + 1] = np.r_[ub[b], stuck[b], len(det[b])]
        for k, d in enumerate(det[b]):
            veh[b, 2 * NT + 1 + k], veh[b, 2 * NT + 1 + HK + k], veh[b, 2 * NT + 1 + 2 * HK + k] = d
    llr, health = np.zeros((HB, NT, HL)), np.zeros((HB, NT))
    lead = [(-1, 0)] * HB
    voided, revised, reinstated = np.zeros(HB, int), np.zeros(HB, int), np.zeros(HB, int)
    rows, ref = np.empty((HT, HB, N_IN)), np.zeros((HT, HB, N_OUT))
    tie_seen = False
    for t in range(HT):
        for b in range(HB):
            xt = np.concatenate([rng.normal(size=6), rng.normal(size=4), 0.3 * rng.normal(size=3)])
            xt[6:10] /= np.linalg.norm(xt[6:10])
            n = float(1 + (t + b) % 3)
            acc = n * rng.uniform(0.0, 0.4 * F_MAX, size=NT)
            lst = PR.listed(ub[b], det[b], HL)
            pacc = np.where(lst & (t % 3 == 0) & (b != 5), 0.5, 0.0) + np.where(lst, 0.0, rng.uniform(0, 1, NT))   # (ignored where not listed)
            model = np.where(ub[b] > 0, acc, n * stuck[b])
            true = np.where(ub[b] > 0, acc, pacc)                  # a healthy thruster delivers what is applied to it
            if b in dead:
                true[dead[b]] = 0.0
            if b == 6 and t >= 8:
                true[6] = n * F_MAX
            extra = true - model
            dv, dw = gv.T @ extra + rs[0] * rng.normal(size=3), gw.T @ extra + rs[1] * rng.normal(size=3)
            y = xt.copy()
            y[3:6] += _body_to_inertial(xt[6:10]) @ dv
            y[10:13] += dw
            rows[t, b] = np.r_[y, xt, n, acc, pacc, 100 + t]
            o = ref[t, b]
            o[HH + NT:HH + NT + 2] = -1.0
            if len(det[b]) < HK:
                r = DG.test_step(llr[b], y, xt, n, acc, ub[b], spec, cfg, isolation=iso, lead=lead[b], stuck=stuck[b],
                                 listed=np.flatnonzero(lst), probe=probe, pacc=pacc, health=health[b])
                o[:HH], o[HH:HH + NT] = r["llr"].reshape(-1), r["health"]
                if not np.isnan(r["qmin"]):
                    o[HH + NT:HH + NT + 2] = r["q0"], r["qmin"]
                voided[b] += r["void"]
                if b == 5 and lst[5]:
                    tie_seen = tie_seen or r["health"][5] == r["llr"][5, 0] > 0
                llr[b], health[b], lead[b] = r["llr"], r["health"], r["lead"]
                if r["decide"]:
                    if r["leader"] >= HH:
                        i = r["leader"] - HH
                        det[b].append((100 + t, i, HL))
                        ub[b, i], stuck[b, i] = RESTORE, 0.0
                        reinstated[b] += 1
                    else:
                        i, l = divmod(r["leader"], HL)
                        det[b].append((100 + t, i, l))
                        revised[b] += int(not ub[b, i] > 0)
                        ub[b, i], stuck[b, i] = 0.0, lv[l]
                    llr[b], health[b], lead[b] = 0.0, 0.0, (-1, 0)
                o[HH + NT + 2:] = r["void"], r["leader"], lead[b][0], lead[b][1], r["decide"]
            else:
                o[:HH], o[HH:HH + NT] = llr[b].reshape(-1), health[b]
                o[HH + NT + 3:HH + NT + 6] = -1, lead[b][0], lead[b][1]
    data = np.concatenate([head, veh.reshape(-1), rows.reshape(-1)])
    got = _run(tmp_path, _build(tmp_path, "probe_test", TEST_MAIN), data)
    steps, fin = got[:HT * HB * N_OUT].reshape(HT, HB, N_OUT), got[HT * HB * N_OUT:].reshape(HB, N_OUT)
    np.testing.assert_allclose(steps[:, :, :HH + NT + 2], ref[:, :, :HH + NT + 2], rtol=1e-12, atol=1e-12)
    assert np.array_equal(steps[:, :, HH + NT + 2:], ref[:, :, HH + NT + 2:])
    K0 = 2 * NT
    for b in range(HB):
        assert np.array_equal(fin[b, :NT], ub[b]) and np.array_equal(fin[b, NT:2 * NT], stuck[b]), b
        got_det = [(int(fin[b, K0 + k]), int(fin[b, K0 + HK + k]), int(fin[b, K0 + 2 * HK + k])) for k in range(int(fin[b, K0 + 3 * HK]))]
        assert got_det == det[b], (b, got_det, det[b])
        assert tuple(fin[b, K0 + 3 * HK + 1:K0 + 3 * HK + 4]) == (voided[b], revised[b], reinstated[b]), b
    print(f"healthy test: detections {det}, voided {voided}, revised {revised}, reinstated {reinstated}")
    # the case exercises what it says
    for b in range(3):
        assert reinstated[b] == 1 and det[b][1][1:] == (b, HL) and ub[b, b] == RESTORE and stuck[b, b] == 0.0, (b, det[b])
        assert ub[b].tolist().count(RESTORE) == 1 and (np.delete(ub[b], b) == F_MAX).all()
    for b in (3, 4):
        assert reinstated[b] == 0 and det[b] == [(0, b, 0)] and (ref[:, b, HH:HH + NT] == 0).all()
    assert tie_seen and reinstated[5] == 0 and revised[5] == 1 and det[5][1][1:] == (5, 0) and stuck[5, 5] == 0.0 and ub[5, 5] == 0.0
    assert reinstated[6] == 0 and det[6][0][1] == 6 and stuck[6, 6] == F_MAX and ub[6, 6] == 0.0
    assert (ref[:, :3, HH + NT + 5] == 1).any()      # a healthy hypothesis that waited for its confirmation


def test_without_a_reinstating_probe_test_step_and_replay_are_what_they_were():
    from test_diagnosis_host import _open_loop
    from test_diagnosis_host import _spec as spec2
    cfg = _cfg()
    run = _open_loop("stuck_on")
    iso = dict(consist=CONSIST, persist=2, revise=True)
    for b in range(0, run["B"], 9):
        for kw in (dict(), dict(isolation=iso)):
            a = DG.replay(run["meas"][:, b], run["u"], run["ub"], run["stuck"], spec2(), cfg, **kw)
            r = DG.replay(run["meas"][:, b], run["u"], run["ub"], run["stuck"], spec2(), cfg, probe=dict(amp=0.5, reinstate=False), **kw)
            assert sorted(a) == sorted(r) and a["detections"] == r["detections"] and a["detections"]
            for k in ("llr_hist", "ub", "stuck", "state", "llr", "fit_hist"):
                assert np.array_equal(a[k], r[k]), (b, k)
        # a reinstating probe on a run without a listed thruster before the detection: the same statistics up to it
        p = DG.replay(run["meas"][:, b], run["u"], run["ub"], run["stuck"], spec2(), cfg, probe=dict(reinstate=True, restore_ub=F_MAX))
        a = DG.replay(run["meas"][:, b], run["u"], run["ub"], run["stuck"], spec2(), cfg)
        t0 = a["detections"][0][0]
        assert p["detections"][0] == a["detections"][0] and np.array_equal(p["llr_hist"][:t0 + 1], a["llr_hist"][:t0 + 1])
        assert (p["health_hist"][:t0 + 1] == 0).all() and p["listed"][t0:, a["detections"][0][1]].all()


def test_pattern_and_score_read_a_reinstatement():
    ub, stuck = np.full(NT, F_MAX), np.zeros(NT)
    det = [(3, 2, 1), (5, 4, 0), (9, 2, 3)]
    u2, s2 = DG.pattern(ub, stuck, det, LEVELS, restore_ub=2.0)
    assert u2[2] == 2.0 and s2[2] == 0.0 and u2[4] == 0.0 and (np.delete(u2, [2, 4]) == F_MAX).all()
    assert DG.pattern(ub, stuck, det[:2], LEVELS)[1][2] == 1.7      # (an existing call: as before)
    with pytest.raises(ValueError, match="restore_ub"):
        DG.pattern(ub, stuck, det, LEVELS)
    ev = [[(4, 4, 0)]]
    plain = DG.score(ev, [det[:2]])
    assert plain == dict(delay=[1], missed=0, wrong_thruster=0, wrong_level=0, false_alarms=1)
    got = DG.score(ev, [det], n_levels=3)
    assert got == dict(delay=[1], missed=0, wrong_thruster=0, wrong_level=0, false_alarms=0, withdrawn=1)
    # a true detection that was withdrawn is a miss
    assert DG.score([[(2, 2, 1)]], [[(3, 2, 1), (9, 2, 3)]], n_levels=3)["missed"] == 1


# ---------------------------------------------------------------------------------------------------------------------------
# the struct, the entries, the refusals, the dispatch
# ---------------------------------------------------------------------------------------------------------------------------
def test_probe_struct_layout_matches_the_header(tmp_path):
    assert [f for f, _ in _lib.ftmpc_probe._fields_] == FIELDS
    src = tmp_path / "layout.c"
    body = "".join(f'printf("{f} %zu\\n", offsetof(ftmpc_probe, {f}));' for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftmpc.h"\nint main(void){printf("sizeof %zu\\n", sizeof(ftmpc_probe));'
                   + body + 'printf("diagnosis %zu\\nisolation %zu\\n", sizeof(ftmpc_diagnosis), sizeof(ftmpc_isolation));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.ftmpc_probe) == 104
    for f, off in zip(FIELDS, OFFSETS):
        assert int(got[f]) == getattr(_lib.ftmpc_probe, f).offset == off, f
    # no existing struct changed
    assert int(got["diagnosis"]) == C.sizeof(_lib.ftmpc_diagnosis) == 152 and int(got["isolation"]) == C.sizeof(_lib.ftmpc_isolation) == 56


def test_library_exports_the_probe_entries():
    _lib.build_library()
    lib = _lib.load_library()
    header = (ROOT / "include" / "ftmpc.h").read_text()
    for n in NEW:
        assert n in _lib.SYMBOLS and getattr(lib, n) is not None
        assert f"int {n}(" in header
    assert lib.ftmpc_simulate_probe_batch.argtypes[:-1] == lib.ftmpc_simulate_isolation_batch.argtypes
    assert lib.ftmpc_simulate_wrench_probe_batch.argtypes[:-1] == lib.ftmpc_simulate_wrench_isolation_batch.argtypes
    assert lib.ftmpc_simulate_probe_batch.argtypes[-1] == C.POINTER(_lib.ftmpc_probe)


def test_python_refuses_what_the_library_refuses():
    nb = 5
    dg = dict(levels=LEVELS, fields=DG.FIELDS)
    nostate = dict(levels=LEVELS, fields=("pattern",))
    good = dict(amp=0.5, quiet=0.05, idle_steps=3)
    ok = PR.request(good, nb, 10, NT, dg)
    assert ok["fields"] == PR.FIELDS and ok["reinstate"] is False and ok["max_pulses"] == 0 and ok["idle"] is None
    assert PR.request(good, nb, 10, NT, nostate)["fields"] == ("thruster_hist", "idle", "pulses", "impulse", "reinstated")
    ints, dbl = np.zeros((nb, NT), np.int32), np.zeros((nb, NT))
    r = PR.request(dict(good, reinstate=True, restore_ub=F_MAX, idle=ints, pacc=dbl, reinstated=np.zeros(nb)), nb, 10, NT, dg)
    assert r["idle"] is not ints and r["idle"].dtype == np.int32 and r["pacc"] is not dbl and r["reinstated"].dtype == np.int32
    nan = dbl.copy()
    nan[2, 1] = np.nan
    bad = [(good, None, "no diagnosis"), (dict(good, amp=0.0), dg, "amp"), (dict(good, amp=np.inf), dg, "amp"),
           (dict(quiet=0.0, idle_steps=3), dg, "amp"), (dict(good, quiet=-0.1), dg, "quiet"), (dict(good, quiet=0.5), dg, "quiet"),
           (dict(good, quiet=np.nan), dg, "quiet"), (dict(good, idle_steps=0), dg, "idle_steps"), (dict(amp=0.5), dg, "idle_steps"),
           (dict(good, idle_steps=2.5), dg, "idle_steps"), (dict(good, max_pulses=-1), dg, "max_pulses"),
           (dict(good, reinstate=2), dg, "reinstate"), (dict(good, reinstate=True), dg, "restore_ub"),
           (dict(good, reinstate=True, restore_ub=0.0), dg, "restore_ub"), (dict(good, reinstate=True, restore_ub=np.inf), dg, "restore_ub"),
           (dict(good, idle=ints - 1), dg, "idle"), (dict(good, pulses=ints - 1), dg, "pulses"), (dict(good, idle=ints[:3]), dg, "idle"),
           (dict(good, impulse=np.full(nb, -1.0)), dg, "impulse"), (dict(good, impulse=np.full(nb, np.nan)), dg, "impulse"),
           (dict(good, pacc=dbl - 1), dg, "pacc"), (dict(good, pacc=nan), dg, "pacc"), (dict(good, health=nan), dg, "health"),
           (dict(good, health=dbl - 1), dg, "health"), (dict(good, reinstated=np.full(nb, -1)), dg, "reinstated"),
           (dict(good, pacc=dbl), nostate, r"ftmpc_probe.pacc without ftmpc_diagnosis.state"),
           (dict(good, health=dbl), nostate, r"ftmpc_probe.health without ftmpc_diagnosis.state"),
           (dict(good, fields=("health",)), nostate, "state"), (dict(good, fields=("llr",)), dg, "fields"),
           (dict(good, pause=3), dg, "unknown")]
    for spec, d, word in bad:
        with pytest.raises(ValueError, match=word):
            PR.request(spec, nb, 10, NT, d)
    # the two checks a reinstating probe widens, and only it
    K = 2
    det = (np.array([[0, -1]] * nb), np.array([[3, -1]] * nb), np.array([[len(LEVELS), -1]] * nb))
    carried = dict(levels=LEVELS, resid_sigma=(1e-2, 1e-2), threshold=18.0, max_detect=K, state=np.zeros((nb, 14 + NT)), detect=det)
    with pytest.raises(ValueError, match="level outside"):
        DG.request(carried, nb, 10, NT)
    assert DG.request(carried, nb, 10, NT, reinstating=True)["detect"][2][0, 0] == len(LEVELS)
    lead = np.zeros((nb, 2), np.int32)
    lead[:, 0] = NT * len(LEVELS) + 3
    with pytest.raises(ValueError, match="leader"):
        DG.isolation_request(dict(lead=lead), nb, NT, dg)
    assert DG.isolation_request(dict(lead=lead), nb, NT, dg, reinstating=True)["lead"][0, 0] == NT * len(LEVELS) + 3
    with pytest.raises(ValueError, match="leader"):
        DG.isolation_request(dict(lead=lead + NT), nb, NT, dg, reinstating=True)


PROBE = dict(amp=0.5, quiet=0.05, idle_steps=3, reinstate=True, restore_ub=F_MAX, fields=("thruster_hist", "pulses", "impulse", "health"))


@pytest.mark.parametrize("wrench", [False, True])
@pytest.mark.parametrize("with_isolation", [False, True])
def test_probe_reaches_its_entry_with_the_struct_last(wrench, with_isolation):
    kw = dict(diagnosis=dict(DIAG, rebuild_hull=True) if wrench else DIAG)
    if with_isolation:
        kw["isolation"] = dict(persist=2)
    obj, rec, real = _stand_in()
    out = _call(obj, False, wrench, probe=PROBE, **kw)
    assert len(rec.calls) == 1
    name, got = rec.calls[0]
    assert name == ("ftmpc_simulate_wrench_probe_batch" if wrench else "ftmpc_simulate_probe_batch")
    assert len(got) == len(getattr(real, name).argtypes)
    pb = _pointee(got[-1])
    assert isinstance(pb, _lib.ftmpc_probe) and pb.struct_size == 104 and pb.reserved == 0
    assert (pb.amp, pb.quiet, pb.idle_steps, pb.max_pulses, pb.reinstate, pb.restore_ub) == (0.5, 0.05, 3, 0, 1, F_MAX)
    assert bool(pb.thruster_hist) and bool(pb.pulses) and bool(pb.impulse) and bool(pb.health) and not pb.idle and not pb.pacc
    assert not pb.reinstated
    if with_isolation:
        assert isinstance(_pointee(got[-2]), _lib.ftmpc_isolation) and _pointee(got[-2]).persist == 2
    else:
        assert got[-2] is None
    assert got[-3] is None and got[-4] is None                                   # no environment, no outage
    assert sorted(out["probe"]) == ["health", "impulse", "pulses", "thruster_hist"]
    assert out["probe"]["thruster_hist"].shape == (ST, SB) and out["probe"]["thruster_hist"].dtype == np.int32
    assert out["probe"]["pulses"].shape == (SB, NT) and out["probe"]["health"].shape == (SB, NT)


def test_without_probe_the_entry_is_the_one_chosen_today_and_the_driver_refuses_a_probe():
    obj, rec, _ = _stand_in()
    out = _call(obj, False, False, diagnosis=DIAG, isolation=dict(persist=2))
    assert rec.calls[0][0] == "ftmpc_simulate_isolation_batch" and "probe" not in out
    obj, rec, _ = _stand_in()
    _call(obj, False, True, diagnosis=dict(DIAG, rebuild_hull=True))
    assert rec.calls[0][0] == "ftmpc_simulate_wrench_diagnosis_batch"
    obj, rec, _ = _stand_in()
    _call(obj, False, False, estimator=EST)
    assert rec.calls[0][0] == "ftmpc_simulate_estimator_batch"
    for wrench in (False, True):
        obj, rec, _ = _stand_in()
        with pytest.raises(ValueError, match="MultiGPUMPC is not built"):
            _call(obj, True, wrench, diagnosis=dict(DIAG, rebuild_hull=True) if wrench else DIAG, probe=PROBE)
        assert not rec.calls
    obj, rec, _ = _stand_in()
    with pytest.raises(ValueError, match="no diagnosis"):
        _call(obj, False, False, probe=PROBE)
    with pytest.raises(ValueError, match="the diagnosis' state"):
        _call(obj, False, False, diagnosis=dict(DIAG, fields=("pattern",)), probe=dict(PROBE, fields=("health",)))
