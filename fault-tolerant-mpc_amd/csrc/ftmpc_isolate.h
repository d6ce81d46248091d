// One vehicle's diagnosis test with the three safeguards of ftmpc_isolation (ftmpc_diagnose_iso_kernel, csrc/ftmpc_sim.hip;
// include/ftmpc.h, ftmpc_isolation), as host / device functions so that a plain C++ program can run what the kernel runs
// (tests/test_isolation_host.py).
//
// The test of campaign step c on the residual of ftmpc_diagnose_kernel (rho_v, r_w, s_v, s_w, the signatures a_v(h), a_w(h), z_h):
//     fit        q_0 = |rho_v|^2 / s_v + |r_w|^2 / s_w, q_h = q_0 - 2 z_h: the normalised energy left once h's signature is
//                subtracted.  With consist > 0 hypothesis h is counted only where q_h <= consist^2: llr_h = max(0, llr_h + z_h);
//                one that is not counted keeps its value.  The test is void when q_0 > consist^2 and nothing was counted
//     eligible   (i, l) of a live thruster, delta = n levels[l] - acc_i; with revise also (i, l) of a thruster that is off and
//                stands in the vehicle's own detection list, delta = n (levels[l] - stuck_i).  Every other statistic is 0
//     leader     the largest statistic strictly above the threshold, the lowest index on a tie; the same leader as at the last
//                test: run + 1, another: run = 1, none: lead = -1, run = 0.  The decision is taken when run >= persist
//     decision   a detection entry (c, i, l), stuck_i = levels[l], every statistic, lead and run reset; a live thruster is switched
//                off (ub_i = 0), a revision leaves ub_i = 0 and counts in `revised`
// The caller's thruster loop stays rolled: thruster() handles one thruster with the levels unrolled and carries the arg-max, the
// smallest q_h and the counts in Scan; no array is indexed by the thruster.
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FTMPC_ISO_HD __host__ __device__ __forceinline__
#else
#define FTMPC_ISO_HD inline
#endif

namespace ftmpc_iso {

// what is uniform over the call
struct Rule {
    double levels[4];
    double threshold;
    double consist_sq;      // consist^2; 0: no gate
    int L, persist, revise, pad0;
};

// the whitened residual of one vehicle's test
struct Resid {
    double rv0, rv1, rv2, rw0, rw1, rw2;
    double isv, isw;        // 1 / s_v, 1 / s_w
    double q0;
};

// what the thruster loop carries
struct Scan {
    double best;            // the threshold, then the leader's statistic
    int besth;              // -1: no leader
    double qmin;            // the smallest q_h of the eligible hypotheses (valid where eligible > 0)
    int eligible, counted;
};

// rho_v = M(q~)' (y_v - v~), r_w = y_w - w~ against the prediction xt [13]; rsq, dsq [2]: resid_sigma^2, drift_sigma^2
FTMPC_ISO_HD void residual(const double* xt, const double* y, double n, const double* rsq, const double* dsq, Resid& r) {
    const double qx = xt[6], qy = xt[7], qz = xt[8], qw = xt[9];
    const double R00 = qx * qx - qy * qy - qz * qz + qw * qw, R01 = 2 * (qx * qy + qz * qw), R02 = 2 * (qx * qz - qy * qw);
    const double R10 = 2 * (qx * qy - qz * qw), R11 = -qx * qx + qy * qy - qz * qz + qw * qw, R12 = 2 * (qy * qz + qx * qw);
    const double R20 = 2 * (qx * qz + qy * qw), R21 = 2 * (qy * qz - qx * qw), R22 = -qx * qx - qy * qy + qz * qz + qw * qw;
    const double e0 = y[3] - xt[3], e1 = y[4] - xt[4], e2 = y[5] - xt[5];
    r.rv0 = R00 * e0 + R01 * e1 + R02 * e2;
    r.rv1 = R10 * e0 + R11 * e1 + R12 * e2;
    r.rv2 = R20 * e0 + R21 * e1 + R22 * e2;
    r.rw0 = y[10] - xt[10], r.rw1 = y[11] - xt[11], r.rw2 = y[12] - xt[12];
    r.isv = 1.0 / (rsq[0] + n * dsq[0]);
    r.isw = 1.0 / (rsq[1] + n * dsq[1]);
    r.q0 = (r.rv0 * r.rv0 + r.rv1 * r.rv1 + r.rv2 * r.rv2) * r.isv + (r.rw0 * r.rw0 + r.rw1 * r.rw1 + r.rw2 * r.rw2) * r.isw;
}

FTMPC_ISO_HD void scan_start(const Rule& R, Scan& s) {
    s.best = R.threshold;
    s.besth = -1;
    s.qmin = 0.0;
    s.eligible = 0;
    s.counted = 0;
}

// the signature of a thruster per unit of delta: gh[0:3] velocity, gh[3:6] rate.  d [6]: the thruster's column of D
FTMPC_ISO_HD void unit_signature(double dt, double inv_mass, const double* Jinv, const double* d, double* gh) {
    const double kv = dt * inv_mass;
    gh[0] = kv * d[0], gh[1] = kv * d[1], gh[2] = kv * d[2];
    gh[3] = dt * (Jinv[0] * d[3] + Jinv[1] * d[4] + Jinv[2] * d[5]);
    gh[4] = dt * (Jinv[3] * d[3] + Jinv[4] * d[4] + Jinv[5] * d[5]);
    gh[5] = dt * (Jinv[6] * d[3] + Jinv[7] * d[4] + Jinv[8] * d[5]);
}

// Thruster i of one vehicle.  live: ub_c,i > 0; listed: off and in the vehicle's detection list (looked at with revise only);
// llr: the statistic of (i, 0), the one of (i, l) stands l * stride further; hist: nullptr or the row's entry of (i, 0), contiguous
FTMPC_ISO_HD void thruster(const Rule& R, const Resid& r, double n, int i, bool live, bool listed, double acci, double stucki,
                           const double* gh, double* llr, long long stride, double* hist, Scan& s) {
    const bool eligible = live || (R.revise != 0 && listed);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        if (l < R.L) {
            double v = 0.0;
            if (eligible) {
                const double delta = live ? n * R.levels[l] - acci : n * (R.levels[l] - stucki);
                const double a0 = gh[0] * delta, a1 = gh[1] * delta, a2 = gh[2] * delta;
                const double w0 = gh[3] * delta, w1 = gh[4] * delta, w2 = gh[5] * delta;
                const double z = ((a0 * r.rv0 + a1 * r.rv1 + a2 * r.rv2) - 0.5 * (a0 * a0 + a1 * a1 + a2 * a2)) * r.isv +
                                 ((w0 * r.rw0 + w1 * r.rw1 + w2 * r.rw2) - 0.5 * (w0 * w0 + w1 * w1 + w2 * w2)) * r.isw;
                const double q = r.q0 - 2.0 * z;
                const double old = llr[l * stride];
                const bool counted = !(R.consist_sq > 0.0) || q <= R.consist_sq;
                v = counted ? fmax(0.0, old + z) : old;
                if (s.eligible == 0 || q < s.qmin) s.qmin = q;
                s.eligible += 1;
                s.counted += counted ? 1 : 0;
            }
            llr[l * stride] = v;
            if (hist) hist[l] = v;
            if (v > s.best) {      // (strictly: a tie stays with the lowest index)
                s.best = v;
                s.besth = i * R.L + l;
            }
        }
    }
}

// void: the residual fits neither the healthy model nor any hypothesis that could be counted
FTMPC_ISO_HD bool is_void(const Rule& R, const Resid& r, const Scan& s) {
    return R.consist_sq > 0.0 && r.q0 > R.consist_sq && s.counted == 0;
}

// the confirmation: lead and run in / out; true: the leader is decided now
FTMPC_ISO_HD bool confirm(const Rule& R, const Scan& s, int& lead, int& run) {
    if (s.besth < 0) {
        lead = -1;
        run = 0;
        return false;
    }
    if (s.besth == lead) {
        run += 1;
    } else {
        lead = s.besth;
        run = 1;
    }
    return run >= R.persist;
}

// The decision for hypothesis h at campaign step c.  ub, stuck [NT], det_* [K]: the vehicle's own rows; cnt: entries used so far
// (< K); llr: the vehicle's first statistic, H of them stride apart.  Returns 1 for a revision, 0 for a live thruster
FTMPC_ISO_HD int decide(const Rule& R, int h, int c, int cnt, int H, double* ub, double* stuck, int* det_step, int* det_thruster,
                        int* det_level, double* llr, long long stride, int& lead, int& run) {
    const int i = h / R.L, l = h - i * R.L;
    const double lv = l == 0 ? R.levels[0] : (l == 1 ? R.levels[1] : (l == 2 ? R.levels[2] : R.levels[3]));
    const int revision = ub[i] > 0.0 ? 0 : 1;
    det_step[cnt] = c;
    det_thruster[cnt] = i;
    det_level[cnt] = l;
    ub[i] = 0.0;
    stuck[i] = lv;
#pragma unroll 1
    for (int k = 0; k < H; ++k) llr[k * stride] = 0.0;
    lead = -1;
    run = 0;
    return revision;
}

}  // namespace ftmpc_iso
