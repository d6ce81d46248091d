// One vehicle's probe step and the "healthy after all" hypotheses of a reinstating probe (ftmpc_probe_kernel and
// ftmpc_diagnose_probe_kernel, csrc/ftmpc_sim.hip; include/ftmpc.h, ftmpc_probe), as host / device functions so that a plain C++
// program can run what the kernels run (tests/test_probes_host.py).
//
// The probe step on the command u of this step's solve, with (ub_c, stuck_c) the controller's pattern of the step:
//     listed     thruster i is off (ub_c,i == 0) and the newest entry for i in the vehicle's detection list has a level below
//                n_levels (an entry at n_levels is a reinstatement)
//     probeable  live (ub_c,i > 0), or listed under reinstate
//     idle       e_i = live ? u_i : 0;  idle_i = (probeable and e_i < quiet) ? idle_i + 1 : 0 (a NaN command compares false)
//     candidate  the probeable thruster with the largest idle_i among those with idle_i >= idle_steps and, with max_pulses > 0,
//                pulses_i < max_pulses; the lowest index on a tie; at most one per vehicle and step
//     pulse      live: u_i = min(u_i + amp, ub_c,i); listed: u_i = amp; pulses_i += 1, impulse += (u_i,new - e_i) dt, idle_i = 0
// The hypothesis H + i "listed thruster i is healthy" of the diagnosis' test: delta = pacc_i - n stuck_c,i with pacc_i the sum of the
// applied command over the window (the model's c_i is 0 for an off thruster), z and q from delta as for a level hypothesis, the
// statistic in health[i]; it is counted by the gate like any other and competes for the leader, a level hypothesis winning a tie.
// The caller's thruster loop stays rolled: thruster() and healthy() handle one thruster and carry the candidate and the arg-max;
// no array is indexed by the thruster.
#pragma once

#include "ftmpc_isolate.h"

#define FTMPC_PROBE_HD FTMPC_ISO_HD

namespace ftmpc_prb {

// what is uniform over the call
struct Rule {
    double amp, quiet, restore_ub, dt;
    int idle_steps, max_pulses, reinstate, n_levels;
};

// what the thruster loop of the probe step carries
struct Pick {
    int cand;               // -1: no candidate
    int idle;               // the candidate's counter
};

// what the thruster loop of the test carries for the healthy hypotheses, beside ftmpc_iso::Scan
struct Lead {
    double best;            // the threshold, then the largest health statistic above it
    int besti;              // -1: none
};

// det_thruster, det_level [cnt]: the vehicle's detection list, oldest first
FTMPC_PROBE_HD bool listed(int i, bool live, int cnt, const int* det_thruster, const int* det_level, int n_levels) {
    if (live) return false;
    int level = n_levels;
#pragma unroll 1
    for (int k = 0; k < cnt; ++k)
        if (det_thruster[k] == i) level = det_level[k];
    return level < n_levels;
}

FTMPC_PROBE_HD void pick_start(Pick& p) {
    p.cand = -1;
    p.idle = 0;
}

// Thruster i of one vehicle: its counter moves, the candidate is carried.  u: the solve's command; idle in/out
FTMPC_PROBE_HD void thruster(const Rule& R, int i, bool live, bool lst, double u, int pulses, int& idle, Pick& p) {
    const bool probeable = live || (R.reinstate != 0 && lst);
    const double e = live ? u : 0.0;
    idle = (probeable && e < R.quiet) ? idle + 1 : 0;
    const bool capped = R.max_pulses > 0 && pulses >= R.max_pulses;
    if (probeable && !capped && idle >= R.idle_steps && idle > p.idle) {      // (strictly: a tie stays with the lowest index)
        p.idle = idle;
        p.cand = i;
    }
}

// The pulse on the candidate.  u in/out; returns what the pulse adds to the vehicle's impulse
FTMPC_PROBE_HD double pulse(const Rule& R, bool live, double ub, double& u, int& pulses, int& idle) {
    const double e = live ? u : 0.0;
    u = live ? fmin(u + R.amp, ub) : R.amp;
    pulses += 1;
    idle = 0;
    return (u - e) * R.dt;
}

FTMPC_PROBE_HD void lead_start(const ftmpc_iso::Rule& R, Lead& h) {
    h.best = R.threshold;
    h.besti = -1;
}

// Hypothesis H + i of one vehicle's test.  lst: thruster i is listed; pacci: the applied command summed over the window; health:
// the statistic, in/out; s counts it for the gate and the fit as ftmpc_iso::thruster counts a level hypothesis
FTMPC_PROBE_HD void healthy(const ftmpc_iso::Rule& R, const ftmpc_iso::Resid& r, double n, int i, bool lst, double pacci, double stucki,
                            const double* gh, double* health, ftmpc_iso::Scan& s, Lead& h) {
    double v = 0.0;
    if (lst) {
        const double delta = pacci - n * stucki;
        const double a0 = gh[0] * delta, a1 = gh[1] * delta, a2 = gh[2] * delta;
        const double w0 = gh[3] * delta, w1 = gh[4] * delta, w2 = gh[5] * delta;
        const double z = ((a0 * r.rv0 + a1 * r.rv1 + a2 * r.rv2) - 0.5 * (a0 * a0 + a1 * a1 + a2 * a2)) * r.isv +
                         ((w0 * r.rw0 + w1 * r.rw1 + w2 * r.rw2) - 0.5 * (w0 * w0 + w1 * w1 + w2 * w2)) * r.isw;
        const double q = r.q0 - 2.0 * z;
        const double old = *health;
        const bool counted = !(R.consist_sq > 0.0) || q <= R.consist_sq;
        v = counted ? fmax(0.0, old + z) : old;
        if (s.eligible == 0 || q < s.qmin) s.qmin = q;
        s.eligible += 1;
        s.counted += counted ? 1 : 0;
    }
    *health = v;
    if (v > h.best) {      // (strictly: a tie stays with the lowest index)
        h.best = v;
        h.besti = i;
    }
}

// After the thruster loop: hypothesis H + i leads only where it is strictly above every level hypothesis (a tie: the lower index)
FTMPC_PROBE_HD void merge(const Lead& h, int H, ftmpc_iso::Scan& s) {
    if (h.besti >= 0 && h.best > s.best) {
        s.best = h.best;
        s.besth = H + h.besti;
    }
}

// The decision for hypothesis H + i at campaign step c: the entry (c, i, n_levels), the thruster back at restore_ub.  The caller
// resets the statistics (llr and health), lead and run, as ftmpc_iso::decide does for a level hypothesis
FTMPC_PROBE_HD void reinstate(const Rule& R, int i, int c, int cnt, double* ub, double* stuck, int* det_step, int* det_thruster,
                              int* det_level) {
    det_step[cnt] = c;
    det_thruster[cnt] = i;
    det_level[cnt] = R.n_levels;
    ub[i] = R.restore_ub;
    stuck[i] = 0.0;
}

}  // namespace ftmpc_prb
