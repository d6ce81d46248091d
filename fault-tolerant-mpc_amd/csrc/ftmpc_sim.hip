// ftmpc_sim.hip -- the caller side of the MPC step on the device:
// plant integration + measurement noise + quaternion renormalisation
//   (reference: SimulationEnvironment.step, ft_mpc/simulation/sim_env.py:77-99, with
//    SystemModel.dx_dt / rk4_integrator, ft_mpc/models/sys_model.py:138-226)
// and the warm-start shift (ft_mpc/controllers/spiraling_mpc.py:324-334), so that a Monte-Carlo
// fault campaign runs T closed-loop steps without host round trips.
#include <hip/hip_runtime.h>

#include "ftmpc_common.h"

namespace ftmpc {

namespace {
// counter-based uniform in [0,1): splitmix64 of (seed, index); oracle/closed_loop.py mirrors it
__device__ __forceinline__ double u01(unsigned long long seed, unsigned long long idx) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (idx + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ void plant_f(const DeviceConsts& C, const double* x, const double* gen, double* dx) {
    const double *v = x + 3, *q = x + 6, *w = x + 10;
    dx[0] = v[0]; dx[1] = v[1]; dx[2] = v[2];
    // v' = Rot(q)^T F / m   (sys_model.py:215)
    const double qx = q[0], qy = q[1], qz = q[2], qw = q[3];
    const double R00 = qx * qx - qy * qy - qz * qz + qw * qw, R01 = 2 * (qx * qy + qz * qw), R02 = 2 * (qx * qz - qy * qw);
    const double R10 = 2 * (qx * qy - qz * qw), R11 = -qx * qx + qy * qy - qz * qz + qw * qw, R12 = 2 * (qy * qz + qx * qw);
    const double R20 = 2 * (qx * qz + qy * qw), R21 = 2 * (qy * qz - qx * qw), R22 = -qx * qx - qy * qy + qz * qz + qw * qw;
    const double f0 = gen[0] * C.inv_mass, f1 = gen[1] * C.inv_mass, f2 = gen[2] * C.inv_mass;
    dx[3] = R00 * f0 + R10 * f1 + R20 * f2;
    dx[4] = R01 * f0 + R11 * f1 + R21 * f2;
    dx[5] = R02 * f0 + R12 * f1 + R22 * f2;
    // q' = 1/2 Omega(w) q   (sys_model.py:18-29,218)
    dx[6] = 0.5 * (w[2] * qy - w[1] * qz + w[0] * qw);
    dx[7] = 0.5 * (-w[2] * qx + w[0] * qz + w[1] * qw);
    dx[8] = 0.5 * (w[1] * qx - w[0] * qy + w[2] * qw);
    dx[9] = 0.5 * (-w[0] * qx - w[1] * qy - w[2] * qz);
    // w' = J^-1 (tau - w x J w)   (sys_model.py:221-224)
    double Jw[3], t[3];
    for (int i = 0; i < 3; ++i) Jw[i] = C.J[3 * i] * w[0] + C.J[3 * i + 1] * w[1] + C.J[3 * i + 2] * w[2];
    t[0] = gen[3] - (w[1] * Jw[2] - w[2] * Jw[1]);
    t[1] = gen[4] - (w[2] * Jw[0] - w[0] * Jw[2]);
    t[2] = gen[5] - (w[0] * Jw[1] - w[1] * Jw[0]);
    for (int i = 0; i < 3; ++i) dx[10 + i] = C.Jinv[3 * i] * t[0] + C.Jinv[3 * i + 1] * t[1] + C.Jinv[3 * i + 2] * t[2];
}
}  // namespace

struct SimParams {
    int64_t B;
    double* x;            // [B*13] in/out
    const double* u0;     // [B*NT] command of this step
    const double* ub;
    const double* stuck;
    double noise[4];      // amplitudes: position, velocity, orientation, angular velocity (U(0, a), sim_env.py:25-30)
    unsigned long long seed;
    int64_t step, index0, index_total;   // noise counter (step * index_total + index0 + b) * 13 + i: vehicles [index0, index0 + B) of a campaign
    double* u_hist;       // nullptr or [T*B*NT]
    const int32_t* status;
    int32_t* bad_count;   // nullptr or [T]
    double* x_hist = nullptr;   // nullptr or [T*B*13]: the state after each step (after noise and renormalisation)
};

__global__ void __launch_bounds__(64) ftmpc_plant_step_kernel(const DeviceConsts C, const SimParams S) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= S.B) return;
    const int NT = C.NT;
    double gen[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < NT; ++i) {
        const double u = S.u0[b * NT + i];
        if (S.u_hist) S.u_hist[(S.step * S.B + b) * NT + i] = u;
        const double t = (S.ub[b * NT + i] > 0.0 ? u : 0.0) + S.stuck[b * NT + i];   // sys_model.py:198-208
        for (int g = 0; g < 6; ++g) gen[g] += C.D[g * MAX_NT + i] * t;
    }
    double x[13], k1[13], k2[13], k3[13], k4[13], s[13];
    for (int i = 0; i < 13; ++i) x[i] = S.x[b * 13 + i];
    const double dt = C.dt;
    plant_f(C, x, gen, k1);
    for (int i = 0; i < 13; ++i) s[i] = x[i] + 0.5 * dt * k1[i];
    plant_f(C, s, gen, k2);
    for (int i = 0; i < 13; ++i) s[i] = x[i] + 0.5 * dt * k2[i];
    plant_f(C, s, gen, k3);
    for (int i = 0; i < 13; ++i) s[i] = x[i] + dt * k3[i];
    plant_f(C, s, gen, k4);
    for (int i = 0; i < 13; ++i) x[i] += dt / 6.0 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]);
    // one-sided uniform measurement noise (sim_env.py:88-91), then quaternion renormalisation (:93)
    for (int i = 0; i < 13; ++i) {
        const double a = i < 3 ? S.noise[0] : (i < 6 ? S.noise[1] : (i < 10 ? S.noise[2] : S.noise[3]));
        if (a > 0.0) x[i] += a * u01(S.seed, (unsigned long long)((S.step * S.index_total + S.index0 + b) * 13 + i));
    }
    const double qn = 1.0 / sqrt(x[6] * x[6] + x[7] * x[7] + x[8] * x[8] + x[9] * x[9]);
    for (int i = 6; i < 10; ++i) x[i] *= qn;
    for (int i = 0; i < 13; ++i) S.x[b * 13 + i] = x[i];
    if (S.x_hist)
        for (int i = 0; i < 13; ++i) S.x_hist[(S.step * S.B + b) * 13 + i] = x[i];
    if (S.bad_count && S.status && S.status[b] != 0) atomicAdd(&S.bad_count[S.step], 1);
}

// warm[b][k] = U[b][k+1] (k < N-1), warm[b][N-1] = 0     (spiraling_mpc.py:327-329)
// last stage: zero (the thruster sequences, spiraling_mpc.py:327-329) or, repeat_last != 0, the previous last stage again
// (the wrench sequences of the two-stage structure)
__global__ void __launch_bounds__(256) ftmpc_shift_warm_kernel(int64_t B, int N, int NT, const double* U, double* warm, int repeat_last) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per = (int64_t)N * NT;
    if (i >= B * per) return;
    const int64_t r = i % per;
    warm[i] = (r < per - NT) ? U[i + NT] : (repeat_last ? U[i] : 0.0);
}

__global__ void __launch_bounds__(256) ftmpc_count_nonzero_kernel(int64_t B, const int32_t* flags, int32_t* count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool bad = i < B && flags[i] != 0;
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, (int32_t)__popcll(m));
}


// ---------------------------------------------------------------------------------------------------------
// Line-search SQP towards the reference's nonlinear program, on the device (reference
// spiraling_mpc.py:87-238 solved by IPOPT :346).  ft_mpc_amd.BatchedMPC.solve_sqp is the host mirror of exactly this
// bookkeeping; here nothing crosses PCIe between the first upload and the last download.
//   per instance:  J (cost at U), Jt (cost at the trial point), alpha, flags {active, todo, improved}, counters
// ---------------------------------------------------------------------------------------------------------
struct SqpState {
    int64_t B;
    int32_t N, NT;
    const double* ub;       // [B*NT]
    double* U;              // [B*N*NT] current iterate
    const double* Uq;       // [B*N*NT] solution of the QP linearised about U
    double* Ut;             // [B*N*NT] trial point U + alpha (clip(Uq) - U)
    double* J;              // [B]
    const double* Jt;       // [B]
    double* alpha;          // [B] current trial step; after a success: the accepted step
    int32_t* active;        // [B]
    int32_t* todo;          // [B]
    int32_t* improved;      // [B]
    int32_t* nmajor;        // [B]
    int32_t* ipm;           // [B]
    int32_t* status;        // [B]
    const int32_t* qstatus; // [B] of the last QP
    const int32_t* qiters;  // [B]
    double tol;
    const double* Jall = nullptr;   // [B*ntrial] costs of all trial points of a line search (ftmpc_cost_kernel, ntrial > 0)
    int32_t ntrial = 0;
};

// U = clip(warm, 0, ub) (or 0); active = 1; counters = 0
__global__ void ftmpc_sqp_init_kernel(const SqpState S, const double* warm) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nw = (int64_t)S.N * S.NT;
    if (i < S.B * nw) {
        const int64_t b = i / nw;
        const int t = (int)(i % S.NT);
        const double ub = S.ub[b * S.NT + t];
        S.U[i] = warm ? fmin(fmax(warm[i], 0.0), ub) : 0.0;
    }
    if (i < S.B) {
        S.active[i] = 1;
        S.todo[i] = 0;
        S.improved[i] = 0;
        S.nmajor[i] = 0;
        S.ipm[i] = 0;
        S.status[i] = 0;
        S.alpha[i] = 1.0;
    }
}
// after the QP of a major iteration: account for it, open the line search
__global__ void ftmpc_sqp_open_kernel(const SqpState S) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= S.B) return;
    const int act = S.active[b];
    if (act) {
        S.ipm[b] += S.qiters[b];
        S.status[b] = S.qstatus[b];
    }
    S.todo[b] = act && S.qstatus[b] != 2;
    S.improved[b] = 0;
    S.alpha[b] = 1.0;
}
// trial point Ut = U + alpha (clip(Uq, 0, ub) - U)   (the fp32 kernels return ub rounded to float32: hence the clip)
__global__ void ftmpc_sqp_trial_kernel(const SqpState S) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nw = (int64_t)S.N * S.NT;
    if (i >= S.B * nw) return;
    const int64_t b = i / nw;
    const int t = (int)(i % S.NT);
    const double ub = S.ub[b * S.NT + t];
    const double step = fmin(fmax(S.Uq[i], 0.0), ub) - S.U[i];
    S.Ut[i] = S.U[i] + S.alpha[b] * step;
}
// accept the trial point where the TRUE cost decreased enough, else halve the step
__global__ void ftmpc_sqp_decide_kernel(const SqpState S) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= S.B || !S.todo[b]) return;
    const double J = S.J[b], Jt = S.Jt[b];
    if (Jt < J - S.tol * (1.0 + fabs(J))) {
        S.J[b] = Jt;
        S.improved[b] = 1;
        S.todo[b] = 0;       // alpha keeps the accepted step
    } else {
        S.alpha[b] *= 0.5;
    }
}
// the whole line search at once: the costs of the trial points alpha = 1, 1/2, ... are all there (S.Jall); the first that decreases the
// TRUE cost enough is accepted -- what `backtracks` rounds of trial / cost / decide arrive at, in one launch instead of 3 x backtracks
__global__ void ftmpc_sqp_pick_kernel(const SqpState S) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= S.B || !S.todo[b]) return;
    const double J = S.J[b];
    double alpha = S.alpha[b];
    for (int j = 0; j < S.ntrial; ++j) {
        const double Jt = S.Jall[b * S.ntrial + j];
        if (Jt < J - S.tol * (1.0 + fabs(J))) {
            S.J[b] = Jt;
            S.improved[b] = 1;
            S.todo[b] = 0;
            break;
        }
        alpha *= 0.5;
    }
    S.alpha[b] = alpha;
}
// close the line search: U += alpha step where a trial point was accepted; an instance without progress stops
__global__ void ftmpc_sqp_close_kernel(const SqpState S) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nw = (int64_t)S.N * S.NT;
    if (i < S.B * nw) {
        const int64_t b = i / nw;
        if (S.improved[b]) {
            const int t = (int)(i % S.NT);
            const double ub = S.ub[b * S.NT + t];
            const double step = fmin(fmax(S.Uq[i], 0.0), ub) - S.U[i];
            S.Ut[i] = S.U[i] + S.alpha[b] * step;      // (U is read by the other threads of this launch: the new iterate goes to Ut)
        } else {
            S.Ut[i] = S.U[i];
        }
    }
}
__global__ void ftmpc_sqp_count_kernel(const SqpState S) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= S.B) return;
    S.nmajor[b] += S.improved[b];
    S.active[b] = S.active[b] && S.improved[b];
}

// The same SQP in the GENERALIZED-FORCE formulation (ftmpc_solve_sqp_wrench_batch): the iterate is the total wrench per stage
// (S.NT = 6, no box: the hull rows hold at the iterate and at the QP solution, so they hold on the segment between).  open, pick
// and count are the kernels above; S.J / S.Jall hold the merit cost + sigma * terminal-set violation.
// G = warm, or tau_k = D stuck for every stage (the wrench QP's own default linearisation point); flags as ftmpc_sqp_init_kernel
__global__ void ftmpc_sqpw_init_kernel(const DeviceConsts C, const SqpState S, const double* warm, const double* stuck) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nw = (int64_t)S.N * 6;
    if (i < S.B * nw) {
        if (warm) {
            S.U[i] = warm[i];
        } else {
            const int64_t b = i / nw;
            const int g = (int)(i % 6);
            double t = 0.0;
            for (int k = 0; k < C.NT; ++k) t += C.D[g * MAX_NT + k] * stuck[b * C.NT + k];
            S.U[i] = finite_or_zero(t);      // (a NaN stuck entry: the vehicle's first QP fails and this point is what comes back)
        }
    }
    if (i < S.B) {
        S.active[i] = 1;
        S.todo[i] = 0;
        S.improved[i] = 0;
        S.nmajor[i] = 0;
        S.ipm[i] = 0;
        S.status[i] = 0;
        S.alpha[i] = 1.0;
    }
}
// The hull pull shared by the tau_0 kernel and the fault-event kernel: the hull centre D (ub/2 + stuck) of an instance's pattern, and the
// smallest factor eps that pulls a wrench t towards it far enough to leave every facet a relative margin of 1e-8:
//   out = ctr + (1 - eps) (t - ctr)   (eps = 0 where t already keeps the margin on every facet)
__device__ __forceinline__ void hull_centre(const DeviceConsts& C, const double* ub, const double* stuck, double* ctr) {
    for (int g = 0; g < 6; ++g) {
        double acc = 0.0;
        for (int i = 0; i < C.NT; ++i) acc += C.D[g * MAX_NT + i] * (0.5 * ub[i] + stuck[i]);
        ctr[g] = acc;
    }
}
__device__ __forceinline__ double hull_pull(const double* t, const double* ctr, const double* A, const double* hb, int32_t hull_rows,
                                            double* out) {
    double eps = 0.0;
    for (int r = 0; r < hull_rows; ++r) {
        const double* a = A + r * 6;
        double s0 = hb[r], st = s0;
        for (int g = 0; g < 6; ++g) {
            s0 -= a[g] * ctr[g];
            st -= a[g] * t[g];
        }
        if (st < 1e-8 * s0 && s0 > st) eps = fmax(eps, (1e-8 * s0 - st) / (s0 - st) * 1.0001);
    }
    for (int g = 0; g < 6; ++g) out[g] = ctr[g] + (1.0 - eps) * (t[g] - ctr[g]);
    return eps;
}

// tau_0 of the final iterate for the allocation: on an fp32 handle the iterate comes from kernel 11, whose active facets are met to fp32
// accuracy only (a few 1e-7 outside as often as inside); as kernel 11 does for its own tau_0, pull it towards the hull centre
// D (ub/2 + stuck) by the smallest factor that leaves every facet a relative margin of 1e-8.  One lane per instance.
__global__ void __launch_bounds__(64) ftmpc_sqpw_tau0_kernel(const DeviceConsts C, int64_t B, const double* G, const double* ub,
                                                             const double* stuck, const double* hullA, const int32_t* hull_set,
                                                             const double* hullb, int32_t hull_rows, double* tau0) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double t[6], ctr[6];
    for (int g = 0; g < 6; ++g) t[g] = G[b * (int64_t)C.N * 6 + g];
    hull_centre(C, ub + b * C.NT, stuck + b * C.NT, ctr);
    const int64_t set = hull_set ? hull_set[b] : 0;
    (void)hull_pull(t, ctr, hullA + set * hull_rows * 6, hullb + b * hull_rows, hull_rows, tau0 + b * 6);
    // (a finite iterate and a finite centre give a finite tau_0: only a vehicle whose stuck entries are not finite has anything replaced)
    for (int g = 0; g < 6; ++g) tau0[b * 6 + g] = finite_or_zero(tau0[b * 6 + g]);
}

// close the line search: Ut = U + alpha (Uq - U) where a trial point was accepted (the point ftmpc_cost_wrench_kernel evaluated), else U
__global__ void ftmpc_sqpw_close_kernel(const SqpState S) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nw = (int64_t)S.N * 6;
    if (i >= S.B * nw) return;
    const int64_t b = i / nw;
    const double u = S.U[i];
    S.Ut[i] = S.improved[b] ? u + S.alpha[b] * (S.Uq[i] - u) : u;
}


// ---------------------------------------------------------------------------------------------------------
// Thruster faults that start mid-run (ftmpc_simulate_faults_batch / ftmpc_simulate_wrench_faults_batch).  Each instance has up to E
// events (full after-event patterns, onset and detection steps; slots sorted, onset = -1 unused).  Launched before the solve of a
// step t at which some instance switches; per instance:
//   - an event with onset == t: the plant pattern becomes that of the last event with onset <= t
//   - an event with detect == t: the controller pattern (d_ub / d_stuck, on the wrench form the hull table number and offsets)
//     becomes that of the last event with detect <= t, and, repair != 0 (t > 0), the shifted warm start is repaired for it:
//     thruster form U clipped to [0, ub]; wrench form every stage pulled into the new hull as hull_pull does for tau_0.
// ---------------------------------------------------------------------------------------------------------
struct FaultEvents {
    int64_t B;
    int32_t E, t, repair;
    const int32_t* onset;    // [B*E]
    const int32_t* detect;   // [B*E]
    const double* ev_ub;     // [B*E*NT]
    const double* ev_stuck;  // [B*E*NT]
    double* plant_ub;        // [B*NT]
    double* plant_stuck;     // [B*NT]
    double* ub;              // [B*NT] the controller's
    double* stuck;           // [B*NT]
    double* warmU;           // thruster form: [B*N*NT] or nullptr
    // wrench form (warmG != nullptr)
    double* warmG;           // [B*N*6]
    const double* hullA;     // [n_sets*hull_rows*6]
    const int32_t* ev_hullset;   // nullptr (one table) or [B*E]
    const double* ev_hullb;  // [B*E*hull_rows]
    int32_t* hullset;        // nullptr or [B]
    double* hullb;           // [B*hull_rows]
    int32_t hull_rows;
};

// One lane per (instance, stage): the lane of stage 0 switches the patterns, every lane repairs its own stage of the warm start (from the
// event's pattern, never from the buffers stage 0 writes).
__global__ void __launch_bounds__(64) ftmpc_fault_event_kernel(const DeviceConsts C, const FaultEvents F) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int NT = C.NT, N = C.N;
    if (i >= F.B * N) return;
    const int64_t b = i / N;
    const int k = (int)(i % N);
    int ep = -1, ec = -1;
    bool sp = false, sc = false;
    for (int e = 0; e < F.E; ++e) {
        const int on = F.onset[b * F.E + e], de = F.detect[b * F.E + e];
        if (on < 0) break;
        if (on <= F.t) ep = e;
        if (de <= F.t) ec = e;
        sp |= on == F.t;
        sc |= de == F.t;
    }
    if (sp && k == 0) {
        const int64_t src = (b * F.E + ep) * NT;
        for (int j = 0; j < NT; ++j) {
            F.plant_ub[b * NT + j] = F.ev_ub[src + j];
            F.plant_stuck[b * NT + j] = F.ev_stuck[src + j];
        }
    }
    if (!sc) return;
    const int64_t src = (b * F.E + ec) * NT;
    if (k == 0) {
        for (int j = 0; j < NT; ++j) {
            F.ub[b * NT + j] = F.ev_ub[src + j];
            F.stuck[b * NT + j] = F.ev_stuck[src + j];
        }
    }
    if (F.warmG) {
        const int R = F.hull_rows;
        const int64_t set = F.ev_hullset ? F.ev_hullset[b * F.E + ec] : 0;
        if (k == 0) {
            for (int r = 0; r < R; ++r) F.hullb[b * R + r] = F.ev_hullb[(b * F.E + ec) * R + r];
            if (F.hullset) F.hullset[b] = (int32_t)set;
        }
        if (!F.repair) return;
        double ctr[6], t[6], p[6];
        hull_centre(C, F.ev_ub + src, F.ev_stuck + src, ctr);
        double* g = F.warmG + (b * N + k) * 6;
        for (int j = 0; j < 6; ++j) t[j] = g[j];
        if (hull_pull(t, ctr, F.hullA + set * R * 6, F.ev_hullb + (b * F.E + ec) * R, R, p) > 0.0)
            for (int j = 0; j < 6; ++j) g[j] = p[j];
    } else if (F.repair && F.warmU) {
        double* w = F.warmU + (b * N + k) * NT;
        for (int j = 0; j < NT; ++j) w[j] = fmin(fmax(w[j], 0.0), F.ev_ub[src + j]);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Per-vehicle outcomes of a fault campaign (ftmpc_simulate_outcomes_batch / ftmpc_simulate_wrench_outcomes_batch): launched after the
// plant kernel of loop step t, only when the call asks for an outcome or for status_hist.  It reduces what the histories would
// carry -- x_{t+1} (what the plant kernel just wrote), the command u_t, the PLANT's pattern and the solve / allocation status of the
// step -- into 84 bytes per vehicle, so that a campaign never needs x_hist / u_hist on the host:
//   e = robot_to_center(x_{t+1})[0:9] - xref[:, t+1];   ep, ev, ew = |e[0:3]|, |e[3:6]|, |e[6:9]|
//   err_int  += dt (ep^2, ev^2, ew^2)          err_max = max(err_max, (ep, ev, ew))
//   impulse  += dt (sum_i a_i, sum_i c_i)      c_i = ub_i > 0 ? u_i : 0 (commanded), a_i = c_i + stuck_i (delivered: sys_model.py:198-208)
//   settle    = t + 1 where a norm is outside its band (last such step + 1; records start at 0)
//   tset      = t at the first step with term_A e <= term_b on every row (records start at -1)
//   unsolved, first_unsolved, alloc_failed: counts / first step of a non-zero status
// The records always exist as a set (the host copies out what the caller asked for); `term` and `astatus` are null where the caller
// did not ask for tset_step / the loop has no allocation.  One lane per vehicle; the rows of the terminal set are the same addresses
// for every lane, and a vehicle stops evaluating them once it has entered the set.
// ---------------------------------------------------------------------------------------------------------
struct OutcomeParams {
    int64_t B;
    int32_t step, term_rows;
    const double* x;          // [B*13] the state after this step
    const double* u0;         // [B*NT] the command of this step
    const double* ub;         // [B*NT] the plant's pattern
    const double* stuck;
    const int32_t* status;    // [B] solve status of this step
    const int32_t* astatus;   // nullptr or [B] allocation status
    const double* xref;       // 9 reference values of column step + 1
    const double* term;       // nullptr or [term_rows*9 | term_rows]
    double tol[3];            // settle band: position, velocity, angular rate
    double* err_int;          // [B*3]
    double* err_max;          // [B*3]
    double* impulse;          // [B*2]
    int32_t* settle;          // [B]
    int32_t* tset;            // [B]
    int32_t* unsolved;        // [B]
    int32_t* first_unsolved;  // [B]
    int32_t* alloc_failed;    // [B]
    int32_t* status_hist;     // nullptr or [T*B]
};

__global__ void __launch_bounds__(64) ftmpc_outcome_kernel(const DeviceConsts C, const OutcomeParams O) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= O.B) return;
    const int NT = C.NT;
    const int32_t t = O.step;
    double x[13];
    for (int i = 0; i < 13; ++i) x[i] = O.x[b * 13 + i];
    // robot -> orbit-centre state (spiral_model.py:91-109), as kernel 1 forms it
    double e[9];
    {
        double RT[9], wxr[3], a[3], c[3];
        rotT(x + 6, RT);
        cross3(x + 10, C.r, wxr);
        mat3vec(RT, C.r, a);
        mat3vec(RT, wxr, c);
        for (int i = 0; i < 3; ++i) {
            e[i] = x[i] + a[i] - O.xref[i];
            e[3 + i] = x[3 + i] + c[i] - O.xref[3 + i];
            e[6 + i] = x[10 + i] - O.xref[6 + i];
        }
    }
    const double dt = C.dt;
    bool inside = true;
    for (int j = 0; j < 3; ++j) {
        const double n2 = e[3 * j] * e[3 * j] + e[3 * j + 1] * e[3 * j + 1] + e[3 * j + 2] * e[3 * j + 2];
        const double n = sqrt(n2);
        O.err_int[b * 3 + j] += dt * n2;
        O.err_max[b * 3 + j] = fmax(O.err_max[b * 3 + j], n);
        inside = inside && n <= O.tol[j];
    }
    if (!inside) O.settle[b] = t + 1;
    double del = 0.0, cmd = 0.0;
    for (int i = 0; i < NT; ++i) {
        const double c = O.ub[b * NT + i] > 0.0 ? O.u0[b * NT + i] : 0.0;
        cmd += c;
        del += c + O.stuck[b * NT + i];
    }
    O.impulse[b * 2] += dt * del;
    O.impulse[b * 2 + 1] += dt * cmd;
    const int32_t st = O.status[b];
    if (st != 0) {
        if (O.unsolved[b]++ == 0) O.first_unsolved[b] = t;
    }
    if (O.astatus && O.astatus[b] != 0) O.alloc_failed[b] += 1;
    if (O.status_hist) O.status_hist[(int64_t)t * O.B + b] = st;
    if (O.term && O.tset[b] < 0) {
        const double* tb = O.term + (int64_t)O.term_rows * 9;
        bool in = true;
        for (int r = 0; r < O.term_rows; ++r) {
            double s = 0.0;
            for (int j = 0; j < 9; ++j) s += O.term[r * 9 + j] * e[j];
            in = in && s <= tb[r];
        }
        if (in) O.tset[b] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Plant dispersion (ftmpc_simulate_plant_batch / ftmpc_simulate_wrench_plant_batch; include/ftmpc.h, ftmpc_plant_model): vehicle b's
// plant has its own mass m_b, inertia J_b, allocation matrix D_b, a constant disturbance force f_b (inertial frame) and torque t_b
// (body frame), while the controller keeps the model of DeviceConsts:
//   [F; tau] = D_b a      v' = (Rot(q)^T F + f_b) / m_b      w' = J_b^-1 (tau + t_b - w x J_b w)      p', q' as plant_f
// ftmpc_plant_step_var_kernel is ftmpc_plant_step_kernel with that right-hand side (same noise, counter, renormalisation, histories
// and bad_count); it is launched in its place only when the call's plant model has at least one array.  (It stands at the end of the
// file, not beside the kernel it generalises, so that the build logs keep the source lines of every kernel above.)
// The arrays are component-major, [k][B]: lane b reads base + k * B + b, so a wave's load covers 512 contiguous bytes (the C ABI is
// vehicle-major; the host transposes once per call while staging, and inverts m_b and J_b there).  A null array is a wave-uniform
// branch to the DeviceConsts value.
// ---------------------------------------------------------------------------------------------------------
struct PlantVar {
    const double* inv_mass;   // nullptr or [B]       1 / m_b
    const double* J;          // nullptr or [18][B]   J_b row-major, then J_b^-1 row-major
    const double* D;          // nullptr or [6*NT][B] k = g * NT + i
    const double* force;      // nullptr or [3][B]
    const double* torque;     // nullptr or [3][B]
};

namespace {
// plant_f with the vehicle's own 1 / m, J, J^-1 and the acceleration fm = f_b / m_b of the disturbance force; the disturbance torque
// is constant over the step in the body frame, so the caller has added it to gen[3..5]
__device__ __forceinline__ void plant_f_var(const double inv_mass, const double* J, const double* Jinv, const double* fm, const double* x,
                                            const double* gen, double* dx) {
    const double *v = x + 3, *q = x + 6, *w = x + 10;
    dx[0] = v[0]; dx[1] = v[1]; dx[2] = v[2];
    const double qx = q[0], qy = q[1], qz = q[2], qw = q[3];
    const double R00 = qx * qx - qy * qy - qz * qz + qw * qw, R01 = 2 * (qx * qy + qz * qw), R02 = 2 * (qx * qz - qy * qw);
    const double R10 = 2 * (qx * qy - qz * qw), R11 = -qx * qx + qy * qy - qz * qz + qw * qw, R12 = 2 * (qy * qz + qx * qw);
    const double R20 = 2 * (qx * qz + qy * qw), R21 = 2 * (qy * qz - qx * qw), R22 = -qx * qx - qy * qy + qz * qz + qw * qw;
    const double f0 = gen[0] * inv_mass, f1 = gen[1] * inv_mass, f2 = gen[2] * inv_mass;
    dx[3] = R00 * f0 + R10 * f1 + R20 * f2 + fm[0];
    dx[4] = R01 * f0 + R11 * f1 + R21 * f2 + fm[1];
    dx[5] = R02 * f0 + R12 * f1 + R22 * f2 + fm[2];
    dx[6] = 0.5 * (w[2] * qy - w[1] * qz + w[0] * qw);
    dx[7] = 0.5 * (-w[2] * qx + w[0] * qz + w[1] * qw);
    dx[8] = 0.5 * (w[1] * qx - w[0] * qy + w[2] * qw);
    dx[9] = 0.5 * (-w[0] * qx - w[1] * qy - w[2] * qz);
    double Jw[3], t[3];
    for (int i = 0; i < 3; ++i) Jw[i] = J[3 * i] * w[0] + J[3 * i + 1] * w[1] + J[3 * i + 2] * w[2];
    t[0] = gen[3] - (w[1] * Jw[2] - w[2] * Jw[1]);
    t[1] = gen[4] - (w[2] * Jw[0] - w[0] * Jw[2]);
    t[2] = gen[5] - (w[0] * Jw[1] - w[1] * Jw[0]);
    for (int i = 0; i < 3; ++i) dx[10 + i] = Jinv[3 * i] * t[0] + Jinv[3 * i + 1] * t[1] + Jinv[3 * i + 2] * t[2];
}
}  // namespace

__global__ void __launch_bounds__(64) ftmpc_plant_step_var_kernel(const DeviceConsts C, const SimParams S, const PlantVar V) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t B = S.B;
    if (b >= B) return;
    const int NT = C.NT;
    double gen[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < NT; ++i) {
        const double u = S.u0[b * NT + i];
        if (S.u_hist) S.u_hist[(S.step * B + b) * NT + i] = u;
        const double t = (S.ub[b * NT + i] > 0.0 ? u : 0.0) + S.stuck[b * NT + i];   // sys_model.py:198-208
        if (V.D) {
            for (int g = 0; g < 6; ++g) gen[g] += V.D[(int64_t)(g * NT + i) * B + b] * t;
        } else {
            for (int g = 0; g < 6; ++g) gen[g] += C.D[g * MAX_NT + i] * t;
        }
    }
    double J[9], Jinv[9], fm[3] = {0, 0, 0};
    const double inv_mass = V.inv_mass ? V.inv_mass[b] : C.inv_mass;
    if (V.J) {
        for (int k = 0; k < 9; ++k) {
            J[k] = V.J[k * B + b];
            Jinv[k] = V.J[(9 + k) * B + b];
        }
    } else {
        for (int k = 0; k < 9; ++k) {
            J[k] = C.J[k];
            Jinv[k] = C.Jinv[k];
        }
    }
    if (V.force)
        for (int k = 0; k < 3; ++k) fm[k] = V.force[k * B + b] * inv_mass;
    if (V.torque)
        for (int k = 0; k < 3; ++k) gen[3 + k] += V.torque[k * B + b];
    double x[13], k1[13], k2[13], k3[13], k4[13], s[13];
    for (int i = 0; i < 13; ++i) x[i] = S.x[b * 13 + i];
    const double dt = C.dt;
    plant_f_var(inv_mass, J, Jinv, fm, x, gen, k1);
    for (int i = 0; i < 13; ++i) s[i] = x[i] + 0.5 * dt * k1[i];
    plant_f_var(inv_mass, J, Jinv, fm, s, gen, k2);
    for (int i = 0; i < 13; ++i) s[i] = x[i] + 0.5 * dt * k2[i];
    plant_f_var(inv_mass, J, Jinv, fm, s, gen, k3);
    for (int i = 0; i < 13; ++i) s[i] = x[i] + dt * k3[i];
    plant_f_var(inv_mass, J, Jinv, fm, s, gen, k4);
    for (int i = 0; i < 13; ++i) x[i] += dt / 6.0 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]);
    // noise, renormalisation, histories and bad_count exactly as ftmpc_plant_step_kernel
    for (int i = 0; i < 13; ++i) {
        const double a = i < 3 ? S.noise[0] : (i < 6 ? S.noise[1] : (i < 10 ? S.noise[2] : S.noise[3]));
        if (a > 0.0) x[i] += a * u01(S.seed, (unsigned long long)((S.step * S.index_total + S.index0 + b) * 13 + i));
    }
    const double qn = 1.0 / sqrt(x[6] * x[6] + x[7] * x[7] + x[8] * x[8] + x[9] * x[9]);
    for (int i = 6; i < 10; ++i) x[i] *= qn;
    for (int i = 0; i < 13; ++i) S.x[b * 13 + i] = x[i];
    if (S.x_hist)
        for (int i = 0; i < 13; ++i) S.x_hist[(S.step * B + b) * 13 + i] = x[i];
    if (S.bad_count && S.status && S.status[b] != 0) atomicAdd(&S.bad_count[S.step], 1);
}

// ---------------------------------------------------------------------------------------------------------
// Reference missions (ftmpc_simulate_mission_batch / ftmpc_simulate_wrench_mission_batch; include/ftmpc.h, ftmpc_mission): K reference
// tables of C columns, and per vehicle a table number and a start column.  At loop step t vehicle b tracks the columns
// offset[b] + t .. offset[b] + t + N of its table.  ftmpc_ref_window_kernel gathers those columns into per-vehicle windows
//   xwin [B][9 (N+1)]   and, when the mission has uref tables,   uwin [B][6 (N+1)]
// once per step before the solve; every consumer of the reference (linearise, cost, outcome kernels) then reads (base, stride) as the
// one-step entries always could.  One lane per double of the output: the writes are contiguous over the launch, the reads contiguous
// within a vehicle (a window is 9 (N+1) consecutive doubles of a column-major table).  The host has checked
// offset[b] + T + N <= C and table[b] in [0, K), so no read leaves a table.  (Both kernels stand at the end of the file so that the
// build logs keep the source lines of every kernel above.)
// ---------------------------------------------------------------------------------------------------------
struct RefWindow {
    int64_t B, C;             // vehicles, columns per table
    int32_t N1, t;            // N + 1 columns per window, loop step
    const double* xtab;       // [K][9*C]
    const double* utab;       // nullptr or [K][6*C]
    const int32_t* table;     // nullptr (table 0) or [B]
    const int32_t* offset;    // nullptr (0) or [B]
    double* xwin;             // [B][9*N1]
    double* uwin;             // nullptr or [B][6*N1]
};

__global__ void __launch_bounds__(256) ftmpc_ref_window_kernel(const RefWindow W) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nx = W.B * 9 * W.N1;
    int rows = 9;
    const double* tab = W.xtab;
    double* win = W.xwin;
    if (i >= nx) {
        if (!W.utab) return;
        i -= nx;
        rows = 6;
        tab = W.utab;
        win = W.uwin;
    }
    const int64_t per = (int64_t)rows * W.N1;
    if (i >= W.B * per) return;
    const int64_t b = i / per, j = i - b * per;
    const int64_t k = W.table ? W.table[b] : 0;
    const int64_t c0 = (W.offset ? W.offset[b] : 0) + W.t;
    win[i] = tab[(k * W.C + c0) * rows + j];
}

// ftmpc_outcome_kernel with a reference column per vehicle and the closed-loop cost (include/ftmpc.h, ftmpc_mission.cost); launched
// in its place when the mission has tables or asks for cost.  The records of OutcomeParams are formed by the same expressions in the
// same order, so with a shared reference (xref_stride = 0) they are the bits ftmpc_outcome_kernel writes.  cost, in step order:
//   cost[0] += e' diag(Q) e                      e = robot_to_center(x_{t+1})[0:9] - (the vehicle's column t + 1)
//   cost[1] += w' diag(R) w                      w = D a - [Rot(q_t)^T uref_t[0:3]; uref_t[3:6]] - [f_virt; 0], a_i as `impulse`
//   cost[2]  = e' P e (+ V_nq(e))                the terminal cost of the last step's error, rewritten each step
// with the rotation ftmpc_cost_kernel applies to ur (mat3vec(rotT(q), .)), D, Q, R, P, f_virt of DeviceConsts, and q_t the
// quaternion of the state step t started from: qprev [B*4], staged from x by the host before the loop and rewritten here with
// x_{t+1}'s (each lane reads and writes its own four values).
struct MissionOut {
    const double* xref;       // column t + 1: per vehicle at xref + b * xref_stride (0: shared)
    int64_t xref_stride;
    const double* uref;       // nullptr (zero) or column t: per vehicle at uref + b * uref_stride
    int64_t uref_stride;
    double* qprev;            // nullptr (no cost) or [B*4]
    double* cost;             // nullptr or [B*3]
    const TermCost* tcost;    // nullptr or the non-quadratic terminal-cost terms
};

__global__ void __launch_bounds__(64) ftmpc_outcome_mission_kernel(const DeviceConsts C, const OutcomeParams O, const MissionOut M) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= O.B) return;
    const int NT = C.NT;
    const int32_t t = O.step;
    const double* xref = M.xref + b * M.xref_stride;
    double x[13];
    for (int i = 0; i < 13; ++i) x[i] = O.x[b * 13 + i];
    double e[9];
    {
        double RT[9], wxr[3], a[3], c[3];
        rotT(x + 6, RT);
        cross3(x + 10, C.r, wxr);
        mat3vec(RT, C.r, a);
        mat3vec(RT, wxr, c);
        for (int i = 0; i < 3; ++i) {
            e[i] = x[i] + a[i] - xref[i];
            e[3 + i] = x[3 + i] + c[i] - xref[3 + i];
            e[6 + i] = x[10 + i] - xref[6 + i];
        }
    }
    const double dt = C.dt;
    bool inside = true;
    for (int j = 0; j < 3; ++j) {
        const double n2 = e[3 * j] * e[3 * j] + e[3 * j + 1] * e[3 * j + 1] + e[3 * j + 2] * e[3 * j + 2];
        const double n = sqrt(n2);
        O.err_int[b * 3 + j] += dt * n2;
        O.err_max[b * 3 + j] = fmax(O.err_max[b * 3 + j], n);
        inside = inside && n <= O.tol[j];
    }
    if (!inside) O.settle[b] = t + 1;
    double del = 0.0, cmd = 0.0;
    double gen[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < NT; ++i) {
        const double c = O.ub[b * NT + i] > 0.0 ? O.u0[b * NT + i] : 0.0;
        cmd += c;
        del += c + O.stuck[b * NT + i];
        if (M.cost) {
            const double a = c + O.stuck[b * NT + i];
            for (int g = 0; g < 6; ++g) gen[g] += C.D[g * MAX_NT + i] * a;
        }
    }
    O.impulse[b * 2] += dt * del;
    O.impulse[b * 2 + 1] += dt * cmd;
    const int32_t st = O.status[b];
    if (st != 0) {
        if (O.unsolved[b]++ == 0) O.first_unsolved[b] = t;
    }
    if (O.astatus && O.astatus[b] != 0) O.alloc_failed[b] += 1;
    if (O.status_hist) O.status_hist[(int64_t)t * O.B + b] = st;
    if (O.term && O.tset[b] < 0) {
        const double* tb = O.term + (int64_t)O.term_rows * 9;
        bool in = true;
        for (int r = 0; r < O.term_rows; ++r) {
            double s = 0.0;
            for (int j = 0; j < 9; ++j) s += O.term[r * 9 + j] * e[j];
            in = in && s <= tb[r];
        }
        if (in) O.tset[b] = t;
    }
    if (M.cost) {
        double cq = 0.0;
        for (int a = 0; a < 9; ++a) cq += C.Q[a] * e[a] * e[a];
        double ur[6] = {0, 0, 0, 0, 0, 0};
        if (M.uref) {
            const double* uref = M.uref + b * M.uref_stride;
            double q[4], RT[9], f3[3] = {uref[0], uref[1], uref[2]}, o[3];
            for (int i = 0; i < 4; ++i) q[i] = M.qprev[b * 4 + i];
            rotT(q, RT);
            mat3vec(RT, f3, o);
            ur[0] = o[0]; ur[1] = o[1]; ur[2] = o[2];
            ur[3] = uref[3]; ur[4] = uref[4]; ur[5] = uref[5];
        }
        double cr = 0.0;
        for (int g = 0; g < 6; ++g) {
            const double w = gen[g] - ur[g] - (g < 3 ? C.fvirt[g] : 0.0);
            cr += C.R[g] * w * w;
        }
        double v = 0.0;
        for (int a = 0; a < 9; ++a)
            for (int c = 0; c < 9; ++c) v += e[a] * C.P[9 * a + c] * e[c];
        if (M.tcost) v += term_cost_nq(*M.tcost, e, nullptr);
        M.cost[b * 3] += cq;
        M.cost[b * 3 + 1] += cr;
        M.cost[b * 3 + 2] = v;
        for (int i = 0; i < 4; ++i) M.qprev[b * 4 + i] = x[6 + i];
    }
}

// ---------------------------------------------------------------------------------------------------------
// Pulsed (PWM) thrusters and valve lag in the plant (ftmpc_simulate_actuator_batch / ftmpc_simulate_wrench_actuator_batch;
// include/ftmpc.h, ftmpc_actuator).  ftmpc_plant_step_act_kernel is ftmpc_plant_step_var_kernel with the step cut into S sub-steps of
// h = dt / S, each one RK4 step under the force the valves deliver in it; launched in place of the plant kernel only when the call's
// actuator is not trivial.  Per thruster i the step has a level L_i and an on-window [s_i, s_i + k_i) of sub-steps:
//   proportional   L_i = ub_i > 0 ? u_i : 0                 k_i = S, s_i = 0
//   PWM            L_i = ub_i, d_i = clamp(u_i / ub_i, 0, 1)   k_i = floor(d_i S + 0.5), 0 where below min_on; s_i by the alignment
// (a dead thruster has L_i = 0, k_i = 0).  In sub-step j the target is g = L_i inside the window, else 0; the valve state a_i moves
// towards it with the on-pair (E, K) where g > a_i, else the off-pair: mean force m = g + (a_i - g) K, then a_i = g + (a_i - g) E.
// The four constants come from the host (no transcendental here); E = K = 0 is a valve without lag.  The sub-step's generalised force
// is D_b (m + stuck) (+ t_b); noise, renormalisation, histories and bad_count come once per step, exactly as the plant kernels'.
// The per-thruster rows (level, stuck, valve state, the step's force sum, ticks) are indexed by a loop whose bound is a run-time
// value; as per-lane arrays they would live in scratch, so they are LDS rows [MAX_NT][64], lane-consecutive (no bank conflict).  The
// nominal D is read at a wave-uniform index (scalar loads), a dispersed D_b in PlantVar's [k][B] layout.  The valve states of the
// call are component-major [NT][B]; delivered [B] and pulses [B] are buffers of the call, zeroed by the host.  (The kernel stands at
// the end of the file so that the build logs keep the source lines of every kernel above.)
// ---------------------------------------------------------------------------------------------------------
struct ActParams {
    int32_t pwm, substeps, min_on, align;   // align: 0 leading, 1 centred, 2 trailing
    double E_on, K_on, E_off, K_off;
    double* state;            // [NT][B] in/out
    double* delivered;        // [B]    += h sum_j sum_i (m_ij + stuck_i)
    int32_t* pulses;          // [B]    += #{i: k_i > 0} (PWM)
    double* applied_hist;     // nullptr or [T*B*NT]: (1/S) sum_j (m_ij + stuck_i)
    int32_t* ticks_hist;      // nullptr or [T*B*NT]: k_i (PWM)
};

__global__ void __launch_bounds__(64) ftmpc_plant_step_act_kernel(const DeviceConsts C, const SimParams S, const PlantVar V,
                                                                  const ActParams A) {
    __shared__ double s_lvl[MAX_NT][64], s_stk[MAX_NT][64], s_val[MAX_NT][64], s_sum[MAX_NT][64];
    __shared__ int32_t s_k[MAX_NT][64];
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t B = S.B;
    if (b >= B) return;      // (no barrier below: every lane touches its own column of the rows only)
    const int l = threadIdx.x;
    const int NT = C.NT, NS = A.substeps;
    int32_t npulse = 0;
    for (int i = 0; i < NT; ++i) {
        const double u = S.u0[b * NT + i];
        if (S.u_hist) S.u_hist[(S.step * B + b) * NT + i] = u;
        const double ub = S.ub[b * NT + i];
        double lvl = ub > 0.0 ? u : 0.0;
        int32_t k = NS;
        if (A.pwm) {
            const double d = ub > 0.0 ? fmin(fmax(u / ub, 0.0), 1.0) : 0.0;
            k = (int32_t)floor(d * NS + 0.5);
            if (k < A.min_on) k = 0;
            lvl = ub > 0.0 ? ub : 0.0;
            npulse += k > 0;
            if (A.ticks_hist) A.ticks_hist[(S.step * B + b) * NT + i] = k;
        }
        s_lvl[i][l] = lvl;
        s_stk[i][l] = S.stuck[b * NT + i];
        s_val[i][l] = A.state[(int64_t)i * B + b];
        s_sum[i][l] = 0.0;
        s_k[i][l] = k;
    }
    double J[9], Jinv[9], fm[3] = {0, 0, 0}, tq[3] = {0, 0, 0};
    const double inv_mass = V.inv_mass ? V.inv_mass[b] : C.inv_mass;
    if (V.J) {
        for (int k = 0; k < 9; ++k) {
            J[k] = V.J[k * B + b];
            Jinv[k] = V.J[(9 + k) * B + b];
        }
    } else {
        for (int k = 0; k < 9; ++k) {
            J[k] = C.J[k];
            Jinv[k] = C.Jinv[k];
        }
    }
    if (V.force)
        for (int k = 0; k < 3; ++k) fm[k] = V.force[k * B + b] * inv_mass;
    if (V.torque)
        for (int k = 0; k < 3; ++k) tq[k] = V.torque[k * B + b];
    double x[13], k1[13], k2[13], k3[13], k4[13], s[13];
    for (int i = 0; i < 13; ++i) x[i] = S.x[b * 13 + i];
    const double h = C.dt / NS;
    double deliv = A.delivered[b];
#pragma unroll 1
    for (int j = 0; j < NS; ++j) {
        double gen[6] = {0, 0, 0, tq[0], tq[1], tq[2]};
        double tot = 0.0;
        for (int i = 0; i < NT; ++i) {
            const int32_t k = s_k[i][l];
            const int32_t s0 = A.align == 0 ? 0 : (A.align == 1 ? (NS - k) / 2 : NS - k);
            const double g = (j >= s0 && j < s0 + k) ? s_lvl[i][l] : 0.0;
            const double a = s_val[i][l];
            const bool on = g > a;
            const double m = g + (a - g) * (on ? A.K_on : A.K_off);
            s_val[i][l] = g + (a - g) * (on ? A.E_on : A.E_off);
            const double f = m + s_stk[i][l];
            s_sum[i][l] += f;
            tot += f;
            if (V.D) {
                for (int c = 0; c < 6; ++c) gen[c] += V.D[(int64_t)(c * NT + i) * B + b] * f;
            } else {
                for (int c = 0; c < 6; ++c) gen[c] += C.D[c * MAX_NT + i] * f;
            }
        }
        deliv += h * tot;
        plant_f_var(inv_mass, J, Jinv, fm, x, gen, k1);
        for (int i = 0; i < 13; ++i) s[i] = x[i] + 0.5 * h * k1[i];
        plant_f_var(inv_mass, J, Jinv, fm, s, gen, k2);
        for (int i = 0; i < 13; ++i) s[i] = x[i] + 0.5 * h * k2[i];
        plant_f_var(inv_mass, J, Jinv, fm, s, gen, k3);
        for (int i = 0; i < 13; ++i) s[i] = x[i] + h * k3[i];
        plant_f_var(inv_mass, J, Jinv, fm, s, gen, k4);
        for (int i = 0; i < 13; ++i) x[i] += h / 6.0 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]);
    }
    A.delivered[b] = deliv;
    if (A.pwm) A.pulses[b] += npulse;
    for (int i = 0; i < NT; ++i) {
        A.state[(int64_t)i * B + b] = s_val[i][l];
        if (A.applied_hist) A.applied_hist[(S.step * B + b) * NT + i] = s_sum[i][l] / NS;
    }
    // noise, renormalisation, histories and bad_count exactly as ftmpc_plant_step_kernel
    for (int i = 0; i < 13; ++i) {
        const double a = i < 3 ? S.noise[0] : (i < 6 ? S.noise[1] : (i < 10 ? S.noise[2] : S.noise[3]));
        if (a > 0.0) x[i] += a * u01(S.seed, (unsigned long long)((S.step * S.index_total + S.index0 + b) * 13 + i));
    }
    const double qn = 1.0 / sqrt(x[6] * x[6] + x[7] * x[7] + x[8] * x[8] + x[9] * x[9]);
    for (int i = 6; i < 10; ++i) x[i] *= qn;
    for (int i = 0; i < 13; ++i) S.x[b * 13 + i] = x[i];
    if (S.x_hist)
        for (int i = 0; i < 13; ++i) S.x_hist[(S.step * B + b) * 13 + i] = x[i];
    if (S.bad_count && S.status && S.status[b] != 0) atomicAdd(&S.bad_count[S.step], 1);
}

// ---------------------------------------------------------------------------------------------------------
// Navigation errors and command latency (ftmpc_simulate_sensor_batch / ftmpc_simulate_wrench_sensor_batch; include/ftmpc.h,
// ftmpc_sensor).  ftmpc_sense_kernel runs before the solve of every step of a loop whose sensor is not trivial: it reads the TRUTH
// (a buffer of the call, which the plant, outcome and actuator kernels then read and write in place of the handle's x0), forms the
// measurement y_t, propagates it over the d queued commands when asked to, and writes the handle's x0, which every solver enqueue
// path reads.  A lane per vehicle.  The queue is a ring of d + 1 slots of [B][NT] (the layout of the handle's u0): slot0 holds a_t,
// the command the plant applies in this step, the following d - 1 slots a_{t+1} .. a_{t+d-1}.  The prediction is the plant
// kernel's RK4 step under the CONTROLLER's pattern and the config's model; gen[6] is accumulated inside the thruster loop and D read
// at wave-uniform indices, so no per-lane array is indexed by the run-time NT.  Gaussian draws by Box-Muller from two counters per
// channel; a group whose sigma is zero draws nothing.
// ---------------------------------------------------------------------------------------------------------
struct SenseParams {
    int64_t B;
    const double* x;          // [B*13] the truth
    double* y;                // [B*13] what the solve reads (the handle's x0)
    const double* ub;         // [B*NT] the controller's pattern
    const double* stuck;
    const double* ring;       // nullptr (d = 0) or [(d+1)][B*NT]
    int32_t nslots, slot0;    // d + 1, slot of a_t
    int32_t latency, predict;
    double sigma[4];
    const double* bias;       // nullptr or [B*12]
    unsigned long long seed;
    int64_t cstep, step, index0, index_total;   // step0 + t (the counter's step), t (the histories' row)
    double* meas_hist;        // nullptr or [T*B*13]
    double* pred_hist;        // nullptr or [T*B*13]
};

namespace {
__device__ __forceinline__ double gauss01(unsigned long long seed, unsigned long long c) {
    const double u1 = u01(seed, 2ull * c), u2 = u01(seed, 2ull * c + 1ull);
    return sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2);
}
}  // namespace

__global__ void __launch_bounds__(64) ftmpc_sense_kernel(const DeviceConsts C, const SenseParams P) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    const int NT = C.NT;
    double x[13];
    for (int i = 0; i < 13; ++i) x[i] = P.x[b * 13 + i];
    const unsigned long long c0 = (unsigned long long)((P.cstep * P.index_total + P.index0 + b) * 12);
    // e[0:3] position, e[3:6] velocity, e[6:9] the rotation vector theta, e[9:12] rate
    double e[12];
    for (int j = 0; j < 12; ++j) {
        const double sg = P.sigma[j / 3];
        double v = P.bias ? P.bias[b * 12 + j] : 0.0;
        if (sg > 0.0) v += sg * gauss01(P.seed, c0 + j);
        e[j] = v;
    }
    for (int i = 0; i < 3; ++i) {
        x[i] += e[i];
        x[3 + i] += e[3 + i];
        x[10 + i] += e[9 + i];
    }
    {
        const double t0 = e[6], t1 = e[7], t2 = e[8];
        const double n = sqrt(t0 * t0 + t1 * t1 + t2 * t2);
        const double cs = cos(0.5 * n), sn = n < 1e-8 ? 0.5 : sin(0.5 * n) / n;
        const double qx = x[6], qy = x[7], qz = x[8], qw = x[9];
        double q[4];
        q[0] = cs * qx + sn * (t2 * qy - t1 * qz + t0 * qw);
        q[1] = cs * qy + sn * (-t2 * qx + t0 * qz + t1 * qw);
        q[2] = cs * qz + sn * (t1 * qx - t0 * qy + t2 * qw);
        q[3] = cs * qw + sn * (-t0 * qx - t1 * qy - t2 * qz);
        const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int i = 0; i < 4; ++i) x[6 + i] = q[i] * qn;
    }
    if (P.meas_hist)
        for (int i = 0; i < 13; ++i) P.meas_hist[(P.step * P.B + b) * 13 + i] = x[i];
    if (P.predict) {
        const double dt = C.dt;
        int32_t slot = P.slot0;
#pragma unroll 1
        for (int j = 0; j < P.latency; ++j) {
            const double* a = P.ring + (int64_t)slot * P.B * NT;
            slot = slot + 1 == P.nslots ? 0 : slot + 1;
            double gen[6] = {0, 0, 0, 0, 0, 0};
            for (int i = 0; i < NT; ++i) {
                const double t = (P.ub[b * NT + i] > 0.0 ? a[b * NT + i] : 0.0) + P.stuck[b * NT + i];
                for (int g = 0; g < 6; ++g) gen[g] += C.D[g * MAX_NT + i] * t;
            }
            double k1[13], k2[13], k3[13], k4[13], s[13];
            plant_f(C, x, gen, k1);
            for (int i = 0; i < 13; ++i) s[i] = x[i] + 0.5 * dt * k1[i];
            plant_f(C, s, gen, k2);
            for (int i = 0; i < 13; ++i) s[i] = x[i] + 0.5 * dt * k2[i];
            plant_f(C, s, gen, k3);
            for (int i = 0; i < 13; ++i) s[i] = x[i] + dt * k3[i];
            plant_f(C, s, gen, k4);
            for (int i = 0; i < 13; ++i) x[i] += dt / 6.0 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]);
            const double qn = 1.0 / sqrt(x[6] * x[6] + x[7] * x[7] + x[8] * x[8] + x[9] * x[9]);
            for (int i = 6; i < 10; ++i) x[i] *= qn;
        }
        if (P.pred_hist)
            for (int i = 0; i < 13; ++i) P.pred_hist[(P.step * P.B + b) * 13 + i] = x[i];
    }
    for (int i = 0; i < 13; ++i) P.y[b * 13 + i] = x[i];
}

// ---------------------------------------------------------------------------------------------------------
// The navigation filter (ftmpc_simulate_estimator_batch / ftmpc_simulate_wrench_estimator_batch; include/ftmpc.h, ftmpc_estimator):
// a multiplicative (error-state) extended Kalman filter per vehicle between ftmpc_sense_kernel and the solve.  A lane per vehicle.
// phase 0 runs before the solve: the measurement update (twelve sequential scalar updates, H = I, diagonal R), est_hist, err_sq
// against the truth, the propagation over the d queued commands when the sensor predicts, and the handle's x0.  phase 1 runs after
// the plant step: P <- Phi P Phi' + Q with Phi = I + dt A(x^, gen) and x^ <- one RK4 step of the controller's model.
// The packed upper triangle of P (78 doubles) lives in registers: every index into it is a compile-time constant (the update loop is
// unrolled, the blocks of the time update are template arguments), so nothing goes to scratch.  Phi is never formed: it is block
// upper-bidiagonal over the 4 x 4 grid of 3 x 3 blocks (p, v, theta, w),
//        [ I  dt I    0      0   ]
//        [ 0    I     G      0   ]      G = -dt M [F/m]x,  H = I - dt [w]x,  W = I + dt J^-1 ([J w]x - [w]x J)
//        [ 0    0     H    dt I  ]
//        [ 0    0     0      W   ]
// so block (I, J) of Phi P Phi' needs the blocks (I, J), (I+1, J), (I, J+1), (I+1, J+1) of P alone, and walking the upper triangle
// row by row updates P in place with one 3 x 3 block of temporaries; the identity blocks are additions.  Device-side P is
// component-major [78][B], so that the lanes of a wave read consecutive addresses.
// ---------------------------------------------------------------------------------------------------------
struct FilterParams {
    int64_t B;
    int32_t init, update;     // phase 0: x^ = y_t and no update (first step of a call without xhat); the update runs (c % every == 0)
    int32_t latency, predict; // phase 0: the sensor's d and predict
    int32_t nslots, slot0;    // d + 1, slot of a_t
    const double* y;          // [B*13] y_t: what ftmpc_sense_kernel wrote, or the truth when the sensor is trivial
    const double* truth;      // [B*13]
    double* x0;               // [B*13] what the solve reads (the handle's x0)
    double* xhat;             // [B*13] the mean, in/out
    double* cov;              // [78][B] the packed covariance, in/out
    const double* ub;         // [B*NT] the controller's pattern
    const double* stuck;
    const double* ring;       // nullptr (d = 0) or [(d+1)][B*NT]
    const double* u;          // phase 1: [B*NT] a_t, the command the plant applied in this step
    double rsq[4], qsq[4];    // meas_sigma^2, proc_sigma^2 by group
    int64_t step;             // t (the histories' row)
    double* est_hist;         // nullptr or [T*B*13]
    double* pred_hist;        // nullptr or [T*B*13]
    double* err_sq;           // nullptr or [B*4], accumulated over the call's steps
};

namespace {
// packed index of P(i, j), upper triangle row-major
__host__ __device__ constexpr int tri(int i, int j) {
    return i <= j ? 12 * i - i * (i - 1) / 2 + (j - i) : 12 * j - j * (j - 1) / 2 + (i - j);
}

// gen = D ((ub > 0 ? a : 0) + stuck), accumulated inside the thruster loop (D at wave-uniform indices)
__device__ __forceinline__ void filter_gen(const DeviceConsts& C, const double* a, const double* ub, const double* stuck, int64_t b,
                                           double* gen) {
    const int NT = C.NT;
    for (int g = 0; g < 6; ++g) gen[g] = 0.0;
    for (int i = 0; i < NT; ++i) {
        const double t = (ub[b * NT + i] > 0.0 ? a[b * NT + i] : 0.0) + stuck[b * NT + i];
        for (int g = 0; g < 6; ++g) gen[g] += C.D[g * MAX_NT + i] * t;
    }
}

// one RK4 step of dt of the controller's model, the quaternion renormalised: the step ftmpc_sense_kernel predicts with
__device__ __forceinline__ void filter_rk4(const DeviceConsts& C, double* x, const double* gen) {
    const double dt = C.dt;
    double k1[13], k2[13], k3[13], k4[13], s[13];
    plant_f(C, x, gen, k1);
    for (int i = 0; i < 13; ++i) s[i] = x[i] + 0.5 * dt * k1[i];
    plant_f(C, s, gen, k2);
    for (int i = 0; i < 13; ++i) s[i] = x[i] + 0.5 * dt * k2[i];
    plant_f(C, s, gen, k3);
    for (int i = 0; i < 13; ++i) s[i] = x[i] + dt * k3[i];
    plant_f(C, s, gen, k4);
    for (int i = 0; i < 13; ++i) x[i] += dt / 6.0 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]);
    const double qn = 1.0 / sqrt(x[6] * x[6] + x[7] * x[7] + x[8] * x[8] + x[9] * x[9]);
    for (int i = 6; i < 10; ++i) x[i] *= qn;
}

// q turned by the body-frame rotation vector t, renormalised (the closed form of the sensor's attitude error)
__device__ __forceinline__ void filter_rotate(double* q, double t0, double t1, double t2) {
    const double n = sqrt(t0 * t0 + t1 * t1 + t2 * t2);
    const double cs = cos(0.5 * n), sn = n < 1e-8 ? 0.5 : sin(0.5 * n) / n;
    const double qx = q[0], qy = q[1], qz = q[2], qw = q[3];
    const double r0 = cs * qx + sn * (t2 * qy - t1 * qz + t0 * qw);
    const double r1 = cs * qy + sn * (-t2 * qx + t0 * qz + t1 * qw);
    const double r2 = cs * qz + sn * (t1 * qx - t0 * qy + t2 * qw);
    const double r3 = cs * qw + sn * (-t0 * qx - t1 * qy - t2 * qz);
    const double qn = 1.0 / sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
    q[0] = r0 * qn; q[1] = r1 * qn; q[2] = r2 * qn; q[3] = r3 * qn;
}

// th with rotate(qh, th) = yq: c = qh . yq, s = Xi(qh)' yq (flipped when c < 0), th = 2 atan2(|s|, c) / |s| s
__device__ __forceinline__ void filter_att_residual(const double* qh, const double* yq, double* th) {
    const double hx = qh[0], hy = qh[1], hz = qh[2], hw = qh[3];
    double c = hx * yq[0] + hy * yq[1] + hz * yq[2] + hw * yq[3];
    double s0 = hw * yq[0] + hz * yq[1] - hy * yq[2] - hx * yq[3];
    double s1 = -hz * yq[0] + hw * yq[1] + hx * yq[2] - hy * yq[3];
    double s2 = hy * yq[0] - hx * yq[1] + hw * yq[2] - hz * yq[3];
    if (c < 0.0) {
        c = -c; s0 = -s0; s1 = -s1; s2 = -s2;
    }
    const double n = sqrt(s0 * s0 + s1 * s1 + s2 * s2);
    const double f = n < 1e-8 ? 2.0 : 2.0 * atan2(n, c) / n;
    th[0] = f * s0; th[1] = f * s1; th[2] = f * s2;
}

// Row k of the component-major covariance, for this block's 64 vehicles, as a wave-uniform global pointer the lane number is added
// to as a 32-bit offset.  Without the readfirstlane the compiler folds the lane into the base and keeps 78 per-lane 64-bit addresses
// alive between the loads and the stores: as many registers as P itself.
typedef __attribute__((address_space(1))) double global_double;
__device__ __forceinline__ global_double* cov_row(const double* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (global_double*)(((unsigned long long)hi << 32) | lo);
}

// kinds of the 3 x 3 blocks of Phi
enum : int { FK_NONE = 0, FK_ID = 1, FK_TAU = 2, FK_DENSE = 3, FK_SKEW = 4 };      // FK_SKEW: I - [h]x, M = h (3 entries)
__host__ __device__ constexpr int fk_diag(int I) { return I < 2 ? FK_ID : (I == 2 ? FK_SKEW : FK_DENSE); }                       // Phi(I, I)
__host__ __device__ constexpr int fk_up(int I) { return I == 1 ? FK_DENSE : (I == 3 ? FK_NONE : FK_TAU); }   // Phi(I, I+1)

template <int I, int J>
__device__ __forceinline__ void cov_load(const double* P, double* X) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) X[3 * r + c] = P[tri(3 * I + r, 3 * J + c)];
}
// out += M X, M of the given kind
template <int KIND>
__device__ __forceinline__ void blk_lmul(const double* M, double tau, const double* X, double* out) {
    if constexpr (KIND == FK_ID) {
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] += X[i];
    } else if constexpr (KIND == FK_TAU) {
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] += tau * X[i];
    } else if constexpr (KIND == FK_DENSE) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) out[3 * r + c] += M[3 * r] * X[c] + M[3 * r + 1] * X[3 + c] + M[3 * r + 2] * X[6 + c];
    } else if constexpr (KIND == FK_SKEW) {      // X - h x (the columns of X)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            out[c] += X[c] - (M[1] * X[6 + c] - M[2] * X[3 + c]);
            out[3 + c] += X[3 + c] - (M[2] * X[c] - M[0] * X[6 + c]);
            out[6 + c] += X[6 + c] - (M[0] * X[3 + c] - M[1] * X[c]);
        }
    }
}
// out += X M'
template <int KIND>
__device__ __forceinline__ void blk_rmul_t(const double* M, double tau, const double* X, double* out) {
    if constexpr (KIND == FK_ID) {
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] += X[i];
    } else if constexpr (KIND == FK_TAU) {
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] += tau * X[i];
    } else if constexpr (KIND == FK_DENSE) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) out[3 * r + c] += X[3 * r] * M[3 * c] + X[3 * r + 1] * M[3 * c + 1] + X[3 * r + 2] * M[3 * c + 2];
    } else if constexpr (KIND == FK_SKEW) {      // X (I - [h]x)' = X + X [h]x: the rows of X
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            out[3 * r] += X[3 * r] + (X[3 * r + 1] * M[2] - X[3 * r + 2] * M[1]);
            out[3 * r + 1] += X[3 * r + 1] + (X[3 * r + 2] * M[0] - X[3 * r] * M[2]);
            out[3 * r + 2] += X[3 * r + 2] + (X[3 * r] * M[1] - X[3 * r + 1] * M[0]);
        }
    }
}
// block (I, J), I <= J, of Phi P Phi' in place.  G, H, W: the dense blocks (1, 2), (2, 2), (3, 3) of Phi
template <int I, int J>
__device__ __forceinline__ void cov_block(double* P, const double* G, const double* H, const double* W, double tau) {
    const double* const dI = I == 2 ? H : W;      // read for the dense kinds only
    const double* const dJ = J == 2 ? H : W;
    double A[9], X[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Nw[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    cov_load<I, J>(P, A);
    blk_lmul<fk_diag(I)>(dI, tau, A, X);
    if constexpr (fk_up(I) != FK_NONE) {
        cov_load<I + 1, J>(P, A);
        blk_lmul<fk_up(I)>(G, tau, A, X);
    }
    blk_rmul_t<fk_diag(J)>(dJ, tau, X, Nw);
    if constexpr (fk_up(J) != FK_NONE) {
        double Y[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        cov_load<I, J + 1>(P, A);
        blk_lmul<fk_diag(I)>(dI, tau, A, Y);
        if constexpr (fk_up(I) != FK_NONE) {
            cov_load<I + 1, J + 1>(P, A);
            blk_lmul<fk_up(I)>(G, tau, A, Y);
        }
        blk_rmul_t<fk_up(J)>(G, tau, Y, Nw);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (I < J || r <= c) P[tri(3 * I + r, 3 * J + c)] = Nw[3 * r + c];
}
}  // namespace

template <int PHASE>
__global__ void __launch_bounds__(64) ftmpc_filter_kernel(const DeviceConsts C, const FilterParams F) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= F.B) return;
    const int64_t B = F.B;
    double* const covb = F.cov + (int64_t)blockIdx.x * blockDim.x;
    const unsigned lane = threadIdx.x;
    double x[13], P[78];
    if constexpr (PHASE == 0) {
        double y[13];
        for (int i = 0; i < 13; ++i) y[i] = F.y[b * 13 + i];
        if (F.init) {
            for (int i = 0; i < 13; ++i) x[i] = y[i];
        } else {
            for (int i = 0; i < 13; ++i) x[i] = F.xhat[b * 13 + i];
        }
        if (!F.init && F.update) {
            // the residual's position, velocity and rate entries are formed from y and x^ where the update of their channel needs
            // them, and x^ is read again afterwards: next to the 156 registers of P only the attitude entries and d stay live
            double th[3], d[12];
            filter_att_residual(x + 6, y + 6, th);
#pragma unroll
            for (int k = 0; k < 78; ++k) P[k] = cov_row(covb + (int64_t)k * B)[lane];
#pragma unroll
            for (int i = 0; i < 12; ++i) d[i] = 0.0;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                const int jx = j < 6 ? j : j + 1;      // channel j's entry of x (rate: past the quaternion)
                const double rj = (j >= 6 && j < 9) ? th[j - 6] : F.y[b * 13 + jx] - F.xhat[b * 13 + jx];
                const double sj = P[tri(j, j)] + F.rsq[j / 3];
                const double inv = 1.0 / sj;
                double k[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) k[i] = P[tri(i, j)] * inv;
                const double e = rj - d[j];
#pragma unroll
                for (int i = 0; i < 12; ++i) d[i] += k[i] * e;
#pragma unroll
                for (int a = 0; a < 12; ++a) {
                    const double ska = sj * k[a];
#pragma unroll
                    for (int c = a; c < 12; ++c) P[tri(a, c)] -= ska * k[c];
                }
            }
#pragma unroll
            for (int k = 0; k < 78; ++k) cov_row(covb + (int64_t)k * B)[lane] = P[k];
            {     // (a volatile read: otherwise the compiler keeps the first read's values, in scratch, instead of reading again)
                const volatile double* const xh = F.xhat + b * 13;
                for (int i = 0; i < 13; ++i) x[i] = xh[i];
            }
            for (int i = 0; i < 3; ++i) {
                x[i] += d[i];
                x[3 + i] += d[3 + i];
                x[10 + i] += d[9 + i];
            }
            filter_rotate(x + 6, d[6], d[7], d[8]);
        }
        for (int i = 0; i < 13; ++i) F.xhat[b * 13 + i] = x[i];
        if (F.est_hist)
            for (int i = 0; i < 13; ++i) F.est_hist[(F.step * B + b) * 13 + i] = x[i];
        if (F.err_sq) {     // against the truth: position, velocity, attitude (the residual's theta), rate
            double xt[13], th[3], e[4] = {0, 0, 0, 0};
            for (int i = 0; i < 13; ++i) xt[i] = F.truth[b * 13 + i];
            filter_att_residual(x + 6, xt + 6, th);
            for (int i = 0; i < 3; ++i) {
                e[0] += (x[i] - xt[i]) * (x[i] - xt[i]);
                e[1] += (x[3 + i] - xt[3 + i]) * (x[3 + i] - xt[3 + i]);
                e[2] += th[i] * th[i];
                e[3] += (x[10 + i] - xt[10 + i]) * (x[10 + i] - xt[10 + i]);
            }
            for (int i = 0; i < 4; ++i) F.err_sq[b * 4 + i] += e[i];
        }
        if (F.predict) {
            int32_t slot = F.slot0;
#pragma unroll 1
            for (int j = 0; j < F.latency; ++j) {
                double gen[6];
                filter_gen(C, F.ring + (int64_t)slot * B * C.NT, F.ub, F.stuck, b, gen);
                slot = slot + 1 == F.nslots ? 0 : slot + 1;
                filter_rk4(C, x, gen);
            }
            if (F.pred_hist)
                for (int i = 0; i < 13; ++i) F.pred_hist[(F.step * B + b) * 13 + i] = x[i];
        }
        for (int i = 0; i < 13; ++i) F.x0[b * 13 + i] = x[i];
        return;
    }
    // PHASE 1: the time update under the command the plant applied in this step
    for (int i = 0; i < 13; ++i) x[i] = F.xhat[b * 13 + i];
#pragma unroll
    for (int k = 0; k < 78; ++k) P[k] = cov_row(covb + (int64_t)k * B)[lane];
    double gen[6];
    filter_gen(C, F.u, F.ub, F.stuck, b, gen);
    {
        const double dt = C.dt;
        const double qx = x[6], qy = x[7], qz = x[8], qw = x[9];
        const double w0 = x[10], w1 = x[11], w2 = x[12];
        // M = Rot(q)^T, the matrix plant_f applies to F / m
        const double M[9] = {qx * qx - qy * qy - qz * qz + qw * qw, 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw),
                             2 * (qx * qy + qz * qw), -qx * qx + qy * qy - qz * qz + qw * qw, 2 * (qy * qz - qx * qw),
                             2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), -qx * qx - qy * qy + qz * qz + qw * qw};
        const double f0 = gen[0] * C.inv_mass, f1 = gen[1] * C.inv_mass, f2 = gen[2] * C.inv_mass;
        double G[9], H[3], W[9];
        for (int r = 0; r < 3; ++r) {      // G = -dt M [f]x
            G[3 * r] = -dt * (M[3 * r + 1] * f2 - M[3 * r + 2] * f1);
            G[3 * r + 1] = -dt * (M[3 * r + 2] * f0 - M[3 * r] * f2);
            G[3 * r + 2] = -dt * (M[3 * r] * f1 - M[3 * r + 1] * f0);
        }
        H[0] = dt * w0; H[1] = dt * w1; H[2] = dt * w2;      // block (2, 2) is I - [H]x
        double Jw[3], S[9];
        for (int i = 0; i < 3; ++i) Jw[i] = C.J[3 * i] * w0 + C.J[3 * i + 1] * w1 + C.J[3 * i + 2] * w2;
        for (int c = 0; c < 3; ++c) {      // S = [J w]x - [w]x J, column c
            S[c] = -(-w2 * C.J[3 + c] + w1 * C.J[6 + c]);
            S[3 + c] = -(w2 * C.J[c] - w0 * C.J[6 + c]);
            S[6 + c] = -(-w1 * C.J[c] + w0 * C.J[3 + c]);
        }
        S[1] += -Jw[2]; S[2] += Jw[1];
        S[3] += Jw[2]; S[5] += -Jw[0];
        S[6] += -Jw[1]; S[7] += Jw[0];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                W[3 * r + c] = (r == c ? 1.0 : 0.0) + dt * (C.Jinv[3 * r] * S[c] + C.Jinv[3 * r + 1] * S[3 + c] + C.Jinv[3 * r + 2] * S[6 + c]);
        cov_block<0, 0>(P, G, H, W, dt);
        cov_block<0, 1>(P, G, H, W, dt);
        cov_block<0, 2>(P, G, H, W, dt);
        cov_block<0, 3>(P, G, H, W, dt);
        cov_block<1, 1>(P, G, H, W, dt);
        cov_block<1, 2>(P, G, H, W, dt);
        cov_block<1, 3>(P, G, H, W, dt);
        cov_block<2, 2>(P, G, H, W, dt);
        cov_block<2, 3>(P, G, H, W, dt);
        cov_block<3, 3>(P, G, H, W, dt);
#pragma unroll
        for (int i = 0; i < 12; ++i) P[tri(i, i)] += F.qsq[i / 3];
    }
#pragma unroll
    for (int k = 0; k < 78; ++k) cov_row(covb + (int64_t)k * B)[lane] = P[k];
    for (int i = 0; i < 13; ++i) x[i] = F.xhat[b * 13 + i];     // read again: not held across the covariance
    filter_rk4(C, x, gen);
    for (int i = 0; i < 13; ++i) F.xhat[b * 13 + i] = x[i];
}
template __global__ void ftmpc_filter_kernel<0>(const DeviceConsts, const FilterParams);
template __global__ void ftmpc_filter_kernel<1>(const DeviceConsts, const FilterParams);

// ---------------------------------------------------------------------------------------------------------
// Thruster fault diagnosis in the closed loop (ftmpc_simulate_diagnosis_batch; include/ftmpc.h, ftmpc_diagnosis): per vehicle a bank
// of one-sided CUSUM tests, one per hypothesis "thruster i is stuck at level l", on a parity residual: y_t against the open-loop
// prediction xt of the controller's model from the last used measurement.  A lane per vehicle.  phase 0 runs after the sense kernel
// and before the filter's phase 0 and the solve: test, decision (the controller's pattern switches here, as a schedule event with
// detect = t switches it), llr_hist, re-anchor.  phase 1 runs after the plant step: xt <- one RK4 step of the model under a_t and the
// controller's pattern, acc += the effective command, n += 1.
// Device-side acc and llr are component-major ([NT][B], [H][B]): the lanes of a wave read consecutive addresses.  The thruster loop
// is rolled; D, J^-1 and the levels are read at wave-uniform indices, acc_i and the statistics of thruster i are read and written
// inside the loop, the levels (at most 4) are unrolled and the arg-max is carried: no local array is indexed by the loop variable.
// A vehicle that switched writes switched[b] = 1; ftmpc_diagnose_repair_kernel then clips its shifted warm start to the new bounds,
// a lane per (vehicle, stage), the repair of ftmpc_fault_event_kernel.
// ---------------------------------------------------------------------------------------------------------
struct DiagParams {
    int64_t B;
    int32_t init, anchor;     // phase 0: first step of a call without state; c % every == 0 (the test may run, xt is re-anchored)
    int32_t L, K;             // levels per thruster, max_detect
    int32_t cstep, pad0;      // c = step0 + t: what detect_step records
    int64_t step;             // t (the history's row)
    const double* y;          // [B*13] y_t
    double* xt;               // [B*14] the prediction and n, in/out
    double* acc;              // [NT][B]
    double* llr;              // [H][B]
    double levels[4];
    double rsq[2], dsq[2];    // resid_sigma^2, drift_sigma^2: velocity, rate
    double threshold;
    double* ub;               // [B*NT] the controller's pattern, switched on a detection
    double* stuck;
    int32_t* count;           // [B] detections made
    int32_t* det_step;        // [B*K]
    int32_t* det_thruster;
    int32_t* det_level;
    int32_t* switched;        // [B] phase 0 writes 1 where the pattern switched at this step, else 0
    double* llr_hist;         // nullptr or [T*B*H]
    const double* u;          // phase 1: [B*NT] a_t, the command the plant applied in this step
};

template <int PHASE>
__global__ void __launch_bounds__(64) ftmpc_diagnose_kernel(const DeviceConsts C, const DiagParams P) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    const int64_t B = P.B;
    const int NT = C.NT, L = P.L, H = NT * L;
    double x[13];
    if constexpr (PHASE == 0) {
        double y[13];
        for (int i = 0; i < 13; ++i) y[i] = P.y[b * 13 + i];
        double* const hist = P.llr_hist ? P.llr_hist + (P.step * B + b) * H : nullptr;
        int32_t sw = 0;
        bool tested = false;
        if (P.init) {
#pragma unroll 1
            for (int k = 0; k < H; ++k) P.llr[(int64_t)k * B + b] = 0.0;
        } else {
            const double n = P.xt[b * 14 + 13];
            const int32_t cnt = P.count[b];
            if (P.anchor && n >= 1.0 && cnt < P.K) {
                tested = true;
                for (int i = 0; i < 13; ++i) x[i] = P.xt[b * 14 + i];
                // rho_v = M(q~)' (y_v - v~), M the matrix plant_f applies to F / m;  r_w = y_w - w~
                const double qx = x[6], qy = x[7], qz = x[8], qw = x[9];
                const double R00 = qx * qx - qy * qy - qz * qz + qw * qw, R01 = 2 * (qx * qy + qz * qw), R02 = 2 * (qx * qz - qy * qw);
                const double R10 = 2 * (qx * qy - qz * qw), R11 = -qx * qx + qy * qy - qz * qz + qw * qw, R12 = 2 * (qy * qz + qx * qw);
                const double R20 = 2 * (qx * qz + qy * qw), R21 = 2 * (qy * qz - qx * qw), R22 = -qx * qx - qy * qy + qz * qz + qw * qw;
                const double e0 = y[3] - x[3], e1 = y[4] - x[4], e2 = y[5] - x[5];
                const double rv0 = R00 * e0 + R01 * e1 + R02 * e2;
                const double rv1 = R10 * e0 + R11 * e1 + R12 * e2;
                const double rv2 = R20 * e0 + R21 * e1 + R22 * e2;
                const double rw0 = y[10] - x[10], rw1 = y[11] - x[11], rw2 = y[12] - x[12];
                const double isv = 1.0 / (P.rsq[0] + n * P.dsq[0]), isw = 1.0 / (P.rsq[1] + n * P.dsq[1]);
                const double kv = C.dt * C.inv_mass, dt = C.dt;
                double best = P.threshold;
                int besth = -1;
#pragma unroll 1
                for (int i = 0; i < NT; ++i) {
                    const bool live = P.ub[b * NT + i] > 0.0;
                    const double acci = P.acc[(int64_t)i * B + b];
                    const double d0 = C.D[i], d1 = C.D[MAX_NT + i], d2 = C.D[2 * MAX_NT + i];
                    const double t0 = C.D[3 * MAX_NT + i], t1 = C.D[4 * MAX_NT + i], t2 = C.D[5 * MAX_NT + i];
                    const double g0 = kv * d0, g1 = kv * d1, g2 = kv * d2;      // the signature per unit of delta
                    const double h0 = dt * (C.Jinv[0] * t0 + C.Jinv[1] * t1 + C.Jinv[2] * t2);
                    const double h1 = dt * (C.Jinv[3] * t0 + C.Jinv[4] * t1 + C.Jinv[5] * t2);
                    const double h2 = dt * (C.Jinv[6] * t0 + C.Jinv[7] * t1 + C.Jinv[8] * t2);
#pragma unroll
                    for (int l = 0; l < 4; ++l) {
                        if (l < L) {
                            const int64_t k = (int64_t)(i * L + l);
                            double v = 0.0;
                            if (live) {
                                const double delta = n * P.levels[l] - acci;
                                const double a0 = g0 * delta, a1 = g1 * delta, a2 = g2 * delta;
                                const double w0 = h0 * delta, w1 = h1 * delta, w2 = h2 * delta;
                                const double z = ((a0 * rv0 + a1 * rv1 + a2 * rv2) - 0.5 * (a0 * a0 + a1 * a1 + a2 * a2)) * isv +
                                                 ((w0 * rw0 + w1 * rw1 + w2 * rw2) - 0.5 * (w0 * w0 + w1 * w1 + w2 * w2)) * isw;
                                v = fmax(0.0, P.llr[k * B + b] + z);
                            }
                            P.llr[k * B + b] = v;
                            if (hist) hist[k] = v;
                            if (v > best) {      // (strictly: a tie stays with the lowest index)
                                best = v;
                                besth = (int)k;
                            }
                        }
                    }
                }
                if (besth >= 0) {
                    const int i = besth / L, l = besth - i * L;
                    const double lv = l == 0 ? P.levels[0] : (l == 1 ? P.levels[1] : (l == 2 ? P.levels[2] : P.levels[3]));
                    P.det_step[b * P.K + cnt] = P.cstep;
                    P.det_thruster[b * P.K + cnt] = i;
                    P.det_level[b * P.K + cnt] = l;
                    P.count[b] = cnt + 1;
                    P.ub[b * NT + i] = 0.0;
                    P.stuck[b * NT + i] = lv;
#pragma unroll 1
                    for (int k = 0; k < H; ++k) P.llr[(int64_t)k * B + b] = 0.0;
                    sw = 1;
                }
            }
        }
        if (hist && !tested) {
#pragma unroll 1
            for (int k = 0; k < H; ++k) hist[k] = P.llr[(int64_t)k * B + b];
        }
        P.switched[b] = sw;
        if (P.init || P.anchor) {
            for (int i = 0; i < 13; ++i) P.xt[b * 14 + i] = y[i];
            P.xt[b * 14 + 13] = 0.0;
#pragma unroll 1
            for (int i = 0; i < NT; ++i) P.acc[(int64_t)i * B + b] = 0.0;
        }
        return;
    }
    // PHASE 1: the model's step under the command the plant applied, c_i = ub_c,i > 0 ? a_t,i : 0
    for (int i = 0; i < 13; ++i) x[i] = P.xt[b * 14 + i];
    double gen[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll 1
    for (int i = 0; i < NT; ++i) {
        const double c = P.ub[b * NT + i] > 0.0 ? P.u[b * NT + i] : 0.0;
        const double t = c + P.stuck[b * NT + i];
        for (int g = 0; g < 6; ++g) gen[g] += C.D[g * MAX_NT + i] * t;
        P.acc[(int64_t)i * B + b] += c;
    }
    filter_rk4(C, x, gen);
    for (int i = 0; i < 13; ++i) P.xt[b * 14 + i] = x[i];
    P.xt[b * 14 + 13] += 1.0;
}
template __global__ void ftmpc_diagnose_kernel<0>(const DeviceConsts, const DiagParams);
template __global__ void ftmpc_diagnose_kernel<1>(const DeviceConsts, const DiagParams);

// The warm-start repair after a detection: U clipped elementwise to [0, ub_new], what ftmpc_fault_event_kernel does at a detected event
__global__ void __launch_bounds__(64) ftmpc_diagnose_repair_kernel(int64_t B, int N, int NT, const int32_t* switched, const double* ub,
                                                                  double* warmU) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * N) return;
    const int64_t b = i / N;
    if (!switched[b]) return;
    double* w = warmU + i * NT;
    for (int j = 0; j < NT; ++j) w[j] = fmin(fmax(w[j], 0.0), ub[b * NT + j]);
}

// ---------------------------------------------------------------------------------------------------------
// The diagnosis on the two-stage form (ftmpc_simulate_wrench_diagnosis_batch, ftmpc_hull_offsets_batch).  The input hull is a zonotope:
// its facet normals are the directions orthogonal to five independent generators, so the normals of a pattern with fewer live
// thrusters are among those of the pattern it started from, and only the offsets change:
//   c_i = a_r . D_i,   b_r = sum_i (c_i (ub_i / 2 + stuck_i) + |c_i| ub_i / 2)
// A row that is no longer a facet stays a supporting half-space.  A row of exactly six zeros is padding (b_r = 1).  The pattern is
// flat (its live thrusters do not span R^6: no two-stage form) when a non-padding row has no width,
//   w_r = sum_i |c_i| ub_i <= 1e-9 |a_r|_1 max|D| max_i ub_i.
// ftmpc_hull_offsets_kernel: a lane per vehicle, the row loop and the thruster loop rolled, six normal entries in registers, D at
// wave-uniform indices; `switched` (nullptr: every vehicle) limits it to the vehicles the diagnosis flagged.  The one kernel serves the
// stand-alone entry and the loop, so both produce the same bits.
// ftmpc_hull_switch_kernel: a lane per (vehicle, stage), after the offsets kernel.  Flat: no_hull takes the campaign step if it was -1,
// nothing else changes.  Otherwise stage 0's lane copies the new offsets into the controller's, and (repair) every lane pulls its own
// stage of the shifted warm start towards the new centre, as ftmpc_fault_event_kernel does at a detected event; the lanes read the
// offsets kernel's buffer, never what stage 0 writes.
// ---------------------------------------------------------------------------------------------------------
struct HullOffsets {
    int64_t B;
    int32_t hull_rows, pad0;
    const int32_t* switched;   // nullptr or [B]
    const double* ub;          // [B*NT]
    const double* stuck;
    const double* hullA;       // [n_sets*hull_rows*6]
    const int32_t* hullset;    // nullptr (one table) or [B]
    double* out_b;             // [B*hull_rows]
    int32_t* flat;             // nullptr or [B]
};

__global__ void __launch_bounds__(64) ftmpc_hull_offsets_kernel(const DeviceConsts C, const HullOffsets P) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    if (P.switched && !P.switched[b]) return;
    const int NT = C.NT, R = P.hull_rows;
    const double* const ub = P.ub + b * NT;
    const double* const stuck = P.stuck + b * NT;
    const double* const A = P.hullA + (P.hullset ? (int64_t)P.hullset[b] : 0) * R * 6;
    double dmax = 0.0, umax = 0.0;
#pragma unroll 1
    for (int i = 0; i < NT; ++i) {
        umax = fmax(umax, ub[i]);
        for (int g = 0; g < 6; ++g) dmax = fmax(dmax, fabs(C.D[g * MAX_NT + i]));
    }
    const double wtol = 1e-9 * dmax * umax;
    int32_t flat = 0;
#pragma unroll 1
    for (int r = 0; r < R; ++r) {
        const double a0 = A[r * 6], a1 = A[r * 6 + 1], a2 = A[r * 6 + 2], a3 = A[r * 6 + 3], a4 = A[r * 6 + 4], a5 = A[r * 6 + 5];
        const double a1n = fabs(a0) + fabs(a1) + fabs(a2) + fabs(a3) + fabs(a4) + fabs(a5);
        double acc = 0.0, w = 0.0;
#pragma unroll 1
        for (int i = 0; i < NT; ++i) {
            double c = a0 * C.D[i];
            c += a1 * C.D[MAX_NT + i];
            c += a2 * C.D[2 * MAX_NT + i];
            c += a3 * C.D[3 * MAX_NT + i];
            c += a4 * C.D[4 * MAX_NT + i];
            c += a5 * C.D[5 * MAX_NT + i];
            const double u = ub[i], ac = fabs(c);
            acc += c * (0.5 * u + stuck[i]) + ac * (0.5 * u);
            w += ac * u;
        }
        const bool pad = a1n == 0.0;
        P.out_b[b * R + r] = pad ? 1.0 : acc;
        if (!pad && w <= a1n * wtol) flat = 1;
    }
    if (P.flat) P.flat[b] = flat;
}

struct HullSwitch {
    int64_t B;
    int32_t hull_rows, repair;
    int32_t cstep, pad0;
    const int32_t* switched;   // [B]
    const int32_t* flat;       // [B]
    const double* ub;          // [B*NT] the controller's pattern after the switch
    const double* stuck;
    const double* hullA;
    const int32_t* hullset;    // nullptr or [B]
    const double* new_b;       // [B*hull_rows] what ftmpc_hull_offsets_kernel wrote
    double* hullb;             // [B*hull_rows] the controller's offsets
    double* warmG;             // [B*N*6]
    int32_t* no_hull;          // [B]
};

__global__ void __launch_bounds__(64) ftmpc_hull_switch_kernel(const DeviceConsts C, const HullSwitch P) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int N = C.N;
    if (i >= P.B * N) return;
    const int64_t b = i / N;
    const int k = (int)(i % N);
    if (!P.switched[b]) return;
    if (P.flat[b]) {
        if (k == 0 && P.no_hull[b] < 0) P.no_hull[b] = P.cstep;
        return;
    }
    const int R = P.hull_rows;
    const double* const nb = P.new_b + b * R;
    if (k == 0)
        for (int r = 0; r < R; ++r) P.hullb[b * R + r] = nb[r];
    if (!P.repair) return;
    double ctr[6], t[6], p[6];
    hull_centre(C, P.ub + b * C.NT, P.stuck + b * C.NT, ctr);
    double* g = P.warmG + (b * N + k) * 6;
    for (int j = 0; j < 6; ++j) t[j] = g[j];
    if (hull_pull(t, ctr, P.hullA + (P.hullset ? (int64_t)P.hullset[b] : 0) * R * 6, nb, R, p) > 0.0)
        for (int j = 0; j < 6; ++j) g[j] = p[j];
}

// ---------------------------------------------------------------------------------------------------------
// Disturbance estimation (ftmpc_simulate_disturbance_batch; include/ftmpc.h, ftmpc_disturbance): the navigation filter augmented by
// six states per vehicle, a constant force f^ [3] in the inertial frame and a constant torque t^ [3] in the body frame (frames and
// units of ftmpc_plant_model.force / .torque).  The error coordinates are (dp, dv, dtheta, dw, df, dt), 18 in all; the covariance
// travels in three pieces, P_xx (the estimator's 78 packed doubles), P_xd (12 x 6, row-major) and P_dd (packed upper triangle, 21), so
// that no lane ever holds all 171 doubles.  With H = [I 0] the x part of the update (P_xx, k_x, s_j, e_j) never reads P_xd or P_dd, and
// Phi = [[Phi_xx, E], [0, I]] with E non-zero in two blocks, (v, f) = (dt / m) I and (w, t) = dt J^-1.  Four launches per loop step,
// a lane per vehicle, every index into a register array a compile-time constant:
//   PHASE 0  before the solve: ftmpc_filter_kernel<0>'s update of x^ and P_xx (78 doubles in registers), est_hist and err_sq; it
//            leaves the twelve gain columns k_x, s_j and e_j = r_j - delta_j in the per-vehicle slot `gain` ([168][B])
//   PHASE 1  holds P_xd and P_dd (93 doubles) and consumes the slot: k_d = P_xd[j, :]' / s_j, delta_d += k_d e_j,
//            P_xd -= s_j k_x k_d', P_dd -= s_j k_d k_d'; then f^ += delta_d[0:3], t^ += delta_d[3:6], force_hist / torque_hist, the
//            propagation of x^ over the queued commands with the model with the estimate (pred_hist), and the solve's x0
//   PHASE 2  after the plant step: P_xx <- Phi_xx P_xx Phi_xx' + Q, ftmpc_filter_kernel<1>'s covariance walk
//   PHASE 3  Y = Phi_xx P_xd, Z = E P_dd;  P_xx += Y E' + E Y' + Z E' (read-modify-write of the rows PHASE 2 wrote),
//            P_xd <- Y + Z, P_dd += Q_d, then x^ <- one RK4 step of the model with the estimate, renormalised (f^, t^ unchanged)
// The model with the estimate is plant_f_var with the config's m and J:  v' = (Rot(q)^T F + f^) / m,  w' = J^-1 (tau + t^ - w x J w).
// Device-side P_xd, P_dd and the slot are component-major ([k][B]) as P_xx is; the estimate itself is vehicle-major [B][6] (f^, t^),
// the array the linearise kernel's DIST instantiations and ftmpc_diagnose_dist_kernel read.  (The kernels stand at the end of the file
// so that the build logs keep the source lines of every kernel above.)
// ---------------------------------------------------------------------------------------------------------
struct DistParams {
    double* cross;            // [72][B] P_xd, k = 6 i + c, in/out
    double* covd;             // [21][B] P_dd packed, in/out
    double* dist;             // [B*6] f^, t^, in/out
    double* gain;             // [168][B]: k_x of channel j at 12 j + i, s_j at 144 + j, e_j at 156 + j
    double qdsq[2];           // proc_sigma^2 of the disturbance: force, torque
    double* force_hist;       // nullptr or [T*B*3]: f^_{t|t}
    double* torque_hist;      // nullptr or [T*B*3]
};

namespace {
// packed index of P_dd(i, j), upper triangle row-major
__host__ __device__ constexpr int tri6(int i, int j) {
    return i <= j ? 6 * i - i * (i - 1) / 2 + (j - i) : 6 * j - j * (j - 1) / 2 + (i - j);
}

// one RK4 step of dt of the model with the estimate d = (f^, t^), the quaternion renormalised
__device__ __forceinline__ void filter_rk4_dist(const DeviceConsts& C, double* x, const double* gen, const double* d) {
    const double dt = C.dt;
    const double g[6] = {gen[0], gen[1], gen[2], gen[3] + d[3], gen[4] + d[4], gen[5] + d[5]};
    const double fm[3] = {d[0] * C.inv_mass, d[1] * C.inv_mass, d[2] * C.inv_mass};
    double k1[13], k2[13], k3[13], k4[13], s[13];
    plant_f_var(C.inv_mass, C.J, C.Jinv, fm, x, g, k1);
    for (int i = 0; i < 13; ++i) s[i] = x[i] + 0.5 * dt * k1[i];
    plant_f_var(C.inv_mass, C.J, C.Jinv, fm, s, g, k2);
    for (int i = 0; i < 13; ++i) s[i] = x[i] + 0.5 * dt * k2[i];
    plant_f_var(C.inv_mass, C.J, C.Jinv, fm, s, g, k3);
    for (int i = 0; i < 13; ++i) s[i] = x[i] + dt * k3[i];
    plant_f_var(C.inv_mass, C.J, C.Jinv, fm, s, g, k4);
    for (int i = 0; i < 13; ++i) x[i] += dt / 6.0 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]);
    const double qn = 1.0 / sqrt(x[6] * x[6] + x[7] * x[7] + x[8] * x[8] + x[9] * x[9]);
    for (int i = 6; i < 10; ++i) x[i] *= qn;
}

// the dense blocks of Phi_xx about x under gen, as ftmpc_filter_kernel<1> forms them: G = -dt M [F/m]x, H = dt w, W
__device__ __forceinline__ void filter_phi(const DeviceConsts& C, const double* x, const double* gen, double* G, double* H, double* W) {
    const double dt = C.dt;
    const double qx = x[6], qy = x[7], qz = x[8], qw = x[9];
    const double w0 = x[10], w1 = x[11], w2 = x[12];
    const double M[9] = {qx * qx - qy * qy - qz * qz + qw * qw, 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw),
                         2 * (qx * qy + qz * qw), -qx * qx + qy * qy - qz * qz + qw * qw, 2 * (qy * qz - qx * qw),
                         2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), -qx * qx - qy * qy + qz * qz + qw * qw};
    const double f0 = gen[0] * C.inv_mass, f1 = gen[1] * C.inv_mass, f2 = gen[2] * C.inv_mass;
    for (int r = 0; r < 3; ++r) {
        G[3 * r] = -dt * (M[3 * r + 1] * f2 - M[3 * r + 2] * f1);
        G[3 * r + 1] = -dt * (M[3 * r + 2] * f0 - M[3 * r] * f2);
        G[3 * r + 2] = -dt * (M[3 * r] * f1 - M[3 * r + 1] * f0);
    }
    H[0] = dt * w0; H[1] = dt * w1; H[2] = dt * w2;
    double Jw[3], S[9];
    for (int i = 0; i < 3; ++i) Jw[i] = C.J[3 * i] * w0 + C.J[3 * i + 1] * w1 + C.J[3 * i + 2] * w2;
    for (int c = 0; c < 3; ++c) {
        S[c] = -(-w2 * C.J[3 + c] + w1 * C.J[6 + c]);
        S[3 + c] = -(w2 * C.J[c] - w0 * C.J[6 + c]);
        S[6 + c] = -(-w1 * C.J[c] + w0 * C.J[3 + c]);
    }
    S[1] += -Jw[2]; S[2] += Jw[1];
    S[3] += Jw[2]; S[5] += -Jw[0];
    S[6] += -Jw[1]; S[7] += Jw[0];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            W[3 * r + c] = (r == c ? 1.0 : 0.0) + dt * (C.Jinv[3 * r] * S[c] + C.Jinv[3 * r + 1] * S[3 + c] + C.Jinv[3 * r + 2] * S[6 + c]);
}

// sum_c M[i][c] E[j][c] for a 6-column row M of P_xd's shape: E[3 + r][r] = kf (j in the v block), E[9 + r][3 + s] = dt J^-1[r][s]
// (j in the w block); i and j are constants once the callers' loops are unrolled
__device__ __forceinline__ double dist_row_et(const DeviceConsts& C, const double* Mi, int j, double kf) {
    if (j >= 3 && j < 6) return kf * Mi[j - 3];
    const int r = j - 9;
    return C.dt * (C.Jinv[3 * r] * Mi[3] + C.Jinv[3 * r + 1] * Mi[4] + C.Jinv[3 * r + 2] * Mi[5]);
}
__host__ __device__ constexpr bool dist_vw(int i) { return (i >= 3 && i < 6) || i >= 9; }
}  // namespace

template <int PHASE>
__global__ void __launch_bounds__(64) ftmpc_filter_dist_kernel(const DeviceConsts C, const FilterParams F, const DistParams D) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= F.B) return;
    const int64_t B = F.B;
    const int64_t blk = (int64_t)blockIdx.x * blockDim.x;
    double* const covb = F.cov + blk;
    double* const gainb = D.gain + blk;
    double* const crossb = D.cross + blk;
    double* const covdb = D.covd + blk;
    const unsigned lane = threadIdx.x;
    if constexpr (PHASE == 0) {
        double x[13], P[78], y[13];
        for (int i = 0; i < 13; ++i) y[i] = F.y[b * 13 + i];
        if (F.init) {
            for (int i = 0; i < 13; ++i) x[i] = y[i];
        } else {
            for (int i = 0; i < 13; ++i) x[i] = F.xhat[b * 13 + i];
        }
        if (!F.init && F.update) {
            double th[3], d[12];
            filter_att_residual(x + 6, y + 6, th);
#pragma unroll
            for (int k = 0; k < 78; ++k) P[k] = cov_row(covb + (int64_t)k * B)[lane];
#pragma unroll
            for (int i = 0; i < 12; ++i) d[i] = 0.0;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                const int jx = j < 6 ? j : j + 1;
                const double rj = (j >= 6 && j < 9) ? th[j - 6] : F.y[b * 13 + jx] - F.xhat[b * 13 + jx];
                const double sj = P[tri(j, j)] + F.rsq[j / 3];
                const double inv = 1.0 / sj;
                double k[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) k[i] = P[tri(i, j)] * inv;
                const double e = rj - d[j];
#pragma unroll
                for (int i = 0; i < 12; ++i) cov_row(gainb + (int64_t)(12 * j + i) * B)[lane] = k[i];
                cov_row(gainb + (int64_t)(144 + j) * B)[lane] = sj;
                cov_row(gainb + (int64_t)(156 + j) * B)[lane] = e;
#pragma unroll
                for (int i = 0; i < 12; ++i) d[i] += k[i] * e;
#pragma unroll
                for (int a = 0; a < 12; ++a) {
                    const double ska = sj * k[a];
#pragma unroll
                    for (int c = a; c < 12; ++c) P[tri(a, c)] -= ska * k[c];
                }
            }
#pragma unroll
            for (int k = 0; k < 78; ++k) cov_row(covb + (int64_t)k * B)[lane] = P[k];
            {     // (a volatile read, as in ftmpc_filter_kernel<0>: x^ is not held across the covariance)
                const volatile double* const xh = F.xhat + b * 13;
                for (int i = 0; i < 13; ++i) x[i] = xh[i];
            }
            for (int i = 0; i < 3; ++i) {
                x[i] += d[i];
                x[3 + i] += d[3 + i];
                x[10 + i] += d[9 + i];
            }
            filter_rotate(x + 6, d[6], d[7], d[8]);
        }
        for (int i = 0; i < 13; ++i) F.xhat[b * 13 + i] = x[i];
        if (F.est_hist)
            for (int i = 0; i < 13; ++i) F.est_hist[(F.step * B + b) * 13 + i] = x[i];
        if (F.err_sq) {
            double xt[13], th[3], e[4] = {0, 0, 0, 0};
            for (int i = 0; i < 13; ++i) xt[i] = F.truth[b * 13 + i];
            filter_att_residual(x + 6, xt + 6, th);
            for (int i = 0; i < 3; ++i) {
                e[0] += (x[i] - xt[i]) * (x[i] - xt[i]);
                e[1] += (x[3 + i] - xt[3 + i]) * (x[3 + i] - xt[3 + i]);
                e[2] += th[i] * th[i];
                e[3] += (x[10 + i] - xt[10 + i]) * (x[10 + i] - xt[10 + i]);
            }
            for (int i = 0; i < 4; ++i) F.err_sq[b * 4 + i] += e[i];
        }
        return;
    } else if constexpr (PHASE == 1) {
        double dd[6];
        for (int c = 0; c < 6; ++c) dd[c] = D.dist[b * 6 + c];
        if (!F.init && F.update) {
            double X[72], Pd[21], del[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 72; ++k) X[k] = cov_row(crossb + (int64_t)k * B)[lane];
#pragma unroll
            for (int k = 0; k < 21; ++k) Pd[k] = cov_row(covdb + (int64_t)k * B)[lane];
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                const double sj = cov_row(gainb + (int64_t)(144 + j) * B)[lane];
                const double e = cov_row(gainb + (int64_t)(156 + j) * B)[lane];
                const double inv = 1.0 / sj;
                double kd[6];
#pragma unroll
                for (int c = 0; c < 6; ++c) kd[c] = X[6 * j + c] * inv;
#pragma unroll
                for (int c = 0; c < 6; ++c) del[c] += kd[c] * e;
#pragma unroll
                for (int i = 0; i < 12; ++i) {
                    const double ski = sj * cov_row(gainb + (int64_t)(12 * j + i) * B)[lane];
#pragma unroll
                    for (int c = 0; c < 6; ++c) X[6 * i + c] -= ski * kd[c];
                }
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    const double ska = sj * kd[a];
#pragma unroll
                    for (int c = a; c < 6; ++c) Pd[tri6(a, c)] -= ska * kd[c];
                }
            }
#pragma unroll
            for (int k = 0; k < 72; ++k) cov_row(crossb + (int64_t)k * B)[lane] = X[k];
#pragma unroll
            for (int k = 0; k < 21; ++k) cov_row(covdb + (int64_t)k * B)[lane] = Pd[k];
            for (int c = 0; c < 6; ++c) dd[c] += del[c];
            for (int c = 0; c < 6; ++c) D.dist[b * 6 + c] = dd[c];
        }
        if (D.force_hist)
            for (int c = 0; c < 3; ++c) D.force_hist[(F.step * B + b) * 3 + c] = dd[c];
        if (D.torque_hist)
            for (int c = 0; c < 3; ++c) D.torque_hist[(F.step * B + b) * 3 + c] = dd[3 + c];
        double x[13];
        for (int i = 0; i < 13; ++i) x[i] = F.xhat[b * 13 + i];
        if (F.predict) {
            int32_t slot = F.slot0;
#pragma unroll 1
            for (int j = 0; j < F.latency; ++j) {
                double gen[6];
                filter_gen(C, F.ring + (int64_t)slot * B * C.NT, F.ub, F.stuck, b, gen);
                slot = slot + 1 == F.nslots ? 0 : slot + 1;
                filter_rk4_dist(C, x, gen, dd);
            }
            if (F.pred_hist)
                for (int i = 0; i < 13; ++i) F.pred_hist[(F.step * B + b) * 13 + i] = x[i];
        }
        for (int i = 0; i < 13; ++i) F.x0[b * 13 + i] = x[i];
        return;
    } else if constexpr (PHASE == 2) {
        double x[13], P[78], gen[6], G[9], H[3], W[9];
        for (int i = 0; i < 13; ++i) x[i] = F.xhat[b * 13 + i];
#pragma unroll
        for (int k = 0; k < 78; ++k) P[k] = cov_row(covb + (int64_t)k * B)[lane];
        filter_gen(C, F.u, F.ub, F.stuck, b, gen);
        filter_phi(C, x, gen, G, H, W);
        const double dt = C.dt;
        cov_block<0, 0>(P, G, H, W, dt);
        cov_block<0, 1>(P, G, H, W, dt);
        cov_block<0, 2>(P, G, H, W, dt);
        cov_block<0, 3>(P, G, H, W, dt);
        cov_block<1, 1>(P, G, H, W, dt);
        cov_block<1, 2>(P, G, H, W, dt);
        cov_block<1, 3>(P, G, H, W, dt);
        cov_block<2, 2>(P, G, H, W, dt);
        cov_block<2, 3>(P, G, H, W, dt);
        cov_block<3, 3>(P, G, H, W, dt);
#pragma unroll
        for (int i = 0; i < 12; ++i) P[tri(i, i)] += F.qsq[i / 3];
#pragma unroll
        for (int k = 0; k < 78; ++k) cov_row(covb + (int64_t)k * B)[lane] = P[k];
        return;
    } else {
        double x[13], gen[6], G[9], H[3], W[9];
        for (int i = 0; i < 13; ++i) x[i] = F.xhat[b * 13 + i];
        filter_gen(C, F.u, F.ub, F.stuck, b, gen);
        filter_phi(C, x, gen, G, H, W);
        const double dt = C.dt, kf = C.dt * C.inv_mass;
        double Zv[18], Zw[18];      // Z = E P_dd: the rows of the v block and of the w block
        {
            double Pd[21];
#pragma unroll
            for (int k = 0; k < 21; ++k) Pd[k] = cov_row(covdb + (int64_t)k * B)[lane];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    Zv[6 * r + c] = kf * Pd[tri6(r, c)];
                    Zw[6 * r + c] = dt * (C.Jinv[3 * r] * Pd[tri6(3, c)] + C.Jinv[3 * r + 1] * Pd[tri6(4, c)] + C.Jinv[3 * r + 2] * Pd[tri6(5, c)]);
                }
#pragma unroll
            for (int i = 0; i < 6; ++i) Pd[tri6(i, i)] += D.qdsq[i / 3];
#pragma unroll
            for (int k = 0; k < 21; ++k) cov_row(covdb + (int64_t)k * B)[lane] = Pd[k];
        }
        double X[72];
#pragma unroll
        for (int k = 0; k < 72; ++k) X[k] = cov_row(crossb + (int64_t)k * B)[lane];
        // Y = Phi_xx P_xd in place: row block I needs the old blocks I and I + 1 alone
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const double p0 = X[c], p1 = X[6 + c], p2 = X[12 + c];
            const double v0 = X[18 + c], v1 = X[24 + c], v2 = X[30 + c];
            const double a0 = X[36 + c], a1 = X[42 + c], a2 = X[48 + c];
            const double r0 = X[54 + c], r1 = X[60 + c], r2 = X[66 + c];
            X[c] = p0 + dt * v0;
            X[6 + c] = p1 + dt * v1;
            X[12 + c] = p2 + dt * v2;
            X[18 + c] = v0 + (G[0] * a0 + G[1] * a1 + G[2] * a2);
            X[24 + c] = v1 + (G[3] * a0 + G[4] * a1 + G[5] * a2);
            X[30 + c] = v2 + (G[6] * a0 + G[7] * a1 + G[8] * a2);
            X[36 + c] = a0 - (H[1] * a2 - H[2] * a1) + dt * r0;
            X[42 + c] = a1 - (H[2] * a0 - H[0] * a2) + dt * r1;
            X[48 + c] = a2 - (H[0] * a1 - H[1] * a0) + dt * r2;
            X[54 + c] = W[0] * r0 + W[1] * r1 + W[2] * r2;
            X[60 + c] = W[3] * r0 + W[4] * r1 + W[5] * r2;
            X[66 + c] = W[6] * r0 + W[7] * r1 + W[8] * r2;
        }
        // P_xx(i, j) += (Y E')(i, j) + (Y E')(j, i) + (Z E')(i, j), i <= j: zero unless i or j lies in the v or the w block
#pragma unroll
        for (int i = 0; i < 12; ++i)
#pragma unroll
            for (int j = i; j < 12; ++j) {
                if (!dist_vw(i) && !dist_vw(j)) continue;
                double t = 0.0;
                if (dist_vw(j)) t += dist_row_et(C, X + 6 * i, j, kf);
                if (dist_vw(i)) t += dist_row_et(C, X + 6 * j, i, kf);
                if (dist_vw(i) && dist_vw(j)) t += dist_row_et(C, i < 6 ? Zv + 6 * (i - 3) : Zw + 6 * (i - 9), j, kf);
                cov_row(covb + (int64_t)tri(i, j) * B)[lane] += t;
            }
        // P_xd = Y + Z
#pragma unroll
        for (int k = 0; k < 18; ++k) {
            X[18 + k] += Zv[k];
            X[54 + k] += Zw[k];
        }
#pragma unroll
        for (int k = 0; k < 72; ++k) cov_row(crossb + (int64_t)k * B)[lane] = X[k];
        double dd[6];
        for (int c = 0; c < 6; ++c) dd[c] = D.dist[b * 6 + c];
        filter_rk4_dist(C, x, gen, dd);
        for (int i = 0; i < 13; ++i) F.xhat[b * 13 + i] = x[i];
    }
}
template __global__ void ftmpc_filter_dist_kernel<0>(const DeviceConsts, const FilterParams, const DistParams);
template __global__ void ftmpc_filter_dist_kernel<1>(const DeviceConsts, const FilterParams, const DistParams);
template __global__ void ftmpc_filter_dist_kernel<2>(const DeviceConsts, const FilterParams, const DistParams);
template __global__ void ftmpc_filter_dist_kernel<3>(const DeviceConsts, const FilterParams, const DistParams);

// phase 1 of ftmpc_diagnose_kernel with the model with the estimate: xt <- one RK4 step under a_t, the controller's pattern and
// (f^, t^) of this step's filter update; acc and n as there.  The test (phase 0) is ftmpc_diagnose_kernel<0>'s.
__global__ void __launch_bounds__(64) ftmpc_diagnose_dist_kernel(const DeviceConsts C, const DiagParams P, const double* dist) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    const int64_t B = P.B;
    const int NT = C.NT;
    double x[13], dd[6];
    for (int i = 0; i < 13; ++i) x[i] = P.xt[b * 14 + i];
    for (int c = 0; c < 6; ++c) dd[c] = dist[b * 6 + c];
    double gen[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll 1
    for (int i = 0; i < NT; ++i) {
        const double c = P.ub[b * NT + i] > 0.0 ? P.u[b * NT + i] : 0.0;
        const double t = c + P.stuck[b * NT + i];
        for (int g = 0; g < 6; ++g) gen[g] += C.D[g * MAX_NT + i] * t;
        P.acc[(int64_t)i * B + b] += c;
    }
    filter_rk4_dist(C, x, gen, dd);
    for (int i = 0; i < 13; ++i) P.xt[b * 14 + i] = x[i];
    P.xt[b * 14 + 13] += 1.0;
}

// ---------------------------------------------------------------------------------------------------------
// Sensor bias estimation (ftmpc_simulate_bias_batch; include/ftmpc.h, ftmpc_bias_estimate): the navigation filter augmented by six
// states per vehicle, a constant velocity bias b_v^ [3] (m/s) and a constant rate bias b_w^ [3] (rad/s):  y_v = v + b_v + n,
// y_w = w + b_w + n.  The pieces travel in the MEASURED error coordinates m = (dp, dv + db_v, dtheta, dw + db_w) with b = (db_v, db_w)
// unchanged, P^m = T P T', T = [[I, HB], [0, I]]: there H = [I 0], so the x pass of the update is the estimator's own on P_mm and the
// structure is ftmpc_filter_dist_kernel's: P_mm (78 packed), P_mb (12 x 6) and P_bb (21 packed), component-major [k][B], the 168-double
// gain slot between the two passes, every index into a register array a compile-time constant.  Four launches per loop step:
//   PHASE 0  before the solve: the estimator's update of P_mm with the residual y [-] x~, x~ = x^ with v^ + b_v^ and w^ + b_w^;
//            x^ <- x^ [+] delta_m; the gain slot as ftmpc_filter_dist_kernel<0> leaves it
//   PHASE 1  holds P_mb and P_bb and consumes the slot (delta_b); v^ -= delta_b[0:3], w^ -= delta_b[3:6] (delta_x = delta_m -
//            HB delta_b), b^ += delta_b; est_hist, bias_hist, err_sq, the propagation of x^ over the queued commands with the plain
//            model (the bias does not enter the dynamics; pred_hist) and the solve's x0
//   PHASE 2  after the plant step: P_mm <- Phi_xx P_mm Phi_xx' + Q_xx, ftmpc_filter_kernel<1>'s covariance walk
//   PHASE 3  csrc/ftmpc_bias_block.h: Y = Phi_xx P_mb, Z = E P_bb, E = (I - Phi_xx) HB;  P_mm += Y E' + E Y' + Z E' + the Q^m
//            diagonal terms,  P_mb <- Y + Z + Q_xb,  P_bb += Q_bb;  then x^ <- one plain RK4 step, renormalised (b^ unchanged)
// On the first step of a call without xhat, x^ = y_t with b^ taken off the velocity and the rate.
// ---------------------------------------------------------------------------------------------------------
}  // namespace ftmpc
#include "ftmpc_bias_block.h"      // (included here, not at the top: the build logs keep the source lines of every kernel above)
namespace ftmpc {
struct BiasParams {
    double* cross;            // [72][B] P_mb, k = 6 i + c, in/out
    double* covb;             // [21][B] P_bb packed, in/out
    double* bias;             // [B*6] b_v^, b_w^, in/out
    double* gain;             // [168][B]: k_x of channel j at 12 j + i, s_j at 144 + j, e_j at 156 + j
    double qbsq[2];           // proc_sigma^2 of the bias: velocity, rate
    double* bias_hist;        // nullptr or [T*B*6]: b^_{t|t}
};

template <int PHASE>
__global__ void __launch_bounds__(64) ftmpc_filter_bias_kernel(const DeviceConsts C, const FilterParams F, const BiasParams D) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= F.B) return;
    const int64_t B = F.B;
    const int64_t blk = (int64_t)blockIdx.x * blockDim.x;
    double* const covb = F.cov + blk;
    double* const gainb = D.gain + blk;
    double* const crossb = D.cross + blk;
    double* const covbb = D.covb + blk;
    const unsigned lane = threadIdx.x;
    if constexpr (PHASE == 0) {
        double x[13], P[78], y[13];
        for (int i = 0; i < 13; ++i) y[i] = F.y[b * 13 + i];
        if (F.init) {
            for (int i = 0; i < 13; ++i) x[i] = y[i];
        } else {
            for (int i = 0; i < 13; ++i) x[i] = F.xhat[b * 13 + i];
        }
        if (!F.init && F.update) {
            double th[3], d[12];
            filter_att_residual(x + 6, y + 6, th);
#pragma unroll
            for (int k = 0; k < 78; ++k) P[k] = cov_row(covb + (int64_t)k * B)[lane];
#pragma unroll
            for (int i = 0; i < 12; ++i) d[i] = 0.0;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                const int jx = j < 6 ? j : j + 1;
                double rj;
                if (j >= 6 && j < 9)
                    rj = th[j - 6];
                else if (j < 3)
                    rj = F.y[b * 13 + jx] - F.xhat[b * 13 + jx];
                else      // velocity and rate: against x~ = x^ + b^
                    rj = F.y[b * 13 + jx] - (F.xhat[b * 13 + jx] + D.bias[b * 6 + (j < 6 ? j - 3 : j - 6)]);
                const double sj = P[tri(j, j)] + F.rsq[j / 3];
                const double inv = 1.0 / sj;
                double k[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) k[i] = P[tri(i, j)] * inv;
                const double e = rj - d[j];
#pragma unroll
                for (int i = 0; i < 12; ++i) cov_row(gainb + (int64_t)(12 * j + i) * B)[lane] = k[i];
                cov_row(gainb + (int64_t)(144 + j) * B)[lane] = sj;
                cov_row(gainb + (int64_t)(156 + j) * B)[lane] = e;
#pragma unroll
                for (int i = 0; i < 12; ++i) d[i] += k[i] * e;
#pragma unroll
                for (int a = 0; a < 12; ++a) {
                    const double ska = sj * k[a];
#pragma unroll
                    for (int c = a; c < 12; ++c) P[tri(a, c)] -= ska * k[c];
                }
            }
#pragma unroll
            for (int k = 0; k < 78; ++k) cov_row(covb + (int64_t)k * B)[lane] = P[k];
            {     // (a volatile read, as in ftmpc_filter_kernel<0>: x^ is not held across the covariance)
                const volatile double* const xh = F.xhat + b * 13;
                for (int i = 0; i < 13; ++i) x[i] = xh[i];
            }
            for (int i = 0; i < 3; ++i) {
                x[i] += d[i];
                x[3 + i] += d[3 + i];
                x[10 + i] += d[9 + i];
            }
            filter_rotate(x + 6, d[6], d[7], d[8]);
        }
        for (int i = 0; i < 13; ++i) F.xhat[b * 13 + i] = x[i];      // x^ [+] delta_m: the bias pass takes HB delta_b off
        return;
    } else if constexpr (PHASE == 1) {
        double bb[6], x[13];
        for (int c = 0; c < 6; ++c) bb[c] = D.bias[b * 6 + c];
        for (int i = 0; i < 13; ++i) x[i] = F.xhat[b * 13 + i];
        if (F.init) {
            for (int c = 0; c < 3; ++c) {
                x[3 + c] -= bb[c];
                x[10 + c] -= bb[3 + c];
            }
        }
        if (!F.init && F.update) {
            double X[72], Pb[21], del[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 72; ++k) X[k] = cov_row(crossb + (int64_t)k * B)[lane];
#pragma unroll
            for (int k = 0; k < 21; ++k) Pb[k] = cov_row(covbb + (int64_t)k * B)[lane];
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                const double sj = cov_row(gainb + (int64_t)(144 + j) * B)[lane];
                const double e = cov_row(gainb + (int64_t)(156 + j) * B)[lane];
                const double inv = 1.0 / sj;
                double kd[6];
#pragma unroll
                for (int c = 0; c < 6; ++c) kd[c] = X[6 * j + c] * inv;
#pragma unroll
                for (int c = 0; c < 6; ++c) del[c] += kd[c] * e;
#pragma unroll
                for (int i = 0; i < 12; ++i) {
                    const double ski = sj * cov_row(gainb + (int64_t)(12 * j + i) * B)[lane];
#pragma unroll
                    for (int c = 0; c < 6; ++c) X[6 * i + c] -= ski * kd[c];
                }
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    const double ska = sj * kd[a];
#pragma unroll
                    for (int c = a; c < 6; ++c) Pb[tri6(a, c)] -= ska * kd[c];
                }
            }
#pragma unroll
            for (int k = 0; k < 72; ++k) cov_row(crossb + (int64_t)k * B)[lane] = X[k];
#pragma unroll
            for (int k = 0; k < 21; ++k) cov_row(covbb + (int64_t)k * B)[lane] = Pb[k];
            for (int c = 0; c < 3; ++c) {      // delta_x = delta_m - HB delta_b
                x[3 + c] -= del[c];
                x[10 + c] -= del[3 + c];
            }
            for (int c = 0; c < 6; ++c) bb[c] += del[c];
            for (int c = 0; c < 6; ++c) D.bias[b * 6 + c] = bb[c];
        }
        if (F.init || F.update)
            for (int i = 0; i < 13; ++i) F.xhat[b * 13 + i] = x[i];
        if (F.est_hist)
            for (int i = 0; i < 13; ++i) F.est_hist[(F.step * B + b) * 13 + i] = x[i];
        if (D.bias_hist)
            for (int c = 0; c < 6; ++c) D.bias_hist[(F.step * B + b) * 6 + c] = bb[c];
        if (F.err_sq) {     // against the truth: position, velocity, attitude (the residual's theta), rate
            double xt[13], th[3], e[4] = {0, 0, 0, 0};
            for (int i = 0; i < 13; ++i) xt[i] = F.truth[b * 13 + i];
            filter_att_residual(x + 6, xt + 6, th);
            for (int i = 0; i < 3; ++i) {
                e[0] += (x[i] - xt[i]) * (x[i] - xt[i]);
                e[1] += (x[3 + i] - xt[3 + i]) * (x[3 + i] - xt[3 + i]);
                e[2] += th[i] * th[i];
                e[3] += (x[10 + i] - xt[10 + i]) * (x[10 + i] - xt[10 + i]);
            }
            for (int i = 0; i < 4; ++i) F.err_sq[b * 4 + i] += e[i];
        }
        if (F.predict) {
            int32_t slot = F.slot0;
#pragma unroll 1
            for (int j = 0; j < F.latency; ++j) {
                double gen[6];
                filter_gen(C, F.ring + (int64_t)slot * B * C.NT, F.ub, F.stuck, b, gen);
                slot = slot + 1 == F.nslots ? 0 : slot + 1;
                filter_rk4(C, x, gen);
            }
            if (F.pred_hist)
                for (int i = 0; i < 13; ++i) F.pred_hist[(F.step * B + b) * 13 + i] = x[i];
        }
        for (int i = 0; i < 13; ++i) F.x0[b * 13 + i] = x[i];
        return;
    } else if constexpr (PHASE == 2) {
        double x[13], P[78], gen[6], G[9], H[3], W[9];
        for (int i = 0; i < 13; ++i) x[i] = F.xhat[b * 13 + i];
#pragma unroll
        for (int k = 0; k < 78; ++k) P[k] = cov_row(covb + (int64_t)k * B)[lane];
        filter_gen(C, F.u, F.ub, F.stuck, b, gen);
        filter_phi(C, x, gen, G, H, W);
        const double dt = C.dt;
        cov_block<0, 0>(P, G, H, W, dt);
        cov_block<0, 1>(P, G, H, W, dt);
        cov_block<0, 2>(P, G, H, W, dt);
        cov_block<0, 3>(P, G, H, W, dt);
        cov_block<1, 1>(P, G, H, W, dt);
        cov_block<1, 2>(P, G, H, W, dt);
        cov_block<1, 3>(P, G, H, W, dt);
        cov_block<2, 2>(P, G, H, W, dt);
        cov_block<2, 3>(P, G, H, W, dt);
        cov_block<3, 3>(P, G, H, W, dt);
#pragma unroll
        for (int i = 0; i < 12; ++i) P[tri(i, i)] += F.qsq[i / 3];
#pragma unroll
        for (int k = 0; k < 78; ++k) cov_row(covb + (int64_t)k * B)[lane] = P[k];
        return;
    } else {
        double x[13], gen[6], G[9], H[3], W[9], EW[9];
        for (int i = 0; i < 13; ++i) x[i] = F.xhat[b * 13 + i];
        filter_gen(C, F.u, F.ub, F.stuck, b, gen);
        filter_phi(C, x, gen, G, H, W);
        const double dt = C.dt;
        const double qb[2] = {D.qbsq[0], D.qbsq[1]};
        ftmpc_bias::e_block(W, EW);
        double Pb[21], Zw[18], X[72];     // Pb stays P_bb of before Q_bb: Z = E P_bb is formed from it where it is used
#pragma unroll
        for (int k = 0; k < 21; ++k) Pb[k] = cov_row(covbb + (int64_t)k * B)[lane];
        ftmpc_bias::z_rows_w(EW, Pb, Zw);
#pragma unroll
        for (int i = 0; i < 6; ++i) cov_row(covbb + (int64_t)tri6(i, i) * B)[lane] = Pb[tri6(i, i)] + qb[i / 3];
#pragma unroll
        for (int k = 0; k < 72; ++k) X[k] = cov_row(crossb + (int64_t)k * B)[lane];
        ftmpc_bias::phi_x(dt, G, H, W, X);
        // (read-modify-write of the rows PHASE 2 wrote)
#pragma unroll
        for (int i = 0; i < 12; ++i)
#pragma unroll
            for (int j = i; j < 12; ++j)
                if (ftmpc_bias::xx_touched(i, j))
                    cov_row(covb + (int64_t)tri(i, j) * B)[lane] += ftmpc_bias::xx_gain(dt, EW, X, Pb, Zw, qb, i, j);
        ftmpc_bias::xb_finish(dt, Pb, Zw, qb, X);
#pragma unroll
        for (int k = 0; k < 72; ++k) cov_row(crossb + (int64_t)k * B)[lane] = X[k];
        filter_rk4(C, x, gen);
        for (int i = 0; i < 13; ++i) F.xhat[b * 13 + i] = x[i];
    }
}
template __global__ void ftmpc_filter_bias_kernel<0>(const DeviceConsts, const FilterParams, const BiasParams);
template __global__ void ftmpc_filter_bias_kernel<1>(const DeviceConsts, const FilterParams, const BiasParams);
template __global__ void ftmpc_filter_bias_kernel<2>(const DeviceConsts, const FilterParams, const BiasParams);
template __global__ void ftmpc_filter_bias_kernel<3>(const DeviceConsts, const FilterParams, const BiasParams);

// ---------------------------------------------------------------------------------------------------------
// Measurement dropouts, outliers and the gated filter (ftmpc_simulate_outage_batch / ftmpc_simulate_wrench_outage_batch;
// include/ftmpc.h, ftmpc_outage).  Three kernels, a lane per vehicle each, all between ftmpc_sense_kernel and the solve:
//   ftmpc_outage_kernel          the availability chain (a two-state Markov chain per vehicle, overridden inside the scripted
//                                window), the outlier draws of an available step and their application to y_t, the counters, the
//                                histories, and the availability word avail[b] the two kernels below read
//   ftmpc_diagnose_gated_kernel  ftmpc_diagnose_kernel<0> with the per-vehicle skip: a lost vehicle neither tests nor re-anchors,
//                                its statistics carry over (llr_hist holds them) and phase 1 keeps counting n
//   ftmpc_filter_gated_kernel    ftmpc_filter_kernel<0> with availability and the innovation gate per vehicle: the update runs where
//                                !init && update && avail[b]; inside it channel j is left out (d and P as they are) when
//                                e^2 > gate^2 s_j.  The gate is two selects per channel (a gain and an innovation of exactly zero), not
//                                a branch around the unrolled channel body (which cost 100 more AGPRs and 36 bytes of scratch), so the
//                                78 packed entries of P stay in registers at compile-time indices, as in the plain kernel
// The plain kernels are siblings, not instantiations of these: their code is what it was.
// Counters: k = cstep * index_total + index0 + b, u_s = u01(seed, 32 k + s); s = 0 the chain, s = 1 + g the outlier of group g,
// s = 8 + 2 j, 9 + 2 j the Box-Muller pair of channel j.
// ---------------------------------------------------------------------------------------------------------
struct OutageParams {
    int64_t B;
    int32_t init, pad0;       // first step of a call without estimator.xhat: available, nothing drawn, y_t untouched
    const double* src;        // [B*13] y_t as the sense kernel left it (the handle's x0), or the truth when the sensor is trivial
    double* y;                // [B*13] the handle's x0: y_t as the filter and the diagnosis see it
    unsigned long long seed;
    double p_loss, p_recover;
    double p_outlier[4], outlier_sigma[4];
    int64_t cstep, step, index0, index_total;   // step0 + t (the counter's step, the window's clock), t (the histories' row)
    const int32_t* window;    // nullptr or [B*2]
    int32_t* state;           // [B*3] run, lost_steps, longest
    int32_t* outliers;        // [B*4]
    int32_t* avail;           // [B] 1 available, 0 lost: what the two consumers read
    int32_t* avail_hist;      // nullptr or [T*B]
    int32_t* outlier_hist;    // nullptr or [T*B]
    double* meas_hist;        // nullptr or [T*B*13]
};

struct GateParams {
    const int32_t* avail;     // [B]
    double gate_sq;           // 0: no gate
    int32_t* rejected;        // [B*4]
    int32_t* gate_hist;       // nullptr or [T*B]
};

__global__ void __launch_bounds__(64) ftmpc_outage_kernel(const OutageParams O) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= O.B) return;
    double y[13];
    for (int i = 0; i < 13; ++i) y[i] = O.src[b * 13 + i];
    int32_t run = 0, obits = 0;
    if (!O.init) {
        const unsigned long long k0 = (unsigned long long)(O.cstep * O.index_total + O.index0 + b) * 32ull;
        const int32_t run_prev = O.state[b * 3];
        const double u0 = u01(O.seed, k0);
        bool lost = run_prev > 0 ? !(u0 < O.p_recover) : (u0 < O.p_loss);
        if (O.window) {
            const int64_t from = O.window[b * 2], to = O.window[b * 2 + 1];
            if (from <= O.cstep && O.cstep < to) lost = true;
        }
        if (lost) {
            run = run_prev + 1;
            O.state[b * 3 + 1] += 1;
            if (run > O.state[b * 3 + 2]) O.state[b * 3 + 2] = run;
        } else {
            double e[12];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const bool hit = O.p_outlier[g] > 0.0 && u01(O.seed, k0 + 1ull + g) < O.p_outlier[g];
                if (hit) {
                    obits |= 1 << g;
                    O.outliers[b * 4 + g] += 1;
                }
#pragma unroll
                for (int j = 3 * g; j < 3 * g + 3; ++j)
                    e[j] = hit ? O.outlier_sigma[g] * sqrt(-2.0 * log(1.0 - u01(O.seed, k0 + 8ull + 2 * j))) *
                                     cos(6.283185307179586 * u01(O.seed, k0 + 9ull + 2 * j))
                               : 0.0;
            }
            for (int i = 0; i < 3; ++i) {
                if (obits & 1) y[i] += e[i];
                if (obits & 2) y[3 + i] += e[3 + i];
                if (obits & 8) y[10 + i] += e[9 + i];
            }
            if (obits & 4) filter_rotate(y + 6, e[6], e[7], e[8]);
        }
        O.state[b * 3] = run;
    } else {
        O.state[b * 3] = 0;
    }
    O.avail[b] = run == 0;
    if (O.avail_hist) O.avail_hist[O.step * O.B + b] = run == 0;
    if (O.outlier_hist) O.outlier_hist[O.step * O.B + b] = obits;
    if (O.meas_hist)
        for (int i = 0; i < 13; ++i) O.meas_hist[(O.step * O.B + b) * 13 + i] = y[i];
    for (int i = 0; i < 13; ++i) O.y[b * 13 + i] = y[i];
}

// phase 0 of ftmpc_diagnose_kernel with the per-vehicle skip (the diagnosis' own first step anchors on y_t whatever avail says)
__global__ void __launch_bounds__(64) ftmpc_diagnose_gated_kernel(const DeviceConsts C, const DiagParams P, const int32_t* avail) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    const int64_t B = P.B;
    const int NT = C.NT, L = P.L, H = NT * L;
    double x[13], y[13];
    double* const hist = P.llr_hist ? P.llr_hist + (P.step * B + b) * H : nullptr;
    if (!P.init && !avail[b]) {     // lost: no test, no re-anchor; xt, n, acc and llr carry over
        if (hist) {
#pragma unroll 1
            for (int k = 0; k < H; ++k) hist[k] = P.llr[(int64_t)k * B + b];
        }
        P.switched[b] = 0;
        return;
    }
    for (int i = 0; i < 13; ++i) y[i] = P.y[b * 13 + i];
    int32_t sw = 0;
    bool tested = false;
    if (P.init) {
#pragma unroll 1
        for (int k = 0; k < H; ++k) P.llr[(int64_t)k * B + b] = 0.0;
    } else {
        const double n = P.xt[b * 14 + 13];
        const int32_t cnt = P.count[b];
        if (P.anchor && n >= 1.0 && cnt < P.K) {
            tested = true;
            for (int i = 0; i < 13; ++i) x[i] = P.xt[b * 14 + i];
            const double qx = x[6], qy = x[7], qz = x[8], qw = x[9];
            const double R00 = qx * qx - qy * qy - qz * qz + qw * qw, R01 = 2 * (qx * qy + qz * qw), R02 = 2 * (qx * qz - qy * qw);
            const double R10 = 2 * (qx * qy - qz * qw), R11 = -qx * qx + qy * qy - qz * qz + qw * qw, R12 = 2 * (qy * qz + qx * qw);
            const double R20 = 2 * (qx * qz + qy * qw), R21 = 2 * (qy * qz - qx * qw), R22 = -qx * qx - qy * qy + qz * qz + qw * qw;
            const double e0 = y[3] - x[3], e1 = y[4] - x[4], e2 = y[5] - x[5];
            const double rv0 = R00 * e0 + R01 * e1 + R02 * e2;
            const double rv1 = R10 * e0 + R11 * e1 + R12 * e2;
            const double rv2 = R20 * e0 + R21 * e1 + R22 * e2;
            const double rw0 = y[10] - x[10], rw1 = y[11] - x[11], rw2 = y[12] - x[12];
            const double isv = 1.0 / (P.rsq[0] + n * P.dsq[0]), isw = 1.0 / (P.rsq[1] + n * P.dsq[1]);
            const double kv = C.dt * C.inv_mass, dt = C.dt;
            double best = P.threshold;
            int besth = -1;
#pragma unroll 1
            for (int i = 0; i < NT; ++i) {
                const bool live = P.ub[b * NT + i] > 0.0;
                const double acci = P.acc[(int64_t)i * B + b];
                const double d0 = C.D[i], d1 = C.D[MAX_NT + i], d2 = C.D[2 * MAX_NT + i];
                const double t0 = C.D[3 * MAX_NT + i], t1 = C.D[4 * MAX_NT + i], t2 = C.D[5 * MAX_NT + i];
                const double g0 = kv * d0, g1 = kv * d1, g2 = kv * d2;
                const double h0 = dt * (C.Jinv[0] * t0 + C.Jinv[1] * t1 + C.Jinv[2] * t2);
                const double h1 = dt * (C.Jinv[3] * t0 + C.Jinv[4] * t1 + C.Jinv[5] * t2);
                const double h2 = dt * (C.Jinv[6] * t0 + C.Jinv[7] * t1 + C.Jinv[8] * t2);
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    if (l < L) {
                        const int64_t k = (int64_t)(i * L + l);
                        double v = 0.0;
                        if (live) {
                            const double delta = n * P.levels[l] - acci;
                            const double a0 = g0 * delta, a1 = g1 * delta, a2 = g2 * delta;
                            const double w0 = h0 * delta, w1 = h1 * delta, w2 = h2 * delta;
                            const double z = ((a0 * rv0 + a1 * rv1 + a2 * rv2) - 0.5 * (a0 * a0 + a1 * a1 + a2 * a2)) * isv +
                                             ((w0 * rw0 + w1 * rw1 + w2 * rw2) - 0.5 * (w0 * w0 + w1 * w1 + w2 * w2)) * isw;
                            v = fmax(0.0, P.llr[k * B + b] + z);
                        }
                        P.llr[k * B + b] = v;
                        if (hist) hist[k] = v;
                        if (v > best) {      // (strictly: a tie stays with the lowest index)
                            best = v;
                            besth = (int)k;
                        }
                    }
                }
            }
            if (besth >= 0) {
                const int i = besth / L, l = besth - i * L;
                const double lv = l == 0 ? P.levels[0] : (l == 1 ? P.levels[1] : (l == 2 ? P.levels[2] : P.levels[3]));
                P.det_step[b * P.K + cnt] = P.cstep;
                P.det_thruster[b * P.K + cnt] = i;
                P.det_level[b * P.K + cnt] = l;
                P.count[b] = cnt + 1;
                P.ub[b * NT + i] = 0.0;
                P.stuck[b * NT + i] = lv;
#pragma unroll 1
                for (int k = 0; k < H; ++k) P.llr[(int64_t)k * B + b] = 0.0;
                sw = 1;
            }
        }
    }
    if (hist && !tested) {
#pragma unroll 1
        for (int k = 0; k < H; ++k) hist[k] = P.llr[(int64_t)k * B + b];
    }
    P.switched[b] = sw;
    if (P.init || P.anchor) {
        for (int i = 0; i < 13; ++i) P.xt[b * 14 + i] = y[i];
        P.xt[b * 14 + 13] = 0.0;
#pragma unroll 1
        for (int i = 0; i < NT; ++i) P.acc[(int64_t)i * B + b] = 0.0;
    }
}

// phase 0 of ftmpc_filter_kernel with availability and the innovation gate per vehicle
__global__ void __launch_bounds__(64) ftmpc_filter_gated_kernel(const DeviceConsts C, const FilterParams F, const GateParams Gt) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= F.B) return;
    const int64_t B = F.B;
    double* const covb = F.cov + (int64_t)blockIdx.x * blockDim.x;
    const unsigned lane = threadIdx.x;
    double x[13], P[78];
    int32_t mask = 0;      // bit j: channel j was rejected
    double y[13];
    for (int i = 0; i < 13; ++i) y[i] = F.y[b * 13 + i];
    if (F.init) {
        for (int i = 0; i < 13; ++i) x[i] = y[i];
    } else {
        for (int i = 0; i < 13; ++i) x[i] = F.xhat[b * 13 + i];
    }
    if (!F.init && F.update && Gt.avail[b]) {
        // A rejected channel runs the channel's straight-line code with a gain of exactly zero and an innovation of exactly zero:
        // d + 0 and P - 0 are d and P, so the 78 entries need no merge across a branch and stay where the plain kernel keeps them
        double th[3], d[12];
        filter_att_residual(x + 6, y + 6, th);
        const double gsq = Gt.gate_sq;
#pragma unroll
        for (int k = 0; k < 78; ++k) P[k] = cov_row(covb + (int64_t)k * B)[lane];
#pragma unroll
        for (int i = 0; i < 12; ++i) d[i] = 0.0;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            const int jx = j < 6 ? j : j + 1;      // channel j's entry of x (rate: past the quaternion)
            const double rj = (j >= 6 && j < 9) ? th[j - 6] : F.y[b * 13 + jx] - F.xhat[b * 13 + jx];
            const double sj = P[tri(j, j)] + F.rsq[j / 3];
            const double ej = rj - d[j];
            const bool rej = gsq > 0.0 && ej * ej > gsq * sj;
            if (rej) mask |= 1 << j;
            const double inv = rej ? 0.0 : 1.0 / sj;
            const double e = rej ? 0.0 : ej;
            double k[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) k[i] = P[tri(i, j)] * inv;
#pragma unroll
            for (int i = 0; i < 12; ++i) d[i] += k[i] * e;
#pragma unroll
            for (int a = 0; a < 12; ++a) {
                const double ska = sj * k[a];
#pragma unroll
                for (int c = a; c < 12; ++c) P[tri(a, c)] -= ska * k[c];
            }
        }
#pragma unroll
        for (int k = 0; k < 78; ++k) cov_row(covb + (int64_t)k * B)[lane] = P[k];
        {     // (a volatile read, as in ftmpc_filter_kernel<0>: x^ is not held across the covariance)
            const volatile double* const xh = F.xhat + b * 13;
            for (int i = 0; i < 13; ++i) x[i] = xh[i];
        }
        for (int i = 0; i < 3; ++i) {
            x[i] += d[i];
            x[3 + i] += d[3 + i];
            x[10 + i] += d[9 + i];
        }
        filter_rotate(x + 6, d[6], d[7], d[8]);
        if (mask)
            for (int g = 0; g < 4; ++g) Gt.rejected[b * 4 + g] += __popc((unsigned)(mask >> (3 * g)) & 7u);
    }
    if (Gt.gate_hist) Gt.gate_hist[F.step * B + b] = mask;
    for (int i = 0; i < 13; ++i) F.xhat[b * 13 + i] = x[i];
    if (F.est_hist)
        for (int i = 0; i < 13; ++i) F.est_hist[(F.step * B + b) * 13 + i] = x[i];
    if (F.err_sq) {     // against the truth: position, velocity, attitude (the residual's theta), rate
        double xt[13], th[3], e[4] = {0, 0, 0, 0};
        for (int i = 0; i < 13; ++i) xt[i] = F.truth[b * 13 + i];
        filter_att_residual(x + 6, xt + 6, th);
        for (int i = 0; i < 3; ++i) {
            e[0] += (x[i] - xt[i]) * (x[i] - xt[i]);
            e[1] += (x[3 + i] - xt[3 + i]) * (x[3 + i] - xt[3 + i]);
            e[2] += th[i] * th[i];
            e[3] += (x[10 + i] - xt[10 + i]) * (x[10 + i] - xt[10 + i]);
        }
        for (int i = 0; i < 4; ++i) F.err_sq[b * 4 + i] += e[i];
    }
    if (F.predict) {
        int32_t slot = F.slot0;
#pragma unroll 1
        for (int j = 0; j < F.latency; ++j) {
            double gen[6];
            filter_gen(C, F.ring + (int64_t)slot * B * C.NT, F.ub, F.stuck, b, gen);
            slot = slot + 1 == F.nslots ? 0 : slot + 1;
            filter_rk4(C, x, gen);
        }
        if (F.pred_hist)
            for (int i = 0; i < 13; ++i) F.pred_hist[(F.step * B + b) * 13 + i] = x[i];
    }
    for (int i = 0; i < 13; ++i) F.x0[b * 13 + i] = x[i];
}

// ---------------------------------------------------------------------------------------------------------
// A disturbance that varies over the run (ftmpc_simulate_environment_batch / ftmpc_simulate_wrench_environment_batch;
// include/ftmpc.h, ftmpc_environment).  One kernel, a lane per vehicle, launched after the step's solve and right before the plant
// step: it forms the wrench w_c = base + g_c + p_c + k_c held over plant step c (csrc/ftmpc_env.h: the Gauss-Markov draws and
// recursion, the periodic term, the kick, the sum) and writes it into the [3][B] force and [3][B] torque arrays that
// ftmpc_plant_step_var_kernel and ftmpc_plant_step_act_kernel read as PlantVar.force / .torque.  Neither plant kernel changes: what
// was a constant per call is rewritten between two of their launches.  The base is the call's own ftmpc_plant_model.force / .torque
// (PlantStage's arrays, which the plant no longer reads directly), the Gauss-Markov state is [6][B] in / out, the amplitudes, the
// kick and every output are component-major as well, so a wave's load or store covers 512 contiguous bytes; the window and the
// error sums keep the caller's layout (two words per lane).  The estimate error is taken against DistStage's estimate [B][6] as it
// stands at this point of the step: the value the step's solve saw.
// Counters: k = cstep * index_total + index0 + b, u_s = u01(seed, 32 k + s); s = 2 j, 2 j + 1 the innovation of component j,
// s = 16 + 2 j, 17 + 2 j its stationary start.
// ---------------------------------------------------------------------------------------------------------
}  // namespace ftmpc
#include "ftmpc_env.h"      // (included here, not at the top: the build logs keep the source lines of every kernel above)
namespace ftmpc {
struct EnvParams {
    int64_t B;
    int32_t init, pad0;       // first step of a call without a handed state: g_c is the stationary draw
    unsigned long long seed;
    int64_t cstep, step, index0, index_total;   // step0 + t (the counter's step, the periodic term's and the window's clock), t
    ftmpc_env::Process proc;
    const double* base_f;     // nullptr or [3][B] ftmpc_plant_model.force
    const double* base_t;     // nullptr or [3][B] ftmpc_plant_model.torque
    const double* amp_f;      // nullptr or [3][B]
    const double* amp_t;      // nullptr or [3][B]
    const double* phase;      // nullptr or [B]
    const double* kick;       // nullptr or [6][B]
    const int32_t* window;    // nullptr or [B*2] (with a kick: never nullptr)
    double* g;                // [6][B] g_c in, g_{c+1} out
    double* force;            // [3][B] out: PlantVar.force
    double* torque;           // [3][B] out: PlantVar.torque
    double* wrench_hist;      // nullptr or [T*B*6]
    const double* est;        // nullptr or [B*6] f^, t^ (with err_sq: never nullptr)
    double* err_sq;           // nullptr or [B*2] in/out
};

__global__ void __launch_bounds__(64) ftmpc_environment_kernel(const EnvParams E) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t B = E.B;
    if (b >= B) return;
    double base[6], amp[6], kick[6], g[6], w[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        base[k] = E.base_f ? E.base_f[k * B + b] : 0.0;
        base[3 + k] = E.base_t ? E.base_t[k * B + b] : 0.0;
        amp[k] = E.amp_f ? E.amp_f[k * B + b] : 0.0;
        amp[3 + k] = E.amp_t ? E.amp_t[k * B + b] : 0.0;
    }
    const bool periodic = E.amp_f || E.amp_t;
    const double phase = E.phase ? E.phase[b] : 0.0;
    bool kicked = false;
    if (E.kick) {
        const int64_t from = E.window[b * 2], to = E.window[b * 2 + 1];
        kicked = from <= E.cstep && E.cstep < to;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        kick[j] = kicked ? E.kick[j * B + b] : 0.0;
        g[j] = E.init ? 0.0 : E.g[j * B + b];
    }
    const unsigned long long k = (unsigned long long)(E.cstep * E.index_total + E.index0 + b);
    ftmpc_env::step(E.proc, E.seed, E.cstep, k, E.init != 0, periodic, kicked, base, amp, phase, kick, g, w);
#pragma unroll
    for (int j = 0; j < 6; ++j) E.g[j * B + b] = g[j];
#pragma unroll
    for (int k3 = 0; k3 < 3; ++k3) {
        E.force[k3 * B + b] = w[k3];
        E.torque[k3 * B + b] = w[3 + k3];
    }
    if (E.wrench_hist) {
#pragma unroll
        for (int j = 0; j < 6; ++j) E.wrench_hist[(E.step * B + b) * 6 + j] = w[j];
    }
    if (E.err_sq) {
        double ef = 0.0, et = 0.0;
#pragma unroll
        for (int k3 = 0; k3 < 3; ++k3) {
            const double df = E.est[b * 6 + k3] - w[k3], dt = E.est[b * 6 + 3 + k3] - w[3 + k3];
            ef += df * df;
            et += dt * dt;
        }
        E.err_sq[b * 2] += ef;
        E.err_sq[b * 2 + 1] += et;
    }
}

// ---------------------------------------------------------------------------------------------------------
// The diagnosis' test with a consistency gate, confirmation and level revision (ftmpc_simulate_isolation_batch /
// ftmpc_simulate_wrench_isolation_batch; include/ftmpc.h, ftmpc_isolation).  One kernel, a lane per vehicle, launched in place of
// ftmpc_diagnose_kernel<0> or ftmpc_diagnose_gated_kernel (avail == nullptr: the call has no outage); phase 1, the repair and the hull
// kernels are the ones every diagnosis runs.  The per-vehicle test is csrc/ftmpc_isolate.h: the residual and q_0 once, then the rolled
// thruster loop with the levels unrolled, which carries the arg-max, the smallest q_h and the counts; the scan of the vehicle's
// detection list (revise: is this off thruster one of the vehicle's own detections?) is a rolled loop of at most max_detect <= 8
// compares, entered for an off thruster only.  The plain kernels are siblings, not instantiations of this one: their code is what
// it was.  lead [B][2] (leader, run), voided [B] and revised [B] keep the caller's layout (a lane reads and writes its own few words
// once per step), fit_hist is [T][B][2].
// ---------------------------------------------------------------------------------------------------------
}  // namespace ftmpc
#include "ftmpc_isolate.h"      // (included here, not at the top: the build logs keep the source lines of every kernel above)
namespace ftmpc {
struct IsoParams {
    double consist_sq;        // 0: no gate
    int32_t persist, revise;
    int32_t* lead;            // [B*2] leader, run: in/out
    int32_t* voided;          // [B] in/out
    int32_t* revised;         // [B] in/out
    double* fit_hist;         // nullptr or [T*B*2]
};

__global__ void __launch_bounds__(64) ftmpc_diagnose_iso_kernel(const DeviceConsts C, const DiagParams P, const IsoParams I,
                                                                const int32_t* avail) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    const int64_t B = P.B;
    const int NT = C.NT, L = P.L, H = NT * L;
    double x[13], y[13];
    double* const hist = P.llr_hist ? P.llr_hist + (P.step * B + b) * H : nullptr;
    double* const fit = I.fit_hist ? I.fit_hist + (P.step * B + b) * 2 : nullptr;
    if (!P.init && avail && !avail[b]) {     // lost: no test, no re-anchor; xt, n, acc, llr, lead and the counters carry over
        if (hist) {
#pragma unroll 1
            for (int k = 0; k < H; ++k) hist[k] = P.llr[(int64_t)k * B + b];
        }
        if (fit) fit[0] = fit[1] = -1.0;
        P.switched[b] = 0;
        return;
    }
    for (int i = 0; i < 13; ++i) y[i] = P.y[b * 13 + i];
    int32_t sw = 0;
    bool tested = false;
    double f0 = -1.0, f1 = -1.0;
    if (P.init) {
#pragma unroll 1
        for (int k = 0; k < H; ++k) P.llr[(int64_t)k * B + b] = 0.0;
    } else {
        const double n = P.xt[b * 14 + 13];
        const int32_t cnt = P.count[b];
        if (P.anchor && n >= 1.0 && cnt < P.K) {
            tested = true;
            for (int i = 0; i < 13; ++i) x[i] = P.xt[b * 14 + i];
            ftmpc_iso::Rule R;
#pragma unroll
            for (int l = 0; l < 4; ++l) R.levels[l] = P.levels[l];
            R.threshold = P.threshold;
            R.consist_sq = I.consist_sq;
            R.L = L, R.persist = I.persist, R.revise = I.revise, R.pad0 = 0;
            ftmpc_iso::Resid r;
            ftmpc_iso::residual(x, y, n, P.rsq, P.dsq, r);
            ftmpc_iso::Scan s;
            ftmpc_iso::scan_start(R, s);
#pragma unroll 1
            for (int i = 0; i < NT; ++i) {
                const bool live = P.ub[b * NT + i] > 0.0;
                bool listed = false;
                if (!live && I.revise) {
#pragma unroll 1
                    for (int k = 0; k < cnt; ++k) listed = listed || P.det_thruster[b * P.K + k] == i;
                }
                const double d[6] = {C.D[i], C.D[MAX_NT + i], C.D[2 * MAX_NT + i], C.D[3 * MAX_NT + i], C.D[4 * MAX_NT + i], C.D[5 * MAX_NT + i]};
                double gh[6];
                ftmpc_iso::unit_signature(C.dt, C.inv_mass, C.Jinv, d, gh);
                ftmpc_iso::thruster(R, r, n, i, live, listed, P.acc[(int64_t)i * B + b], P.stuck[b * NT + i], gh,
                                    P.llr + (int64_t)i * L * B + b, B, hist ? hist + i * L : nullptr, s);
            }
            if (s.eligible > 0) f0 = r.q0, f1 = s.qmin;
            if (ftmpc_iso::is_void(R, r, s)) I.voided[b] += 1;
            int lead = I.lead[b * 2], run = I.lead[b * 2 + 1];
            if (ftmpc_iso::confirm(R, s, lead, run)) {
                const int rev = ftmpc_iso::decide(R, s.besth, P.cstep, cnt, H, P.ub + b * NT, P.stuck + b * NT, P.det_step + b * P.K,
                                                  P.det_thruster + b * P.K, P.det_level + b * P.K, P.llr + b, B, lead, run);
                P.count[b] = cnt + 1;
                if (rev) I.revised[b] += 1;
                sw = 1;
            }
            I.lead[b * 2] = lead;
            I.lead[b * 2 + 1] = run;
        }
    }
    if (hist && !tested) {
#pragma unroll 1
        for (int k = 0; k < H; ++k) hist[k] = P.llr[(int64_t)k * B + b];
    }
    if (fit) fit[0] = f0, fit[1] = f1;
    P.switched[b] = sw;
    if (P.init || P.anchor) {
        for (int i = 0; i < 13; ++i) P.xt[b * 14 + i] = y[i];
        P.xt[b * 14 + 13] = 0.0;
#pragma unroll 1
        for (int i = 0; i < NT; ++i) P.acc[(int64_t)i * B + b] = 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Probe pulses (ftmpc_simulate_probe_batch / ftmpc_simulate_wrench_probe_batch; include/ftmpc.h, ftmpc_probe).  A lane per vehicle,
// the per-vehicle rule is csrc/ftmpc_probe.h.
//   ftmpc_probe_kernel<0>         after the step's solve (and the allocation) and before the command enters the latency ring: the
//                                 idle counters move, at most one thruster per vehicle is pulsed in the handle's u0, in place
//   ftmpc_probe_kernel<1>         after the plant step, beside the diagnosis' phase 1, under reinstate only: pacc_i += a_t,i for the
//                                 listed thrusters (the model's c_i is 0 for a thruster that is off)
//   ftmpc_diagnose_probe_kernel   under reinstate, in place of the call's phase-0 diagnosis kernel: ftmpc_diagnose_iso_kernel's test
//                                 (the call's ftmpc_isolation, or the trivial rule) with the NT further hypotheses H + i "listed
//                                 thruster i is healthy" and their decision.  A sibling of that kernel, whose code is what it was
// idle and pulses keep the caller's layout [B][NT] beside ub and u0, which have it; pacc and health are component-major ([NT][B]) as
// acc and llr are.  `listed` scans the vehicle's detection list (at most max_detect <= 8 entries), for an off thruster only.
// ---------------------------------------------------------------------------------------------------------
}  // namespace ftmpc
#include "ftmpc_probe.h"
namespace ftmpc {
struct ProbeParams {
    int64_t B;
    int64_t step;             // t (the history's row)
    double amp, quiet, restore_ub, dt;
    int32_t idle_steps, max_pulses, reinstate, n_levels;
    int32_t K, pad0;          // max_detect
    double* u0;               // [B*NT] phase 0: the step's command, edited in place
    const double* u;          // [B*NT] phase 1: a_t, the command the plant applied in this step
    const double* ub;         // [B*NT] the controller's pattern
    const int32_t* count;     // [B] the diagnosis' detection list
    const int32_t* det_thruster;      // [B*K]
    const int32_t* det_level;
    int32_t* idle;            // [B*NT] in/out
    int32_t* pulses;          // [B*NT] in/out
    double* impulse;          // [B] in/out
    double* pacc;             // [NT][B]
    double* health;           // [NT][B]
    int32_t* reinstated;      // [B] in/out
    int32_t* hist;            // nullptr or [T*B]
};

__device__ __forceinline__ ftmpc_prb::Rule probe_rule(const ProbeParams& Q) {
    ftmpc_prb::Rule R;
    R.amp = Q.amp, R.quiet = Q.quiet, R.restore_ub = Q.restore_ub, R.dt = Q.dt;
    R.idle_steps = Q.idle_steps, R.max_pulses = Q.max_pulses, R.reinstate = Q.reinstate, R.n_levels = Q.n_levels;
    return R;
}

template <int PHASE>
__global__ void __launch_bounds__(64) ftmpc_probe_kernel(const DeviceConsts C, const ProbeParams Q) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Q.B) return;
    const int64_t B = Q.B;
    const int NT = C.NT;
    const ftmpc_prb::Rule R = probe_rule(Q);
    const int32_t cnt = Q.count[b];
    const int32_t* const dth = Q.det_thruster + b * Q.K;
    const int32_t* const dlv = Q.det_level + b * Q.K;
    if constexpr (PHASE == 0) {
        ftmpc_prb::Pick p;
        ftmpc_prb::pick_start(p);
#pragma unroll 1
        for (int i = 0; i < NT; ++i) {
            const bool live = Q.ub[b * NT + i] > 0.0;
            const bool lst = R.reinstate != 0 && ftmpc_prb::listed(i, live, cnt, dth, dlv, R.n_levels);
            int idle = Q.idle[b * NT + i];
            ftmpc_prb::thruster(R, i, live, lst, Q.u0[b * NT + i], Q.pulses[b * NT + i], idle, p);
            Q.idle[b * NT + i] = idle;
        }
        if (p.cand >= 0) {
            const int64_t k = b * NT + p.cand;
            const double ubi = Q.ub[k];
            double u = Q.u0[k];
            int pulses = Q.pulses[k], idle = p.idle;
            Q.impulse[b] += ftmpc_prb::pulse(R, ubi > 0.0, ubi, u, pulses, idle);
            Q.u0[k] = u;
            Q.pulses[k] = pulses;
            Q.idle[k] = idle;
        }
        if (Q.hist) Q.hist[Q.step * B + b] = p.cand;
        return;
    }
    // PHASE 1: the applied command of the listed thrusters, which the model's acc leaves out
#pragma unroll 1
    for (int i = 0; i < NT; ++i) {
        const bool live = Q.ub[b * NT + i] > 0.0;
        if (ftmpc_prb::listed(i, live, cnt, dth, dlv, R.n_levels)) Q.pacc[(int64_t)i * B + b] += Q.u[b * NT + i];
    }
}
template __global__ void ftmpc_probe_kernel<0>(const DeviceConsts, const ProbeParams);
template __global__ void ftmpc_probe_kernel<1>(const DeviceConsts, const ProbeParams);

__global__ void __launch_bounds__(64) ftmpc_diagnose_probe_kernel(const DeviceConsts C, const DiagParams P, const IsoParams I,
                                                                  const ProbeParams Q, const int32_t* avail) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    const int64_t B = P.B;
    const int NT = C.NT, L = P.L, H = NT * L;
    double x[13], y[13];
    double* const hist = P.llr_hist ? P.llr_hist + (P.step * B + b) * H : nullptr;
    double* const fit = I.fit_hist ? I.fit_hist + (P.step * B + b) * 2 : nullptr;
    if (!P.init && avail && !avail[b]) {     // lost: no test, no re-anchor; every statistic, pacc, lead and the counters carry over
        if (hist) {
#pragma unroll 1
            for (int k = 0; k < H; ++k) hist[k] = P.llr[(int64_t)k * B + b];
        }
        if (fit) fit[0] = fit[1] = -1.0;
        P.switched[b] = 0;
        return;
    }
    for (int i = 0; i < 13; ++i) y[i] = P.y[b * 13 + i];
    int32_t sw = 0;
    bool tested = false;
    double f0 = -1.0, f1 = -1.0;
    if (P.init) {
#pragma unroll 1
        for (int k = 0; k < H; ++k) P.llr[(int64_t)k * B + b] = 0.0;
#pragma unroll 1
        for (int i = 0; i < NT; ++i) Q.health[(int64_t)i * B + b] = 0.0;
    } else {
        const double n = P.xt[b * 14 + 13];
        const int32_t cnt = P.count[b];
        if (P.anchor && n >= 1.0 && cnt < P.K) {
            tested = true;
            for (int i = 0; i < 13; ++i) x[i] = P.xt[b * 14 + i];
            ftmpc_iso::Rule R;
#pragma unroll
            for (int l = 0; l < 4; ++l) R.levels[l] = P.levels[l];
            R.threshold = P.threshold;
            R.consist_sq = I.consist_sq;
            R.L = L, R.persist = I.persist, R.revise = I.revise, R.pad0 = 0;
            const ftmpc_prb::Rule PR = probe_rule(Q);
            ftmpc_iso::Resid r;
            ftmpc_iso::residual(x, y, n, P.rsq, P.dsq, r);
            ftmpc_iso::Scan s;
            ftmpc_iso::scan_start(R, s);
            ftmpc_prb::Lead hl;
            ftmpc_prb::lead_start(R, hl);
#pragma unroll 1
            for (int i = 0; i < NT; ++i) {
                const bool live = P.ub[b * NT + i] > 0.0;
                const bool lst = ftmpc_prb::listed(i, live, cnt, P.det_thruster + b * P.K, P.det_level + b * P.K, L);
                const double d[6] = {C.D[i], C.D[MAX_NT + i], C.D[2 * MAX_NT + i], C.D[3 * MAX_NT + i], C.D[4 * MAX_NT + i], C.D[5 * MAX_NT + i]};
                double gh[6];
                ftmpc_iso::unit_signature(C.dt, C.inv_mass, C.Jinv, d, gh);
                const double stucki = P.stuck[b * NT + i];
                ftmpc_iso::thruster(R, r, n, i, live, lst, P.acc[(int64_t)i * B + b], stucki, gh, P.llr + (int64_t)i * L * B + b, B,
                                    hist ? hist + i * L : nullptr, s);
                ftmpc_prb::healthy(R, r, n, i, lst, Q.pacc[(int64_t)i * B + b], stucki, gh, Q.health + (int64_t)i * B + b, s, hl);
            }
            ftmpc_prb::merge(hl, H, s);
            if (s.eligible > 0) f0 = r.q0, f1 = s.qmin;
            if (ftmpc_iso::is_void(R, r, s)) I.voided[b] += 1;
            int lead = I.lead[b * 2], run = I.lead[b * 2 + 1];
            if (ftmpc_iso::confirm(R, s, lead, run)) {
                if (s.besth >= H) {
                    ftmpc_prb::reinstate(PR, s.besth - H, P.cstep, cnt, P.ub + b * NT, P.stuck + b * NT, P.det_step + b * P.K,
                                           P.det_thruster + b * P.K, P.det_level + b * P.K);
#pragma unroll 1
                    for (int k = 0; k < H; ++k) P.llr[(int64_t)k * B + b] = 0.0;
                    lead = -1;
                    run = 0;
                    Q.reinstated[b] += 1;
                } else {
                    const int rev = ftmpc_iso::decide(R, s.besth, P.cstep, cnt, H, P.ub + b * NT, P.stuck + b * NT, P.det_step + b * P.K,
                                                      P.det_thruster + b * P.K, P.det_level + b * P.K, P.llr + b, B, lead, run);
                    if (rev) I.revised[b] += 1;
                }
#pragma unroll 1
                for (int i = 0; i < NT; ++i) Q.health[(int64_t)i * B + b] = 0.0;
                P.count[b] = cnt + 1;
                sw = 1;
            }
            I.lead[b * 2] = lead;
            I.lead[b * 2 + 1] = run;
        }
    }
    if (hist && !tested) {
#pragma unroll 1
        for (int k = 0; k < H; ++k) hist[k] = P.llr[(int64_t)k * B + b];
    }
    if (fit) fit[0] = f0, fit[1] = f1;
    P.switched[b] = sw;
    if (P.init || P.anchor) {
        for (int i = 0; i < 13; ++i) P.xt[b * 14 + i] = y[i];
        P.xt[b * 14 + 13] = 0.0;
#pragma unroll 1
        for (int i = 0; i < NT; ++i) {
            P.acc[(int64_t)i * B + b] = 0.0;
            Q.pacc[(int64_t)i * B + b] = 0.0;
        }
    }
}

}  // namespace ftmpc
