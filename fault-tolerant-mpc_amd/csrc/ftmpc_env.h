// One vehicle's step of the time-varying disturbance (ftmpc_environment_kernel, csrc/ftmpc_sim.hip; include/ftmpc.h,
// ftmpc_environment), as host / device functions so that a plain C++ program can run what the kernel runs
// (tests/test_env_step_host.py).
//
// Campaign step c, vehicle number g of index_total: counter k = c * index_total + g, u_s = u01(seed, 32 k + s).  The wrench held over
// plant step c is w_c = base + g_c + p_c + k_c (force, inertial frame, then torque, body frame):
//     g_c   six first-order Gauss-Markov processes, g_{c+1,j} = phi_a g_{c,j} + innov_a n_{c,j}, a = j / 3, n_{c,j} the Gaussian of
//           the slots 2j, 2j+1; a stationary start is sigma_a times the Gaussian of the slots 16+2j, 17+2j
//     p_c   amp sin(2 pi (c dt / period) + phase)
//     k_c   the kick, while the caller says so (from <= c < to)
// phi_a = exp(-dt / tau_a) and innov_a = sigma_a sqrt(1 - phi_a^2) come from the host, once per call (process()).
// Every index is a constant once the loops are unrolled: the kernel holds the six-vectors in registers.
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FTMPC_ENV_HD __host__ __device__ __forceinline__
#else
#define FTMPC_ENV_HD inline
#endif

namespace ftmpc_env {

constexpr unsigned long long DRAWS = 32ull;      // counters per (step, vehicle)

// the counter-based uniform in [0, 1) of csrc/ftmpc_sim.hip (splitmix64 of (seed, index)), restated for the host
FTMPC_ENV_HD double u01(unsigned long long seed, unsigned long long idx) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (idx + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// the Gaussian of the slot pair (s, s + 1) of counter k: gauss01's closed form
FTMPC_ENV_HD double gauss(unsigned long long seed, unsigned long long k, int s) {
    const double u1 = u01(seed, DRAWS * k + (unsigned long long)s), u2 = u01(seed, DRAWS * k + (unsigned long long)s + 1ull);
    return sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2);
}

// what is uniform over the call
struct Process {
    double sigma[2], phi[2], innov[2];      // force, torque
    double dt, period;                      // period is read only where an amplitude is given
};

// sigma_a = 0 switches the process off: tau_a is not looked at, phi_a = 0 (a handed state is held for its first step and is gone)
FTMPC_ENV_HD void process(const double sigma[2], const double tau[2], double dt, double period, Process& p) {
    for (int a = 0; a < 2; ++a) {
        p.sigma[a] = sigma[a];
        p.phi[a] = sigma[a] > 0.0 ? exp(-dt / tau[a]) : 0.0;
        p.innov[a] = sigma[a] * sqrt(1.0 - p.phi[a] * p.phi[a]);
    }
    p.dt = dt;
    p.period = period;
}

// One step of one vehicle.  g [6]: in g_c (not read on a stationary start, `init`), out g_{c+1}; w [6]: out w_c.
// base, amp, kick [6]: zeros where the call has none; periodic / kicked: whether p_c / k_c are formed at all.
FTMPC_ENV_HD void step(const Process& p, unsigned long long seed, long long c, unsigned long long k, bool init, bool periodic,
                       bool kicked, const double* base, const double* amp, double phase, const double* kick, double* g, double* w) {
    const double s = periodic ? sin(6.283185307179586 * ((double)c * p.dt / p.period) + phase) : 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int a = j / 3;
        const bool live = p.sigma[a] > 0.0;
        const double gc = init ? (live ? p.sigma[a] * gauss(seed, k, 16 + 2 * j) : 0.0) : g[j];
        const double pc = periodic ? amp[j] * s : 0.0;
        const double kc = kicked ? kick[j] : 0.0;
        w[j] = ((base[j] + gc) + pc) + kc;
        g[j] = p.phi[a] * gc + (live ? p.innov[a] * gauss(seed, k, 2 * j) : 0.0);
    }
}

}  // namespace ftmpc_env
