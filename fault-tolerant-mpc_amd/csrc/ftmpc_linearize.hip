// ftmpc_linearize.hip -- kernel 1 of the MPC QP-step path: nonlinear rollout + RK4 Jacobians.
//
// One LANE per instance, float64 arithmetic.  A lane's record (152 words per stage) is contiguous per
// instance because kernel 2 reads it that way, so storing word by word from the lanes would touch 64
// different cache lines per store instruction (measured: 4.6 GB written + 2.4 GB read-modify-write
// for a 1.6 GB payload).  The words are therefore staged through LDS and written out by the whole wave
// as contiguous runs.  Full-record kernel: one LDS row per instance at an odd stride (a put is one
// ds_write_b64 at a constant offset from the lane's row), written out 16 bytes per lane with the
// addresses stepped by adds and eight LDS reads in flight (flush_half below).
// For each horizon stage it evaluates the orbit-centre dynamics
//   (reference: SpiralModel.dx_dt, ft_mpc/models/spiral_model.py:44-76)
// at the four RK4 stage points (SystemModel.rk4_integrator, ft_mpc/models/sys_model.py:138-162),
// and propagates forward-mode tangents for the 13 non-trivial input directions
// (omega0, q0, F, tau) -- the Jacobians the reference obtains from CasADi AD
// (ft_mpc/controllers/spiraling_mpc.py:217-230).  SURVEY.md Appendix A lists the formulas.
//
// Work per instance ~ N * (4 dynamics evaluations + 13 * 4 tangent steps), but the kernel is not bound by
// that arithmetic.  It runs one wave per SIMD (256 VGPRs + 256 AGPRs, 40 448 B of LDS), so nothing hides
// a wait, and the four stage blocks (4 x 67 doubles = 536 registers) do not fit the register file: what
// bounds it is the issue rate of an instruction stream that is mostly the tangent section, arithmetic plus
// copies between the register halves.  Much of the generic tangent step multiplies by exact zeros (the q0
// directions never move w, the F directions move neither w nor q, ...), so the full-record kernel runs the
// tangents by direction group (w0, q0, F, tau), each group with only the terms that can be non-zero
// (ftmpc_tangent.h: contraction off, every fma spelled out in the shape the compiler gives the generic
// expression, so the record values are those of the generic loop).  The split kernels keep the generic
// loop, contracted by the compiler: they are the reference the full-record kernel is tested against
// (tests/test_gpu_linearize_records.py, tests/test_gpu_linearize_groups.py).  The write-out is not part of
// the bound (CHANGELOG, "Linearise kernel: lean record write-out").
#include <hip/hip_runtime.h>

#include "ftmpc_common.h"
#include "ftmpc_tangent.h"

namespace ftmpc {

namespace {

__device__ inline void cross3(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ inline void mat3vec(const double M[9], const double v[3], double o[3]) {
    for (int i = 0; i < 3; ++i) o[i] = M[3 * i] * v[0] + M[3 * i + 1] * v[1] + M[3 * i + 2] * v[2];
}

// skew(a) * M  (3x3)
__device__ inline void skew_mul(const double a[3], const double M[9], double o[9]) {
    for (int j = 0; j < 3; ++j) {
        o[0 + j] = -a[2] * M[3 + j] + a[1] * M[6 + j];
        o[3 + j] = a[2] * M[0 + j] - a[0] * M[6 + j];
        o[6 + j] = -a[1] * M[0 + j] + a[0] * M[3 + j];
    }
}

// The same three helpers with contraction off: every product and every sum rounds on its own, whatever code surrounds them.
// They carry the r_xz = (r[0], 0, r[2]) part of the lever arm (DeviceConsts::r_y, r_xz).  The sums over the whole r have two
// non-zero products once r[0] or r[2] is non-zero, and the compiler then contracted them one way in the full-record and the
// one-direction kernels and another way in the shares kernel (records 1e-14 apart); with r_xz = 0 every term here is an exact
// zero, so the reference vehicle's records keep their bits.
__device__ inline void cross3_plain(const double a[3], const double b[3], double o[3]) {
    FTMPC_TAN_NOCONTRACT
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ inline void mat3vec_plain(const double M[9], const double v[3], double o[3]) {
    FTMPC_TAN_NOCONTRACT
    for (int i = 0; i < 3; ++i) o[i] = (M[3 * i] * v[0] + M[3 * i + 1] * v[1]) + M[3 * i + 2] * v[2];
}

__device__ inline void skew_mul_plain(const double a[3], const double M[9], double o[9]) {
    FTMPC_TAN_NOCONTRACT
    for (int j = 0; j < 3; ++j) {
        o[0 + j] = a[1] * M[6 + j] - a[2] * M[3 + j];
        o[3 + j] = a[2] * M[0 + j] - a[0] * M[6 + j];
        o[6 + j] = a[0] * M[3 + j] - a[1] * M[0 + j];
    }
}

// Rot(q)^T for q = [x,y,z,w]; no unit-norm assumption (utils.py:15-19)
__device__ inline void rotT(const double q[4], double RT[9]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    // R rows (world->body); RT[i][j] = R[j][i]
    const double R00 = x * x - y * y - z * z + w * w, R01 = 2 * (x * y + z * w), R02 = 2 * (x * z - y * w);
    const double R10 = 2 * (x * y - z * w), R11 = -x * x + y * y - z * z + w * w, R12 = 2 * (y * z + x * w);
    const double R20 = 2 * (x * z + y * w), R21 = 2 * (y * z - x * w), R22 = -x * x - y * y + z * z + w * w;
    RT[0] = R00; RT[1] = R10; RT[2] = R20;
    RT[3] = R01; RT[4] = R11; RT[5] = R21;
    RT[6] = R02; RT[7] = R12; RT[8] = R22;
}

// one evaluation of the centre dynamics at (w, q) with total wrench (F, tau), plus its blocks
__device__ inline void stage_eval(const DeviceConsts& C, const double w[3], const double q[4],
                                  const double F[3], const double tau[3], double dw[3], double dq[4],
                                  double dv[3], StageBlk& S) {
    double Jw[3], wxJw[3], t[3];
    mat3vec(C.J, w, Jw);
    cross3(w, Jw, wxJw);
    for (int i = 0; i < 3; ++i) t[i] = tau[i] - wxJw[i];
    mat3vec(C.Jinv, t, dw);  // spiral_model.py:63-65
    // qdot = 1/2 Omega(w) q  (sys_model.py:18-29)
    dq[0] = 0.5 * (w[2] * q[1] - w[1] * q[2] + w[0] * q[3]);
    dq[1] = 0.5 * (-w[2] * q[0] + w[0] * q[2] + w[1] * q[3]);
    dq[2] = 0.5 * (w[1] * q[0] - w[0] * q[1] + w[2] * q[3]);
    dq[3] = 0.5 * (-w[0] * q[0] - w[1] * q[1] - w[2] * q[2]);
    // a_b = F/m + wdot x r + w x (w x r)   (spiral_model.py:67-71)
    double wxr[3], wxwxr[3], dwxr[3], ab[3];
    cross3(w, C.r_y, wxr);
    cross3(w, wxr, wxwxr);
    cross3(dw, C.r_y, dwxr);
    for (int i = 0; i < 3; ++i) ab[i] = F[i] * C.inv_mass + dwxr[i] + wxwxr[i];
    double wxrx[3];      // w x r_xz: its part of a_b here, of d a_b / d w below
    {
        FTMPC_TAN_NOCONTRACT
        double wxwxrx[3], dwxrx[3];
        cross3_plain(w, C.r_xz, wxrx);
        cross3_plain(w, wxrx, wxwxrx);
        cross3_plain(dw, C.r_xz, dwxrx);
        for (int i = 0; i < 3; ++i) ab[i] = ab[i] + (dwxrx[i] + wxwxrx[i]);
    }
    rotT(q, S.RT);
    mat3vec(S.RT, ab, dv);
    // ---- blocks ----
    // Fww = -Jinv ( [w]x J - [Jw]x )
    double M1[9], M2[9];
    skew_mul(w, C.J, M1);
    M2[0] = 0; M2[1] = -Jw[2]; M2[2] = Jw[1];
    M2[3] = Jw[2]; M2[4] = 0; M2[5] = -Jw[0];
    M2[6] = -Jw[1]; M2[7] = Jw[0]; M2[8] = 0;
    for (int i = 0; i < 9; ++i) M1[i] -= M2[i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            S.Fww[3 * i + j] = -(C.Jinv[3 * i] * M1[j] + C.Jinv[3 * i + 1] * M1[3 + j] + C.Jinv[3 * i + 2] * M1[6 + j]);
    // d a_b / d w = -[r]x Fww - [w x r]x - [w]x [r]x
    double rF[9], wr[9], dab[9];
    skew_mul(C.r_y, S.Fww, rF);
    const double SR[9] = {0, -C.r_y[2], C.r_y[1], C.r_y[2], 0, -C.r_y[0], -C.r_y[1], C.r_y[0], 0};
    skew_mul(w, SR, wr);
    const double SW[9] = {0, -wxr[2], wxr[1], wxr[2], 0, -wxr[0], -wxr[1], wxr[0], 0};
    for (int i = 0; i < 9; ++i) dab[i] = -rF[i] - SW[i] - wr[i];
    {
        FTMPC_TAN_NOCONTRACT
        double rFx[9], wrx[9];
        skew_mul_plain(C.r_xz, S.Fww, rFx);
        const double SRx[9] = {0, -C.r_xz[2], C.r_xz[1], C.r_xz[2], 0, -C.r_xz[0], -C.r_xz[1], C.r_xz[0], 0};
        skew_mul_plain(w, SRx, wrx);
        const double SWx[9] = {0, -wxrx[2], wxrx[1], wxrx[2], 0, -wxrx[0], -wxrx[1], wxrx[0], 0};
        for (int i = 0; i < 9; ++i) dab[i] = dab[i] - ((rFx[i] + SWx[i]) + wrx[i]);
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            S.Vw[3 * i + j] = S.RT[3 * i] * dab[j] + S.RT[3 * i + 1] * dab[3 + j] + S.RT[3 * i + 2] * dab[6 + j];
    // d (Rot(q)^T a_b) / d q   (3x4), entries linear in q
    {
        const double x = q[0], y = q[1], z = q[2], ww = q[3];
        const double d0[12] = {x, -y, -z, ww, y, x, ww, z, z, -ww, x, -y};
        const double d1[12] = {y, x, -ww, -z, -x, y, -z, ww, ww, z, y, x};
        const double d2[12] = {z, ww, x, y, -ww, z, y, -x, -x, -y, z, ww};
        for (int i = 0; i < 12; ++i) S.Vq[i] = 2.0 * (ab[0] * d0[i] + ab[1] * d1[i] + ab[2] * d2[i]);
    }
    // Fqw = 1/2 Xi(q) (4x3), Fqq = 1/2 Omega(w) (4x4)
    {
        const double x = q[0], y = q[1], z = q[2], ww = q[3];
        const double xi[12] = {ww, -z, y, z, ww, -x, -y, x, ww, -x, -y, -z};
        for (int i = 0; i < 12; ++i) S.Fqw[i] = 0.5 * xi[i];
        const double om[16] = {0, w[2], -w[1], w[0], -w[2], 0, w[0], w[1], w[1], -w[0], 0, w[2], -w[0], -w[1], -w[2], 0};
        for (int i = 0; i < 16; ++i) S.Fqq[i] = 0.5 * om[i];
    }
}

}  // namespace

// Staging of the full-record kernel: one LDS row per instance, STG_ROW words apart.  The row stride is odd, so the
// 32 lanes of one LDS pass hit 32 different bank pairs when every lane stores word `wd` of its own row, and a put is
// one ds_write_b64 at lane base + constant.  A stage goes out in two halves, split at the even word STG_SPLIT so that
// both halves start 16-byte aligned in the record: words [0, 78) after direction 6, words [78, 152) at the end of the
// stage.  Word 78 (AQQ[3][3], direction 6) waits in the row's spare slot 78 over the first flush.
constexpr int STG_SPLIT = 78;
constexpr int STG_ROW = 79;                       // 64 * 79 * 8 = 40 448 B of LDS per wave
static_assert(STG_SPLIT % 2 == 0 && (REC_STRIDE - STG_SPLIT) % 2 == 0 && REC_STRIDE % 2 == 0, "halves are whole 16-byte pairs");
static_assert(STG_SPLIT == REC_BPF - 1 && REC_AQQ + 15 == STG_SPLIT, "word 78 is the one A word of the second half");
static_assert(STG_ROW % 2 == 1 && STG_ROW > STG_SPLIT && STG_ROW > REC_STRIDE - STG_SPLIT, "odd row stride that holds either half and the spare slot");
static_assert(64 * STG_ROW * 8 <= 40960, "four blocks per CU: one wave per SIMD");

// The wave writes words [0, W) of the staged half of its 64 instances to g[inst * rowg + wd]: the same contiguous W-word runs,
// 16 bytes per lane and store.  Pair p = lane + 64 t of the flattened [inst][W / 2] list belongs to lane `lane`; its instance,
// LDS index and record offset follow from the previous pair's by adds and compares.  UN LDS reads are issued before the first
// store; the stores do not wait for each other.  Rows at or past `nreal` are not written.
template <int W>
__device__ inline void flush_half(const double* stg, double* g, int rowg, int nreal, int lane) {
    static_assert(W % 2 == 0 && W / 2 < 64 && W / 2 > 32, "at most two row changes per step of 64 pairs");
    constexpr int PW = W / 2, UN = 8;
    int inst = lane >= PW ? 1 : 0;
    int pw = lane - inst * PW;
    int la = inst * STG_ROW + 2 * pw;       // LDS word index
    int ga = inst * rowg + 2 * pw;          // record word offset from g
    auto group = [&](auto un) {
        constexpr int U = decltype(un)::value;
        double v0[U], v1[U];
        int go[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            v0[u] = stg[la];
            v1[u] = stg[la + 1];
            go[u] = ga;
            ok[u] = inst < nreal;
            // 64 pairs on: PW < 64, so always into the next row, and into the one after it if the rest still overshoots
            pw += 64 - PW; ++inst; la += 128 + STG_ROW - W; ga += 128 + rowg - W;
            if (pw >= PW) { pw -= PW; ++inst; la += STG_ROW - W; ga += rowg - W; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (ok[u]) *reinterpret_cast<double2*>(g + go[u]) = make_double2(v0[u], v1[u]);
    };
#pragma unroll 1
    for (int t = 0; t + UN <= PW; t += UN) group(std::integral_constant<int, UN>{});
    if constexpr (PW % UN != 0) group(std::integral_constant<int, PW % UN>{});
}

// DIRS = false: the whole record of 64 instances per wave (full batches).  DIRS = true: blockIdx.y picks a contiguous
// share of the 13 tangent directions (gridDim.y = 13, 4 or 2 shares; y = 0 also writes the words that are not tangents,
// the work lists and e_N); every block repeats the cheap nonlinear rollout and stage blocks, so a small batch spreads
// over more waves and each wave does a fraction of the work -- same arithmetic per direction, same record bits
// (tests/test_gpu_parity.py).  The host takes it where the full-record kernel would leave most of the device idle.
// DIST = 1 (ftmpc_simulate_disturbance_batch with compensate = 1, ftmpc_debug_records_disturbance): the rollout and the stage blocks take
// the estimated disturbance P.dist [B*6] = (f^ inertial, t^ body): every RK4 stage is evaluated at tau + t^, and f^ / m is added to
// dv after the rotation (it is inertial, so it enters neither ab nor Vq).  rut keeps the COMMANDED gen; the tangent loop is the same code.
template <typename OutT, int SHARE, int DIST = 0>   // SHARE 0: full records; 1: one direction per block; 2: gridDim.y shares of the 13 directions
__global__ void __launch_bounds__(64) ftmpc_linearize_kernel(const DeviceConsts C, const LinParams P) {
    static_assert(sizeof(OutT) == 8, "records are float64");
    constexpr bool DIRS = SHARE != 0;
    __shared__ double stg[DIRS ? 1 : STG_ROW * 64];
    const int lane = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * 64;
    // lanes past the end of the batch redo the last instance (they take part in the cooperative stores)
    const int64_t b = (b0 + lane < P.B) ? b0 + lane : P.B - 1;
    const int N = C.N, NT = C.NT;
    OutT* const recw = reinterpret_cast<OutT*>(P.rec);
    const int jlo = SHARE == 0 ? 0 : (SHARE == 1 ? (int)blockIdx.y : 13 * (int)blockIdx.y / (int)gridDim.y);
    const int jhi = SHARE == 0 ? 13 : (SHARE == 1 ? jlo + 1 : 13 * ((int)blockIdx.y + 1) / (int)gridDim.y);
    const bool writes_rest = !DIRS || blockIdx.y == 0;
    int pk = 0, pbase = 0;     // DIRS: stage and half (0 / REC_BPF) the next put belongs to
    // stage one record word of this lane (word index relative to the current half)
    auto put = [&](int wd, double v) {
        if constexpr (DIRS) {
            if (b0 + lane < P.B) recw[(b * N + pk) * (int64_t)REC_STRIDE + pbase + wd] = (OutT)v;
        } else {
            // second half: word pbase + wd of the record sits at row slot pbase + wd - STG_SPLIT
            stg[lane * STG_ROW + wd + (pbase ? REC_BPF - STG_SPLIT : 0)] = v;
        }
    };
    // the wave writes one half of stage k for its 64 instances (flush_half): second = false words [0, STG_SPLIT) and
    // word STG_SPLIT moves from the spare slot to slot 0 of the lane's own row, second = true words [STG_SPLIT, REC_STRIDE)
    const int nreal = (int)((P.B - b0 < 64) ? P.B - b0 : 64);
    auto flush = [&](int k, bool second) {
        if constexpr (!DIRS) {
            double* const g = recw + (b0 * N + k) * (int64_t)REC_STRIDE;
            __syncthreads();
            if (!second) {
                flush_half<STG_SPLIT>(stg, g, N * REC_STRIDE, nreal, lane);
            } else {
                flush_half<REC_STRIDE - STG_SPLIT>(stg, g + STG_SPLIT, N * REC_STRIDE, nreal, lane);
            }
            __syncthreads();
            if (!second) stg[lane * STG_ROW] = stg[lane * STG_ROW + STG_SPLIT];
        }
    };

    // ---- robot -> orbit-centre state (spiral_model.py:91-109) ----
    double x[13];
    for (int i = 0; i < 13; ++i) x[i] = P.x0[b * 13 + i];
    double pos[3], vel[3], w[3], q[4];
    for (int i = 0; i < 4; ++i) q[i] = x[6 + i];
    for (int i = 0; i < 3; ++i) w[i] = x[10 + i];
    {
        double RT[9], wxr[3], a[3], c[3];
        rotT(q, RT);
        cross3(w, C.r_y, wxr);
        mat3vec(RT, C.r_y, a);
        mat3vec(RT, wxr, c);
        for (int i = 0; i < 3; ++i) {
            pos[i] = x[i] + a[i];
            vel[i] = x[3 + i] + c[i];
        }
        {   // the r_xz part of the lever arm, in a fixed shape (see cross3_plain)
            FTMPC_TAN_NOCONTRACT
            double wxrx[3], ax[3], cx[3];
            cross3_plain(w, C.r_xz, wxrx);
            mat3vec_plain(RT, C.r_xz, ax);
            mat3vec_plain(RT, wxrx, cx);
            for (int i = 0; i < 3; ++i) {
                pos[i] = pos[i] + ax[i];
                vel[i] = vel[i] + cx[i];
            }
        }
    }
    double ubv[MAX_NT], stk[MAX_NT];
    for (int i = 0; i < NT; ++i) {
        ubv[i] = P.ub[b * NT + i];
        stk[i] = P.stuck[b * NT + i];
    }
    // ---- work lists of the fp32 solve instantiations: one atomic per wave and list ----
    if (P.qlist && writes_rest) {
        int na = 0;
        for (int i = 0; i < NT; ++i) na += (ubv[i] > 0.0) ? 1 : 0;
        const int nbk = (N * na + 15) >> 4;
        int v = (na == 0 || nbk <= 8) ? 0 : nbk - 8;      // 0..2: one-wave kernels NB = 8 / 9 / 10; 3: workgroup kernel
        v = v > P.qvmax ? P.qvmax : v;
        const bool real = b0 + lane < P.B;
        for (int vv = 0; vv <= P.qvmax; ++vv) {
            const unsigned long long m = __ballot(real && v == vv);
            if (m == 0ull) continue;
            const int leader = __ffsll((long long)m) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(P.qcount + vv, __popcll(m));
            base = __builtin_amdgcn_readlane(base, leader);
            if (real && v == vv) P.qlist[(int64_t)vv * P.B + base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)b;
        }
    }
    const double* xref = P.xref + b * P.xref_stride;
    const double* uref = P.uref ? P.uref + b * P.uref_stride : nullptr;
    const double dt = C.dt;
    const double acoef[4] = {0.0, 0.5 * dt, 0.5 * dt, dt};
    const double wcoef[4] = {1.0, 2.0, 2.0, 1.0};
    double dfm[3] = {0, 0, 0}, dtq[3] = {0, 0, 0};      // DIST: f^ / m and t^
    if constexpr (DIST != 0) {
        for (int i = 0; i < 3; ++i) {
            dfm[i] = P.dist[b * 6 + i] * C.inv_mass;
            dtq[i] = P.dist[b * 6 + 3 + i];
        }
    }

    for (int k = 0; k < N; ++k) {
        // total wrench gen = D (ubar + stuck), ubar = clip(warm, 0, ub) (0 for broken thrusters)
        double gen[6] = {0, 0, 0, 0, 0, 0}, rut[6];
        for (int i = 0; i < NT; ++i) {
            double u = 0.0;
            if (P.warmU && ubv[i] > 0.0) {
                u = P.warmU[(b * N + k) * NT + i];
                u = fmin(fmax(u, 0.0), ubv[i]);
            }
            const double t = u + stk[i];
            for (int g = 0; g < 6; ++g) gen[g] += C.D[g * MAX_NT + i] * t;
        }
        if (P.warmG) {
            for (int g = 0; g < 6; ++g) gen[g] = P.warmG[(b * N + k) * 6 + g];
        }
        // R .* (gen - ur - [f_virt;0]),  ur = [Rot(q_k)^T uref[0:3]; uref[3:6]]  (spiraling_mpc.py:156-171)
        {
            double ur[6] = {0, 0, 0, 0, 0, 0};
            if (uref) {
                double RT[9], f3[3] = {uref[6 * k], uref[6 * k + 1], uref[6 * k + 2]}, o[3];
                rotT(q, RT);
                mat3vec(RT, f3, o);
                ur[0] = o[0]; ur[1] = o[1]; ur[2] = o[2];
                ur[3] = uref[6 * k + 3]; ur[4] = uref[6 * k + 4]; ur[5] = uref[6 * k + 5];
            }
            for (int g = 0; g < 6; ++g) {
                const double fv = g < 3 ? C.fvirt[g] : 0.0;
                rut[g] = C.R[g] * (gen[g] - ur[g] - fv);
            }
        }
        const double* F = gen;
        const double* tau = gen + 3;
        double taud[3];
        if constexpr (DIST != 0) {
            for (int i = 0; i < 3; ++i) taud[i] = gen[3 + i] + dtq[i];
            tau = taud;
        }

        // ---- RK4 stage points + blocks ----
        StageBlk S[4];
        double kw[4][3], kq[4][4], kv[4][3];
        for (int i = 0; i < 4; ++i) {
            double wi[3], qi[4];
            for (int j = 0; j < 3; ++j) wi[j] = w[j] + (i ? acoef[i] * kw[i - 1][j] : 0.0);
            for (int j = 0; j < 4; ++j) qi[j] = q[j] + (i ? acoef[i] * kq[i - 1][j] : 0.0);
            stage_eval(C, wi, qi, F, tau, kw[i], kq[i], kv[i], S[i]);
            if constexpr (DIST != 0)
                for (int j = 0; j < 3; ++j) kv[i][j] += dfm[j];
        }

        // ---- tangents for the 13 input directions [w0(3), q0(4), F(3), tau(3)] ----
        pk = k;
        if constexpr (SHARE == 0) {
            // S[0].Vq and S[0].Fqq are used here, in the basic block that evaluates them.  The w0 loop does not read them (tq = 0 at
            // stage point 0), and what only a later group reads the compiler moves down to that group -- away from the products it
            // is contracted with in stage_eval (F / m into a_b, which Vq is formed from), which then round on their own: other record
            // bits than the split kernels'.  The statements are empty; the zero diagonal of Fqq stays a constant.
            for (int e = 0; e < 12; ++e) asm volatile("" ::"v"(S[0].Vq[e]));
            for (int e = 0; e < 16; ++e)
                if (e % 5 != 0) asm volatile("" ::"v"(S[0].Fqq[e]));
            const tangent::Coef K = {acoef[1], acoef[3], dt / 6.0, dt * dt / 6.0};
            tangent::Words o;
            pbase = 0;
#pragma unroll 1
            for (int j = 0; j < 3; ++j) {       // w0
                const double tw0[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
                tangent::dir_w0(S, K, tw0, o);
                for (int a = 0; a < 3; ++a) {
                    put(REC_APW + 3 * a + j, o.p[a]);
                    put(REC_AVW + 3 * a + j, o.v[a]);
                    put(REC_AWW + 3 * a + j, o.w[a]);
                }
                for (int a = 0; a < 4; ++a) put(REC_AQW + 3 * a + j, o.q[a]);
            }
#pragma unroll 1
            for (int jj = 0; jj < 4; ++jj) {    // q0
                const double tq0[4] = {jj == 0 ? 1.0 : 0.0, jj == 1 ? 1.0 : 0.0, jj == 2 ? 1.0 : 0.0, jj == 3 ? 1.0 : 0.0};
                tangent::dir_q0(S, K, tq0, o);
                for (int a = 0; a < 3; ++a) {
                    put(REC_APQ + 4 * a + jj, o.p[a]);
                    put(REC_AVQ + 4 * a + jj, o.v[a]);
                }
                for (int a = 0; a < 4; ++a) put(REC_AQQ + 4 * a + jj, o.q[a]);
            }
            flush(k, false);   // the A blocks (words 0..78) are complete
            pbase = REC_BPF;
            auto put_F = [&](int jj) {
                for (int a = 0; a < 3; ++a) {
                    put(REC_BPF - REC_BPF + 3 * a + jj, o.p[a]);
                    put(REC_BVF - REC_BPF + 3 * a + jj, o.v[a]);
                }
            };
            tangent::dir_F<0>(S, K, C.inv_mass, o); put_F(0);
            tangent::dir_F<1>(S, K, C.inv_mass, o); put_F(1);
            tangent::dir_F<2>(S, K, C.inv_mass, o); put_F(2);
#pragma unroll 1
            for (int jj = 0; jj < 3; ++jj) {    // tau
                const double tT[3] = {jj == 0 ? 1.0 : 0.0, jj == 1 ? 1.0 : 0.0, jj == 2 ? 1.0 : 0.0};
                tangent::dir_tau(S, K, C.Jinv, C.ArT, tT, o);
                for (int a = 0; a < 3; ++a) {
                    put(REC_BPT - REC_BPF + 3 * a + jj, o.p[a]);
                    put(REC_BVT - REC_BPF + 3 * a + jj, o.v[a]);
                    put(REC_BWT - REC_BPF + 3 * a + jj, o.w[a]);
                }
                for (int a = 0; a < 4; ++a) put(REC_BQT - REC_BPF + 3 * a + jj, o.q[a]);
            }
        } else {
            // the split kernels: one generic loop over their share of the directions, contracted by the compiler
            for (int j = jlo; j < jhi; ++j) {
                pbase = (j < 7) ? 0 : REC_BPF;
                double tw0[3] = {0, 0, 0}, tq0[4] = {0, 0, 0, 0}, tF[3] = {0, 0, 0}, tT[3] = {0, 0, 0};
                if (j < 3) tw0[j] = 1.0;
                else if (j < 7) tq0[j - 3] = 1.0;
                else if (j < 10) tF[j - 7] = 1.0;
                else tT[j - 10] = 1.0;
                // wrench contributions common to all stage points
                double jt[3], at[3];
                mat3vec(C.Jinv, tT, jt);   // d wdot / d tau * tT
                mat3vec(C.ArT, tT, at);    // d a_b / d tau * tT
                for (int i = 0; i < 3; ++i) at[i] += tF[i] * C.inv_mass;
                double tkw[3] = {0, 0, 0}, tkq[4] = {0, 0, 0, 0};
                double sw[3] = {0, 0, 0}, sq[4] = {0, 0, 0, 0}, sv[3] = {0, 0, 0}, sp[3] = {0, 0, 0};
                for (int i = 0; i < 4; ++i) {
                    double tw[3], tq[4];
                    for (int a = 0; a < 3; ++a) tw[a] = tw0[a] + acoef[i] * tkw[a];
                    for (int a = 0; a < 4; ++a) tq[a] = tq0[a] + acoef[i] * tkq[a];
                    const StageBlk& B = S[i];
                    double nkw[3], nkq[4], nkv[3], rv[3];
                    for (int a = 0; a < 3; ++a)
                        nkw[a] = B.Fww[3 * a] * tw[0] + B.Fww[3 * a + 1] * tw[1] + B.Fww[3 * a + 2] * tw[2] + jt[a];
                    for (int a = 0; a < 4; ++a)
                        nkq[a] = B.Fqw[3 * a] * tw[0] + B.Fqw[3 * a + 1] * tw[1] + B.Fqw[3 * a + 2] * tw[2] +
                                 B.Fqq[4 * a] * tq[0] + B.Fqq[4 * a + 1] * tq[1] + B.Fqq[4 * a + 2] * tq[2] + B.Fqq[4 * a + 3] * tq[3];
                    mat3vec(B.RT, at, rv);
                    for (int a = 0; a < 3; ++a)
                        nkv[a] = B.Vw[3 * a] * tw[0] + B.Vw[3 * a + 1] * tw[1] + B.Vw[3 * a + 2] * tw[2] +
                                 B.Vq[4 * a] * tq[0] + B.Vq[4 * a + 1] * tq[1] + B.Vq[4 * a + 2] * tq[2] + B.Vq[4 * a + 3] * tq[3] + rv[a];
                    for (int a = 0; a < 3; ++a) { tkw[a] = nkw[a]; sw[a] += wcoef[i] * nkw[a]; }
                    for (int a = 0; a < 4; ++a) { tkq[a] = nkq[a]; sq[a] += wcoef[i] * nkq[a]; }
                    for (int a = 0; a < 3; ++a) { sv[a] += wcoef[i] * nkv[a]; if (i < 3) sp[a] += nkv[a]; }
                }
                const double c6 = dt / 6.0, c26 = dt * dt / 6.0;
                if (j < 3) {
                    for (int a = 0; a < 3; ++a) {
                        put(REC_APW + 3 * a + j, c26 * sp[a]);
                        put(REC_AVW + 3 * a + j, c6 * sv[a]);
                        put(REC_AWW + 3 * a + j, tw0[a] + c6 * sw[a]);
                    }
                    for (int a = 0; a < 4; ++a) put(REC_AQW + 3 * a + j, c6 * sq[a]);
                } else if (j < 7) {
                    const int jj = j - 3;
                    for (int a = 0; a < 3; ++a) {
                        put(REC_APQ + 4 * a + jj, c26 * sp[a]);
                        put(REC_AVQ + 4 * a + jj, c6 * sv[a]);
                    }
                    for (int a = 0; a < 4; ++a) put(REC_AQQ + 4 * a + jj, tq0[a] + c6 * sq[a]);
                } else if (j < 10) {
                    const int jj = j - 7;
                    for (int a = 0; a < 3; ++a) {
                        put(REC_BPF - REC_BPF + 3 * a + jj, c26 * sp[a]);
                        put(REC_BVF - REC_BPF + 3 * a + jj, c6 * sv[a]);
                    }
                } else {
                    const int jj = j - 10;
                    for (int a = 0; a < 3; ++a) {
                        put(REC_BPT - REC_BPF + 3 * a + jj, c26 * sp[a]);
                        put(REC_BVT - REC_BPF + 3 * a + jj, c6 * sv[a]);
                        put(REC_BWT - REC_BPF + 3 * a + jj, c6 * sw[a]);
                    }
                    for (int a = 0; a < 4; ++a) put(REC_BQT - REC_BPF + 3 * a + jj, c6 * sq[a]);
                }
            }
        }

        // ---- advance the nonlinear rollout (no quaternion renormalisation, sys_model.py:152-158) ----
        for (int a = 0; a < 3; ++a) {
            pos[a] += dt * vel[a] + dt * dt / 6.0 * (kv[0][a] + kv[1][a] + kv[2][a]);
            vel[a] += dt / 6.0 * (kv[0][a] + 2 * kv[1][a] + 2 * kv[2][a] + kv[3][a]);
        }
        for (int a = 0; a < 3; ++a) w[a] += dt / 6.0 * (kw[0][a] + 2 * kw[1][a] + 2 * kw[2][a] + kw[3][a]);
        for (int a = 0; a < 4; ++a) q[a] += dt / 6.0 * (kq[0][a] + 2 * kq[1][a] + 2 * kq[2][a] + kq[3][a]);

        // ---- the linearisation trajectory itself, for the state-bound rows (xlb <= c_{k+1} <= xub, spiraling_mpc.py:179-185) ----
        if (P.out_cbar && writes_rest && b0 + lane < P.B) {
            double* cb = P.out_cbar + (b * N + k) * 13;
            for (int a = 0; a < 3; ++a) {
                cb[a] = pos[a];
                cb[3 + a] = vel[a];
                cb[6 + a] = w[a];
            }
            for (int a = 0; a < 4; ++a) cb[9 + a] = q[a];
        }
        // ---- weighted tracking error of stage k+1: W (c[0:9] - xref) ----
        pbase = REC_BPF;
        if (writes_rest) {
            double e[9];
            for (int a = 0; a < 3; ++a) {
                e[a] = pos[a] - xref[9 * (k + 1) + a];
                e[3 + a] = vel[a] - xref[9 * (k + 1) + 3 + a];
                e[6 + a] = w[a] - xref[9 * (k + 1) + 6 + a];
            }
            if (k + 1 < N) {
                for (int a = 0; a < 9; ++a) put(REC_WE - REC_BPF + a, C.Q[a] * e[a]);
            } else {
                if (P.out_eN && b0 + lane < P.B) {
                    for (int a = 0; a < 9; ++a) P.out_eN[b * 9 + a] = e[a];
                }
                double gnq[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                if (P.tcost) (void)term_cost_nq(*P.tcost, e, gnq);      // exact gradient of the non-quadratic terminal terms
                for (int a = 0; a < 9; ++a) {
                    double s = 0.0;
                    for (int c = 0; c < 9; ++c) s += C.P[9 * a + c] * e[c];
                    put(REC_WE - REC_BPF + a, s + 0.5 * gnq[a]);
                }
            }
            for (int g = 0; g < 6; ++g) put(REC_RUT - REC_BPF + g, rut[g]);
            put(REC_USED - REC_BPF, 0.0);
        }
        flush(k, true);   // AQQ[3][3], B blocks, W e, R ut (words 78..151)
    }
}

template __global__ void ftmpc_linearize_kernel<double, 0>(const DeviceConsts, const LinParams);
template __global__ void ftmpc_linearize_kernel<double, 1>(const DeviceConsts, const LinParams);
template __global__ void ftmpc_linearize_kernel<double, 2>(const DeviceConsts, const LinParams);
template __global__ void ftmpc_linearize_kernel<double, 0, 1>(const DeviceConsts, const LinParams);
template __global__ void ftmpc_linearize_kernel<double, 1, 1>(const DeviceConsts, const LinParams);
template __global__ void ftmpc_linearize_kernel<double, 2, 1>(const DeviceConsts, const LinParams);

// ---------------------------------------------------------------------------------------------------------
// Cost of the nonlinear program for given thruster sequences (merit function of the line-search SQP; include/ftmpc.h
// ftmpc_eval_cost_batch).  One lane per instance, float64.
// ---------------------------------------------------------------------------------------------------------
struct CostParams {
    int64_t B;
    const double* x0;
    const double* ub;
    const double* stuck;
    const double* xref;
    int64_t xref_stride;
    const double* uref;
    int64_t uref_stride;
    const double* U;        // [B*N*NT]
    const TermCost* tcost;  // or nullptr
    double* out;            // [B]  (ntrial > 0: [B*ntrial])
    // line search of the SQP, all trial points in one launch (ntrial > 0): lane b * ntrial + j evaluates the point
    // U + 2^-j (clip(Uq, 0, ub) - U) of instance b -- what ftmpc_sqp_trial_kernel would store for alpha = 2^-j -- for the instances with todo set
    const double* Uq = nullptr;
    const int32_t* todo = nullptr;
    int32_t ntrial = 0;
};

namespace {
// centre dynamics (spiral_model.py:44-76): s = [p, v, w, q]
__device__ inline void centre_rhs(const DeviceConsts& C, const double s[13], const double gen[6], double ds[13]) {
    const double* v = s + 3;
    const double* w = s + 6;
    const double* q = s + 9;
    double Jw[3], wxJw[3], t[3], dw[3];
    mat3vec(C.J, w, Jw);
    cross3(w, Jw, wxJw);
    for (int i = 0; i < 3; ++i) t[i] = gen[3 + i] - wxJw[i];
    mat3vec(C.Jinv, t, dw);
    double wxr[3], wxwxr[3], dwxr[3], ab[3], RT[9], dv[3];
    cross3(w, C.r, wxr);
    cross3(w, wxr, wxwxr);
    cross3(dw, C.r, dwxr);
    for (int i = 0; i < 3; ++i) ab[i] = gen[i] * C.inv_mass + dwxr[i] + wxwxr[i];
    rotT(q, RT);
    mat3vec(RT, ab, dv);
    for (int i = 0; i < 3; ++i) {
        ds[i] = v[i];
        ds[3 + i] = dv[i];
        ds[6 + i] = dw[i];
    }
    ds[9] = 0.5 * (w[2] * q[1] - w[1] * q[2] + w[0] * q[3]);
    ds[10] = 0.5 * (-w[2] * q[0] + w[0] * q[2] + w[1] * q[3]);
    ds[11] = 0.5 * (w[1] * q[0] - w[0] * q[1] + w[2] * q[3]);
    ds[12] = 0.5 * (-w[0] * q[0] - w[1] * q[1] - w[2] * q[2]);
}
}  // namespace

__global__ void __launch_bounds__(64) ftmpc_cost_kernel(const DeviceConsts C, const CostParams P) {
    const int64_t lane_id = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int64_t b = P.ntrial > 0 ? lane_id / P.ntrial : lane_id;
    if (b >= P.B) return;
    const int jt = P.ntrial > 0 ? (int)(lane_id - b * P.ntrial) : 0;
    if (P.ntrial > 0 && !P.todo[b]) return;
    const double alpha = ldexp(1.0, -jt);      // (a power of two: alpha * step is exact, the point is the one the trial kernel stores)
    const int N = C.N, NT = C.NT;
    double s[13];
    {
        double x[13];
        for (int i = 0; i < 13; ++i) x[i] = P.x0[b * 13 + i];
        double RT[9], wxr[3], a[3], c[3];
        rotT(x + 6, RT);
        cross3(x + 10, C.r, wxr);
        mat3vec(RT, C.r, a);
        mat3vec(RT, wxr, c);
        for (int i = 0; i < 3; ++i) {
            s[i] = x[i] + a[i];
            s[3 + i] = x[3 + i] + c[i];
            s[6 + i] = x[10 + i];
        }
        for (int i = 0; i < 4; ++i) s[9 + i] = x[6 + i];
    }
    const double* xref = P.xref + b * P.xref_stride;
    const double* uref = P.uref ? P.uref + b * P.uref_stride : nullptr;
    const double dt = C.dt;
    double cost = 0.0;
    for (int k = 0; k < N; ++k) {
        double gen[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < NT; ++i) {
            const bool healthy = P.ub[b * NT + i] > 0.0;
            double u = healthy ? P.U[(b * N + k) * NT + i] : 0.0;
            if (P.ntrial > 0 && healthy) u = u + alpha * (fmin(fmax(P.Uq[(b * N + k) * NT + i], 0.0), P.ub[b * NT + i]) - u);
            cost += C.rho * u * u;
            const double t = u + P.stuck[b * NT + i];
            for (int g = 0; g < 6; ++g) gen[g] += C.D[g * MAX_NT + i] * t;
        }
        double ur[6] = {0, 0, 0, 0, 0, 0};
        if (uref) {
            double RT[9], f3[3] = {uref[6 * k], uref[6 * k + 1], uref[6 * k + 2]}, o[3];
            rotT(s + 9, RT);
            mat3vec(RT, f3, o);
            ur[0] = o[0]; ur[1] = o[1]; ur[2] = o[2];
            ur[3] = uref[6 * k + 3]; ur[4] = uref[6 * k + 4]; ur[5] = uref[6 * k + 5];
        }
        for (int g = 0; g < 6; ++g) {
            const double ut = gen[g] - ur[g] - (g < 3 ? C.fvirt[g] : 0.0);
            cost += C.R[g] * ut * ut;
        }
        // RK4 (sys_model.py:152-158), no quaternion renormalisation
        double k1[13], k2[13], k3[13], k4[13], t[13];
        centre_rhs(C, s, gen, k1);
        for (int i = 0; i < 13; ++i) t[i] = s[i] + 0.5 * dt * k1[i];
        centre_rhs(C, t, gen, k2);
        for (int i = 0; i < 13; ++i) t[i] = s[i] + 0.5 * dt * k2[i];
        centre_rhs(C, t, gen, k3);
        for (int i = 0; i < 13; ++i) t[i] = s[i] + dt * k3[i];
        centre_rhs(C, t, gen, k4);
        for (int i = 0; i < 13; ++i) s[i] += dt / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
        double e[9];
        for (int a = 0; a < 9; ++a) e[a] = s[a] - xref[9 * (k + 1) + a];
        if (k + 1 < N) {
            for (int a = 0; a < 9; ++a) cost += C.Q[a] * e[a] * e[a];
        } else {
            for (int a = 0; a < 9; ++a)
                for (int c = 0; c < 9; ++c) cost += e[a] * C.P[9 * a + c] * e[c];
            if (P.tcost) cost += term_cost_nq(*P.tcost, e, nullptr);
        }
    }
    P.out[lane_id] = cost;
}

// ---------------------------------------------------------------------------------------------------------
// The same cost in the GENERALIZED-FORCE formulation (include/ftmpc.h ftmpc_eval_cost_wrench_batch; merit function of
// ftmpc_solve_sqp_wrench_batch): the decision is the total wrench tau_k per stage, ut_k = tau_k - ur_k(q_k) - [f_virt; 0],
// no rho term (the wrench QP has none), plus the terminal-set violation sum_r max(0, (term_A e_N - term_b)_r).
// One lane per instance, float64.
// ---------------------------------------------------------------------------------------------------------
struct CostWrenchParams {
    int64_t B;
    const double* x0;
    const double* xref;
    int64_t xref_stride;
    const double* uref;
    int64_t uref_stride;
    const double* G;        // [B*N*6] total wrenches
    const TermCost* tcost;  // or nullptr
    const double* termA;    // [term_rows*9] or nullptr (no terminal set: violation 0)
    const double* termb;
    int32_t term_rows;
    double sigma;           // merit = cost + sigma * violation
    double* out_merit;      // [B]  (ntrial > 0: [B*ntrial])
    double* out_cost;       // or nullptr; indexed as out_merit
    double* out_tviol;      // or nullptr; indexed as out_merit
    double* out_X;          // [B*(N+1)*13] centre states of the rollout, or nullptr (ntrial == 0 only)
    // line search (ntrial > 0): lane b * ntrial + j evaluates G + 2^-j (Gq - G) of instance b, for the instances with todo set
    const double* Gq = nullptr;
    const int32_t* todo = nullptr;
    int32_t ntrial = 0;
    // the estimated disturbance [B*6] = (f^ inertial in N, t^ body in N m) of the DIST = 1 instantiation; nullptr: the plain one
    const double* dist = nullptr;
};

// DIST = 1 (ftmpc_eval_cost_wrench_disturbance_batch, the wrench SQP under an estimate): the rollout takes the estimate exactly where
// ftmpc_linearize_kernel<.., 1> puts it -- every RK4 stage is evaluated at tau + t^, and f^ / m is added to dv after the rotation (it
// is inertial, so it enters neither ab nor the dw x r term).  The R .* (gen - ur - f_virt) term keeps the COMMANDED wrench; the tracking
// terms, the terminal cost, the terminal-set violation and out_X are those of the disturbed rollout.  Lane b * ntrial + j reads the
// estimate of instance b.
template <int DIST = 0>
__global__ void __launch_bounds__(64) ftmpc_cost_wrench_kernel(const DeviceConsts C, const CostWrenchParams P) {
    const int64_t lane_id = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int64_t b = P.ntrial > 0 ? lane_id / P.ntrial : lane_id;
    if (b >= P.B) return;
    const int jt = P.ntrial > 0 ? (int)(lane_id - b * P.ntrial) : 0;
    if (P.ntrial > 0 && !P.todo[b]) return;
    const double alpha = ldexp(1.0, -jt);      // (a power of two: the point is the one ftmpc_sqpw_close_kernel stores)
    const int N = C.N;
    double s[13];
    {
        double x[13];
        for (int i = 0; i < 13; ++i) x[i] = P.x0[b * 13 + i];
        double RT[9], wxr[3], a[3], c[3];
        rotT(x + 6, RT);
        cross3(x + 10, C.r, wxr);
        mat3vec(RT, C.r, a);
        mat3vec(RT, wxr, c);
        for (int i = 0; i < 3; ++i) {
            s[i] = x[i] + a[i];
            s[3 + i] = x[3 + i] + c[i];
            s[6 + i] = x[10 + i];
        }
        for (int i = 0; i < 4; ++i) s[9 + i] = x[6 + i];
    }
    double* X = P.out_X ? P.out_X + b * (int64_t)(N + 1) * 13 : nullptr;
    if (X)
        for (int i = 0; i < 13; ++i) X[i] = s[i];
    const double* xref = P.xref + b * P.xref_stride;
    const double* uref = P.uref ? P.uref + b * P.uref_stride : nullptr;
    const double dt = C.dt;
    double dfm[3] = {0, 0, 0}, dtq[3] = {0, 0, 0};      // DIST: f^ / m and t^
    if constexpr (DIST != 0) {
        for (int i = 0; i < 3; ++i) {
            dfm[i] = P.dist[b * 6 + i] * C.inv_mass;
            dtq[i] = P.dist[b * 6 + 3 + i];
        }
    }
    double cost = 0.0, viol = 0.0;
    for (int k = 0; k < N; ++k) {
        double gen[6];
        for (int g = 0; g < 6; ++g) {
            const double t = P.G[(b * N + k) * 6 + g];
            gen[g] = P.ntrial > 0 ? t + alpha * (P.Gq[(b * N + k) * 6 + g] - t) : t;
        }
        double ur[6] = {0, 0, 0, 0, 0, 0};
        if (uref) {
            double RT[9], f3[3] = {uref[6 * k], uref[6 * k + 1], uref[6 * k + 2]}, o[3];
            rotT(s + 9, RT);
            mat3vec(RT, f3, o);
            ur[0] = o[0]; ur[1] = o[1]; ur[2] = o[2];
            ur[3] = uref[6 * k + 3]; ur[4] = uref[6 * k + 4]; ur[5] = uref[6 * k + 5];
        }
        for (int g = 0; g < 6; ++g) {
            const double ut = gen[g] - ur[g] - (g < 3 ? C.fvirt[g] : 0.0);
            cost += C.R[g] * ut * ut;
        }
        // RK4 (sys_model.py:152-158), no quaternion renormalisation; the stage sum k1 + 2 k2 + 2 k3 + k4 accumulated in
        // the order ftmpc_cost_kernel evaluates it (four 13-vectors live instead of six)
        double acc[13], kk[13], t[13];
        // (the commanded wrench is spent: under DIST the torque the model sees is tau + t^, as in the linearise kernel)
        if constexpr (DIST != 0)
            for (int i = 0; i < 3; ++i) gen[3 + i] += dtq[i];
        centre_rhs(C, s, gen, kk);
        if constexpr (DIST != 0)
            for (int i = 0; i < 3; ++i) kk[3 + i] += dfm[i];
        for (int i = 0; i < 13; ++i) {
            acc[i] = kk[i];
            t[i] = s[i] + 0.5 * dt * kk[i];
        }
        centre_rhs(C, t, gen, kk);
        if constexpr (DIST != 0)
            for (int i = 0; i < 3; ++i) kk[3 + i] += dfm[i];
        for (int i = 0; i < 13; ++i) {
            acc[i] += 2.0 * kk[i];
            t[i] = s[i] + 0.5 * dt * kk[i];
        }
        centre_rhs(C, t, gen, kk);
        if constexpr (DIST != 0)
            for (int i = 0; i < 3; ++i) kk[3 + i] += dfm[i];
        for (int i = 0; i < 13; ++i) {
            acc[i] += 2.0 * kk[i];
            t[i] = s[i] + dt * kk[i];
        }
        centre_rhs(C, t, gen, kk);
        if constexpr (DIST != 0)
            for (int i = 0; i < 3; ++i) kk[3 + i] += dfm[i];
        for (int i = 0; i < 13; ++i) s[i] += dt / 6.0 * (acc[i] + kk[i]);
        if (X)
            for (int i = 0; i < 13; ++i) X[(k + 1) * 13 + i] = s[i];
        double e[9];
        for (int a = 0; a < 9; ++a) e[a] = s[a] - xref[9 * (k + 1) + a];
        if (k + 1 < N) {
            for (int a = 0; a < 9; ++a) cost += C.Q[a] * e[a] * e[a];
        } else {
            for (int a = 0; a < 9; ++a)
                for (int c = 0; c < 9; ++c) cost += e[a] * C.P[9 * a + c] * e[c];
            if (P.tcost) cost += term_cost_nq(*P.tcost, e, nullptr);
            for (int r = 0; r < P.term_rows; ++r) {
                double v = -P.termb[r];
                for (int a = 0; a < 9; ++a) v += P.termA[9 * r + a] * e[a];
                viol += fmax(v, 0.0);
            }
        }
    }
    P.out_merit[lane_id] = cost + P.sigma * viol;
    if (P.out_cost) P.out_cost[lane_id] = cost;
    if (P.out_tviol) P.out_tviol[lane_id] = viol;
}

template __global__ void ftmpc_cost_wrench_kernel<0>(const DeviceConsts, const CostWrenchParams);
template __global__ void ftmpc_cost_wrench_kernel<1>(const DeviceConsts, const CostWrenchParams);

}  // namespace ftmpc
