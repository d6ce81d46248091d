// Diagnostic: the in-register 16x16 potrf + inverse that reads W = L^-1 from the eliminated columns of the tile, against a
// verbatim copy of the form it replaced (a second tile E that starts as I and takes the same row operations), on the same
// matrices in the same run.  One wave per matrix.  tests/test_gpu_potrf_merged.py parses the lines printed here.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "../fault-tolerant-mpc_amd/csrc/ftmpc_solve.hip"
namespace ftmpc {
// ---- the earlier form, kept as the reference ------------------------------------------------------------------------------
template <int J, class Work>
__device__ __forceinline__ void ref_potrf_inv_step(float (&c)[4], float (&e)[4], float (&w)[4], int bperm_base, const Work& work) {
    constexpr int QJ = J >> 2, RJ = J & 3;
    const float ej = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(bperm_base + 64 * QJ, __builtin_bit_cast(int, e[RJ])));
    const float d = readlane_f(c[RJ], 16 * QJ + J);
    const float inv = __builtin_amdgcn_rsqf(d);
    const float nrd = -inv * inv;
    work.template run<5 * J + 0>();
    if constexpr (J < 15) {
        const float rowj = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(bperm_base + 64 * QJ, __builtin_bit_cast(int, c[RJ])));   // A[J][col] in every row-group
        work.template run<5 * J + 1>();
        // the pivot column itself stays as it is (multiplier 0): the inverse below still needs it unscaled
        fmac4_rowbcast<J>(c, c, sel<StepMasks<J>::piv>(rowj * nrd, 0.f));
        work.template run<5 * J + 2>();
    } else {
        work.template run<5 * J + 1>();
        work.template run<5 * J + 2>();
    }
    asm("s_nop 1\n\tv_mul_f32_dpp %0, %1, %2 quad_perm:[0,1,2,3] row_mask:%3 bank_mask:0xf" : "+v"(w[RJ]) : "v"(ej), "v"(inv), "n"(1 << QJ));
    work.template run<5 * J + 3>();
    if constexpr (J < 15) fmac4_rowbcast<J>(e, c, ej * nrd);
    work.template run<5 * J + 4>();
}
template <class Work>
__device__ __forceinline__ void ref_potrf_inv16(float (&c)[4], float (&w)[4], int lane, const Work& work) {
    const int q = lane >> 4, col = lane & 15;
    float e[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        e[rr] = (4 * q + rr == col) ? 1.f : 0.f;
        w[rr] = 0.f;
    }
    const int bb = 4 * col;   // ds_bpermute byte address of lane `col` of row-group 0
#if FTMPC_POTRF_PRIO
    __builtin_amdgcn_s_setprio(FTMPC_POTRF_PRIO);
#endif
    ref_potrf_inv_step<0>(c, e, w, bb, work);   ref_potrf_inv_step<1>(c, e, w, bb, work);
    ref_potrf_inv_step<2>(c, e, w, bb, work);   ref_potrf_inv_step<3>(c, e, w, bb, work);
    ref_potrf_inv_step<4>(c, e, w, bb, work);   ref_potrf_inv_step<5>(c, e, w, bb, work);
    ref_potrf_inv_step<6>(c, e, w, bb, work);   ref_potrf_inv_step<7>(c, e, w, bb, work);
    ref_potrf_inv_step<8>(c, e, w, bb, work);   ref_potrf_inv_step<9>(c, e, w, bb, work);
    ref_potrf_inv_step<10>(c, e, w, bb, work);  ref_potrf_inv_step<11>(c, e, w, bb, work);
    ref_potrf_inv_step<12>(c, e, w, bb, work);  ref_potrf_inv_step<13>(c, e, w, bb, work);
    ref_potrf_inv_step<14>(c, e, w, bb, work);  ref_potrf_inv_step<15>(c, e, w, bb, work);
#if FTMPC_POTRF_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
}
__device__ __forceinline__ void ref_potrf_inv16_half(float (&c)[4], float (&w)[4], int lane) {
    const int q = lane >> 4, col = lane & 15;
    float e[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        e[rr] = (4 * q + rr == col) ? 1.f : 0.f;
        w[rr] = 0.f;
    }
    const int bb = 4 * col;
    const NoWork work{};
#if FTMPC_POTRF_PRIO
    __builtin_amdgcn_s_setprio(FTMPC_POTRF_PRIO);
#endif
    ref_potrf_inv_step<0>(c, e, w, bb, work);   ref_potrf_inv_step<1>(c, e, w, bb, work);
    ref_potrf_inv_step<2>(c, e, w, bb, work);   ref_potrf_inv_step<3>(c, e, w, bb, work);
    ref_potrf_inv_step<4>(c, e, w, bb, work);   ref_potrf_inv_step<5>(c, e, w, bb, work);
    ref_potrf_inv_step<6>(c, e, w, bb, work);   ref_potrf_inv_step<7>(c, e, w, bb, work);
#if FTMPC_POTRF_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) w[rr] = (q >= 2) ? e[rr] : w[rr];
}

// ---- kernels: block b (one wave) factors matrix b -------------------------------------------------------------------------
// MODE 0: potrf_inv16, 1: the reference copy, 2: potrf_inv16_half, 3: the reference copy of the half tile
template <int MODE>
__global__ void __launch_bounds__(64) k_potrf(const float* A, float* W, int nmat) {
    const int b = blockIdx.x;
    if (b >= nmat) return;
    const int lane = threadIdx.x, q = lane >> 4, col = lane & 15;
    float c[4], w[4];
    for (int rr = 0; rr < 4; ++rr) c[rr] = A[(size_t)b * 256 + (4 * q + rr) * 16 + col];
    if constexpr (MODE == 0) potrf_inv16(c, w, lane);
    else if constexpr (MODE == 1) ref_potrf_inv16(c, w, lane, NoWork{});
    else if constexpr (MODE == 2) potrf_inv16_half(c, w, lane);
    else ref_potrf_inv16_half(c, w, lane);
    for (int rr = 0; rr < 4; ++rr) W[(size_t)b * 256 + (4 * q + rr) * 16 + col] = w[rr];
}
// A work object in the shape of SchurWork: NM slots, one MFMA each, consecutive slots on different accumulators; it counts
// the slots that ran.
template <int NM>
struct CountWork {
    static_assert(NM <= 80, "more MFMAs than potrf slots");
    const f32x4 (&X)[4];
    f32x4 (&b)[3];
    int& count;
    template <int S>
    __device__ __forceinline__ void run() const {
        if constexpr (S < NM) {
            b[S % 3] = mfma4(X[S % 4][(S / 4) % 4], X[(S + 1) % 4][(S / 3) % 4], b[S % 3]);
            ++count;
        }
    }
};
template <int NM>
__global__ void __launch_bounds__(64) k_call(const float* A, float* W, float* acc, float* acc_plain, int* count, int nmat) {
    const int b = blockIdx.x;
    if (b >= nmat) return;
    const int lane = threadIdx.x, q = lane >> 4, col = lane & 15;
    f32x4 cin, X[4], ba[3], bp[3];
    for (int rr = 0; rr < 4; ++rr) cin[rr] = A[(size_t)b * 256 + (4 * q + rr) * 16 + col];
    for (int t = 0; t < 4; ++t)
        for (int rr = 0; rr < 4; ++rr) X[t][rr] = 0.25f * cin[(rr + t) & 3] + 0.01f * (float)(t + 1);
    for (int t = 0; t < 3; ++t) ba[t] = bp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    int n = 0;
    const f32x4 w = potrf_inv16_call(cin, lane, CountWork<NM>{X, ba, n});
#pragma unroll
    for (int S = 0; S < NM; ++S) bp[S % 3] = mfma4(X[S % 4][(S / 4) % 4], X[(S + 1) % 4][(S / 3) % 4], bp[S % 3]);
    for (int rr = 0; rr < 4; ++rr) W[(size_t)b * 256 + (4 * q + rr) * 16 + col] = w[rr];
    for (int t = 0; t < 3; ++t)
        for (int rr = 0; rr < 4; ++rr) {
            acc[((size_t)b * 3 + t) * 256 + 4 * lane + rr] = ba[t][rr];
            acc_plain[((size_t)b * 3 + t) * 256 + 4 * lane + rr] = bp[t][rr];
        }
    if (lane == 0) count[b] = n;
}
}   // namespace ftmpc

#define CHECK(x)                                                                        \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                         \
            printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__);      \
            return 2;                                                                   \
        }                                                                               \
    } while (0)

// kind 'a': B B' + I;  'b': the same plus a diagonal 10^[-3, 8] on a random subset of rows;  'c': 8 x 8 of kind b, rows 8..15 identity
static void make_matrix(std::mt19937& g, char kind, float* A) {
    std::uniform_real_distribution<double> u(-0.5, 0.5), e(-3.0, 8.0), p(0.0, 1.0);
    const int n = (kind == 'c') ? 8 : 16;
    double Bm[16][16];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) Bm[i][j] = u(g);
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) A[i * 16 + j] = (i == j) ? 1.f : 0.f;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = (i == j) ? 1.0 : 0.0;
            for (int k = 0; k < n; ++k) s += Bm[i][k] * Bm[j][k];
            A[i * 16 + j] = A[j * 16 + i] = (float)s;
        }
    if (kind != 'a')
        for (int i = 0; i < n; ++i) {
            const double sig = pow(10.0, e(g));
            if (p(g) < 0.5) A[i * 16 + i] += (float)sig;
        }
}
// float64 Cholesky factor and its inverse of the float32 matrix
static void chol64(const float* A, double* L, double* Wi) {
    for (int i = 0; i < 256; ++i) L[i] = Wi[i] = 0.0;
    for (int j = 0; j < 16; ++j) {
        double d = A[j * 16 + j];
        for (int k = 0; k < j; ++k) d -= L[j * 16 + k] * L[j * 16 + k];
        L[j * 16 + j] = sqrt(d);
        for (int i = j + 1; i < 16; ++i) {
            double s = A[i * 16 + j];
            for (int k = 0; k < j; ++k) s -= L[i * 16 + k] * L[j * 16 + k];
            L[i * 16 + j] = s / L[j * 16 + j];
        }
    }
    for (int j = 0; j < 16; ++j)        // column j of L^-1 by forward substitution
        for (int i = j; i < 16; ++i) {
            double s = (i == j) ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) s -= L[i * 16 + k] * Wi[k * 16 + j];
            Wi[i * 16 + j] = s / L[i * 16 + i];
        }
}
struct Err { double wl = 0, w = 0; };
static Err errors(const float* W, const double* L, const double* Wi) {
    Err r;
    double wmax = 0;
    for (int i = 0; i < 256; ++i) wmax = fmax(wmax, fabs(Wi[i]));
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) {
            double s = 0;
            for (int k = 0; k < 16; ++k) s += (double)W[i * 16 + k] * L[k * 16 + j];
            r.wl = fmax(r.wl, fabs(s - (i == j)));
            r.w = fmax(r.w, fabs(W[i * 16 + j] - Wi[i * 16 + j]) / wmax);
        }
    return r;
}

int main() {
    const int Bs[3] = {1, 2, 130};
    const int BMAX = 130;
    float *dA, *dW, *dAcc, *dAccP;
    int* dCount;
    CHECK(hipMalloc(&dA, BMAX * 1024));
    CHECK(hipMalloc(&dW, BMAX * 1024));
    CHECK(hipMalloc(&dAcc, BMAX * 3 * 1024));
    CHECK(hipMalloc(&dAccP, BMAX * 3 * 1024));
    CHECK(hipMalloc(&dCount, BMAX * 4));
    std::vector<float> A(BMAX * 256), Wn(BMAX * 256), Wr(BMAX * 256), acc(BMAX * 768), accp(BMAX * 768);
    std::vector<int> count(BMAX);
    std::vector<double> L(256), Wi(256);
    for (char kind : {'a', 'b', 'c'})
        for (int B : Bs) {
            // matrices b and b + nuniq are equal: the same bits must come out wherever their wave ran
            const int nuniq = (B + 1) / 2;
            std::mt19937 g(1000 * kind + B);
            for (int b = 0; b < nuniq; ++b) make_matrix(g, kind, &A[b * 256]);
            for (int b = nuniq; b < B; ++b) memcpy(&A[b * 256], &A[(b - nuniq) * 256], 1024);
            CHECK(hipMemcpy(dA, A.data(), B * 1024, hipMemcpyHostToDevice));
            CHECK(hipMemset(dW, 0xff, B * 1024));
            if (kind == 'c') hipLaunchKernelGGL(ftmpc::k_potrf<2>, dim3(B), dim3(64), 0, 0, dA, dW, B);
            else hipLaunchKernelGGL(ftmpc::k_potrf<0>, dim3(B), dim3(64), 0, 0, dA, dW, B);
            CHECK(hipMemcpy(Wn.data(), dW, B * 1024, hipMemcpyDeviceToHost));
            CHECK(hipMemset(dW, 0xff, B * 1024));
            if (kind == 'c') hipLaunchKernelGGL(ftmpc::k_potrf<3>, dim3(B), dim3(64), 0, 0, dA, dW, B);
            else hipLaunchKernelGGL(ftmpc::k_potrf<1>, dim3(B), dim3(64), 0, 0, dA, dW, B);
            CHECK(hipMemcpy(Wr.data(), dW, B * 1024, hipMemcpyDeviceToHost));
            Err en, er;
            double upper = 0, worst_ratio = 0;
            int dup = 0, ident = 0;
            for (int b = 0; b < B; ++b) {
                chol64(&A[b * 256], L.data(), Wi.data());
                const Err n1 = errors(&Wn[b * 256], L.data(), Wi.data()), r1 = errors(&Wr[b * 256], L.data(), Wi.data());
                en.wl = fmax(en.wl, n1.wl); en.w = fmax(en.w, n1.w);
                er.wl = fmax(er.wl, r1.wl); er.w = fmax(er.w, r1.w);
                if (r1.wl > 0) worst_ratio = fmax(worst_ratio, n1.wl / r1.wl);
                for (int i = 0; i < 16; ++i)
                    for (int j = i + 1; j < 16; ++j) upper = fmax(upper, fabs(Wn[b * 256 + i * 16 + j]));
                if (b >= nuniq && memcmp(&Wn[b * 256], &Wn[(b - nuniq) * 256], 1024) != 0) ++dup;
                if (kind == 'c')      // rows 8..15 of W are rows of the identity, exactly
                    for (int i = 8; i < 16; ++i)
                        for (int j = 0; j < 16; ++j) ident += Wn[b * 256 + i * 16 + j] != ((i == j) ? 1.f : 0.f);
            }
            printf("case=%c B=%d new_wl=%.6e ref_wl=%.6e new_w=%.6e ref_w=%.6e upper=%.6e dup_mismatch=%d pad_rows_wrong=%d worst_matrix_ratio=%.3f\n",
                   kind, B, en.wl, er.wl, en.w, er.w, upper, dup, ident, worst_ratio);
            if (kind != 'a') continue;
            // (d) the same matrices through potrf_inv16_call with a counting work object
            auto run_call = [&](auto nm_tag) -> int {
                constexpr int NM = decltype(nm_tag)::value;
                CHECK(hipMemset(dCount, 0, B * 4));
                hipLaunchKernelGGL(ftmpc::k_call<NM>, dim3(B), dim3(64), 0, 0, dA, dW, dAcc, dAccP, dCount, B);
                CHECK(hipMemcpy(Wr.data(), dW, B * 1024, hipMemcpyDeviceToHost));
                CHECK(hipMemcpy(acc.data(), dAcc, B * 3072, hipMemcpyDeviceToHost));
                CHECK(hipMemcpy(accp.data(), dAccP, B * 3072, hipMemcpyDeviceToHost));
                CHECK(hipMemcpy(count.data(), dCount, B * 4, hipMemcpyDeviceToHost));
                int cmin = 1 << 30, cmax = -1;
                for (int b = 0; b < B; ++b) { cmin = count[b] < cmin ? count[b] : cmin; cmax = count[b] > cmax ? count[b] : cmax; }
                printf("case=d B=%d NM=%d count_min=%d count_max=%d acc_mismatch=%d w_mismatch=%d\n", B, NM, cmin, cmax,
                       memcmp(acc.data(), accp.data(), B * 3072) != 0, memcmp(Wr.data(), Wn.data(), B * 1024) != 0);
                return 0;
            };
            if (run_call(std::integral_constant<int, 48>{})) return 2;
            if (run_call(std::integral_constant<int, 80>{})) return 2;
        }
    // (e) a negative pivot at step 3 and a zero pivot: W[15][15] (lane 63, register 3) must not be finite
    {
        std::mt19937 g(5);
        make_matrix(g, 'a', &A[0]);
        make_matrix(g, 'a', &A[256]);
        A[3 * 16 + 3] = -5.f;
        for (int i = 0; i < 16; ++i) A[256 + i] = A[256 + i * 16] = 0.f;
        CHECK(hipMemcpy(dA, A.data(), 2 * 1024, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(ftmpc::k_potrf<0>, dim3(2), dim3(64), 0, 0, dA, dW, 2);
        CHECK(hipMemcpy(Wn.data(), dW, 2 * 1024, hipMemcpyDeviceToHost));
        printf("case=e negative_pivot_w1515_finite=%d zero_pivot_w1515_finite=%d\n", (int)std::isfinite(Wn[255]), (int)std::isfinite(Wn[256 + 255]));
    }
    CHECK(hipDeviceSynchronize());
    printf("done\n");
    return 0;
}
