// ftmpc_capi.hip -- host side of the C-ABI declared in include/ftmpc.h.
//
// Owns the device workspace (DevBuf: every device allocation frees itself with its owner), converts the double-precision
// problem constants into the kernel argument blocks and enqueues, per entry point, ftmpc_linearize_kernel and the solve kernel
// the handle's shape is routed to (the instantiation of a templated family is picked in ONE place, pick_*,
// for the occupancy query that sizes its persistent grid and for the launch alike), the allocation, cost, SQP and plant kernels.
// There is deliberately NO CPU fallback: every entry point fails with FTMPC_ERR_NODEVICE /
// FTMPC_ERR_HIP when the gfx950 device or the code object is unusable.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/ftmpc.h"
#include "ftmpc_common.h"

// single translation unit: the kernels are compiled together with their launcher
#include "ftmpc_linearize.hip"
#include "ftmpc_solve.hip"
#include "ftmpc_solve_f64.hip"
#include "ftmpc_solve_wg.hip"
#include "ftmpc_solve_ws.hip"
#include "ftmpc_solve_ws64.hip"
#include "ftmpc_solve_wsw.hip"
#include "ftmpc_solve_hull.hip"
#include "ftmpc_solve_ric.hip"
#include "ftmpc_solve_ricw.hip"
#include "ftmpc_sim.hip"
#include "ftmpc_alloc.hip"

using ftmpc::DeviceConsts;
using ftmpc::LinParams;
using ftmpc::SolveParams;
using ftmpc::Solve64Params;
using ftmpc::TermCost;
using ftmpc::SolveWgParams;
using ftmpc::SolveWs64Params;

static thread_local std::string g_create_error;

// A device allocation and its capacity in elements.  Freed with its owner; reads as the pointer it holds.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    operator T*() const { return p; }
    int ensure(ftmpc_handle* h, int64_t count);      // room for `count` elements (contents are not kept)
};

struct ftmpc_handle {
    ftmpc_config cfg;
    DeviceConsts dc;
    int device = 0;
    int num_cu = 0;
    int nb_max = 0;  // ceil(N*NT/16)
    std::string err;
    hipStream_t stream = nullptr;  // internal stream of the host-buffer entry point
    // workspace
    int64_t cap_batch = 0;      // instances the ftmpc_reserve set holds: rec, d_x0 .. d_iters (not the reference windows), d_qlist, d_eN, d_cbar
    DevBuf<float> rec;          // (float64 records)
    // device mirrors of host buffers
    DevBuf<double> d_x0, d_ub, d_stuck, d_xref, d_uref;
    DevBuf<double> d_warm, d_u0, d_U;
    DevBuf<int32_t> d_status, d_iters;
    // where the last closed loop with a sensor left off (ftmpc_sensor.step0): the warm start its last step shifted, the truth it
    // returned, the number of the step that would follow.  A call whose step0, batch, form and x are these continues from it.
    DevBuf<double> d_keep_warm;
    std::vector<double> keep_x;
    int64_t keep_B = 0, keep_step = -1;
    bool keep_wrench = false;
    // the estimated disturbance [B*6] the next linearisation takes (ftmpc_disturbance.compensate = 1: set around the solve of a loop
    // step; ftmpc_debug_records_disturbance), nullptr: the plain instantiations
    const double* lin_dist = nullptr;
    // allocation operator (ftmpc_allocate_batch)
    DevBuf<double> d_atau, d_aub, d_au;
    DevBuf<int32_t> d_ast, d_ait;
    int64_t cap_alloc = 0;
    // per-instantiation Hessian slots
    DevBuf<float> hs[3];   // NB = 8, 9, 10 instantiations
    int grid[3] = {0, 0, 0};
    // work lists of the fp32 instantiations: qlist [3][cap_batch], qctl = {count[3], pad, head[3], pad}
    DevBuf<int32_t> d_qlist;
    DevBuf<int32_t> d_qctl;
    // Hint from the previous step: the list lengths it ended with, copied to pinned memory behind its kernels.  A list that was
    // empty then gets a SMALL grid now (the kernels are persistent: any grid drains any list, a small one just slower if the hint
    // is wrong: one step, then the hint is right again) -- most batches fill one list, and an idle launch of a full grid costs
    // 0.05 - 0.09 ms.
    int32_t* h_qcnt = nullptr;      // pinned, 4 ints
    hipEvent_t ev_qcnt = nullptr;
    bool qcnt_pending = false, qcnt_valid = false;
    int32_t last_cnt[4] = {0, 0, 0, 0};
    // pinned staging of the host-buffer entry points (hipHostMalloc; mirrors of the device buffers)
    struct Pinned {
        void* p = nullptr;
        size_t bytes = 0;
    };
    Pinned pin_in, pin_out;
    hipStream_t s_in = nullptr, s_out = nullptr;
    static constexpr int MAX_CHUNKS = 8;
    hipEvent_t ev_in[MAX_CHUNKS] = {}, ev_k[MAX_CHUNKS] = {}, ev_out[MAX_CHUNKS] = {};
    int64_t lin_split_max = 8192;   // ftmpc_config.lin_split_max overrides (0 here: never split)
    int stage_chunks = 0;   // 0: whole blocks of 65 536 instances (a persistent launch below that does not fill the device twice)
    // fp32 workgroup-per-instance kernel with the factor in LDS (160 < N*NT <= 240)
    bool use_ws = false;            // kernel 8 (wrench-space Schur form) takes the lists of NB = 9, 10 and of the workgroup kernel
    int ws_nb = 8, grid_ws = 0;
    DevBuf<float> ws_slot;
    int64_t ws_slot_words = 0;
    // kernel 10: the wrench-space form on ONE wave per instance (takes kernel 8's list when it applies)
    bool use_wsw = false;
    int grid_wsw = 0;
    DevBuf<float> wsw_slot;
    int64_t wsw_slot_words = 0;
    // kernel 11 (the generalized-force formulation with hull rows, one wave per instance, fp32): float64 scratch of its reference gradient
    DevBuf<float> hull_slot;
    int64_t hull_slot_words = 0;
    int grid_hull = 0;
    bool use_wg = false;
    DevBuf<float> wg_slot;
    int grid_wg = 0;
    int64_t wg_slot_words = 0;
    // float64 through the wrench-space form (kernel 9): 6 N <= 256, N * NT <= 768, ten or more thrusters
    bool tset_thruster = true;         // the thruster form with the terminal set is served: dense float64 kernel (n <= 256) or kernel 12 (N <= 40)
    bool tset_ric = false;             // ... by kernel 12's terminal-set instantiation (n > 256, or kernel_select = FTMPC_KERNEL_RICCATI)
    bool sbounds = false;              // state bounds: the thruster-space solve runs on kernel 12's state-bound instantiation
    DevBuf<double> d_cbar;             // [B*N*13] linearisation trajectory (state bounds only)
    bool use_ric64 = false;            // kernel 12: float64, Newton systems by the Riccati recursion, one wave per instance
    int ric_nv = 10;
    int grid_ric = 0;
    DevBuf<double> ric_slot;
    int64_t ric_slot_doubles = 0;
    bool use_ws64 = false;
    int ws64_nvt = 1, grid_ws64 = 0;
    DevBuf<double> ws64_slot;
    int64_t ws64_slot_doubles = 0;
    // float64 general-size path
    bool use_f64 = false;
    int npad_max = 0;
    int grid64 = 0;
    int64_t tile_doubles = 0, e_doubles = 0;
    DevBuf<double> Hs, Ls, Eall;
    DevBuf<double> d_dbgH64, d_dbgv64;
    // general-constraint modes of the float64 kernel (terminal set; generalized-force formulation)
    bool tset = false;
    DevBuf<double> d_term;             // [term_rows*9 | term_rows]
    DevBuf<double> d_eN;               // [cap_batch*9]
    int grid_gen = 0, npad_gen = 0;
    int64_t tile_doubles_gen = 0, e_doubles_gen = 0;
    DevBuf<double> gHs, gLs, gEall;    // slots of the wrench formulation (n = 6 N)
    // the two-stage step.  cap_wrench instances: d_hullb, d_hullset, d_warmG, d_tau0, d_G, d_taud, d_ast2; the last is [allocation
    // status | iterations | kernel 11's hand-over list], the list at 2 * cap_wrench (handover_list)
    DevBuf<double> d_hullA, d_hullb, d_warmG, d_tau0, d_G, d_taud;
    DevBuf<int32_t> d_hullset;
    DevBuf<int32_t> d_ast2;
    int64_t cap_wrench = 0;
    DevBuf<TermCost> d_tcost;          // non-quadratic terminal-cost terms (terminal_cost_terms != 0)
    DevBuf<double> d_cost;
    // on-device SQP (ftmpc_solve_sqp_batch): iterate, QP solution, trial point | J, Jt, J0, alpha | flags and counters (cap_sqp
    // instances); the merits of all trial points on their own
    DevBuf<double> d_sqU, d_sqQ, d_sqT, d_sqJ, d_sqJall;
    DevBuf<int32_t> d_sqF;
    int64_t cap_sqp = 0;
    // ... its launch sequence (a few hundred small launches per call) as a hipGraph: recorded the second time a call repeats the
    // previous one's shape, replayed from then on; any reallocation or change of the constants starts over
    hipStream_t stream2 = nullptr;     // the two-stage step: allocation beside kernel 13's hand-over pass
    hipEvent_t ev_fork = nullptr, ev_alloc = nullptr;
    uint64_t alloc_epoch = 0;          // bumped by every (re)allocation of a device buffer
    struct SqpKey {
        int64_t B = -1, xs = 0, us = 0;
        const void *xref = nullptr, *uref = nullptr, *warm = nullptr;
        int32_t iters = 0, backtracks = 0;
        double tol = 0;
        uint64_t epoch = 0, consts = 0;
        bool operator==(const SqpKey& o) const {
            return B == o.B && xs == o.xs && us == o.us && xref == o.xref && uref == o.uref && warm == o.warm && iters == o.iters &&
                   backtracks == o.backtracks && tol == o.tol && epoch == o.epoch && consts == o.consts;
        }
    } sqp_key, sqp_seen;
    hipGraphExec_t sqp_exec = nullptr;
    int64_t sqp_graph_launches = 0;    // (diagnostic: ftmpc_sqp_graph_launches)
    // line-search SQP of the generalized-force formulation (ftmpc_solve_sqp_wrench_batch): iterate, next iterate | merit, -, alpha,
    // cost and terminal-set violation of the start point and of the result | flags and counters (as d_sqF) | merits of all trial points
    // (cap_swsqp instances: d_swG, d_swT, d_swJ, d_swF)
    DevBuf<double> d_swG, d_swT, d_swJ, d_swJall, d_swX;
    DevBuf<double> d_ldist;            // the caller's estimate [B*6] of the ftmpc_*_wrench_disturbance_batch entries (lin_dist points at it)
    DevBuf<int32_t> d_swF;
    int64_t cap_swsqp = 0;
    // kernel 13: the two-stage form in float64 by the Riccati recursion (no terminal set, N <= 40, up to 128 hull rows)
    DevBuf<double> ricw_slot;
    int64_t ricw_slot_doubles = 0;
    int grid_ricw = 0;
    bool wrench_handed = false;        // the last two-stage step ran kernel 11 with its hand-over list (d_qctl[0] = its length)
    // debug
    DevBuf<float> d_dbgH, d_dbgv;
    // profiling
    bool profiling = false;
    hipEvent_t ev[2 * FTMPC_KERNEL_SLOTS] = {};  // start/stop per kernel slot
    bool ev_valid = false;
    bool ev_used[FTMPC_KERNEL_SLOTS] = {};
};

namespace {

int fail(ftmpc_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    else g_create_error = msg;
    return code;
}

#define HIP_TRY(h, expr)                                                                          \
    do {                                                                                          \
        hipError_t e__ = (expr);                                                                  \
        if (e__ != hipSuccess)                                                                    \
            return fail((h), FTMPC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

bool inv3(const double* M, double* out) {
    const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    if (!(std::fabs(det) > 1e-300)) return false;
    const double s = 1.0 / det;
    out[0] = (e * i - f * h) * s; out[1] = (c * h - b * i) * s; out[2] = (b * f - c * e) * s;
    out[3] = (f * g - d * i) * s; out[4] = (a * i - c * g) * s; out[5] = (c * d - a * f) * s;
    out[6] = (d * h - e * g) * s; out[7] = (b * g - a * h) * s; out[8] = (a * e - b * d) * s;
    return true;
}

// lower Cholesky of a 9x9 PSD matrix (zero pivots give zero columns)
bool chol9(const double* P, double* L) {
    std::memset(L, 0, 81 * sizeof(double));
    for (int j = 0; j < 9; ++j) {
        double d = P[9 * j + j];
        for (int k = 0; k < j; ++k) d -= L[9 * j + k] * L[9 * j + k];
        if (d < -1e-9 * std::fabs(P[9 * j + j]) - 1e-300) return false;
        const double l = d > 0 ? std::sqrt(d) : 0.0;
        L[9 * j + j] = l;
        for (int i = j + 1; i < 9; ++i) {
            double s = P[9 * i + j];
            for (int k = 0; k < j; ++k) s -= L[9 * i + k] * L[9 * j + k];
            L[9 * i + j] = l > 0 ? s / l : 0.0;
        }
    }
    return true;
}

int build_consts(const ftmpc_config& c, DeviceConsts& d, std::string& why) {
    if (c.N < 1 || c.N > 64) { why = "N out of range 1..64"; return FTMPC_ERR_ARG; }
    if (c.NT < 1 || c.NT > FTMPC_MAX_NT) { why = "NT out of range 1..16"; return FTMPC_ERR_ARG; }
    if (!(c.dt > 0) || !(c.mass > 0)) { why = "dt and mass must be positive"; return FTMPC_ERR_ARG; }
    if (!(c.rho > 0)) { why = "rho must be positive (strict convexity)"; return FTMPC_ERR_ARG; }
    std::memset(&d, 0, sizeof(d));
    d.N = c.N;
    d.NT = c.NT;
    d.max_iters = c.max_iters > 0 ? c.max_iters : 30;
    if ((c.dtype == FTMPC_DTYPE_F64 || c.N * c.NT > 240) && c.max_iters <= 0) d.max_iters = 30;
    d.dt = c.dt;
    d.inv_mass = 1.0 / c.mass;
    std::memcpy(d.J, c.J, sizeof(d.J));
    if (!inv3(c.J, d.Jinv)) { why = "J is singular"; return FTMPC_ERR_ARG; }
    std::memcpy(d.r, c.r, sizeof(d.r));
    d.r_y[1] = c.r[1];      // (the other components stay 0 from the memset)
    d.r_xz[0] = c.r[0];
    d.r_xz[2] = c.r[2];
    std::memcpy(d.fvirt, c.f_virt, sizeof(d.fvirt));
    // ArT = -[r]x Jinv
    const double* r = c.r;
    const double S[9] = {0, -r[2], r[1], r[2], 0, -r[0], -r[1], r[0], 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += S[3 * i + k] * d.Jinv[3 * k + j];
            d.ArT[3 * i + j] = -s;
        }
    for (int g = 0; g < 6; ++g)
        for (int t = 0; t < c.NT; ++t) d.D[g * ftmpc::MAX_NT + t] = c.D[g * c.NT + t];
    for (int i = 0; i < 9; ++i) {
        if (!(c.Q[i] >= 0)) { why = "Q must be non-negative"; return FTMPC_ERR_ARG; }
        d.Q[i] = c.Q[i];
        d.sq2Q[i] = std::sqrt(2.0 * c.Q[i]);
    }
    for (int i = 0; i < 6; ++i) {
        if (!(c.R[i] >= 0)) { why = "R must be non-negative"; return FTMPC_ERR_ARG; }
        d.R[i] = c.R[i];
    }
    std::memcpy(d.P, c.P, sizeof(d.P));
    double L[81];
    if (!chol9(c.P, L)) { why = "P must be symmetric positive semi-definite"; return FTMPC_ERR_ARG; }
    const double s2 = std::sqrt(2.0);
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) d.LPt[9 * i + j] = s2 * L[9 * j + i];  // sqrt(2) L'
    d.rho = c.rho;
    d.mu_stop = c.mu_stop > 0 ? c.mu_stop : ((c.dtype == FTMPC_DTYPE_F64 || c.N * c.NT > 240) ? 1e-13 : 1e-11);
    if (c.terminal_set && !(c.mu_stop > 0)) d.mu_stop = 1e-10;   // general rows: C' W C ruins the conditioning below that
    d.mu_refine = 1e-3;
    return FTMPC_OK;
}

}  // namespace

template <typename T>
int DevBuf<T>::ensure(ftmpc_handle* h, int64_t count) {
    if (count <= cap) return FTMPC_OK;
    cap = 0;   // (a failed growth must not leave a stale capacity)
    ++h->alloc_epoch;
    if (p) (void)hipFree(p);
    p = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), (size_t)count * sizeof(T));
    if (e != hipSuccess) {
        (void)hipGetLastError();   // the runtime keeps the failure as its "last error": left there, the next launch check would report it
        return fail(h, FTMPC_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    cap = count;
    return FTMPC_OK;
}

namespace {

// Buffers that share ONE capacity `cap`, in instances (layouts and entry points read it: handover_list, ftmpc_reserve): it is 0 while
// `each` grows them, so after a failure part-way the next call grows them again instead of launching on freed pointers.
template <typename F>
int ensure_group(int64_t& cap, int64_t n, F&& each) {
    if (n <= cap) return FTMPC_OK;
    cap = 0;
    const int rc = each();
    if (rc == FTMPC_OK) cap = n;
    return rc;
}

// kernel 11's hand-over list (written by kernel 11, read by kernel 13 / the dense float64 kernel and by the allocation in list
// mode): behind the allocation status and iterations in d_ast2, at the CAPACITY of that buffer, whatever the batch
int32_t* handover_list(const ftmpc_handle* h) { return h->d_ast2 + 2 * h->cap_wrench; }

// the rows of the terminal set on the device (term_A | term_b), once per handle: at create for the thruster form, at the first call
// of the generalized-force formulation otherwise
int term_upload(ftmpc_handle* h) {
    if (!h->cfg.terminal_set || h->d_term) return FTMPC_OK;
    if (h->cfg.term_rows < 1 || h->cfg.term_rows > FTMPC_MAX_TERM_ROWS) return fail(h, FTMPC_ERR_ARG, "term_rows out of range");
    int rc = h->d_term.ensure(h, (int64_t)h->cfg.term_rows * 10);
    if (rc != FTMPC_OK) return rc;
    std::vector<double> t((size_t)h->cfg.term_rows * 10);
    std::memcpy(t.data(), h->cfg.term_A, (size_t)h->cfg.term_rows * 9 * sizeof(double));
    std::memcpy(t.data() + (size_t)h->cfg.term_rows * 9, h->cfg.term_b, (size_t)h->cfg.term_rows * sizeof(double));
    HIP_TRY(h, hipMemcpy(h->d_term, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    return FTMPC_OK;
}

// ---- one pick per templated kernel family: the occupancy query that sizes a persistent grid (and its per-workgroup slots) and the
// launch both take the instantiation from here, so they cannot disagree.  The wrench-side families also take the hull row count.
using F32Kernel = void (*)(DeviceConsts, SolveParams);
using WgKernel = void (*)(DeviceConsts, SolveWgParams);
using Ws64Kernel = void (*)(DeviceConsts, SolveWs64Params);
using Ric64Kernel = void (*)(DeviceConsts, ftmpc::SolveRicParams);
using F64Kernel = void (*)(DeviceConsts, Solve64Params);
using HullKernel = void (*)(DeviceConsts, ftmpc::SolveHullParams);
using RicwKernel = void (*)(DeviceConsts, ftmpc::SolveRicwParams);

F32Kernel pick_f32(int v) {      // work list v: ceil(n / 16) <= 8 + v
    return v == 0 ? ftmpc::ftmpc_solve_f32_kernel<8> : (v == 1 ? ftmpc::ftmpc_solve_f32_kernel<9> : ftmpc::ftmpc_solve_f32_kernel<10>);
}
WgKernel pick_ws32(const ftmpc_handle* h) { return h->ws_nb == 6 ? ftmpc::ftmpc_solve_ws32_kernel<6> : ftmpc::ftmpc_solve_ws32_kernel<8>; }
F32Kernel pick_wsw32(const ftmpc_handle* h) { return h->ws_nb == 6 ? ftmpc::ftmpc_solve_wsw32_kernel<6> : ftmpc::ftmpc_solve_wsw32_kernel<8>; }
Ws64Kernel pick_ws64(const ftmpc_handle* h) { return h->ws64_nvt == 1 ? ftmpc::ftmpc_solve_ws64_kernel<1> : ftmpc::ftmpc_solve_ws64_kernel<3>; }
Ric64Kernel pick_ric64(const ftmpc_handle* h) {
    if (h->tset_ric && h->ric_nv == 4) return ftmpc::ftmpc_solve_ric64_kernel<4, false, true>;
    if (h->tset_ric && h->ric_nv == 6) return ftmpc::ftmpc_solve_ric64_kernel<6, false, true>;
    if (h->tset_ric) return ftmpc::ftmpc_solve_ric64_kernel<10, false, true>;
    if (h->sbounds && h->ric_nv == 6) return ftmpc::ftmpc_solve_ric64_kernel<6, true>;
    if (h->sbounds) return ftmpc::ftmpc_solve_ric64_kernel<10, true>;
    if (h->ric_nv == 4) return ftmpc::ftmpc_solve_ric64_kernel<4>;
    if (h->ric_nv == 6) return ftmpc::ftmpc_solve_ric64_kernel<6>;
    return ftmpc::ftmpc_solve_ric64_kernel<10>;
}
// the dense float64 kernel; wrench: the generalized-force formulation (6 N variables, hull rows) instead of the thruster form
F64Kernel pick_f64(const ftmpc_handle* h, bool wrench) {
    if (wrench) return h->cfg.terminal_set ? ftmpc::ftmpc_solve_f64_kernel<4, 1, 3> : ftmpc::ftmpc_solve_f64_kernel<4, 1, 1>;
    if (h->tset && !h->tset_ric) return ftmpc::ftmpc_solve_f64_kernel<4, 1, 2>;      // (tset_ric: the dense kernel only dumps the box QP)
    if (h->npad_max <= 256) return ftmpc::ftmpc_solve_f64_kernel<4, 1>;
    if (h->npad_max <= 640) return ftmpc::ftmpc_solve_f64_kernel<ftmpc::f64k::RPF, 3>;
    return ftmpc::ftmpc_solve_f64_kernel<ftmpc::f64k::RPF, ftmpc::f64k::NVT_MAX>;
}
HullKernel pick_hull32(const ftmpc_handle* h, int32_t /*hull_rows*/) {
    return h->cfg.terminal_set ? ftmpc::ftmpc_solve_hull32_kernel<6, true> : ftmpc::ftmpc_solve_hull32_kernel<6, false>;
}
RicwKernel pick_ricw64(const ftmpc_handle* h, int32_t /*hull_rows*/) {
    if (h->sbounds && h->cfg.N <= 24) return ftmpc::ftmpc_solve_ricw64_kernel<6, false, true>;
    if (h->sbounds) return ftmpc::ftmpc_solve_ricw64_kernel<10, false, true>;
    if (h->cfg.terminal_set && h->cfg.N <= 24) return ftmpc::ftmpc_solve_ricw64_kernel<6, true>;
    if (h->cfg.terminal_set) return ftmpc::ftmpc_solve_ricw64_kernel<10, true>;
    if (h->cfg.N <= 24) return ftmpc::ftmpc_solve_ricw64_kernel<6>;
    return ftmpc::ftmpc_solve_ricw64_kernel<10>;
}

// resident workgroups of `block` threads per CU (0 when the query fails: every caller clamps)
template <typename K>
int blocks_per_cu(K kernel, int block) {
    int per = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, block, 0);
    return per;
}

// One launch inside the event pair of kernel slot k (ftmpc_last_kernel_ms: events 2k and 2k + 1, ev_used[k]) when profiling is on.
template <typename L>
int profiled(ftmpc_handle* h, int k, hipStream_t s, L&& launch) {
    if (h->profiling) HIP_TRY(h, hipEventRecord(h->ev[2 * k], s));
    launch();
    HIP_TRY(h, hipGetLastError());
    if (h->profiling) {
        HIP_TRY(h, hipEventRecord(h->ev[2 * k + 1], s));
        h->ev_used[k] = true;
    }
    return FTMPC_OK;
}

// ---- argument-block fields that several kernels take alike
template <typename P>
void fill_term(const ftmpc_handle* h, P& q) {      // the rows of the terminal set (term_upload)
    q.termA = h->cfg.terminal_set ? h->d_term.p : nullptr;
    q.termb = h->cfg.terminal_set ? h->d_term + (int64_t)h->cfg.term_rows * 9 : nullptr;
    q.term_rows = h->cfg.terminal_set ? h->cfg.term_rows : 0;
}

template <typename P>
void fill_state_bounds(const ftmpc_handle* h, P& q) {
    for (int i = 0; i < FTMPC_NX; ++i) {
        q.xlb[i] = h->cfg.xlb[i];
        q.xub[i] = h->cfg.xub[i];
    }
    q.cbar = h->sbounds ? h->d_cbar.p : nullptr;
}

// a zeroed block of the generalized-force formulation (kernels 11 and 13, the dense float64 kernel's wrench mode): batch, hull
// rows, terminal set and outputs
template <typename P>
void fill_wrench(const ftmpc_handle* h, P& q, int64_t B, int32_t hull_rows, bool has_set, const double* d_warmG) {
    std::memset(&q, 0, sizeof(q));
    q.base.B = B;
    q.base.rec = h->rec;
    q.base.ub = h->d_ub; q.base.stuck = h->d_stuck;
    q.base.status = h->d_status; q.base.iters = h->d_iters;
    q.base.dbg_inst = -1;
    q.warmG = d_warmG;
    q.hullA = h->d_hullA;
    q.hull_set = has_set ? h->d_hullset.p : nullptr;
    q.hullb = h->d_hullb;
    q.hull_rows = hull_rows;
    q.out_tau0 = h->d_tau0;
    q.out_G = h->d_G;
    fill_term(h, q);
    q.eN = h->d_eN;
}

int tiles_of(int nb) { return nb * (nb + 1) / 2; }
// per-workgroup slots of the dense float64 kernel (thruster form)
int dense_ensure(ftmpc_handle* h) {
    int rc;
    if ((rc = h->Hs.ensure(h, h->grid64 * h->tile_doubles)) != FTMPC_OK || (rc = h->Ls.ensure(h, h->grid64 * h->tile_doubles)) != FTMPC_OK) return rc;
    return h->Eall.ensure(h, h->grid64 * h->e_doubles);
}
// per-workgroup global slot of the fp32 kernels (layout: ftmpc_common.h): sweep scratch, then the Hessian tiles
// Linearisation: full records per wave for large batches; below `lin_split_max` instances the direction-split grid
// (13 blocks per 64 instances, ftmpc_linearize.hip), which fills the device from a few hundred instances on.
void launch_linearize(ftmpc_handle* h, int64_t B, int blocks, hipStream_t s, const ftmpc::LinParams& lp) {
    // shares of the 13 directions per 64 instances: as many as keep about one wave per SIMD (1024 on the device)
    const int shares = B <= h->lin_split_max ? 13 : (B <= 2 * h->lin_split_max ? 4 : (B <= 5 * h->lin_split_max ? 2 : 1));
    if (lp.dist) {     // the same grids with the estimated disturbance in the rollout
        if (shares == 13)
            hipLaunchKernelGGL((ftmpc::ftmpc_linearize_kernel<double, 1, 1>), dim3(blocks, 13), dim3(64), 0, s, h->dc, lp);
        else if (shares > 1)
            hipLaunchKernelGGL((ftmpc::ftmpc_linearize_kernel<double, 2, 1>), dim3(blocks, shares), dim3(64), 0, s, h->dc, lp);
        else
            hipLaunchKernelGGL((ftmpc::ftmpc_linearize_kernel<double, 0, 1>), dim3(blocks), dim3(64), 0, s, h->dc, lp);
        return;
    }
    if (shares == 13)
        hipLaunchKernelGGL((ftmpc::ftmpc_linearize_kernel<double, 1>), dim3(blocks, 13), dim3(64), 0, s, h->dc, lp);
    else if (shares > 1)
        hipLaunchKernelGGL((ftmpc::ftmpc_linearize_kernel<double, 2>), dim3(blocks, shares), dim3(64), 0, s, h->dc, lp);
    else
        hipLaunchKernelGGL((ftmpc::ftmpc_linearize_kernel<double, 0>), dim3(blocks), dim3(64), 0, s, h->dc, lp);
}

int64_t slot_words(int nb, int N) { return ftmpc::slot_tile_off_words(N) + (int64_t)tiles_of(nb) * 256; }

int enqueue(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
            const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride,
            const double* warmU, double* out_u0, double* out_U, int32_t* status, int32_t* iters,
            hipStream_t s, int64_t dbg_inst) {
    if (h->tset && !h->tset_thruster)
        return fail(h, FTMPC_ERR_ARG, "the thruster form with the terminal set needs N <= 40 (the Riccati kernel), and N * NT <= 256 with kernel_select = FTMPC_KERNEL_DENSE "
                                      "(ftmpc_solve_wrench_batch, the reference's two-stage form, also serves N > 40)");
    if (B <= 0) return FTMPC_OK;
    LinParams lp;
    lp.B = B;
    lp.x0 = x0; lp.ub = ub; lp.stuck = stuck;
    lp.xref = xref; lp.xref_stride = xref_stride;
    lp.uref = uref; lp.uref_stride = uref_stride;
    lp.warmU = warmU;
    lp.rec = h->rec;
    lp.warmG = nullptr;
    lp.out_eN = h->tset ? h->d_eN : nullptr;
    lp.tcost = h->d_tcost;
    lp.out_cbar = h->sbounds ? h->d_cbar : nullptr;
    lp.dist = h->lin_dist;
    const int nvar = h->use_f64 ? 0 : (h->nb_max <= 8 ? 1 : (h->nb_max == 9 ? 2 : 3));   // one-wave fp32 instantiations in use
    lp.qlist = h->use_f64 ? nullptr : h->d_qlist;
    lp.qcount = h->d_qctl;
    lp.qvmax = h->use_wg ? 3 : nvar - 1;   // list 3: ceil(n/16) >= 11, the workgroup kernel
    if (!h->use_f64) HIP_TRY(h, hipMemsetAsync(h->d_qctl, 0, 8 * sizeof(int32_t), s));
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
    if (h->qcnt_pending && !capturing) {
        if (hipEventQuery(h->ev_qcnt) == hipSuccess) {
            for (int v = 0; v < 4; ++v) h->last_cnt[v] = h->h_qcnt[v];
            h->qcnt_pending = false;
            h->qcnt_valid = true;
        } else {
            (void)hipGetLastError();      // (not ready yet is not an error)
        }
    }
    auto grid_for = [&](int v, int64_t full) -> int {   // list v: the full persistent grid, or a small one when the list was empty last step
        const int64_t g = std::min<int64_t>(B, full);
        return (int)((h->qcnt_valid && !capturing && h->last_cnt[v] == 0) ? std::min<int64_t>(g, h->num_cu) : g);     // (one workgroup per CU)
    };
    const int lin_blocks = (int)((B + 63) / 64);
    for (bool& u : h->ev_used) u = false;
    int rc = profiled(h, 0, s, [&] { launch_linearize(h, B, lin_blocks, s, lp); });
    if (rc != FTMPC_OK) return rc;
    SolveParams sp;
    sp.B = B;
    sp.rec = h->rec;
    sp.ub = ub; sp.stuck = stuck; sp.warmU = warmU;
    sp.out_u0 = out_u0; sp.out_U = out_U; sp.status = status; sp.iters = iters;
    sp.dbg_inst = dbg_inst;
    sp.dbg_H = h->d_dbgH;
    sp.dbg_vec = h->d_dbgv;
    if (h->use_f64) {      // one float64 kernel takes the whole batch: no work lists
        sp.hscratch = nullptr;
        sp.tile_words = 0;
        sp.qlist = nullptr;
        sp.qcount = nullptr;
        sp.qhead = nullptr;
        if (h->use_ric64) {
            ftmpc::SolveRicParams w;
            HIP_TRY(h, hipMemsetAsync(h->d_qctl + 4, 0, sizeof(int32_t), s));
            sp.qhead = h->d_qctl + 4;       // shared instance cursor
            sp.dbg_H = reinterpret_cast<float*>(h->d_dbgH64.p);     // (diagnostic build: phase stamps)
            w.base = sp;
            w.slot = h->ric_slot;
            w.slot_doubles = h->ric_slot_doubles;
            fill_state_bounds(h, w);
            fill_term(h, w);
            w.eN = h->d_eN;
            // with state bounds the iteration stops at mu 1e-10 unless the caller asked otherwise, as the other general-constraint
            // modes do: the barrier weight of an active state row enters the Riccati recursion's state weight (see the kernel)
            DeviceConsts dcr = h->dc;
            if (h->sbounds && !(h->cfg.mu_stop > 0)) dcr.mu_stop = 1e-10;      // (terminal set: build_consts has done the same)
            const int grid = (int)std::min<int64_t>(B, h->grid_ric);
            rc = profiled(h, 6, s, [&] { hipLaunchKernelGGL(pick_ric64(h), dim3(grid), dim3(64), 0, s, dcr, w); });
        } else if (h->use_ws64) {
            SolveWs64Params w;
            sp.dbg_H = reinterpret_cast<float*>(h->d_dbgH64.p);     // (diagnostic build: phase stamps)
            w.base = sp;
            w.slot = h->ws64_slot;
            w.slot_doubles = h->ws64_slot_doubles;
            const int grid = (int)std::min<int64_t>(B, h->grid_ws64);
            rc = profiled(h, 6, s, [&] { hipLaunchKernelGGL(pick_ws64(h), dim3(grid), dim3(ftmpc::ws64k::WG), 0, s, h->dc, w); });
        } else {
            Solve64Params q;
            q.base = sp;
            q.Hs = h->Hs; q.Ls = h->Ls; q.Eall = h->Eall;
            q.tile_doubles = h->tile_doubles;
            q.e_doubles = h->e_doubles;
            q.npad_max = h->npad_max;
            q.nb_lo = 0;
            q.dbg_H = h->d_dbgH64;
            q.dbg_vec = h->d_dbgv64;
            q.warmG = nullptr; q.hullA = nullptr; q.hull_set = nullptr; q.hullb = nullptr; q.out_tau0 = nullptr; q.out_G = nullptr;
            q.hull_rows = 0;
            fill_term(h, q);
            q.eN = h->d_eN;
            const int grid = (int)std::min<int64_t>(B, h->grid64);
            rc = profiled(h, 4, s, [&] { hipLaunchKernelGGL(pick_f64(h, false), dim3(grid), dim3(ftmpc::f64k::WG), 0, s, h->dc, q); });
        }
        if (rc == FTMPC_OK && h->profiling) h->ev_valid = true;
        return rc;
    }
    // fp32 instantiations NB = 8, 9, 10: each pulls the instances with ceil(n/16) <= NB (the first also the empty
    // ones, the last also shapes beyond every instantiation, which it reports) from the list the linearise kernel
    // wrote for it; a launch whose list is empty returns at once
    auto on_list = [&](int v) {
        sp.qlist = h->d_qlist + (int64_t)v * B;
        sp.qcount = h->d_qctl + v;
        sp.qhead = h->d_qctl + 4 + v;
    };
    for (int v = 0; v < nvar; ++v) {
        sp.hscratch = h->hs[v];
        sp.tile_words = slot_words(8 + v, h->dc.N);
        on_list(v);
        const int grid = grid_for(v, h->grid[v]);
        rc = profiled(h, 1 + v, s, [&] { hipLaunchKernelGGL(pick_f32(v), dim3(grid), dim3(64), 0, s, h->dc, sp); });
        if (rc != FTMPC_OK) return rc;
    }
    if (h->use_wg) {      // work list 3 (ceil(n / 16) >= 11): kernel 10, kernel 8 or the workgroup kernel with the factor in LDS
        on_list(3);
        if (h->use_wsw) {
            sp.hscratch = h->wsw_slot;
            sp.tile_words = h->wsw_slot_words;
            const int grid = grid_for(3, h->grid_wsw);
            rc = profiled(h, 5, s, [&] { hipLaunchKernelGGL(pick_wsw32(h), dim3(grid), dim3(64), 0, s, h->dc, sp); });
        } else {
            SolveWgParams w;
            sp.hscratch = nullptr;
            sp.tile_words = 0;
            w.base = sp;
            w.slot = h->use_ws ? h->ws_slot.p : h->wg_slot.p;
            w.slot_words = h->use_ws ? h->ws_slot_words : h->wg_slot_words;
            const int grid = grid_for(3, h->use_ws ? h->grid_ws : h->grid_wg);
            rc = profiled(h, 5, s, [&] {
                if (h->use_ws) hipLaunchKernelGGL(pick_ws32(h), dim3(grid), dim3(ftmpc::wsk::WG), 0, s, h->dc, w);
                else hipLaunchKernelGGL(ftmpc::ftmpc_solve_wg32_kernel<15>, dim3(grid), dim3(ftmpc::wgk::WG), 0, s, h->dc, w);
            });
        }
        if (rc != FTMPC_OK) return rc;
    }
    if (h->profiling) h->ev_valid = true;
    if (h->h_qcnt && !capturing && !h->qcnt_pending) {     // this step's list lengths, for the next one
        HIP_TRY(h, hipMemcpyAsync(h->h_qcnt, h->d_qctl, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipEventRecord(h->ev_qcnt, s));
        h->qcnt_pending = true;
    }
    return FTMPC_OK;
}

}  // namespace

extern "C" {

int32_t ftmpc_version(void) { return 540; }

#ifndef FTMPC_BUILD_ID
#define FTMPC_BUILD_ID "unknown"
#endif
const char* ftmpc_build_id(void) { return FTMPC_BUILD_ID; }

int ftmpc_default_config(ftmpc_config* cfg, int32_t N, int32_t NT) {
    if (!cfg || N < 1 || N > 64 || NT < 1 || NT > FTMPC_MAX_NT) return FTMPC_ERR_ARG;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (int32_t)sizeof(ftmpc_config);
    cfg->N = N;
    cfg->NT = NT;
    cfg->dtype = FTMPC_DTYPE_F32;
    cfg->max_iters = 30;
    cfg->device_id = 0;
    cfg->dt = 0.1;                                   // reactive.yaml:2
    cfg->mass = 16.8;                                // sys_model.py:52
    cfg->J[0] = 0.2; cfg->J[4] = 0.3; cfg->J[8] = 0.25;  // sys_model.py:53-57
    const double Q[9] = {1, 1, 1, 1, 1, 1, 2, 2, 2};       // reactive.yaml:32
    const double R[6] = {0.1, 0.1, 0.1, 0.01, 0.01, 0.01}; // reactive.yaml:33
    std::memcpy(cfg->Q, Q, sizeof(Q));
    std::memcpy(cfg->R, R, sizeof(R));
    // quadratic part of config/terminal.yaml
    const double pp = 19.574136382485836, pv = 28.1433488118291, vv = 98.382994426126402;
    const double po[3] = {645.23036107820451, 645.43124119008723, 645.70261416462426};
    for (int a = 0; a < 3; ++a) {
        cfg->P[9 * a + a] = pp;
        cfg->P[9 * a + 3 + a] = pv;
        cfg->P[9 * (3 + a) + a] = pv;
        cfg->P[9 * (3 + a) + 3 + a] = vv;
        cfg->P[9 * (6 + a) + 6 + a] = po[a];
    }
    // spiral_parameters.py:33-39: omega_des = [0,0,.6], f_virt = 3.5 y, r = |f_virt|/(m |omega_des|^2) y
    cfg->f_virt[1] = 3.5;
    cfg->r[1] = 3.5 / (cfg->mass * 0.6 * 0.6);
    cfg->rho = 0.05;
    cfg->mu_stop = 0.0;  /* library default by dtype */
    for (int i = 0; i < FTMPC_NX; ++i) {      // no state bounds (the reference's default: params "xub" / "xlb" are None)
        cfg->xlb[i] = -FTMPC_NO_BOUND;
        cfg->xub[i] = FTMPC_NO_BOUND;
    }
    if (NT == 16) {
        // sys_model.py:73-123 restated from the thruster geometry
        const double d1 = 0.12, d2 = 0.09, d3 = 0.05;
        const double fx[8] = {-1, -1, 1, 1, -1, -1, 1, 1};
        const double ty[8] = {-1, 1, 1, -1, -1, 1, 1, -1};
        const double tz[8] = {1, 1, -1, -1, -1, -1, 1, 1};
        for (int i = 0; i < 8; ++i) {
            cfg->D[0 * 16 + i] = fx[i];
            cfg->D[4 * 16 + i] = d3 * ty[i];
            cfg->D[5 * 16 + i] = d1 * tz[i];
        }
        const double fy[4] = {-1, -1, 1, 1}, tzy[4] = {-1, 1, 1, -1};
        const double fz[4] = {-1, 1, -1, 1}, txz[4] = {-1, 1, 1, -1};
        for (int i = 0; i < 4; ++i) {
            cfg->D[1 * 16 + 8 + i] = fy[i];
            cfg->D[5 * 16 + 8 + i] = d2 * tzy[i];
            cfg->D[2 * 16 + 12 + i] = fz[i];
            cfg->D[3 * 16 + 12 + i] = d1 * txz[i];
        }
    }
    return FTMPC_OK;
}

int ftmpc_create(const ftmpc_config* cfg, ftmpc_handle** out) {
    if (!cfg || !out) return fail(nullptr, FTMPC_ERR_ARG, "null argument");
    *out = nullptr;
    // ABI guard first: nothing beyond the first 24 bytes of *cfg is read before the caller's struct is known to be ours
    if (cfg->struct_size != (int32_t)sizeof(ftmpc_config))
        return fail(nullptr, FTMPC_ERR_ARG, "ftmpc_config.struct_size is " + std::to_string(cfg->struct_size) + ", this library expects " +
                                                std::to_string(sizeof(ftmpc_config)) + " (caller built against another include/ftmpc.h? use ftmpc_default_config)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, FTMPC_ERR_NODEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(nullptr, FTMPC_ERR_ARG, "device_id out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device_id) != hipSuccess)
        return fail(nullptr, FTMPC_ERR_HIP, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, FTMPC_ERR_NODEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    if (cfg->dtype != FTMPC_DTYPE_F32 && cfg->dtype != FTMPC_DTYPE_F64)
        return fail(nullptr, FTMPC_ERR_ARG, "dtype must be FTMPC_DTYPE_F32 or FTMPC_DTYPE_F64");
    if (cfg->kernel_select != FTMPC_KERNEL_AUTO && cfg->kernel_select != FTMPC_KERNEL_DENSE && cfg->kernel_select != FTMPC_KERNEL_WORKGROUP &&
        cfg->kernel_select != FTMPC_KERNEL_RICCATI)
        return fail(nullptr, FTMPC_ERR_ARG, "kernel_select must be FTMPC_KERNEL_AUTO, FTMPC_KERNEL_DENSE, FTMPC_KERNEL_WORKGROUP or FTMPC_KERNEL_RICCATI");
    if (cfg->stage_chunks < 0 || cfg->stage_chunks > ftmpc_handle::MAX_CHUNKS)
        return fail(nullptr, FTMPC_ERR_ARG, "stage_chunks out of range 0..8");
    ftmpc_handle* h = new (std::nothrow) ftmpc_handle();
    if (!h) return fail(nullptr, FTMPC_ERR_ALLOC, "out of host memory");
    h->cfg = *cfg;
    // FTMPC_KERNEL_RICCATI: the Riccati kernel where the terminal-set thruster form would take the dense one (N <= 40); routed as AUTO
    // everywhere else (every other test of kernel_select asks "is it DENSE" or "is it WORKGROUP")
    const bool ask_ric = cfg->kernel_select == FTMPC_KERNEL_RICCATI;
    const bool sel_auto = cfg->kernel_select == FTMPC_KERNEL_AUTO || ask_ric;
    std::string why;
    int rc = build_consts(*cfg, h->dc, why);
    if (rc != FTMPC_OK) {
        delete h;
        return fail(nullptr, rc, why);
    }
    h->nb_max = (cfg->N * cfg->NT + 15) / 16;
    if (cfg->N * cfg->NT > ftmpc::f64k::NMAX) {
        delete h;
        return fail(nullptr, FTMPC_ERR_ARG, "N*NT > 1024 is not supported");
    }
    // fp32 LDS-resident kernels cover n <= 160; larger problems and dtype F64 use the float64
    // workgroup-per-instance kernel
    // fp32: one-wave register-resident kernels up to n = 160, the workgroup kernel with the factor in LDS up to n = 240;
    // beyond that, and for dtype F64, the float64 workgroup kernel with its tiles in a global slot
    // kernel 8 (the thruster QP through wrench space) takes the workgroup kernel's list -- ceil(n / 16) >= 11 -- when the
    // wrench-space system fits eight tiles a side (N <= 21) and the thruster variables fit its threads (one per thread up
    // to N = 16, two beyond); kernel_select = FTMPC_KERNEL_DENSE: kernel 7 (n <= 240) or the float64 kernel instead.
    // The one-wave kernels keep n <= 160: a workgroup per instance does not compete with a wave per instance there.
    h->ws_nb = (6 * cfg->N <= 96) ? 6 : 8;
    // the terminal set: the thruster-space solve with those rows exists in float64 only, so an fp32 handle that asks for it
    // solves THAT form on the float64 kernel; its two-stage form (ftmpc_solve_wrench_batch) still runs on kernel 11
    const bool solve_f64 = cfg->dtype == FTMPC_DTYPE_F64 || cfg->terminal_set != 0 || cfg->state_bounds != 0;
    h->use_ws = !solve_f64 && cfg->kernel_select != FTMPC_KERNEL_DENSE && h->nb_max > 10 && 6 * cfg->N <= 128 &&
                cfg->N * cfg->NT <= ftmpc::wsk::WG * ftmpc::wsk::nvt_of(h->ws_nb);
    // ... on one wave per instance (kernel 10) when the thruster variables fit four (N <= 16) / six (N <= 21) per lane;
    // kernel_select = FTMPC_KERNEL_WORKGROUP keeps the workgroup-per-instance kernel 8
    h->use_wsw = h->use_ws && cfg->kernel_select != FTMPC_KERNEL_WORKGROUP && cfg->N * cfg->NT <= 64 * ftmpc::wswk::nvt_of(h->ws_nb);
    h->use_f64 = solve_f64 || (h->nb_max > 15 && !h->use_ws);
    h->use_wg = !h->use_f64 && h->nb_max > 10;
    // float64: through the wrench-space form where the thrusters outnumber the wrench components by enough to pay for the
    // assembly of K (ten or more thrusters), the wrench-space system fits sixteen tiles a side and three thruster variables
    // per thread cover N * NT; the terminal-set mode and kernel_select = FTMPC_KERNEL_DENSE keep the dense float64 kernel
    h->use_ws64 = h->use_f64 && cfg->terminal_set == 0 && cfg->kernel_select != FTMPC_KERNEL_DENSE && 6 * cfg->N <= ftmpc::ws64k::NPADW &&
                  cfg->N * cfg->NT <= 3 * ftmpc::ws64k::WG && cfg->NT >= 10;
    h->ws64_nvt = (cfg->N * cfg->NT <= ftmpc::ws64k::WG) ? 1 : 3;
    // float64 box QP (no terminal set): the Riccati recursion on one wave per instance (kernel 12) for every horizon up to 40;
    // kernel_select = FTMPC_KERNEL_WORKGROUP keeps kernel 9 (the wrench-space form), FTMPC_KERNEL_DENSE the dense float64 kernel
    h->sbounds = cfg->state_bounds != 0;
    if (h->sbounds && (cfg->terminal_set != 0 || cfg->N > 40)) {
        delete h;
        return fail(nullptr, FTMPC_ERR_ARG, "state_bounds needs N <= 40 and no terminal_set (the state-bound rows live on the Riccati kernel)");
    }
    if (h->sbounds)
        for (int i = 0; i < FTMPC_NX; ++i)
            if (!(cfg->xlb[i] < cfg->xub[i])) {
                delete h;
                return fail(nullptr, FTMPC_ERR_ARG, "state_bounds: xlb[i] < xub[i] is required for every component (use +-FTMPC_NO_BOUND for none)");
            }
    h->use_ric64 = h->use_f64 && cfg->terminal_set == 0 && (sel_auto || h->sbounds) && cfg->N <= 40;
    h->ric_nv = (cfg->N <= 16 && !h->sbounds) ? 4 : (cfg->N <= 24 ? 6 : 10);
    if (h->use_ric64) h->use_ws64 = false;
    h->tset = cfg->terminal_set != 0;
    if (h->tset) {
        if (cfg->term_rows < 1 || cfg->term_rows > FTMPC_MAX_TERM_ROWS) {
            delete h;
            return fail(nullptr, FTMPC_ERR_ARG, "term_rows out of range 1..80");
        }
        // the THRUSTER form with terminal rows: the dense float64 kernel's n <= 256 mode where it fits (and kernel_select does not ask for
        // the Riccati kernel), kernel 12's terminal-set instantiation beyond that up to N = 40; FTMPC_KERNEL_DENSE keeps the dense kernel
        // and its limit.  (The two-stage form -- ftmpc_solve_wrench_batch -- has no such limit: kernel 13.)
        const bool dense_fits = 16 * h->nb_max <= 256;
        h->tset_ric = cfg->N <= 40 && sel_auto && (ask_ric || !dense_fits);
        h->tset_thruster = dense_fits || h->tset_ric;
        if (h->tset_ric) {
            h->use_ric64 = true;
            h->ric_nv = cfg->N <= 16 ? 4 : (cfg->N <= 24 ? 6 : 10);
        }
    }
    h->npad_max = 16 * h->nb_max;
    h->device = cfg->device_id;
    h->num_cu = prop.multiProcessorCount;
    if (hipSetDevice(h->device) != hipSuccess) {
        delete h;
        return fail(nullptr, FTMPC_ERR_HIP, "hipSetDevice failed");
    }
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete h;
        return fail(nullptr, FTMPC_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    for (int i = 0; i < 2 * FTMPC_KERNEL_SLOTS; ++i) (void)hipEventCreate(&h->ev[i]);
    bool sbad = hipStreamCreateWithFlags(&h->s_in, hipStreamNonBlocking) != hipSuccess ||
                hipStreamCreateWithFlags(&h->s_out, hipStreamNonBlocking) != hipSuccess;
    for (int i = 0; i < ftmpc_handle::MAX_CHUNKS; ++i)
        sbad = sbad || hipEventCreateWithFlags(&h->ev_in[i], hipEventDisableTiming) != hipSuccess ||
               hipEventCreateWithFlags(&h->ev_k[i], hipEventDisableTiming) != hipSuccess ||
               hipEventCreateWithFlags(&h->ev_out[i], hipEventDisableTiming) != hipSuccess;
    if (hipHostMalloc(reinterpret_cast<void**>(&h->h_qcnt), 4 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_qcnt, hipEventDisableTiming) != hipSuccess) {
        if (h->h_qcnt) (void)hipHostFree(h->h_qcnt);
        h->h_qcnt = nullptr;      // (no hint: every launch takes its full grid)
        (void)hipGetLastError();
    }
    if (hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_alloc, hipEventDisableTiming) != hipSuccess) {
        if (h->stream2) (void)hipStreamDestroy(h->stream2);
        h->stream2 = nullptr;      // (no overlap: the two-stage step allocates after kernel 13, on the one stream)
        (void)hipGetLastError();
    }
    if (sbad || h->d_qctl.ensure(h, 8) != FTMPC_OK) {
        g_create_error = "stream / event / work-list allocation failed";
        ftmpc_destroy(h);
        return FTMPC_ERR_HIP;
    }
    if (cfg->lin_split_max != 0) h->lin_split_max = cfg->lin_split_max < 0 ? 0 : cfg->lin_split_max;
    if (cfg->stage_chunks >= 1 && cfg->stage_chunks <= ftmpc_handle::MAX_CHUNKS) h->stage_chunks = cfg->stage_chunks;
    // persistent grids: resident workgroups per CU from the occupancy query (LDS-bound)
    for (int v = 0; v < 3; ++v) h->grid[v] = h->num_cu * std::max(1, blocks_per_cu(pick_f32(v), 64));
    // (the general-constraint instantiations hold ~50 KiB of LDS and one workgroup per CU)
    const int per64 = (h->tset && !h->tset_ric) ? 1 : std::min(2, std::max(1, blocks_per_cu(pick_f64(h, false), ftmpc::f64k::WG)));
    h->grid64 = h->num_cu * per64;
    h->tile_doubles = (int64_t)tiles_of(h->nb_max) * 256;
    h->e_doubles = (int64_t)(cfg->N + 2) * 9 * h->npad_max;     // + raw terminal rows GN and the terminal-set panel
    bool bad = false;
    if (h->use_f64) {
        // (a terminal-set handle beyond the dense kernel's n <= 256 -- served by kernel 12 or not at all -- never solves on the dense
        // slots: ftmpc_debug_build_qp allocates them when it is first called)
        const bool dense_slots = !h->tset || 16 * h->nb_max <= 256;
        bad = (dense_slots && dense_ensure(h) != FTMPC_OK) ||
              h->d_dbgH64.ensure(h, (int64_t)h->npad_max * h->npad_max) != FTMPC_OK ||
              h->d_dbgv64.ensure(h, 3 * (int64_t)h->npad_max + 4) != FTMPC_OK;
        if (!bad && h->use_ric64) {
            h->grid_ric = h->num_cu * std::max(1, blocks_per_cu(pick_ric64(h), 64));
            h->ric_slot_doubles = h->tset_ric ? ftmpc::rick::slot_doubles_ts(cfg->N) : ftmpc::rick::slot_doubles(cfg->N);
            bad = h->ric_slot.ensure(h, (int64_t)h->grid_ric * h->ric_slot_doubles) != FTMPC_OK;
        }
        if (!bad && h->use_ws64) {
            h->grid_ws64 = h->num_cu * std::max(1, std::min(blocks_per_cu(pick_ws64(h), ftmpc::ws64k::WG), FTMPC_WS64_WPC));
            h->ws64_slot_doubles = ftmpc::ws64k::slot_doubles(cfg->N);
            bad = h->ws64_slot.ensure(h, (int64_t)h->grid_ws64 * h->ws64_slot_doubles) != FTMPC_OK;
        }
        if (!bad && h->tset) bad = term_upload(h) != FTMPC_OK;
    } else {
        bad = h->hs[0].ensure(h, (int64_t)h->grid[0] * slot_words(8, cfg->N)) != FTMPC_OK ||
              (h->nb_max > 8 && h->hs[1].ensure(h, (int64_t)h->grid[1] * slot_words(9, cfg->N)) != FTMPC_OK) ||
              (h->nb_max > 9 && h->hs[2].ensure(h, (int64_t)h->grid[2] * slot_words(10, cfg->N)) != FTMPC_OK) ||
              h->d_dbgH.ensure(h, 4096 * 24 + 256 * 256) != FTMPC_OK || h->d_dbgv.ensure(h, 3 * 256 + 4) != FTMPC_OK;
        if (!bad && h->use_ws) {
            h->grid_ws = h->num_cu * std::max(1, blocks_per_cu(pick_ws32(h), ftmpc::wsk::WG));
            h->ws_slot_words = ftmpc::wsk::slot_words(h->ws_nb, cfg->N);
            bad = h->ws_slot.ensure(h, (int64_t)h->grid_ws * h->ws_slot_words) != FTMPC_OK;
        }
        if (!bad && h->use_wsw) {
            h->grid_wsw = h->num_cu * std::max(1, blocks_per_cu(pick_wsw32(h), 64));
            h->wsw_slot_words = ftmpc::wswk::slot_words(h->ws_nb, cfg->N);
            bad = h->wsw_slot.ensure(h, (int64_t)h->grid_wsw * h->wsw_slot_words) != FTMPC_OK;
        }
        if (!bad && h->use_wg) {
            h->grid_wg = h->num_cu;      // ~150 KiB of LDS: one workgroup per CU
            h->wg_slot_words = ftmpc::wgk::slot_words(15, cfg->N);
            bad = h->wg_slot.ensure(h, (int64_t)h->grid_wg * h->wg_slot_words) != FTMPC_OK;
        }
    }
    if (!bad && cfg->terminal_cost_terms) {
        if (cfg->tc_npoly < 0 || cfg->tc_npoly > FTMPC_MAX_TCOST_TERMS || cfg->tc_nroot < 0 || cfg->tc_nroot > FTMPC_MAX_TCOST_TERMS) {
            ftmpc_destroy(h);
            return fail(nullptr, FTMPC_ERR_ARG, "tc_npoly / tc_nroot out of range 0..24");
        }
        TermCost t;
        std::memset(&t, 0, sizeof(t));
        t.npoly = cfg->tc_npoly;
        t.nroot = cfg->tc_nroot;
        std::memcpy(t.poly_coef, cfg->tc_poly_coef, sizeof(t.poly_coef));
        std::memcpy(t.root_coef, cfg->tc_root_coef, sizeof(t.root_coef));
        std::memcpy(t.root_eps, cfg->tc_root_eps, sizeof(t.root_eps));
        std::memcpy(t.root_pow, cfg->tc_root_pow, sizeof(t.root_pow));
        for (int i = 0; i < FTMPC_MAX_TCOST_TERMS * 9; ++i) {
            t.poly_exp[i] = cfg->tc_poly_exp[i];
            t.root_exp[i] = cfg->tc_root_exp[i];
            if (t.poly_exp[i] < 0 || t.poly_exp[i] > 16 || t.root_exp[i] < 0 || t.root_exp[i] > 16) bad = true;
        }
        t.cconst = cfg->tc_const;
        bad = bad || h->d_tcost.ensure(h, 1) != FTMPC_OK;
        bad = bad || hipMemcpy(h->d_tcost, &t, sizeof(TermCost), hipMemcpyHostToDevice) != hipSuccess;
        if (bad) h->err = "terminal-cost tables: bad exponent or allocation failure";
    }
    if (bad) {
        g_create_error = h->err;
        ftmpc_destroy(h);
        return FTMPC_ERR_ALLOC;
    }
    *out = h;
    return FTMPC_OK;
}

int ftmpc_destroy(ftmpc_handle* h) {
    if (!h) return FTMPC_OK;
    (void)hipSetDevice(h->device);
    if (h->sqp_exec) (void)hipGraphExecDestroy(h->sqp_exec);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_alloc) (void)hipEventDestroy(h->ev_alloc);
    if (h->stream2) (void)hipStreamDestroy(h->stream2);
    if (h->h_qcnt) (void)hipHostFree(h->h_qcnt);
    if (h->ev_qcnt) (void)hipEventDestroy(h->ev_qcnt);
    if (h->pin_in.p) (void)hipHostFree(h->pin_in.p);
    if (h->pin_out.p) (void)hipHostFree(h->pin_out.p);
    for (int i = 0; i < 2 * FTMPC_KERNEL_SLOTS; ++i)
        if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
    for (int i = 0; i < ftmpc_handle::MAX_CHUNKS; ++i) {
        if (h->ev_in[i]) (void)hipEventDestroy(h->ev_in[i]);
        if (h->ev_k[i]) (void)hipEventDestroy(h->ev_k[i]);
        if (h->ev_out[i]) (void)hipEventDestroy(h->ev_out[i]);
    }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->s_in) (void)hipStreamDestroy(h->s_in);
    if (h->s_out) (void)hipStreamDestroy(h->s_out);
    delete h;      // (the device buffers go with it)
    return FTMPC_OK;
}

const char* ftmpc_last_error(const ftmpc_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int ftmpc_reserve(ftmpc_handle* h, int64_t max_batch) {
    if (!h || max_batch < 0) return FTMPC_ERR_ARG;
    if (max_batch <= h->cap_batch) return FTMPC_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const int N = h->cfg.N, NT = h->cfg.NT;
    const int64_t B = max_batch;
    // each buffer is freed before it is re-allocated; until all of them exist again the handle holds NO batch capacity
    return ensure_group(h->cap_batch, B, [&] {
        int rc;
        if ((rc = h->rec.ensure(h, B * N * ftmpc::REC_STRIDE * 2)) != FTMPC_OK) return rc;   // float64 records
        if ((rc = h->d_x0.ensure(h, B * 13)) != FTMPC_OK) return rc;
        if ((rc = h->d_ub.ensure(h, B * NT)) != FTMPC_OK) return rc;
        if ((rc = h->d_stuck.ensure(h, B * NT)) != FTMPC_OK) return rc;
        if ((rc = h->d_warm.ensure(h, B * N * NT)) != FTMPC_OK) return rc;
        if ((rc = h->d_u0.ensure(h, B * NT)) != FTMPC_OK) return rc;
        if ((rc = h->d_U.ensure(h, B * N * NT)) != FTMPC_OK) return rc;
        if ((rc = h->d_status.ensure(h, B)) != FTMPC_OK) return rc;
        if ((rc = h->d_iters.ensure(h, B)) != FTMPC_OK) return rc;
        if (!h->use_f64 && (rc = h->d_qlist.ensure(h, 4 * B)) != FTMPC_OK) return rc;
        if ((rc = h->d_eN.ensure(h, B * 9)) != FTMPC_OK) return rc;
        if (h->sbounds && (rc = h->d_cbar.ensure(h, B * h->cfg.N * 13)) != FTMPC_OK) return rc;
        return rc;
    });
}

static int stage_refs(ftmpc_handle* h, int64_t B, const double* xref, int64_t xref_stride, const double* uref,
                      int64_t uref_stride) {
    const int N = h->cfg.N;
    const int64_t nx = xref_stride == 0 ? 9 * (N + 1) : B * xref_stride;
    int rc = h->d_xref.ensure(h, nx);
    if (rc != FTMPC_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->d_xref, xref, nx * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (uref) {
        const int64_t nu = uref_stride == 0 ? 6 * (N + 1) : B * uref_stride;
        if ((rc = h->d_uref.ensure(h, nu)) != FTMPC_OK) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->d_uref, uref, nu * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    return FTMPC_OK;
}

static int check_strides(ftmpc_handle* h, int64_t xref_stride, int64_t uref_stride, const double* uref) {
    const int N = h->cfg.N;
    if (xref_stride != 0 && xref_stride < 9 * (N + 1)) return fail(h, FTMPC_ERR_ARG, "xref_stride must be 0 or >= 9*(N+1)");
    if (uref && uref_stride != 0 && uref_stride < 6 * (N + 1)) return fail(h, FTMPC_ERR_ARG, "uref_stride must be 0 or >= 6*(N+1)");
    return FTMPC_OK;
}

// the state, bounds and stuck thrusts of a batch into the handle's mirrors (ftmpc_reserve'd by the caller), on the handle's stream
static int stage_inputs(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck) {
    const int NT = h->cfg.NT;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->d_x0, x0, B * 13 * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->d_ub, ub, B * NT * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->d_stuck, stuck, B * NT * sizeof(double), hipMemcpyHostToDevice, s));
    return FTMPC_OK;
}

static int pin_grow(ftmpc_handle* h, ftmpc_handle::Pinned& P, size_t bytes) {
    if (bytes <= P.bytes) return FTMPC_OK;
    if (P.p) (void)hipHostFree(P.p);
    P.p = nullptr;
    P.bytes = 0;
    const size_t want = bytes + bytes / 8;
    hipError_t e = hipHostMalloc(&P.p, want, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, FTMPC_ERR_ALLOC, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    }
    P.bytes = want;
    return FTMPC_OK;
}

// Host-buffer entry: the caller's (pageable) arrays go through PINNED staging buffers in up to `stage_chunks`
// contiguous instance ranges, each on its way independently: host copy -> H2D on the input stream -> kernels on
// the compute stream -> D2H on the output stream -> host copy, so that the copies of one range run under the
// kernels of its neighbours (pinned staging, async H2D -> kernel -> D2H).
int ftmpc_solve_batch(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                      const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride,
                      double* warmU, double* out_u0, double* out_U, int32_t* status, int32_t* iters) {
    if (!h) return FTMPC_ERR_ARG;
    if (B < 0 || !x0 || !ub || !stuck || !xref || !out_u0) return fail(h, FTMPC_ERR_ARG, "null buffer or negative batch");
    if (B == 0) return FTMPC_OK;
    int rc = check_strides(h, xref_stride, uref_stride, uref);
    if (rc != FTMPC_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = ftmpc_reserve(h, B)) != FTMPC_OK) return rc;
    const int N = h->cfg.N, NT = h->cfg.NT;
    const int64_t nw = (int64_t)N * NT;
    const bool wantU = out_U != nullptr || warmU != nullptr;
    // reference windows on the device (shared: once; per instance: with the ranges below)
    const int64_t nxr = xref_stride == 0 ? 9 * (N + 1) : B * xref_stride;
    const int64_t nur = !uref ? 0 : (uref_stride == 0 ? 6 * (N + 1) : B * uref_stride);
    if ((rc = h->d_xref.ensure(h, nxr)) != FTMPC_OK || (rc = h->d_uref.ensure(h, nur)) != FTMPC_OK) return rc;
    // pinned mirrors: inputs [x0 | ub | stuck | warm | xref | uref], outputs [u0 | U | status | iters]
    const int64_t o_x0 = 0, o_ub = o_x0 + B * 13, o_st = o_ub + B * NT, o_wm = o_st + B * NT, o_xr = o_wm + (warmU ? B * nw : 0),
                  o_ur = o_xr + nxr, in_words = o_ur + nur;
    const int64_t p_u0 = 0, p_U = p_u0 + B * NT, out_words = p_U + (wantU ? B * nw : 0);
    if ((rc = pin_grow(h, h->pin_in, (size_t)in_words * 8)) != FTMPC_OK) return rc;
    if ((rc = pin_grow(h, h->pin_out, (size_t)out_words * 8 + (size_t)B * 8)) != FTMPC_OK) return rc;
    double* pin = static_cast<double*>(h->pin_in.p);
    double* pout = static_cast<double*>(h->pin_out.p);
    int32_t* pst = reinterpret_cast<int32_t*>(pout + out_words);
    int32_t* pit = pst + B;
    // Measured at B = 65 536 (scripts/host_entry_perf.py): one range 3.20 M QP/s, four ranges 2.74 M -- a range of 16 384
    // instances leaves the persistent grid with a ragged tail four times per call; so ranges are whole 65 536-blocks
    // unless ftmpc_config.stage_chunks says otherwise.
    int nch = h->stage_chunks > 0 ? (int)std::min<int64_t>(h->stage_chunks, (B + 16383) / 16384)
                                  : (int)std::min<int64_t>(ftmpc_handle::MAX_CHUNKS, (B + 65535) / 65536);
    if (nch < 1) nch = 1;
    int64_t edge[ftmpc_handle::MAX_CHUNKS + 1];
    for (int c = 0; c <= nch; ++c) edge[c] = (c == nch) ? B : ((B * c / nch) / 64) * 64;
    auto up = [&](double* dst_dev, int64_t poff, const double* src, int64_t off, int64_t cnt) -> hipError_t {
        std::memcpy(pin + poff + off, src + off, (size_t)cnt * 8);
        return hipMemcpyAsync(dst_dev + off, pin + poff + off, (size_t)cnt * 8, hipMemcpyHostToDevice, h->s_in);
    };
    for (int c = 0; c < nch; ++c) {
        const int64_t lo = edge[c], cnt = edge[c + 1] - edge[c];
        if (cnt <= 0) {
            HIP_TRY(h, hipEventRecord(h->ev_out[c], h->s_out));
            continue;
        }
        HIP_TRY(h, up(h->d_x0, o_x0, x0, lo * 13, cnt * 13));
        HIP_TRY(h, up(h->d_ub, o_ub, ub, lo * NT, cnt * NT));
        HIP_TRY(h, up(h->d_stuck, o_st, stuck, lo * NT, cnt * NT));
        if (warmU) HIP_TRY(h, up(h->d_warm, o_wm, warmU, lo * nw, cnt * nw));
        if (xref_stride != 0) HIP_TRY(h, up(h->d_xref, o_xr, xref, lo * xref_stride, cnt * xref_stride));
        else if (c == 0) HIP_TRY(h, up(h->d_xref, o_xr, xref, 0, nxr));
        if (uref && uref_stride != 0) HIP_TRY(h, up(h->d_uref, o_ur, uref, lo * uref_stride, cnt * uref_stride));
        else if (uref && c == 0) HIP_TRY(h, up(h->d_uref, o_ur, uref, 0, nur));
        HIP_TRY(h, hipEventRecord(h->ev_in[c], h->s_in));
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_in[c], 0));
        rc = enqueue(h, cnt, h->d_x0 + lo * 13, h->d_ub + lo * NT, h->d_stuck + lo * NT, h->d_xref + lo * xref_stride, xref_stride,
                     uref ? h->d_uref + lo * uref_stride : nullptr, uref_stride, warmU ? h->d_warm + lo * nw : nullptr,
                     h->d_u0 + lo * NT, wantU ? h->d_U + lo * nw : nullptr, h->d_status + lo, h->d_iters + lo, h->stream, -1);
        if (rc != FTMPC_OK) return rc;
        HIP_TRY(h, hipEventRecord(h->ev_k[c], h->stream));
        HIP_TRY(h, hipStreamWaitEvent(h->s_out, h->ev_k[c], 0));
        HIP_TRY(h, hipMemcpyAsync(pout + p_u0 + lo * NT, h->d_u0 + lo * NT, (size_t)cnt * NT * 8, hipMemcpyDeviceToHost, h->s_out));
        if (wantU) HIP_TRY(h, hipMemcpyAsync(pout + p_U + lo * nw, h->d_U + lo * nw, (size_t)cnt * nw * 8, hipMemcpyDeviceToHost, h->s_out));
        if (status) HIP_TRY(h, hipMemcpyAsync(pst + lo, h->d_status + lo, (size_t)cnt * 4, hipMemcpyDeviceToHost, h->s_out));
        if (iters) HIP_TRY(h, hipMemcpyAsync(pit + lo, h->d_iters + lo, (size_t)cnt * 4, hipMemcpyDeviceToHost, h->s_out));
        HIP_TRY(h, hipEventRecord(h->ev_out[c], h->s_out));
    }
    for (int c = 0; c < nch; ++c) {
        const int64_t lo = edge[c], cnt = edge[c + 1] - edge[c];
        HIP_TRY(h, hipEventSynchronize(h->ev_out[c]));
        if (cnt <= 0) continue;
        std::memcpy(out_u0 + lo * NT, pout + p_u0 + lo * NT, (size_t)cnt * NT * 8);
        if (out_U) std::memcpy(out_U + lo * nw, pout + p_U + lo * nw, (size_t)cnt * nw * 8);
        if (warmU) std::memcpy(warmU + lo * nw, pout + p_U + lo * nw, (size_t)cnt * nw * 8);
        if (status) std::memcpy(status + lo, pst + lo, (size_t)cnt * 4);
        if (iters) std::memcpy(iters + lo, pit + lo, (size_t)cnt * 4);
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FTMPC_OK;
}

int ftmpc_eval_cost_batch(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck, const double* xref,
                          int64_t xref_stride, const double* uref, int64_t uref_stride, const double* U, double* out_cost) {
    if (!h) return FTMPC_ERR_ARG;
    if (B < 0 || !x0 || !ub || !stuck || !xref || !U || !out_cost) return fail(h, FTMPC_ERR_ARG, "null buffer or negative batch");
    if (B == 0) return FTMPC_OK;
    int rc = check_strides(h, xref_stride, uref_stride, uref);
    if (rc != FTMPC_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = ftmpc_reserve(h, B)) != FTMPC_OK) return rc;
    if ((rc = h->d_cost.ensure(h, B)) != FTMPC_OK) return rc;
    const int N = h->cfg.N, NT = h->cfg.NT;
    hipStream_t s = h->stream;
    if ((rc = stage_inputs(h, B, x0, ub, stuck)) != FTMPC_OK) return rc;
    if ((rc = stage_refs(h, B, xref, xref_stride, uref, uref_stride)) != FTMPC_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->d_U, U, B * N * NT * sizeof(double), hipMemcpyHostToDevice, s));
    ftmpc::CostParams cp;
    cp.B = B;
    cp.x0 = h->d_x0; cp.ub = h->d_ub; cp.stuck = h->d_stuck;
    cp.xref = h->d_xref; cp.xref_stride = xref_stride;
    cp.uref = uref ? h->d_uref : nullptr; cp.uref_stride = uref_stride;
    cp.U = h->d_U;
    cp.tcost = h->d_tcost;
    cp.out = h->d_cost;
    hipLaunchKernelGGL(ftmpc::ftmpc_cost_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, h->dc, cp);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out_cost, h->d_cost, B * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return FTMPC_OK;
}

// The line-search SQP over DEVICE buffers (h->d_x0 / d_ub / d_stuck and the given reference windows), enqueued on h->stream:
// on return S describes where the results are (S.U the final sequences, S.J their cost, J0 the cost of the start point).
#ifndef FTMPC_SQP_LINESEARCH_AT_ONCE
#define FTMPC_SQP_LINESEARCH_AT_ONCE 1
#endif
// the launches of one SQP solve on the handle's stream (launch = false: a replay, only the state the caller reads back is formed)
static int sqp_record(ftmpc_handle* h, int64_t B, const double* d_xref, int64_t xref_stride, const double* d_uref, int64_t uref_stride,
                      const double* d_warm, int32_t sqp_iters, int32_t backtracks, double tol, ftmpc::SqpState& S, double** J0_out, bool launch) {
    const int N = h->cfg.N, NT = h->cfg.NT;
    const int64_t nw = (int64_t)N * NT;
    int rc;
    hipStream_t s = h->stream;
    double *J = h->d_sqJ, *Jt = h->d_sqJ + B, *J0 = h->d_sqJ + 2 * B, *alpha = h->d_sqJ + 3 * B;
    S.B = B; S.N = N; S.NT = NT;
    S.ub = h->d_ub;
    S.U = h->d_sqU; S.Uq = h->d_sqQ; S.Ut = h->d_sqT;
    S.J = J; S.Jt = Jt; S.alpha = alpha;
    S.active = h->d_sqF; S.todo = h->d_sqF + B; S.improved = h->d_sqF + 2 * B; S.nmajor = h->d_sqF + 3 * B; S.ipm = h->d_sqF + 4 * B;
    S.status = h->d_sqF + 5 * B;
    S.qstatus = h->d_status; S.qiters = h->d_iters;
    S.tol = tol;
    if (!launch) {      // the iterate's buffer after the swaps of the major iterations
        if (sqp_iters & 1) std::swap(S.U, S.Ut);
        *J0_out = J0;
        return FTMPC_OK;
    }
    const unsigned gE = (unsigned)((B * nw + 255) / 256), gB = (unsigned)((B + 255) / 256);
    ftmpc::CostParams cp;
    cp.B = B;
    cp.x0 = h->d_x0; cp.ub = h->d_ub; cp.stuck = h->d_stuck;
    cp.xref = d_xref; cp.xref_stride = xref_stride;
    cp.uref = d_uref; cp.uref_stride = uref_stride;
    cp.tcost = h->d_tcost;
    auto cost = [&](const double* U, double* out) {
        cp.U = U;
        cp.out = out;
        hipLaunchKernelGGL(ftmpc::ftmpc_cost_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, h->dc, cp);
    };
    hipLaunchKernelGGL(ftmpc::ftmpc_sqp_init_kernel, dim3(gE > gB ? gE : gB), dim3(256), 0, s, S, d_warm);
    cost(S.U, J);
    HIP_TRY(h, hipMemcpyAsync(J0, J, B * sizeof(double), hipMemcpyDeviceToDevice, s));
    for (int it = 0; it < sqp_iters; ++it) {
        // the QP linearised about the current iterate (every instance: a stopped one costs a solve but changes nothing)
        rc = enqueue(h, B, h->d_x0, h->d_ub, h->d_stuck, d_xref, xref_stride, d_uref, uref_stride, S.U, h->d_u0, h->d_sqQ, h->d_status,
                     h->d_iters, s, -1);
        if (rc != FTMPC_OK) return rc;
        hipLaunchKernelGGL(ftmpc::ftmpc_sqp_open_kernel, dim3(gB), dim3(256), 0, s, S);
        if (FTMPC_SQP_LINESEARCH_AT_ONCE) {
            // every trial point of the line search in one launch, the first acceptable one picked in a second (the alpha = 1,
            // 1/2, ... rounds of trial / cost / decide are 3 x backtracks dependent launches for the same result)
            ftmpc::CostParams ct = cp;
            ct.U = S.U;
            ct.Uq = S.Uq;
            ct.todo = S.todo;
            ct.ntrial = backtracks;
            ct.out = h->d_sqJall;
            hipLaunchKernelGGL(ftmpc::ftmpc_cost_kernel, dim3((unsigned)((B * backtracks + 63) / 64)), dim3(64), 0, s, h->dc, ct);
            S.Jall = h->d_sqJall;
            S.ntrial = backtracks;
            hipLaunchKernelGGL(ftmpc::ftmpc_sqp_pick_kernel, dim3(gB), dim3(256), 0, s, S);
        } else {
            for (int bt = 0; bt < backtracks; ++bt) {
                hipLaunchKernelGGL(ftmpc::ftmpc_sqp_trial_kernel, dim3(gE), dim3(256), 0, s, S);
                cost(S.Ut, Jt);
                hipLaunchKernelGGL(ftmpc::ftmpc_sqp_decide_kernel, dim3(gB), dim3(256), 0, s, S);
            }
        }
        hipLaunchKernelGGL(ftmpc::ftmpc_sqp_close_kernel, dim3(gE), dim3(256), 0, s, S);     // new iterate -> Ut
        hipLaunchKernelGGL(ftmpc::ftmpc_sqp_count_kernel, dim3(gB), dim3(256), 0, s, S);
        std::swap(S.U, S.Ut);
        HIP_TRY(h, hipGetLastError());
    }
    *J0_out = J0;
    return FTMPC_OK;
}

// One SQP solve on the handle's stream.  The sequence is sqp_iters x (linearise, QP kernels, open, backtracks x (trial, cost, decide),
// close, count): ~300 launches of mostly tiny kernels for ten major iterations, launch-bound on small batches.  A call that repeats
// the previous call's shape (batch, buffers, strides, counts, constants; no reallocation in between) is recorded into a hipGraph and
// every further one replays it with ONE launch (small batches; see FTMPC_SQP_GRAPH below).  Profiling or a failed capture leave the
// direct launches.  A closed loop with the shared reference moves its reference pointer every step: direct launches.  Under a mission
// with tables (simulate_core) the reference is the call's window buffer, the same pointer at every step, so such a loop replays its
// graph from the third step on.  The recorded graph then holds pointers to buffers of that CALL (windows, warm start), which are
// freed when it returns; it is replayed only on a key match, and the key holds those pointers, the batch and the strides: a later call
// matches only if its own live buffers sit at the same addresses, and their sizes follow from B and the config, so they are the same.
static int sqp_enqueue(ftmpc_handle* h, int64_t B, const double* d_xref, int64_t xref_stride, const double* d_uref, int64_t uref_stride,
                       const double* d_warm, int32_t sqp_iters, int32_t backtracks, double tol, ftmpc::SqpState& S, double** J0_out) {
    const int64_t nw = (int64_t)h->cfg.N * h->cfg.NT;
    int rc;
    rc = ensure_group(h->cap_sqp, B, [&] {
        int r;
        if ((r = h->d_sqU.ensure(h, B * nw)) != FTMPC_OK || (r = h->d_sqQ.ensure(h, B * nw)) != FTMPC_OK ||
            (r = h->d_sqT.ensure(h, B * nw)) != FTMPC_OK || (r = h->d_sqJ.ensure(h, 4 * B)) != FTMPC_OK)
            return r;
        return h->d_sqF.ensure(h, 6 * B);
    });
    if (rc != FTMPC_OK || (rc = h->d_sqJall.ensure(h, B * backtracks)) != FTMPC_OK) return rc;
    // FTMPC_SQP_GRAPH: 0 never, 1 always; unset: batches up to 512 (measured, ten major iterations: 7.0 -> 6.2 ms at B = 256; at
    // B = 1 024 the replay is SLOWER than the direct launches, 10.0 against 7.6 ms -- a captured step always launches the full
    // persistent grids, the direct path shrinks those whose work list was empty the step before)
    static const int graphs_mode = [] {
        const char* e = std::getenv("FTMPC_SQP_GRAPH");
        return !e ? 2 : (e[0] == '0' ? 0 : 1);
    }();
    const bool graphs_on = graphs_mode == 1 || (graphs_mode == 2 && B <= 512);
    hipStream_t s = h->stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool outer_capture = hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
    if (!graphs_on || h->profiling || outer_capture || sqp_iters == 0)
        return sqp_record(h, B, d_xref, xref_stride, d_uref, uref_stride, d_warm, sqp_iters, backtracks, tol, S, J0_out, true);
    ftmpc_handle::SqpKey key;
    key.B = B; key.xs = xref_stride; key.us = uref_stride;
    key.xref = d_xref; key.uref = d_uref; key.warm = d_warm;
    key.iters = sqp_iters; key.backtracks = backtracks; key.tol = tol;
    key.epoch = h->alloc_epoch;
    {   // the constants the kernels take by value, and the switches that pick kernels: FNV-1a over their bytes
        uint64_t f = 1469598103934665603ull;
        auto mix = [&](const void* p, size_t n) {
            const unsigned char* b = static_cast<const unsigned char*>(p);
            for (size_t i = 0; i < n; ++i) f = (f ^ b[i]) * 1099511628211ull;
        };
        mix(&h->dc, sizeof(h->dc));
        const void* ptrs[2] = {h->d_tcost, h->rec};
        mix(ptrs, sizeof(ptrs));
        const int sw[9] = {h->use_f64, h->use_wg, h->use_ric64, h->nb_max, h->tset, h->sbounds, h->cfg.kernel_select, (int)h->lin_split_max, h->tset_ric};
        mix(sw, sizeof(sw));
        key.consts = f;
    }
    if (h->sqp_exec && key == h->sqp_key) {
        if ((rc = sqp_record(h, B, d_xref, xref_stride, d_uref, uref_stride, d_warm, sqp_iters, backtracks, tol, S, J0_out, false)) != FTMPC_OK)
            return rc;
        HIP_TRY(h, hipGraphLaunch(h->sqp_exec, s));
        ++h->sqp_graph_launches;
        return FTMPC_OK;
    }
    if (h->sqp_exec) {
        (void)hipGraphExecDestroy(h->sqp_exec);
        h->sqp_exec = nullptr;
    }
    if (!(key == h->sqp_seen)) {      // first call of this shape: direct launches (it may still be a one-off)
        h->sqp_seen = key;
        return sqp_record(h, B, d_xref, xref_stride, d_uref, uref_stride, d_warm, sqp_iters, backtracks, tol, S, J0_out, true);
    }
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        return sqp_record(h, B, d_xref, xref_stride, d_uref, uref_stride, d_warm, sqp_iters, backtracks, tol, S, J0_out, true);
    }
    ftmpc::SqpState Sc;
    double* J0c = nullptr;
    rc = sqp_record(h, B, d_xref, xref_stride, d_uref, uref_stride, d_warm, sqp_iters, backtracks, tol, Sc, &J0c, true);
    hipGraph_t g = nullptr;
    const hipError_t ec = hipStreamEndCapture(s, &g);
    hipGraphExec_t ex = nullptr;
    if (rc == FTMPC_OK && ec == hipSuccess && g && hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess && ex) {
        (void)hipGraphDestroy(g);
        h->sqp_exec = ex;
        h->sqp_key = key;
        if ((rc = sqp_record(h, B, d_xref, xref_stride, d_uref, uref_stride, d_warm, sqp_iters, backtracks, tol, S, J0_out, false)) != FTMPC_OK)
            return rc;
        HIP_TRY(h, hipGraphLaunch(h->sqp_exec, s));
        ++h->sqp_graph_launches;
        return FTMPC_OK;
    }
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    h->sqp_seen = ftmpc_handle::SqpKey();      // (do not try again on every call)
    h->sqp_seen.B = -2;
    return sqp_record(h, B, d_xref, xref_stride, d_uref, uref_stride, d_warm, sqp_iters, backtracks, tol, S, J0_out, true);
}

int ftmpc_solve_sqp_batch(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck, const double* xref,
                          int64_t xref_stride, const double* uref, int64_t uref_stride, const double* warmU, int32_t sqp_iters,
                          int32_t backtracks, double tol, double* out_u0, double* out_U, double* out_cost, double* out_cost0,
                          int32_t* out_sqp_iters, int32_t* out_iters, int32_t* status) {
    if (!h) return FTMPC_ERR_ARG;
    if (B < 0 || !x0 || !ub || !stuck || !xref || !out_u0 || sqp_iters < 0 || backtracks < 1 || !(tol >= 0))
        return fail(h, FTMPC_ERR_ARG, "null buffer, negative batch or bad iteration counts");
    if (B == 0) return FTMPC_OK;
    int rc = check_strides(h, xref_stride, uref_stride, uref);
    if (rc != FTMPC_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = ftmpc_reserve(h, B)) != FTMPC_OK) return rc;
    const int N = h->cfg.N, NT = h->cfg.NT;
    const int64_t nw = (int64_t)N * NT;
    hipStream_t s = h->stream;
    if ((rc = stage_inputs(h, B, x0, ub, stuck)) != FTMPC_OK) return rc;
    if ((rc = stage_refs(h, B, xref, xref_stride, uref, uref_stride)) != FTMPC_OK) return rc;
    if (warmU) HIP_TRY(h, hipMemcpyAsync(h->d_warm, warmU, B * nw * sizeof(double), hipMemcpyHostToDevice, s));
    ftmpc::SqpState S;
    double* J0 = nullptr;
    if ((rc = sqp_enqueue(h, B, h->d_xref, xref_stride, uref ? h->d_uref : nullptr, uref_stride, warmU ? h->d_warm : nullptr, sqp_iters,
                          backtracks, tol, S, &J0)) != FTMPC_OK)
        return rc;
    // u0 = stage 0 of the final sequences
    HIP_TRY(h, hipMemcpy2DAsync(out_u0, NT * sizeof(double), S.U, nw * sizeof(double), NT * sizeof(double), (size_t)B, hipMemcpyDeviceToHost, s));
    if (out_U) HIP_TRY(h, hipMemcpyAsync(out_U, S.U, B * nw * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_cost) HIP_TRY(h, hipMemcpyAsync(out_cost, S.J, B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_cost0) HIP_TRY(h, hipMemcpyAsync(out_cost0, J0, B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_sqp_iters) HIP_TRY(h, hipMemcpyAsync(out_sqp_iters, S.nmajor, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (out_iters) HIP_TRY(h, hipMemcpyAsync(out_iters, S.ipm, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (status) HIP_TRY(h, hipMemcpyAsync(status, S.status, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return FTMPC_OK;
}

int64_t ftmpc_sqp_graph_launches(const ftmpc_handle* h) { return h ? h->sqp_graph_launches : -1; }

int ftmpc_solve_batch_device(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                             const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride,
                             const double* warmU, double* out_u0, double* out_U, int32_t* status, int32_t* iters,
                             void* stream) {
    if (!h) return FTMPC_ERR_ARG;
    if (B < 0 || !x0 || !ub || !stuck || !xref || !out_u0) return fail(h, FTMPC_ERR_ARG, "null buffer or negative batch");
    if (B == 0) return FTMPC_OK;
    int rc = check_strides(h, xref_stride, uref_stride, uref);
    if (rc != FTMPC_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    // growing the workspace allocates: callers that time or graph-capture must ftmpc_reserve first
    if ((rc = ftmpc_reserve(h, B)) != FTMPC_OK) return rc;
    return enqueue(h, B, x0, ub, stuck, xref, xref_stride, uref, uref_stride, warmU, out_u0, out_U, status, iters,
                   reinterpret_cast<hipStream_t>(stream), -1);
}

// The generalized-force formulation runs on kernel 11 (fp32, one wave per instance; hull rows, and the terminal set when the
// handle has one) when the handle computes in fp32 and the problem fits six tiles a side (N <= 16) and eight row slots per
// lane; the instances kernel 11 does not certify, and everything else (dtype FTMPC_DTYPE_F64, kernel_select =
// FTMPC_KERNEL_DENSE, longer horizons), on the float64 kernel.
static bool hull_fp32(const ftmpc_handle* h, int32_t hull_rows) {
    if (h->sbounds) return false;      // kernel 11 has no state rows: a state-bound handle runs the whole batch on kernel 13
    return h->cfg.dtype != FTMPC_DTYPE_F64 && h->cfg.kernel_select != FTMPC_KERNEL_DENSE && 6 * h->cfg.N <= 96 && hull_rows <= 32 &&
           (int64_t)h->cfg.N * 32 <= 64 * ftmpc::hullk::nvc_of(6) && (!h->cfg.terminal_set || h->cfg.term_rows <= 80);
}

// ... and on kernel 13 (float64, Riccati recursion, one wave per instance: any horizon up to 40, up to 128 hull rows, with or
// without the terminal set) unless kernel_select is FTMPC_KERNEL_DENSE: the whole batch where kernel 11 does not apply (float64
// handles, N > 16, more than 32 rows, a handle with state bounds: kernel 13's state-bound instantiation), and otherwise the
// instances kernel 11 hands over.  The dense float64 kernel keeps kernel_select = FTMPC_KERNEL_DENSE and N > 40 (no state bounds there).
static bool hull_ricw(const ftmpc_handle* h, int32_t hull_rows) {
    return h->cfg.kernel_select != FTMPC_KERNEL_DENSE && h->cfg.N <= 40 && hull_rows <= ftmpc::rickw::MHMAX &&
           (!h->cfg.terminal_set || h->cfg.term_rows <= 80);
}

// Validation, workspace and hull tables of the generalized-force formulation (shared by the one-step entry and the closed loop).
static int wrench_prepare(ftmpc_handle* h, int64_t B, const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                          int32_t hull_rows) {
    const int N = h->cfg.N;
    if (6 * N > 256) return fail(h, FTMPC_ERR_ARG, "the generalized-force formulation needs 6 N <= 256");
    if (hull_rows < 1 || hull_rows > FTMPC_MAX_HULL_ROWS || n_sets < 1) return fail(h, FTMPC_ERR_ARG, "hull_rows out of range (1..128) or no hull table");
    if (!hull_ricw(h, hull_rows) && (hull_rows > 32 || (int64_t)N * hull_rows > 1024))
        return fail(h, FTMPC_ERR_ARG, "with kernel_select = FTMPC_KERNEL_DENSE or N > 40 the generalized-force formulation needs hull_rows <= 32 and N * hull_rows <= 1024");
    if (h->cfg.terminal_set && (h->cfg.term_rows < 1 || h->cfg.term_rows > FTMPC_MAX_TERM_ROWS)) return fail(h, FTMPC_ERR_ARG, "term_rows out of range");
    if (h->sbounds && !hull_ricw(h, hull_rows))      // (ftmpc_create keeps state_bounds to N <= 40 without terminal_set)
        return fail(h, FTMPC_ERR_ARG, "state_bounds on the generalized-force formulation run on the Riccati kernel only (kernel_select must not be FTMPC_KERNEL_DENSE)");
    if (hull_set)   // the kernel indexes hull_A by these: a table number outside [0, n_sets) would be an out-of-bounds device read
        for (int64_t b = 0; b < B; ++b)
            if (hull_set[b] < 0 || hull_set[b] >= n_sets)
                return fail(h, FTMPC_ERR_ARG, "hull_set[" + std::to_string(b) + "] = " + std::to_string(hull_set[b]) + " is not a table number in [0, n_sets)");
    int rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = ftmpc_reserve(h, B)) != FTMPC_OK) return rc;
    if (hull_fp32(h, hull_rows) && !h->hull_slot) {     // kernel 11: one wave per instance, H_w tiles in LDS; only the float64 gradient scratch is global
        h->grid_hull = h->num_cu * std::max(1, blocks_per_cu(pick_hull32(h, hull_rows), 64));
        h->hull_slot_words = ftmpc::wswk::slot_words(6, N);
        if ((rc = h->hull_slot.ensure(h, (int64_t)h->grid_hull * h->hull_slot_words)) != FTMPC_OK) return rc;
    }
    if (hull_ricw(h, hull_rows)) {     // kernel 13's per-wave slots (sized by the row count)
        const int64_t need = ftmpc::rickw::slot_doubles(N, hull_rows, h->sbounds);
        if (!h->ricw_slot || need > h->ricw_slot_doubles) {
            h->grid_ricw = h->num_cu * std::max(1, blocks_per_cu(pick_ricw64(h, hull_rows), 64));
            if ((rc = h->ricw_slot.ensure(h, (int64_t)h->grid_ricw * need)) != FTMPC_OK) return rc;
            h->ricw_slot_doubles = need;
        }
    }
    if ((rc = term_upload(h)) != FTMPC_OK) return rc;
    // the dense float64 kernel's slots: kernel_select = FTMPC_KERNEL_DENSE, N > 40 -- the whole batch, or what kernel 11 hands over
    // (hull and terminal rows active together, a polish that did not settle: SolveHullParams::fb_list)
    if (!hull_ricw(h, hull_rows) && !h->gHs) {   // per-workgroup slots of the 6N-variable problem (separate from the thruster-space slots of this handle)
        const int nbg = (6 * N + 15) / 16;
        h->npad_gen = 16 * nbg;
        h->grid_gen = h->num_cu;
        h->tile_doubles_gen = (int64_t)tiles_of(nbg) * 256;
        h->e_doubles_gen = (int64_t)(N + 2) * 9 * h->npad_gen;
        if ((rc = h->gHs.ensure(h, h->grid_gen * h->tile_doubles_gen)) != FTMPC_OK || (rc = h->gLs.ensure(h, h->grid_gen * h->tile_doubles_gen)) != FTMPC_OK ||
            (rc = h->gEall.ensure(h, h->grid_gen * h->e_doubles_gen)) != FTMPC_OK)
            return rc;
    }
    const int64_t nA = (int64_t)n_sets * hull_rows * 6;
    if ((rc = h->d_hullA.ensure(h, nA)) != FTMPC_OK) return rc;
    rc = ensure_group(h->cap_wrench, B, [&] {
        int r;
        if ((r = h->d_hullb.ensure(h, B * FTMPC_MAX_HULL_ROWS)) != FTMPC_OK || (r = h->d_hullset.ensure(h, B)) != FTMPC_OK ||
            (r = h->d_warmG.ensure(h, B * N * 6)) != FTMPC_OK || (r = h->d_tau0.ensure(h, B * 6)) != FTMPC_OK ||
            (r = h->d_G.ensure(h, B * N * 6)) != FTMPC_OK || (r = h->d_taud.ensure(h, B * 6)) != FTMPC_OK)
            return r;
        return h->d_ast2.ensure(h, 3 * B);      // allocation status | iterations | kernel 11's hand-over list
    });
    if (rc != FTMPC_OK) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->d_hullA, hull_A, nA * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->d_hullb, hull_b, B * hull_rows * sizeof(double), hipMemcpyHostToDevice, s));
    if (hull_set) HIP_TRY(h, hipMemcpyAsync(h->d_hullset, hull_set, B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    return FTMPC_OK;
}

// The allocation half of a two-stage step on stream st: u0 in h->d_u0 = min-norm allocation of h->d_tau0 - D stuck, status /
// iterations in h->d_ast2; of every instance, or (list mode) of the *count instances in list.
static void wrench_allocate(ftmpc_handle* h, int64_t B, hipStream_t st, const int32_t* list, const int32_t* count) {
    hipLaunchKernelGGL(ftmpc::ftmpc_healthy_wrench_kernel, dim3((unsigned)((B * 6 + 255) / 256)), dim3(256), 0, st, h->dc, B,
                       (const double*)h->d_tau0, (const double*)h->d_stuck, h->d_taud.p, list, count);
    ftmpc::AllocParams a;
    a.B = B;
    a.tau = h->d_taud;
    a.ub = h->d_ub;
    a.out_u = h->d_u0;
    a.status = h->d_ast2;
    a.iters = h->d_ast2 + B;
    a.max_iters = 50;
    a.tol = 1e-8;
    a.list = list;
    a.count = count;
    hipLaunchKernelGGL(ftmpc::ftmpc_allocate_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, h->dc, a);
}

// The QP half of a two-stage step over DEVICE buffers (h->d_x0 / d_ub / d_stuck, the staged hull tables, the given reference
// windows): linearise about d_warmG (NULL: D stuck), the 6N-variable QP with the hull rows.  Leaves tau_0 in h->d_tau0, the wrenches in
// h->d_G, status / iterations in h->d_status / d_iters.  fork_alloc: where kernel 11 hands over to kernel 13, the allocation of what
// kernel 11 certified starts on the second stream before kernel 13's pass (*forked reports it; wrench_alloc_enqueue finishes it);
// otherwise everything stays on the handle's stream.
static int wrench_qp_enqueue(ftmpc_handle* h, int64_t B, int32_t hull_rows, bool has_set, const double* d_xref, int64_t xref_stride,
                             const double* d_uref, int64_t uref_stride, const double* d_warmG, bool fork_alloc, bool* forked) {
    hipStream_t s = h->stream;
    *forked = false;
    LinParams lp;
    lp.B = B;
    lp.x0 = h->d_x0; lp.ub = h->d_ub; lp.stuck = h->d_stuck;
    lp.xref = d_xref; lp.xref_stride = xref_stride;
    lp.uref = d_uref; lp.uref_stride = uref_stride;
    lp.warmU = nullptr;
    lp.rec = h->rec;
    lp.qlist = nullptr; lp.qcount = nullptr; lp.qvmax = -1;
    lp.warmG = d_warmG;
    lp.out_eN = h->d_eN;
    lp.tcost = h->d_tcost;
    lp.out_cbar = h->sbounds ? h->d_cbar.p : nullptr;      // the linearisation trajectory (about warmG, or D stuck) for the state rows
    lp.dist = h->lin_dist;      // (launch_linearize picks the DIST grid)
    launch_linearize(h, B, (int)((B + 63) / 64), s, lp);
    HIP_TRY(h, hipGetLastError());
    // the wrench problem stops at mu 1e-10 unless the caller asked otherwise (general rows: see ftmpc_config.mu_stop)
    DeviceConsts dcg = h->dc;
    if (!(h->cfg.mu_stop > 0)) dcg.mu_stop = 1e-10;
    const bool handed = hull_fp32(h, hull_rows);
    if (handed) {
        HIP_TRY(h, hipMemsetAsync(h->d_qctl, 0, 8 * sizeof(int32_t), s));
        ftmpc::SolveHullParams q;
        fill_wrench(h, q, B, hull_rows, has_set, d_warmG);
        q.base.out_u0 = h->d_u0;
        q.base.hscratch = h->hull_slot;
        q.base.tile_words = h->hull_slot_words;
        q.base.qhead = h->d_qctl + 7;
        q.base.dbg_H = h->use_f64 ? reinterpret_cast<float*>(h->d_dbgH64.p) : h->d_dbgH.p;     // (diagnostic build: phase stamps)
        const int grid = (int)std::min<int64_t>(B, h->grid_hull);
        q.fb_list = handover_list(h);
        q.fb_count = h->d_qctl;      // (the generalized-force path builds no work lists: the counter of list 0 is free)
        // kernel 11 leaves the interior-point iteration at mu 1e-7 for its polish: below that the fp32 slacks and duals of the
        // active rows are noise that spoils the active set they are read for (measured on 16 384 instances: 253 polishes do not
        // settle from mu 1e-10, 66 from 1e-7, same 1.9e-6 f_max worst error; from 1e-6 a wrong set is "verified")
        DeviceConsts dch = dcg;
        if (!(h->cfg.mu_stop > 0)) dch.mu_stop = 1e-7;
        hipLaunchKernelGGL(pick_hull32(h, hull_rows), dim3(grid), dim3(64), 0, s, dch, q);
        HIP_TRY(h, hipGetLastError());
    }
    h->wrench_handed = handed;
    // allocation of the batch on a second stream, beside kernel 13's pass over the hand-over list (not while profiling: the
    // event pairs of ftmpc_last_kernel_ms sit on one stream)
    const bool overlap = fork_alloc && handed && hull_ricw(h, hull_rows) && !h->profiling && h->stream2 != nullptr;
    *forked = overlap;
    if (overlap) {
        HIP_TRY(h, hipEventRecord(h->ev_fork, s));
        HIP_TRY(h, hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
        wrench_allocate(h, B, h->stream2, nullptr, nullptr);
        HIP_TRY(h, hipEventRecord(h->ev_alloc, h->stream2));
    }
    if (hull_ricw(h, hull_rows)) {      // kernel 13: the whole batch, or what kernel 11 handed over
        ftmpc::SolveRicwParams q;
        fill_wrench(h, q, B, hull_rows, has_set, d_warmG);
        q.base.qlist = handed ? handover_list(h) : nullptr;
        q.base.qcount = handed ? h->d_qctl.p : nullptr;
        HIP_TRY(h, hipMemsetAsync(h->d_qctl + 4, 0, sizeof(int32_t), s));
        q.base.qhead = h->d_qctl + 4;
        q.slot = h->ricw_slot;
        q.slot_doubles = h->ricw_slot_doubles;
        fill_state_bounds(h, q);
        const int grid = (int)std::min<int64_t>(B, h->grid_ricw);
        hipLaunchKernelGGL(pick_ricw64(h, hull_rows), dim3(grid), dim3(64), 0, s, dcg, q);
    } else {      // the dense float64 kernel: the whole batch, or what kernel 11 handed over
        Solve64Params q;
        fill_wrench(h, q, B, hull_rows, has_set, d_warmG);
        q.base.out_u0 = h->d_u0;
        q.base.qlist = handed ? handover_list(h) : nullptr;
        q.base.qcount = handed ? h->d_qctl.p : nullptr;
        q.Hs = h->gHs; q.Ls = h->gLs; q.Eall = h->gEall;
        q.tile_doubles = h->tile_doubles_gen;
        q.e_doubles = h->e_doubles_gen;
        q.npad_max = h->npad_gen;
        const int grid = (int)std::min<int64_t>(B, h->grid_gen);
        hipLaunchKernelGGL(pick_f64(h, true), dim3(grid), dim3(ftmpc::f64k::WG), 0, s, dcg, q);
    }
    HIP_TRY(h, hipGetLastError());
    return FTMPC_OK;
}

// The allocation half: u0 in h->d_u0 = min-norm allocation of h->d_tau0 - D stuck, status / iterations in h->d_ast2.  forked: the
// QP half started it on the second stream; only the instances kernel 11 handed over remain (list mode).
static int wrench_alloc_enqueue(ftmpc_handle* h, int64_t B, bool forked) {
    hipStream_t s = h->stream;
    if (forked) {
        // the handed-over instances (a few dozen of a regular batch, one wave each: ~2 ms of latency, the device nearly idle) run
        // on kernel 13 while the second stream allocates everything kernel 11 certified; their own allocation follows in list mode
        HIP_TRY(h, hipStreamWaitEvent(s, h->ev_alloc, 0));
        wrench_allocate(h, B, s, handover_list(h), h->d_qctl);
    } else {
        wrench_allocate(h, B, s, nullptr, nullptr);
    }
    HIP_TRY(h, hipGetLastError());
    return FTMPC_OK;
}

// One two-stage step: the QP half, then the allocation half (beside kernel 13's hand-over pass where that applies).
static int wrench_enqueue(ftmpc_handle* h, int64_t B, int32_t hull_rows, bool has_set, const double* d_xref, int64_t xref_stride,
                          const double* d_uref, int64_t uref_stride, const double* d_warmG) {
    bool forked = false;
    int rc = wrench_qp_enqueue(h, B, hull_rows, has_set, d_xref, xref_stride, d_uref, uref_stride, d_warmG, true, &forked);
    if (rc != FTMPC_OK) return rc;
    return wrench_alloc_enqueue(h, B, forked);
}

// The estimate of a ftmpc_*_wrench_disturbance_batch entry: dist [B*6] staged into h->d_ldist and h->lin_dist pointed at it for as
// long as the scope lives (wrench_qp_enqueue, cost_wrench_params read it), cleared on every way out.  dist = nullptr: nothing is set.
struct LinDistScope {
    ftmpc_handle* h;
    explicit LinDistScope(ftmpc_handle* hh) : h(hh) {}
    LinDistScope(const LinDistScope&) = delete;
    LinDistScope& operator=(const LinDistScope&) = delete;
    ~LinDistScope() { h->lin_dist = nullptr; }
    int stage(int64_t B, const double* dist) {
        if (!dist) return FTMPC_OK;
        int rc = h->d_ldist.ensure(h, B * 6);
        if (rc != FTMPC_OK) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->d_ldist, dist, (size_t)B * 6 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        h->lin_dist = h->d_ldist;
        return FTMPC_OK;
    }
};
static int check_dist(ftmpc_handle* h, int64_t B, const double* dist) {
    if (!dist) return fail(h, FTMPC_ERR_ARG, "dist is NULL (the plain entry takes no estimate)");
    for (int64_t i = 0; i < B * 6; ++i)
        if (!std::isfinite(dist[i]))
            return fail(h, FTMPC_ERR_ARG, "dist: vehicle " + std::to_string(i / 6) + " has a non-finite entry (" + std::to_string(i % 6) + ")");
    return FTMPC_OK;
}

static int solve_wrench(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                        const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                        const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride, double* warmG,
                        double* out_u0, double* out_tau0, double* out_G, int32_t* status, int32_t* iters, int32_t* alloc_status,
                        const double* dist);

int ftmpc_solve_wrench_batch(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                             const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                             const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride, double* warmG,
                             double* out_u0, double* out_tau0, double* out_G, int32_t* status, int32_t* iters, int32_t* alloc_status) {
    return solve_wrench(h, B, x0, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref, xref_stride, uref, uref_stride, warmG, out_u0,
                        out_tau0, out_G, status, iters, alloc_status, nullptr);
}

int ftmpc_solve_wrench_disturbance_batch(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                                         const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                         int32_t hull_rows, const double* xref, int64_t xref_stride, const double* uref,
                                         int64_t uref_stride, double* warmG, const double* dist, double* out_u0, double* out_tau0,
                                         double* out_G, int32_t* status, int32_t* iters, int32_t* alloc_status) {
    if (!h) return FTMPC_ERR_ARG;
    if (B < 0) return fail(h, FTMPC_ERR_ARG, "null buffer or negative batch");
    const int rc = check_dist(h, B, dist);
    if (rc != FTMPC_OK) return rc;
    return solve_wrench(h, B, x0, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref, xref_stride, uref, uref_stride, warmG, out_u0,
                        out_tau0, out_G, status, iters, alloc_status, dist);
}

static int solve_wrench(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                        const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                        const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride, double* warmG,
                        double* out_u0, double* out_tau0, double* out_G, int32_t* status, int32_t* iters, int32_t* alloc_status,
                        const double* dist) {
    if (!h) return FTMPC_ERR_ARG;
    if (B < 0 || !x0 || !ub || !stuck || !xref || !out_u0 || !hull_A || !hull_b)
        return fail(h, FTMPC_ERR_ARG, "null buffer or negative batch");
    if (B == 0) return FTMPC_OK;
    const int N = h->cfg.N, NT = h->cfg.NT;
    int rc = check_strides(h, xref_stride, uref_stride, uref);
    if (rc != FTMPC_OK) return rc;
    if ((rc = wrench_prepare(h, B, hull_A, n_sets, hull_set, hull_b, hull_rows)) != FTMPC_OK) return rc;
    hipStream_t s = h->stream;
    if ((rc = stage_inputs(h, B, x0, ub, stuck)) != FTMPC_OK) return rc;
    if ((rc = stage_refs(h, B, xref, xref_stride, uref, uref_stride)) != FTMPC_OK) return rc;
    if (warmG) HIP_TRY(h, hipMemcpyAsync(h->d_warmG, warmG, B * N * 6 * sizeof(double), hipMemcpyHostToDevice, s));
    LinDistScope ds(h);
    if ((rc = ds.stage(B, dist)) != FTMPC_OK) return rc;
    if ((rc = wrench_enqueue(h, B, hull_rows, hull_set != nullptr, h->d_xref, xref_stride, uref ? h->d_uref : nullptr, uref_stride,
                             warmG ? h->d_warmG : nullptr)) != FTMPC_OK)
        return rc;
    HIP_TRY(h, hipMemcpyAsync(out_u0, h->d_u0, B * NT * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_tau0) HIP_TRY(h, hipMemcpyAsync(out_tau0, h->d_tau0, B * 6 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_G) HIP_TRY(h, hipMemcpyAsync(out_G, h->d_G, B * N * 6 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (warmG) HIP_TRY(h, hipMemcpyAsync(warmG, h->d_G, B * N * 6 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (status) HIP_TRY(h, hipMemcpyAsync(status, h->d_status, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (iters) HIP_TRY(h, hipMemcpyAsync(iters, h->d_iters, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (alloc_status) HIP_TRY(h, hipMemcpyAsync(alloc_status, h->d_ast2, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return FTMPC_OK;
}

int ftmpc_last_handed_over(ftmpc_handle* h, int64_t* count) {
    if (!h || !count) return FTMPC_ERR_ARG;
    *count = 0;
    if (!h->wrench_handed) return FTMPC_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    int32_t c = 0;
    HIP_TRY(h, hipMemcpyAsync(&c, h->d_qctl, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *count = c;
    return FTMPC_OK;
}

// ---- the line-search SQP of the generalized-force formulation -------------------------------------------------------------
// Default weight sigma of the terminal-set violation in the merit (penalty <= 0).  An exact l1 penalty needs sigma above the
// largest terminal-row multiplier of the QPs; the largest one oracle/qp_oracle.py:ipm_general returns on the batches of
// tests/test_gpu_wrench_sqp.py is 9.4e3; the default is ten times that, rounded.
#define FTMPC_SQPW_PENALTY 1.0e5

// workspace of the wrench SQP: iterates [B*N*6] x 2, per-instance doubles [6B] (merit | alpha | cost0 | cost | violation | spare),
// flags [6B] (the layout of d_sqF), trial merits [B*backtracks], centre states [B*(N+1)*13] when wanted
static int sqpw_grow(ftmpc_handle* h, int64_t B, int32_t backtracks, bool want_X) {
    const int N = h->cfg.N;
    int rc;
    rc = ensure_group(h->cap_swsqp, B, [&] {
        int r;
        if ((r = h->d_swG.ensure(h, B * N * 6)) != FTMPC_OK || (r = h->d_swT.ensure(h, B * N * 6)) != FTMPC_OK ||
            (r = h->d_swJ.ensure(h, 6 * B)) != FTMPC_OK)
            return r;
        return h->d_swF.ensure(h, 6 * B);
    });
    if (rc != FTMPC_OK || (rc = h->d_swJall.ensure(h, B * backtracks)) != FTMPC_OK) return rc;
    return want_X ? h->d_swX.ensure(h, B * (N + 1) * 13) : FTMPC_OK;
}

static ftmpc::CostWrenchParams cost_wrench_params(const ftmpc_handle* h, int64_t B, const double* d_xref, int64_t xref_stride,
                                                  const double* d_uref, int64_t uref_stride, double sigma) {
    ftmpc::CostWrenchParams cw;
    cw.B = B;
    cw.x0 = h->d_x0;
    cw.xref = d_xref; cw.xref_stride = xref_stride;
    cw.uref = d_uref; cw.uref_stride = uref_stride;
    cw.G = nullptr;
    cw.tcost = h->d_tcost;
    fill_term(h, cw);
    cw.sigma = sigma;
    cw.out_merit = cw.out_cost = cw.out_tviol = cw.out_X = nullptr;
    cw.dist = h->lin_dist;
    return cw;
}

// the wrench cost / merit kernel over `lanes` lanes: the DIST instantiation under an estimate (cw.dist), else the plain one
static void launch_cost_wrench(const ftmpc_handle* h, int64_t lanes, hipStream_t s, const ftmpc::CostWrenchParams& cw) {
    if (cw.dist)
        hipLaunchKernelGGL(ftmpc::ftmpc_cost_wrench_kernel<1>, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, s, h->dc, cw);
    else
        hipLaunchKernelGGL(ftmpc::ftmpc_cost_wrench_kernel<0>, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, s, h->dc, cw);
}

// One wrench SQP solve over DEVICE buffers (h->d_x0 / d_ub / d_stuck, the hull tables staged by wrench_prepare, the given reference
// windows), direct launches on the handle's stream, no second stream.  Per major iteration: the wrench QP linearised about the iterate
// (wrench_qp_enqueue: kernel 11 with its hand-over, kernel 13 or the dense float64 kernel), every trial point of the line search in one
// launch, the first acceptable one picked.  After the last iteration: the cost, the violation and (d_X) the centre states of the final
// iterate, u0 = allocation of its tau_0 - D stuck in h->d_u0.  On return S.U is the final iterate, S.status / nmajor / ipm the counters.
static int sqpw_enqueue(ftmpc_handle* h, int64_t B, int32_t hull_rows, bool has_set, const double* d_xref, int64_t xref_stride,
                        const double* d_uref, int64_t uref_stride, const double* d_warm, int32_t sqp_iters, int32_t backtracks, double tol,
                        double sigma, bool want_X, ftmpc::SqpState& S) {
    const int N = h->cfg.N;
    int rc = sqpw_grow(h, B, backtracks, want_X);      // (the terminal rows: wrench_prepare)
    if (rc != FTMPC_OK) return rc;
    hipStream_t s = h->stream;
    S.B = B; S.N = N; S.NT = 6;
    S.ub = nullptr;
    S.U = h->d_swG; S.Uq = h->d_G; S.Ut = h->d_swT;
    S.J = h->d_swJ; S.Jt = nullptr; S.alpha = h->d_swJ + B;
    S.active = h->d_swF; S.todo = h->d_swF + B; S.improved = h->d_swF + 2 * B; S.nmajor = h->d_swF + 3 * B; S.ipm = h->d_swF + 4 * B;
    S.status = h->d_swF + 5 * B;
    S.qstatus = h->d_status; S.qiters = h->d_iters;
    S.tol = tol;
    S.Jall = h->d_swJall;
    S.ntrial = backtracks;
    const int64_t nw = (int64_t)N * 6;
    const unsigned gE = (unsigned)((B * nw + 255) / 256), gB = (unsigned)((B + 255) / 256);
    const ftmpc::CostWrenchParams cw = cost_wrench_params(h, B, d_xref, xref_stride, d_uref, uref_stride, sigma);
    hipLaunchKernelGGL(ftmpc::ftmpc_sqpw_init_kernel, dim3(gE > gB ? gE : gB), dim3(256), 0, s, h->dc, S, d_warm, (const double*)h->d_stuck);
    {   // merit and cost of the start point
        ftmpc::CostWrenchParams c0 = cw;
        c0.G = S.U;
        c0.out_merit = S.J;
        c0.out_cost = h->d_swJ + 2 * B;
        launch_cost_wrench(h, B, s, c0);
    }
    HIP_TRY(h, hipGetLastError());
    for (int it = 0; it < sqp_iters; ++it) {
        // the QP linearised about the current iterate (every instance: a stopped one costs a solve but changes nothing)
        bool forked = false;
        if ((rc = wrench_qp_enqueue(h, B, hull_rows, has_set, d_xref, xref_stride, d_uref, uref_stride, S.U, false, &forked)) != FTMPC_OK)
            return rc;
        hipLaunchKernelGGL(ftmpc::ftmpc_sqp_open_kernel, dim3(gB), dim3(256), 0, s, S);
        ftmpc::CostWrenchParams ct = cw;
        ct.G = S.U;
        ct.Gq = S.Uq;
        ct.todo = S.todo;
        ct.ntrial = backtracks;
        ct.out_merit = h->d_swJall;
        launch_cost_wrench(h, B * backtracks, s, ct);
        hipLaunchKernelGGL(ftmpc::ftmpc_sqp_pick_kernel, dim3(gB), dim3(256), 0, s, S);
        hipLaunchKernelGGL(ftmpc::ftmpc_sqpw_close_kernel, dim3(gE), dim3(256), 0, s, S);     // new iterate -> Ut
        hipLaunchKernelGGL(ftmpc::ftmpc_sqp_count_kernel, dim3(gB), dim3(256), 0, s, S);
        std::swap(S.U, S.Ut);
        HIP_TRY(h, hipGetLastError());
    }
    {   // cost, violation and rollout of the result
        ftmpc::CostWrenchParams cf = cw;
        cf.G = S.U;
        cf.out_merit = h->d_swJ + 5 * B;
        cf.out_cost = h->d_swJ + 3 * B;
        cf.out_tviol = h->d_swJ + 4 * B;
        cf.out_X = want_X ? h->d_swX : nullptr;
        launch_cost_wrench(h, B, s, cf);
    }
    // second stage, once: allocation of the final tau_0 (on an fp32 handle pulled inside the float64 hull first, as kernel 11 does)
    if (hull_fp32(h, hull_rows))
        hipLaunchKernelGGL(ftmpc::ftmpc_sqpw_tau0_kernel, dim3(gB * 4), dim3(64), 0, s, h->dc, B, (const double*)S.U,
                           (const double*)h->d_ub, (const double*)h->d_stuck, (const double*)h->d_hullA,
                           (const int32_t*)(has_set ? h->d_hullset : nullptr), (const double*)h->d_hullb, hull_rows, h->d_tau0);
    else
        HIP_TRY(h, hipMemcpy2DAsync(h->d_tau0, 6 * sizeof(double), S.U, nw * sizeof(double), 6 * sizeof(double), (size_t)B,
                                    hipMemcpyDeviceToDevice, s));
    return wrench_alloc_enqueue(h, B, false);
}

static int eval_cost_wrench(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck, const double* xref,
                            int64_t xref_stride, const double* uref, int64_t uref_stride, const double* G, const double* dist,
                            double* out_cost, double* out_tviol);

int ftmpc_eval_cost_wrench_batch(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck, const double* xref,
                                 int64_t xref_stride, const double* uref, int64_t uref_stride, const double* G, double* out_cost,
                                 double* out_tviol) {
    return eval_cost_wrench(h, B, x0, ub, stuck, xref, xref_stride, uref, uref_stride, G, nullptr, out_cost, out_tviol);
}

int ftmpc_eval_cost_wrench_disturbance_batch(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                                             const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride,
                                             const double* G, const double* dist, double* out_cost, double* out_tviol) {
    if (!h) return FTMPC_ERR_ARG;
    if (B < 0) return fail(h, FTMPC_ERR_ARG, "null buffer or negative batch");
    const int rc = check_dist(h, B, dist);
    if (rc != FTMPC_OK) return rc;
    return eval_cost_wrench(h, B, x0, ub, stuck, xref, xref_stride, uref, uref_stride, G, dist, out_cost, out_tviol);
}

static int eval_cost_wrench(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck, const double* xref,
                            int64_t xref_stride, const double* uref, int64_t uref_stride, const double* G, const double* dist,
                            double* out_cost, double* out_tviol) {
    (void)ub;
    (void)stuck;
    if (!h) return FTMPC_ERR_ARG;
    if (B < 0 || !x0 || !xref || !G || !out_cost) return fail(h, FTMPC_ERR_ARG, "null buffer or negative batch");
    if (B == 0) return FTMPC_OK;
    int rc = check_strides(h, xref_stride, uref_stride, uref);
    if (rc != FTMPC_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = ftmpc_reserve(h, B)) != FTMPC_OK) return rc;
    if ((rc = sqpw_grow(h, B, 1, false)) != FTMPC_OK) return rc;
    if ((rc = term_upload(h)) != FTMPC_OK) return rc;
    const int N = h->cfg.N;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->d_x0, x0, B * 13 * sizeof(double), hipMemcpyHostToDevice, s));
    if ((rc = stage_refs(h, B, xref, xref_stride, uref, uref_stride)) != FTMPC_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->d_swG, G, B * N * 6 * sizeof(double), hipMemcpyHostToDevice, s));
    LinDistScope ds(h);
    if ((rc = ds.stage(B, dist)) != FTMPC_OK) return rc;
    ftmpc::CostWrenchParams cw = cost_wrench_params(h, B, h->d_xref, xref_stride, uref ? h->d_uref : nullptr, uref_stride, 0.0);
    cw.G = h->d_swG;
    cw.out_merit = h->d_swJ;
    cw.out_tviol = h->d_swJ + B;
    launch_cost_wrench(h, B, s, cw);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out_cost, h->d_swJ, B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_tviol) HIP_TRY(h, hipMemcpyAsync(out_tviol, h->d_swJ + B, B * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return FTMPC_OK;
}

// the arguments every entry of the wrench SQP refuses alike.  sqp_used: the call runs the SQP (the closed loops with sqp_iters = 0
// run one QP step per control step, which has the state-bound rows: kernel 13's state-bound instantiation)
static int sqpw_check(ftmpc_handle* h, int32_t sqp_iters, int32_t backtracks, double tol, double penalty, bool sqp_used) {
    if (sqp_iters < 0 || (sqp_iters > 0 && backtracks < 1) || !(tol >= 0) || std::isnan(penalty) || std::isinf(penalty))
        return fail(h, FTMPC_ERR_ARG, "bad SQP iteration counts, tolerance or penalty");
    if (h->cfg.state_bounds && sqp_used)
        return fail(h, FTMPC_ERR_ARG, "the generalized-force SQP has no state-bound rows (state_bounds must be 0)");
    return FTMPC_OK;
}

static int solve_sqp_wrench(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                            const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                            const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride, const double* warmG,
                            const double* dist, int32_t sqp_iters, int32_t backtracks, double tol, double penalty, double* out_u0,
                            double* out_tau0, double* out_G, double* out_X, double* out_cost, double* out_cost0, double* out_tviol,
                            int32_t* out_sqp_iters, int32_t* out_iters, int32_t* status, int32_t* alloc_status);

int ftmpc_solve_sqp_wrench_batch(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                                 const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                 const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride, const double* warmG,
                                 int32_t sqp_iters, int32_t backtracks, double tol, double penalty, double* out_u0, double* out_tau0,
                                 double* out_G, double* out_X, double* out_cost, double* out_cost0, double* out_tviol, int32_t* out_sqp_iters,
                                 int32_t* out_iters, int32_t* status, int32_t* alloc_status) {
    return solve_sqp_wrench(h, B, x0, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref, xref_stride, uref, uref_stride, warmG,
                            nullptr, sqp_iters, backtracks, tol, penalty, out_u0, out_tau0, out_G, out_X, out_cost, out_cost0, out_tviol,
                            out_sqp_iters, out_iters, status, alloc_status);
}

int ftmpc_solve_sqp_wrench_disturbance_batch(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                                             const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                             int32_t hull_rows, const double* xref, int64_t xref_stride, const double* uref,
                                             int64_t uref_stride, const double* warmG, const double* dist, int32_t sqp_iters,
                                             int32_t backtracks, double tol, double penalty, double* out_u0, double* out_tau0,
                                             double* out_G, double* out_X, double* out_cost, double* out_cost0, double* out_tviol,
                                             int32_t* out_sqp_iters, int32_t* out_iters, int32_t* status, int32_t* alloc_status) {
    if (!h) return FTMPC_ERR_ARG;
    if (B < 0) return fail(h, FTMPC_ERR_ARG, "null buffer or negative batch");
    const int rc = check_dist(h, B, dist);
    if (rc != FTMPC_OK) return rc;
    return solve_sqp_wrench(h, B, x0, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref, xref_stride, uref, uref_stride, warmG,
                            dist, sqp_iters, backtracks, tol, penalty, out_u0, out_tau0, out_G, out_X, out_cost, out_cost0, out_tviol,
                            out_sqp_iters, out_iters, status, alloc_status);
}

static int solve_sqp_wrench(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                            const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                            const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride, const double* warmG,
                            const double* dist, int32_t sqp_iters, int32_t backtracks, double tol, double penalty, double* out_u0,
                            double* out_tau0, double* out_G, double* out_X, double* out_cost, double* out_cost0, double* out_tviol,
                            int32_t* out_sqp_iters, int32_t* out_iters, int32_t* status, int32_t* alloc_status) {
    if (!h) return FTMPC_ERR_ARG;
    if (B < 0 || !x0 || !ub || !stuck || !xref || !out_u0 || !hull_A || !hull_b)
        return fail(h, FTMPC_ERR_ARG, "null buffer or negative batch");
    int rc = sqpw_check(h, sqp_iters, backtracks, tol, penalty, true);
    if (rc != FTMPC_OK) return rc;
    if (backtracks < 1) return fail(h, FTMPC_ERR_ARG, "backtracks must be at least 1");
    if (B == 0) return FTMPC_OK;
    const int N = h->cfg.N, NT = h->cfg.NT;
    if ((rc = check_strides(h, xref_stride, uref_stride, uref)) != FTMPC_OK) return rc;
    if ((rc = wrench_prepare(h, B, hull_A, n_sets, hull_set, hull_b, hull_rows)) != FTMPC_OK) return rc;
    hipStream_t s = h->stream;
    if ((rc = stage_inputs(h, B, x0, ub, stuck)) != FTMPC_OK) return rc;
    if ((rc = stage_refs(h, B, xref, xref_stride, uref, uref_stride)) != FTMPC_OK) return rc;
    if (warmG) HIP_TRY(h, hipMemcpyAsync(h->d_warmG, warmG, B * N * 6 * sizeof(double), hipMemcpyHostToDevice, s));
    LinDistScope ds(h);
    if ((rc = ds.stage(B, dist)) != FTMPC_OK) return rc;
    ftmpc::SqpState S;
    if ((rc = sqpw_enqueue(h, B, hull_rows, hull_set != nullptr, h->d_xref, xref_stride, uref ? h->d_uref : nullptr, uref_stride,
                           warmG ? h->d_warmG : nullptr, sqp_iters, backtracks, tol, penalty > 0 ? penalty : FTMPC_SQPW_PENALTY,
                           out_X != nullptr, S)) != FTMPC_OK)
        return rc;
    HIP_TRY(h, hipMemcpyAsync(out_u0, h->d_u0, B * NT * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_tau0) HIP_TRY(h, hipMemcpyAsync(out_tau0, h->d_tau0, B * 6 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_G) HIP_TRY(h, hipMemcpyAsync(out_G, S.U, B * N * 6 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_X) HIP_TRY(h, hipMemcpyAsync(out_X, h->d_swX, B * (N + 1) * 13 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_cost) HIP_TRY(h, hipMemcpyAsync(out_cost, h->d_swJ + 3 * B, B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_cost0) HIP_TRY(h, hipMemcpyAsync(out_cost0, h->d_swJ + 2 * B, B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_tviol) HIP_TRY(h, hipMemcpyAsync(out_tviol, h->d_swJ + 4 * B, B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_sqp_iters) HIP_TRY(h, hipMemcpyAsync(out_sqp_iters, S.nmajor, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (out_iters) HIP_TRY(h, hipMemcpyAsync(out_iters, S.ipm, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (status) HIP_TRY(h, hipMemcpyAsync(status, S.status, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (alloc_status) HIP_TRY(h, hipMemcpyAsync(alloc_status, h->d_ast2, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return FTMPC_OK;
}

int ftmpc_allocate_batch(ftmpc_handle* h, int64_t B, const double* tau, const double* ub, double* out_u, int32_t* status,
                         int32_t* iters) {
    if (!h) return FTMPC_ERR_ARG;
    if (B < 0 || !tau || !ub || !out_u) return fail(h, FTMPC_ERR_ARG, "null buffer or negative batch");
    if (B == 0) return FTMPC_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const int NT = h->cfg.NT;
    const int rc = ensure_group(h->cap_alloc, B, [&] {
        int r;
        if ((r = h->d_atau.ensure(h, B * 6)) != FTMPC_OK || (r = h->d_aub.ensure(h, B * NT)) != FTMPC_OK ||
            (r = h->d_au.ensure(h, B * NT)) != FTMPC_OK || (r = h->d_ast.ensure(h, B)) != FTMPC_OK)
            return r;
        return h->d_ait.ensure(h, B);
    });
    if (rc != FTMPC_OK) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->d_atau, tau, B * 6 * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->d_aub, ub, B * NT * sizeof(double), hipMemcpyHostToDevice, s));
    ftmpc::AllocParams ap;
    ap.B = B;
    ap.tau = h->d_atau;
    ap.ub = h->d_aub;
    ap.out_u = h->d_au;
    ap.status = h->d_ast;
    ap.iters = h->d_ait;
    ap.max_iters = 50;
    ap.tol = 1e-8;
    hipLaunchKernelGGL(ftmpc::ftmpc_allocate_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, h->dc, ap);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out_u, h->d_au, B * NT * sizeof(double), hipMemcpyDeviceToHost, s));
    if (status) HIP_TRY(h, hipMemcpyAsync(status, h->d_ast, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (iters) HIP_TRY(h, hipMemcpyAsync(iters, h->d_ait, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return FTMPC_OK;
}

int ftmpc_shift_warm(int64_t B, int32_t N, int32_t NT, double* warmU) {
    if (B < 0 || N < 1 || NT < 1 || !warmU) return FTMPC_ERR_ARG;
    for (int64_t b = 0; b < B; ++b) {
        double* w = warmU + b * (int64_t)N * NT;
        std::memmove(w, w + NT, (size_t)(N - 1) * NT * sizeof(double));
        std::memset(w + (size_t)(N - 1) * NT, 0, NT * sizeof(double));
    }
    return FTMPC_OK;
}

int ftmpc_set_profiling(ftmpc_handle* h, int32_t enabled) {
    if (!h) return FTMPC_ERR_ARG;
    h->profiling = enabled != 0;
    h->ev_valid = false;
    return FTMPC_OK;
}

int ftmpc_last_kernel_ms(ftmpc_handle* h, float* ms, int32_t n_slots) {
    if (!h || !ms || n_slots < 0) return FTMPC_ERR_ARG;
    if (!h->ev_valid) return fail(h, FTMPC_ERR_ARG, "no profiled solve recorded");
    for (int k = 0; k < std::min<int>(n_slots, FTMPC_KERNEL_SLOTS); ++k) {
        ms[k] = 0.f;
        if (!h->ev_used[k]) continue;
        HIP_TRY(h, hipEventSynchronize(h->ev[2 * k + 1]));
        HIP_TRY(h, hipEventElapsedTime(&ms[k], h->ev[2 * k], h->ev[2 * k + 1]));
    }
    return FTMPC_OK;
}

static const char* const k_kernel_names[FTMPC_KERNEL_SLOTS] = {"ftmpc_linearize_kernel", "ftmpc_solve_f32_kernel<8>", "ftmpc_solve_f32_kernel<9>",
                                                                "ftmpc_solve_f32_kernel<10>", "ftmpc_solve_f64_kernel", "ftmpc_solve_wsw32_kernel | ftmpc_solve_ws32_kernel | ftmpc_solve_wg32_kernel<15>",
                                                                "ftmpc_solve_ws64_kernel"};

const char* ftmpc_kernel_name(int32_t slot) { return (slot >= 0 && slot < FTMPC_KERNEL_SLOTS) ? k_kernel_names[slot] : ""; }

const char* ftmpc_routed_kernel_name(const ftmpc_handle* h, int32_t slot) {
    if (h && slot == 6) return h->use_ric64 ? "ftmpc_solve_ric64_kernel" : "ftmpc_solve_ws64_kernel";      // (kernel 12 also with the terminal set: tset_ric)
    if (h && slot == 5) return h->use_wsw ? "ftmpc_solve_wsw32_kernel" : (h->use_ws ? "ftmpc_solve_ws32_kernel" : "ftmpc_solve_wg32_kernel<15>");
    return ftmpc_kernel_name(slot);
}

int ftmpc_debug_build_qp(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                         const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride,
                         const double* warmU, int64_t inst, double* H, int64_t H_cap, double* g, double* lo,
                         double* hi, int32_t* n_out) {
    if (!h || !H || !g || !lo || !hi || !n_out || inst < 0 || inst >= B) return FTMPC_ERR_ARG;
    int rc = check_strides(h, xref_stride, uref_stride, uref);
    if (rc != FTMPC_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = ftmpc_reserve(h, B)) != FTMPC_OK) return rc;
    const int N = h->cfg.N, NT = h->cfg.NT;
    hipStream_t s = h->stream;
    if ((rc = stage_inputs(h, B, x0, ub, stuck)) != FTMPC_OK) return rc;
    if ((rc = stage_refs(h, B, xref, xref_stride, uref, uref_stride)) != FTMPC_OK) return rc;
    if (warmU) HIP_TRY(h, hipMemcpyAsync(h->d_warm, warmU, B * N * NT * sizeof(double), hipMemcpyHostToDevice, s));
    if (!h->use_f64) HIP_TRY(h, hipMemsetAsync(h->d_dbgv, 0, (3 * 256 + 4) * sizeof(float), s));
    if (h->use_ws && h->nb_max > 15)
        return fail(h, FTMPC_ERR_ARG, "the QP dump needs N * NT <= 240 on the fp32 path (create the handle with dtype FTMPC_DTYPE_F64 for larger shapes)");
    const bool ws64_was = h->use_ws64, ric_was = h->use_ric64;      // (the dump comes from the dense float64 kernel: the only one that forms H)
    if (h->use_f64 && (rc = dense_ensure(h)) != FTMPC_OK) return rc;     // (not allocated by ftmpc_create where no solve uses them)
    h->use_ws64 = false;
    h->use_ric64 = false;
    const bool wsw_was = h->use_wsw;
    h->use_wsw = false;
    const bool ws_was = h->use_ws;
    h->use_ws = false;     // the dump hook (the condensed thruster-space QP) lives in kernel 7; kernel 8 never forms that matrix
    rc = enqueue(h, B, h->d_x0, h->d_ub, h->d_stuck, h->d_xref, xref_stride, uref ? h->d_uref : nullptr, uref_stride,
                 warmU ? h->d_warm : nullptr, h->d_u0, nullptr, h->d_status, h->d_iters, s, inst);
    h->use_ws = ws_was;
    h->use_wsw = wsw_was;
    h->use_ws64 = ws64_was;
    h->use_ric64 = ric_was;
    if (rc != FTMPC_OK) return rc;
    if (h->use_f64) {
        const int64_t pm = h->npad_max;
        std::vector<double> Hd((size_t)(pm * pm)), vd((size_t)(3 * pm + 4));
        HIP_TRY(h, hipMemcpyAsync(Hd.data(), h->d_dbgH64, Hd.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(vd.data(), h->d_dbgv64, vd.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        const int n = (int)vd[3 * pm], npad = (int)vd[3 * pm + 1];
        if (n <= 0) return fail(h, FTMPC_ERR_ARG, "instance has no active thruster or was not dumped");
        if ((int64_t)n * n > H_cap) return fail(h, FTMPC_ERR_ARG, "H buffer too small");
        for (int i = 0; i < n; ++i) {
            for (int j = 0; j < n; ++j) H[(int64_t)i * n + j] = Hd[(size_t)i * npad + j];
            g[i] = vd[i];
            lo[i] = vd[pm + i];
            hi[i] = vd[2 * pm + i];
        }
        *n_out = n;
        return FTMPC_OK;
    }
    std::vector<float> Hf(256 * 256), vf(3 * 256 + 4);
    HIP_TRY(h, hipMemcpyAsync(Hf.data(), h->d_dbgH, Hf.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(vf.data(), h->d_dbgv, vf.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    // the one-wave kernels leave (n, npad) at words 480 / 481, the workgroup kernel at 720 / 721
    const int mk = (vf[720] > 0.f) ? 720 : 480;
    const int n = (int)vf[mk], npad = (int)vf[mk + 1];
    if (n == 0) return fail(h, FTMPC_ERR_ARG, "instance has no active thruster or was not dumped");
    if ((int64_t)n * n > H_cap) return fail(h, FTMPC_ERR_ARG, "H buffer too small");
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) H[(int64_t)i * n + j] = Hf[(size_t)i * npad + j];
        g[i] = vf[i];
        lo[i] = vf[npad + i];
        hi[i] = vf[2 * npad + i];
    }
    *n_out = n;
    return FTMPC_OK;
}

static int debug_records(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                         const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride,
                         const double* warmU, const double* dist, double* rec_out);

int ftmpc_debug_records(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                        const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride,
                        const double* warmU, double* rec_out) {
    return debug_records(h, B, x0, ub, stuck, xref, xref_stride, uref, uref_stride, warmU, nullptr, rec_out);
}

int ftmpc_debug_records_disturbance(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                                    const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride,
                                    const double* warmU, const double* dist, double* rec_out) {
    if (!h || !dist) return FTMPC_ERR_ARG;
    return debug_records(h, B, x0, ub, stuck, xref, xref_stride, uref, uref_stride, warmU, dist, rec_out);
}

// dist != nullptr: the DIST instantiation of the linearise kernel with that estimate
static int debug_records(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                         const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride,
                         const double* warmU, const double* dist, double* rec_out) {
    if (!h || !rec_out || B <= 0) return FTMPC_ERR_ARG;
    int rc = check_strides(h, xref_stride, uref_stride, uref);
    if (rc != FTMPC_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = ftmpc_reserve(h, B)) != FTMPC_OK) return rc;
    const int N = h->cfg.N, NT = h->cfg.NT;
    hipStream_t s = h->stream;
    if ((rc = stage_inputs(h, B, x0, ub, stuck)) != FTMPC_OK) return rc;
    if ((rc = stage_refs(h, B, xref, xref_stride, uref, uref_stride)) != FTMPC_OK) return rc;
    if (warmU) HIP_TRY(h, hipMemcpyAsync(h->d_warm, warmU, B * N * NT * sizeof(double), hipMemcpyHostToDevice, s));
    LinParams lp;      // as enqueue fills it, work lists included
    lp.B = B;
    lp.x0 = h->d_x0; lp.ub = h->d_ub; lp.stuck = h->d_stuck;
    lp.xref = h->d_xref; lp.xref_stride = xref_stride;
    lp.uref = uref ? h->d_uref : nullptr; lp.uref_stride = uref_stride;
    lp.warmU = warmU ? h->d_warm : nullptr;
    lp.rec = h->rec;
    lp.warmG = nullptr;
    lp.out_eN = h->tset ? h->d_eN : nullptr;
    lp.tcost = h->d_tcost;
    lp.out_cbar = h->sbounds ? h->d_cbar : nullptr;
    DevBuf<double> d_dist;
    if (dist) {
        HIP_TRY(h, hipMalloc(&d_dist.p, (size_t)B * 6 * sizeof(double)));
        HIP_TRY(h, hipMemcpyAsync(d_dist, dist, (size_t)B * 6 * sizeof(double), hipMemcpyHostToDevice, s));
        lp.dist = d_dist;
    }
    const int nvar = h->use_f64 ? 0 : (h->nb_max <= 8 ? 1 : (h->nb_max == 9 ? 2 : 3));
    lp.qlist = h->use_f64 ? nullptr : h->d_qlist;
    lp.qcount = h->d_qctl;
    lp.qvmax = h->use_wg ? 3 : nvar - 1;
    if (!h->use_f64) HIP_TRY(h, hipMemsetAsync(h->d_qctl, 0, 8 * sizeof(int32_t), s));
    launch_linearize(h, B, (int)((B + 63) / 64), s, lp);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(rec_out, h->rec, (size_t)B * N * ftmpc::REC_STRIDE * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return FTMPC_OK;
}

int ftmpc_debug_struct_grad(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                            const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride,
                            const double* warmU, const float* d, int32_t form, double* g_out) {
    if (!h || !d || !g_out || B <= 0 || form < 0 || form > 1) return FTMPC_ERR_ARG;
    const int N = h->cfg.N, NT = h->cfg.NT;
    if (h->use_f64 || N > ftmpc::SGD_NMAX || NT > 8)
        return fail(h, FTMPC_ERR_ARG, "the gradient hook serves the fp32 path with N <= 21 and NT <= 8 (the shapes whose sweeps exchange through LDS)");
    // the records, as ftmpc_debug_records leaves them on the device
    std::vector<double> rec((size_t)B * N * ftmpc::REC_STRIDE);
    int rc = ftmpc_debug_records(h, B, x0, ub, stuck, xref, xref_stride, uref, uref_stride, warmU, rec.data());
    if (rc != FTMPC_OK) return rc;
    hipStream_t s = h->stream;
    const int64_t words = B * N * NT;
    DevBuf<float> d_d;
    DevBuf<double> d_g;
    if ((rc = d_d.ensure(h, words)) != FTMPC_OK || (rc = d_g.ensure(h, words)) != FTMPC_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(d_d, d, (size_t)words * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemsetAsync(d_g, 0, (size_t)words * sizeof(double), s));
    ftmpc::StructGradDebugParams q;
    q.B = B;
    q.rec = h->rec;
    q.ub = h->d_ub;
    q.d = d_d;
    q.g = d_g;
    // fewer workgroups than instances (from B = 2 on): a wave meets the LDS its previous instance left behind
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((B + 2) / 3, 4 * (int64_t)h->num_cu));
    if (form == 1)
        hipLaunchKernelGGL(ftmpc::ftmpc_struct_grad_debug_kernel<true>, dim3(grid), dim3(64), 0, s, h->dc, q);
    else
        hipLaunchKernelGGL(ftmpc::ftmpc_struct_grad_debug_kernel<false>, dim3(grid), dim3(64), 0, s, h->dc, q);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(g_out, d_g, (size_t)words * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return FTMPC_OK;
}

int ftmpc_hull_offsets_batch(ftmpc_handle* h, int64_t B, const double* ub, const double* stuck, const double* hull_A, int32_t n_sets,
                             const int32_t* hull_set, int32_t hull_rows, double* out_b, int32_t* out_flat) {
    if (!h) return FTMPC_ERR_ARG;
    if (B < 0 || !ub || !stuck || !hull_A || !out_b) return fail(h, FTMPC_ERR_ARG, "null buffer or negative size");
    if (hull_rows < 1 || hull_rows > FTMPC_MAX_HULL_ROWS || n_sets < 1) return fail(h, FTMPC_ERR_ARG, "hull_rows out of range (1..128) or no hull table");
    if (hull_set)   // the kernel indexes hull_A by these
        for (int64_t b = 0; b < B; ++b)
            if (hull_set[b] < 0 || hull_set[b] >= n_sets)
                return fail(h, FTMPC_ERR_ARG, "hull_set[" + std::to_string(b) + "] = " + std::to_string(hull_set[b]) + " is not a table number in [0, n_sets)");
    if (B == 0) return FTMPC_OK;
    const int NT = h->cfg.NT;
    const size_t nA = (size_t)n_sets * hull_rows * 6, nP = (size_t)B * NT, nB = (size_t)B * hull_rows;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    DevBuf<double> d_A, d_pat, d_b;
    DevBuf<int32_t> d_int;      // [flat B | hull_set B]
    HIP_TRY(h, hipMalloc(&d_A.p, nA * sizeof(double)));
    HIP_TRY(h, hipMalloc(&d_pat.p, 2 * nP * sizeof(double)));
    HIP_TRY(h, hipMalloc(&d_b.p, nB * sizeof(double)));
    HIP_TRY(h, hipMalloc(&d_int.p, 2 * (size_t)B * sizeof(int32_t)));
    HIP_TRY(h, hipMemcpyAsync(d_A, hull_A, nA * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(d_pat, ub, nP * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(d_pat + nP, stuck, nP * sizeof(double), hipMemcpyHostToDevice, s));
    if (hull_set) HIP_TRY(h, hipMemcpyAsync(d_int + B, hull_set, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    ftmpc::HullOffsets ho{};
    ho.B = B;
    ho.hull_rows = hull_rows;
    ho.ub = d_pat;
    ho.stuck = d_pat + nP;
    ho.hullA = d_A;
    ho.hullset = hull_set ? d_int + B : nullptr;
    ho.out_b = d_b;
    ho.flat = d_int;
    hipLaunchKernelGGL(ftmpc::ftmpc_hull_offsets_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, h->dc, ho);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out_b, d_b, nB * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_flat) HIP_TRY(h, hipMemcpyAsync(out_flat, d_int, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return FTMPC_OK;
}

}  // extern "C"

#include "ftmpc_loop.hip"

extern "C" {

#ifdef FTMPC_STAMPS
/* diagnostic build only: copies the per-instance phase cycle totals (12 u64 per instance, first
 * `count` <= 4096 instances) of the last fp32 solve */
int ftmpc_debug_read_stamps(ftmpc_handle* h, int64_t count, unsigned long long* out) {
    const void* src = h ? (h->use_f64 ? (const void*)h->d_dbgH64.p : (const void*)h->d_dbgH.p) : nullptr;
    if (!h || !out || count < 0 || count > 4096 || !src || (h->use_f64 && count > 512)) return FTMPC_ERR_ARG;
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(out, src, (size_t)count * 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return FTMPC_OK;
}
#endif

}  // extern "C"

#include "ftmpc_multi.hip"
