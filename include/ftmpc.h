/*
 * ftmpc.h -- C-ABI of the MI355X-native batched MPC QP-step path.
 *
 * Drop-in boundary.  The reference (DISCOWER/fault-tolerant-mpc) has
 * no FFI: its seam is the duck-typed Python controller consumed by
 * ft_mpc/simulation/sim_env.py:82.  These entry points are what a ctypes binding behind
 *     SpiralingController.get_control(x0, t)   ft_mpc/controllers/spiraling_mpc.py:288-317
 *     SpiralingController.solve_mpc(c0)        ft_mpc/controllers/spiraling_mpc.py:319-354
 * calls; INTEGRATION.md shows that binding.  Plain C types only, caller-owned buffers, int
 * return codes (0 ok, <0 error) and per-instance status/iters arrays instead of the
 * reference's logged-but-ignored IPOPT status (spiraling_mpc.py:347-352) or the allocator's
 * exit() (controllers/tools/control_allocator.py:88-93).  No global state: one opaque
 * handle per GPU; distinct handles may be used concurrently from distinct host threads.
 *
 * All host-visible numbers are IEEE double (the reference works in numpy float64).
 * State layout x0 = [p(3), v(3), q(4; x,y,z,w), omega(3)]   ft_mpc/models/sys_model.py:35-41.
 */
#ifndef FTMPC_H
#define FTMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTMPC_MAX_NT 16
#define FTMPC_MAX_TERM_ROWS 80   /* rows of the terminal set (config/terminal.yaml: 72) */
#define FTMPC_MAX_TCOST_TERMS 24  /* non-quadratic terms of the terminal cost (config/terminal.yaml: 13 polynomial + 12 root terms) */
#define FTMPC_MAX_HULL_ROWS 128  /* facets of the generalized-force hull (26 for every fault set of the reference vehicle; 112 for a
                                    generic 8-thruster allocation matrix).  More than 32: float64 Riccati kernel only (kernel 13, with or without
                                    the terminal set: see ftmpc_solve_wrench_batch) */
#define FTMPC_NX 13
#define FTMPC_NOPT 9
#define FTMPC_NG 6

/* return codes */
#define FTMPC_OK 0
#define FTMPC_ERR_ARG (-1)       /* bad argument / unsupported shape */
#define FTMPC_ERR_HIP (-2)       /* HIP runtime failure; see ftmpc_last_error */
#define FTMPC_ERR_NODEVICE (-3)  /* no usable gfx950 device */
#define FTMPC_ERR_ALLOC (-4)

/* per-instance status[] values */
#define FTMPC_STATUS_CONVERGED 0   /* complementarity gap fell below mu_stop */
#define FTMPC_STATUS_MAXITER 1     /* stopped at max_iters (last iterate returned, like the reference) */
#define FTMPC_STATUS_NUMERIC 2     /* non-finite value met / factorisation broke down (e.g. an unreachable terminal set);
                                      the linearisation point (clip(warm start)) is returned */

#define FTMPC_STATUS_NO_HULL 3     /* generalized-force formulation only: the healthy thrusters do not span R^6, the input hull
                                      is flat (the reference's Qhull call fails on such fault sets); set by the host front-end */

/*
 * A NON-FINITE VEHICLE (a NaN or Inf in its x0 or in a stuck entry of a broken thruster: a vehicle of a fault campaign that has
 * diverged).  The solve entries do not validate x0 / stuck; such an instance is answered per instance and touches nothing else: every
 * output of every other instance of the batch, and of every later call on the handle, has the bits it has without it
 * (tests/test_gpu_poisoned_instances.py).  What comes back for the instance itself:
 *   ftmpc_solve_batch          status FTMPC_STATUS_NUMERIC, iters >= 0; out_U = the linearisation point clip(warm start, 0, ub)
 *                              (zeros on a cold start and on broken thrusters; the fp32 kernels return it rounded to float32), out_u0
 *                              its first stage.  Always finite and inside [0, ub].
 *   ftmpc_solve_wrench_batch   status FTMPC_STATUS_NUMERIC; out_G = the linearisation point (warmG; D stuck on a cold start), out_tau0
 *                              its first stage pulled into the hull as for a solved instance, out_u0 the allocation of
 *                              out_tau0 - D stuck with its own alloc_status (0 on a cold start: the point needs no thrust; 2 where a
 *                              stuck entry is not finite, with out_u0 = 0).  An entry of that point that is not finite itself (D stuck
 *                              of a NaN stuck entry; out_tau0 without a finite hull centre) is returned as 0: every output is finite,
 *                              out_u0 inside [0, ub].
 *   ftmpc_solve_sqp_batch / ftmpc_solve_sqp_wrench_batch   the first QP ends with FTMPC_STATUS_NUMERIC, so no line search opens:
 *                              status 2, out_sqp_iters 0, the start point as out_U / out_G (as above), out_cost = out_cost0 = the
 *                              cost there, which is NaN or +Inf (the wrench cost does not read stuck: finite for a NaN stuck entry).
 *   ftmpc_eval_cost_batch / ftmpc_eval_cost_wrench_batch   out_cost NaN or +Inf, never a finite number; out_tviol sums max(0, .), which
 *                              drops a NaN row: it is >= 0 and never NaN (+Inf for an infinite error).
 *   ftmpc_allocate_batch       (a NaN or Inf in tau) status 2, iters 0, out_u = 0.
 *   the closed loops           the vehicle counts in not_converged[t] and in the outcome `unsolved` at every step, status_hist shows
 *                              its status 2; its own state, command history and error outcomes are not meaningful.
 * A state that is huge but finite in the handle's arithmetic (1e30 on an fp32 handle, 1e200 in float64) is an ordinary instance: it
 * ends with one of the three status values and finite outputs inside their bounds, status 0 only with the solution (at those two
 * magnitudes, where intermediate products overflow, no kernel answers 0: FTMPC_STATUS_NUMERIC, on a long horizon of the two-stage
 * form FTMPC_STATUS_MAXITER).
 * Not covered: a non-finite warm start, reference, ub, or hull table.
 */

/* arithmetic of the solve path */
#define FTMPC_DTYPE_F32 0
#define FTMPC_DTYPE_F64 1

/*
 * Problem constants.  Replaces what the reference hard-codes or reads from YAML:
 *   N        tuning.spiraling.horizon          ft_mpc/config/reactive.yaml:26, spiraling_mpc.py:38
 *   dt       time_step                         reactive.yaml:2
 *   mass,J   SystemModel                       ft_mpc/models/sys_model.py:52-57
 *   D        6 x NT allocation matrix, row-major, sys_model.py:73-123 (NT=16); runtime data so
 *            that the NT=8 benchmark can pass its synthetic matrix
 *   Q,R      diag weights                      reactive.yaml:32-33, spiraling_mpc.py:91-93
 *   P        9x9 terminal weight, row-major (quadratic part of ft_mpc/config/terminal.yaml)
 *   r        orbit radius vector               controllers/tools/spiral_parameters.py:39
 *   f_virt   virtual force                     spiral_parameters.py:34-36
 *   rho      min-energy allocation weight      controllers/tools/control_allocator.py:32
 *            (folded into the QP as strict-convexity regulariser; QP-spec)
 */
typedef struct ftmpc_config {
    int32_t N;          /* horizon stages, 1..64 */
    int32_t NT;         /* thrusters, 1..FTMPC_MAX_NT */
    int32_t dtype;      /* FTMPC_DTYPE_F32 | FTMPC_DTYPE_F64 : arithmetic of the IPM/KKT solve */
    int32_t max_iters;  /* IPM iteration cap (fixed upper bound; early exit at mu_stop) */
    int32_t device_id;  /* HIP device ordinal */
    int32_t struct_size; /* sizeof(ftmpc_config) of the header the caller was built against; ftmpc_default_config fills it and
                            ftmpc_create refuses any other value (FTMPC_ERR_ARG), so a caller built against an older, shorter
                            struct is told instead of being read past its end */
    double dt;
    double mass;
    double J[9];
    double D[FTMPC_NG * FTMPC_MAX_NT]; /* row-major 6 x NT, row stride NT */
    double Q[FTMPC_NOPT];
    double R[FTMPC_NG];
    double P[FTMPC_NOPT * FTMPC_NOPT];
    double r[3];
    double f_virt[3];
    double rho;
    double mu_stop;     /* stop when mean complementarity < mu_stop (<=0: library default) */
    /*
     * Terminal set  term_A (c_N[0:9] - xref_N) <= term_b  (the polytope of config/terminal.yaml, term_set; reference
     * spiraling_mpc.py:199-202).  terminal_set != 0 adds these rows to the QP; ftmpc_solve_batch then runs in float64 whatever
     * the dtype: on the dense float64 kernel where N * NT <= 256 (padded to 16), on the Riccati kernel ftmpc_solve_ric64_kernel
     * beyond that up to N = 40 (and for every N <= 40 with kernel_select = FTMPC_KERNEL_RICCATI).  N > 40 with N * NT > 256, and
     * kernel_select = FTMPC_KERNEL_DENSE with N * NT > 256, are refused with FTMPC_ERR_ARG when a solve is called.  As in the dense
     * kernel's general-row modes, a factorisation that breaks down once mu < 1e-7 with the rows' primal residual below 1e-9 ends the
     * iteration as converged, as oracle/qp_oracle.py:ipm_general does: FTMPC_STATUS_OK with the interior-point iterate of that mu
     * (the active-set polish has been tried on it or on an earlier one and did not settle, so the exact-solution accuracy of a
     * polished result does not hold for such an instance); an earlier breakdown is
     * FTMPC_STATUS_NUMERIC;
     * ftmpc_solve_wrench_batch as described there (no such limit).  An instance whose terminal set cannot
     * be reached within the horizon ends with FTMPC_STATUS_MAXITER / _NUMERIC (the reference logs IPOPT's failure
     * and carries on, spiraling_mpc.py:347-352).
     */
    int32_t terminal_set;
    int32_t term_rows;  /* <= FTMPC_MAX_TERM_ROWS */
    double term_A[FTMPC_MAX_TERM_ROWS * FTMPC_NOPT];   /* row-major term_rows x 9 */
    double term_b[FTMPC_MAX_TERM_ROWS];
    /*
     * Non-quadratic part of the terminal cost (config/terminal.yaml `cost` beyond e'P e; reference spiraling_mpc.py:196):
     *     V_nq(e) = sum_i tc_poly_coef[i] prod_j e_j^tc_poly_exp[i][j] + sum_r tc_root_coef[r] (prod_j e_j^tc_root_exp[r][j] + tc_root_eps[r])^tc_root_pow[r] + tc_const
     * terminal_cost_terms != 0: every QP carries the exact gradient of V_nq at its linearisation point (the Hessian
     * stays 2P: the root terms are concave away from 0), and ftmpc_eval_cost_batch includes V_nq -- the two pieces of
     * the line-search SQP towards the reference's nonlinear program (ft_mpc_amd.BatchedMPC.solve_sqp).
     */
    int32_t terminal_cost_terms;
    int32_t tc_npoly, tc_nroot, tc_reserved;
    double tc_poly_coef[FTMPC_MAX_TCOST_TERMS];
    int32_t tc_poly_exp[FTMPC_MAX_TCOST_TERMS * FTMPC_NOPT];
    double tc_root_coef[FTMPC_MAX_TCOST_TERMS];
    double tc_root_eps[FTMPC_MAX_TCOST_TERMS];
    double tc_root_pow[FTMPC_MAX_TCOST_TERMS];
    int32_t tc_root_exp[FTMPC_MAX_TCOST_TERMS * FTMPC_NOPT];
    double tc_const;
    /*
     * Implementation switches (diagnostics and A/B runs; 0 = the library's choice everywhere).  They live here, per handle:
     * the library reads no environment variable and keeps no process-global state.
     *   kernel_select   FTMPC_KERNEL_AUTO | FTMPC_KERNEL_DENSE | FTMPC_KERNEL_WORKGROUP | FTMPC_KERNEL_RICCATI: with DENSE the Newton systems
     *                   are always factorised in the thruster variables (kernel 7 / the dense float64 kernel) even where the
     *                   library would go through the 6N-variable wrench-space form (kernel 8 / its float64 sibling); with
     *                   RICCATI the thruster form with the terminal set runs on the Riccati kernel for every N <= 40, also
     *                   where AUTO keeps the dense float64 kernel (N * NT <= 256) -- everything else is routed as with AUTO
     *   lin_split_max   batch size up to which the linearisation is split by tangent direction (0: library default 8192;
     *                   < 0: never split)
     *   stage_chunks    ranges the host-buffer entry point stages a batch in (0: whole blocks of 65 536 instances; 1..8)
     */
    int32_t kernel_select;
    int32_t stage_chunks;
    int64_t lin_split_max;
    /*
     * State bounds  xlb <= c_k <= xub  on the orbit-centre state [p, v, omega, q] of the stages k = 1 .. N-1 (the reference's
     * optional params "xub" / "xlb", spiraling_mpc.py:129-130,179-185: `con_ineq.append(x_t)` for t < N; the row of stage 0 does not
     * depend on the decision variables).  state_bounds != 0 adds them to the thruster-space QP of ftmpc_solve_batch; a component
     * with |bound| >= FTMPC_NO_BOUND has no row.  The solve then runs in float64 on the Riccati kernel whatever the dtype (N <= 40,
     * no terminal set; kernel_select is ignored): there the rows are a diagonal barrier term on the state weight of their stage,
     * not dense rows through the sensitivities.  Bounds that cannot be met within the horizon end with FTMPC_STATUS_MAXITER /
     * _NUMERIC (the reference logs IPOPT's failure and carries on, spiraling_mpc.py:347-352).
     * The generalized-force formulation (ftmpc_solve_wrench_batch and the closed loops built on it) carries the same rows: a
     * state-bound handle runs its whole batch in float64 on the Riccati kernel of that formulation whatever the dtype; with
     * kernel_select = FTMPC_KERNEL_DENSE those entries return FTMPC_ERR_ARG (the dense kernel has no state rows), and so do the
     * entries of the generalized-force SQP.  No entry accepts a state-bound handle without applying the rows.
     */
    int32_t state_bounds;
    int32_t sb_reserved;
    double xlb[FTMPC_NX];
    double xub[FTMPC_NX];
} ftmpc_config;
#define FTMPC_NO_BOUND 1e300

#define FTMPC_KERNEL_AUTO 0
#define FTMPC_KERNEL_DENSE 1
#define FTMPC_KERNEL_WORKGROUP 2   /* the wrench-space form on a 4-wave workgroup per instance (kernel 8) where the library would
                                      give the instance one wave (kernel 10) */
#define FTMPC_KERNEL_RICCATI 3     /* ftmpc_solve_ric64_kernel (Riccati recursion, one wave per instance) where the library would take the
                                      dense float64 kernel for the thruster form with the terminal set (N <= 40); otherwise as AUTO */

typedef struct ftmpc_handle ftmpc_handle;

/* Fills *cfg with the reference constants for (N, NT) and struct_size.  NT==16 gets the reference D
 * (sys_model.py:73-123); any other NT leaves D zero for the caller to fill. */
int ftmpc_default_config(ftmpc_config* cfg, int32_t N, int32_t NT);

/* Creates a solver bound to cfg->device_id.  Fails (FTMPC_ERR_NODEVICE) when no gfx950
 * device is present: there is no CPU fallback in this library. */
int ftmpc_create(const ftmpc_config* cfg, ftmpc_handle** out);
int ftmpc_destroy(ftmpc_handle* h);
const char* ftmpc_last_error(const ftmpc_handle* h); /* h may be NULL: last create error */

/* Pre-allocates device workspace for batches up to max_batch (optional; solve calls grow
 * the workspace on demand, which allocates and must not happen inside a timed region). */
int ftmpc_reserve(ftmpc_handle* h, int64_t max_batch);

/*
 * One MPC step for B independent instances -- the batched form of get_control()
 * (spiraling_mpc.py:288-317) up to and including the thruster command.  HOST buffers.
 *
 *   x0      [B*13]        robot states
 *   ub      [B*NT]        per-thruster upper bound, 0 for a broken thruster (u_ub_physical,
 *                         sys_model.py:237-240)
 *   stuck   [B*NT]        intensity*f_max for a broken thruster else 0 (faulty_force,
 *                         sys_model.py:236)
 *   xref    [9*(N+1)] if xref_stride==0 (shared) else [B*xref_stride]; column-major 9 x (N+1)
 *                         exactly the reference's x_sp (spiraling_mpc.py:295)
 *   uref    NULL (== hover, u_ref = 0) or as xref with 6 x (N+1)   (spiraling_mpc.py:296)
 *   warmU   NULL (cold start: linearise about thrusters-off) or [B*N*NT] in/out: on entry the
 *           previous solution ALREADY shifted by the caller's policy (the reference shifts by
 *           one stage, spiraling_mpc.py:324-334; ftmpc_shift_warm does that); on exit U*.
 *   out_u0  [B*NT]        thruster forces of stage 0 (0 at broken thrusters)
 *   out_U   NULL or [B*N*NT]
 *   status  NULL or [B]   FTMPC_STATUS_*
 *   iters   NULL or [B]   IPM iterations run
 */
int ftmpc_solve_batch(ftmpc_handle* h, int64_t B,
                      const double* x0, const double* ub, const double* stuck,
                      const double* xref, int64_t xref_stride,
                      const double* uref, int64_t uref_stride,
                      double* warmU,
                      double* out_u0, double* out_U,
                      int32_t* status, int32_t* iters);

/*
 * Value of the NONLINEAR program's cost for given thruster sequences -- the merit function of the line-search SQP:
 * nonlinear RK4 rollout of the orbit-centre model from robot_to_center(x0) under U (spiral_model.py:44-76,
 * sys_model.py:138-162), then
 *     sum_{k=1}^{N-1} e_k'Q e_k + V(e_N) + sum_{k<N} [ut_k'R ut_k + rho |u_k|^2],   V(e) = e'P e [+ V_nq(e) when
 * terminal_cost_terms != 0],  ut_k = D (u_k + stuck) - [Rot(q_k)^T uref_k[0:3]; uref_k[3:6]] - [f_virt; 0]
 * (spiraling_mpc.py:156-171,188,196; q_k is the rollout's own quaternion, as the decision-variable quaternion is there).
 *   U [B*N*NT] thruster forces (entries of broken thrusters are ignored);  out_cost [B].   HOST buffers.
 */
int ftmpc_eval_cost_batch(ftmpc_handle* h, int64_t B,
                          const double* x0, const double* ub, const double* stuck,
                          const double* xref, int64_t xref_stride,
                          const double* uref, int64_t uref_stride,
                          const double* U, double* out_cost);

/*
 * Line-search sequential QP towards the reference's NONLINEAR program (nonlinear RK4 dynamics, full terminal cost when
 * terminal_cost_terms != 0; spiraling_mpc.py:87-238 as IPOPT solves it, :346), entirely on the device: per major iteration
 * one QP step linearised about the current thruster sequences U (ftmpc_solve_batch's QP; Hessian 2 (B'QB + R + rho I) with
 * the quadratic terminal weight, gradient exact), then backtracking alpha = 1, 1/2, ... (`backtracks` trial points) along
 * clip(U_qp) - U on the TRUE cost (ftmpc_eval_cost_batch's kernel) until it decreases by more than tol (1 + |J|); an
 * instance without such a step stops.  Nothing crosses PCIe between the upload of the inputs and the download of the results.
 *   warmU         NULL (start from thrusters off) or [B*N*NT] start sequences (clipped to the bounds)
 *   out_cost / out_cost0   [B] cost of the returned sequences / of the start point;  out_sqp_iters [B] major iterations that
 *   made progress;  out_iters [B] interior-point iterations summed;  status [B] of the last QP.   HOST buffers.
 */
int ftmpc_solve_sqp_batch(ftmpc_handle* h, int64_t B,
                          const double* x0, const double* ub, const double* stuck,
                          const double* xref, int64_t xref_stride,
                          const double* uref, int64_t uref_stride,
                          const double* warmU, int32_t sqp_iters, int32_t backtracks, double tol,
                          double* out_u0, double* out_U, double* out_cost, double* out_cost0,
                          int32_t* out_sqp_iters, int32_t* out_iters, int32_t* status);

/* ftmpc_solve_sqp_batch is a few hundred small launches per call; a call that repeats the previous call's shape (batch size,
 * strides, warm start or not, iteration counts, tolerance; the same handle constants, no workspace growth in between) is recorded
 * into a hipGraph the second time and replayed with one launch from the third on -- for batches up to 512 instances, where it
 * pays (FTMPC_SQP_GRAPH=1 in the environment: for every batch size; =0: never; profiling keeps the direct launches too).  Returns how many calls of this handle were replayed from a graph (diagnostic; -1: NULL). */
int64_t ftmpc_sqp_graph_launches(const ftmpc_handle* h);

/* Same contract with DEVICE pointers (HBM-resident inputs/outputs) enqueued on `stream`
 * (a hipStream_t passed as void*; NULL = the default stream).  Asynchronous: returns after
 * enqueue.  warmU is read only; pass the same buffer as out_U to update it in place. */
int ftmpc_solve_batch_device(ftmpc_handle* h, int64_t B,
                             const double* x0, const double* ub, const double* stuck,
                             const double* xref, int64_t xref_stride,
                             const double* uref, int64_t uref_stride,
                             const double* warmU,
                             double* out_u0, double* out_U,
                             int32_t* status, int32_t* iters,
                             void* stream);

/*
 * The reference's own two-stage structure: one MPC step in the 6-D GENERALIZED-FORCE space with the
 * input hull as constraint (spiraling_mpc.py:133-137,175-177; controllers/tools/input_bounds.py:43-76), followed by the
 * min-norm thruster allocation (control_allocator.py:65-94).  Per instance
 *     decision  tau_k in R^6, k < N: the TOTAL generalized force on the body ( = the reference's u_t + u_r + u_comp + D f_fault )
 *     cost      as ftmpc_solve_batch with ut_k = tau_k - ur_k - [f_virt;0] ( = the reference's deviation input u_t ), no rho term
 *     s.t.      hull_A tau_k <= hull_b  for every stage  [+ the terminal set when the handle's config has terminal_set != 0]
 * and u0 = argmin |u|^2 s.t. D u = tau_0 - D stuck, 0 <= u <= ub.  Needs N <= 40 and hull_rows <= FTMPC_MAX_HULL_ROWS (with
 * kernel_select = FTMPC_KERNEL_DENSE or N > 40: 6 N <= 256, hull_rows <= 32, N * hull_rows <= 1024).
 * Every converged interior-point iterate is finished by an active-set polish (the exact solution on the active set the iterate
 * identifies, its multiplier and slack signs verified; each polish round that factorises counts in iters[]): the float64 kernels
 * return the oracle's polished solution to 1e-9 f_max.  Routing: dtype FTMPC_DTYPE_F32 with N <= 16 and hull_rows <= 32 runs on one
 * fp32 wave per instance (ftmpc_solve_hull32_kernel; measured on 8 192 boundary vehicles: 1.4e-6 f_max worst; specification 1e-4
 * f_max on wrenches and on the allocated thrust command) and hands what it does not certify to the float64 path inside the same
 * call (ftmpc_last_handed_over); everything else -- float64 handles, N up to 40, up to 128 hull rows, with or without the terminal
 * set -- on ftmpc_solve_ricw64_kernel (float64, Riccati recursion, one wave per instance).
 *   hull_A    [n_sets][hull_rows*6] row-major facet normals, one table per fault INDEX SET (the normals do not depend on
 *             the fault intensities);  hull_set [B] table number of every instance (NULL: table 0 for all)
 *   hull_b    [B*hull_rows] facet offsets (they carry the intensities: b = n . D (ub/2 + stuck) + sum_i |n . D_i| ub_i / 2);
 *             pad unused rows with a zero normal and b = 1
 *   warmG     NULL (linearise about thrusters off: tau = D stuck) or [B*N*6] in/out: previous wrench solution, already shifted
 *   out_u0    [B*NT] allocated thruster forces;  out_tau0 NULL or [B*6];  out_G NULL or [B*N*6] whole-horizon wrenches
 *   status / iters: IPM (as above);  alloc_status NULL or [B]: as ftmpc_allocate_batch
 * A handle with state_bounds != 0: the rows xlb <= c_k <= xub of the stages 1 .. N-1 are part of the program (linearised about warmG
 * as everything else; iteration to mu 1e-10 unless mu_stop is set, no active-set polish); FTMPC_ERR_ARG with kernel_select =
 * FTMPC_KERNEL_DENSE.
 * HOST buffers.
 */
int ftmpc_solve_wrench_batch(ftmpc_handle* h, int64_t B,
                             const double* x0, const double* ub, const double* stuck,
                             const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                             const double* xref, int64_t xref_stride,
                             const double* uref, int64_t uref_stride,
                             double* warmG,
                             double* out_u0, double* out_tau0, double* out_G,
                             int32_t* status, int32_t* iters, int32_t* alloc_status);

/*
 * Cost of the NONLINEAR program in the generalized-force formulation for given wrench sequences -- the merit function of
 * ftmpc_solve_sqp_wrench_batch: nonlinear RK4 rollout of the orbit-centre model from robot_to_center(x0) under gen_k = tau_k, then
 *     sum_{k=1}^{N-1} e_k'Q e_k + V(e_N) + sum_{k<N} ut_k'R ut_k,   ut_k = tau_k - [Rot(q_k)^T uref_k[0:3]; uref_k[3:6]] - [f_virt; 0]
 * (V as ftmpc_eval_cost_batch; no rho term, as the wrench QP has none), and the violation of the terminal set
 *     sum_r max(0, (term_A e_N - term_b)_r)   (0 when the handle has no terminal set).
 *   G [B*N*6] total wrenches;  out_cost [B];  out_tviol NULL or [B].  ub and stuck may be NULL (the cost of a total wrench does
 *   not depend on them; the arguments keep the shape of ftmpc_eval_cost_batch).   HOST buffers.
 */
int ftmpc_eval_cost_wrench_batch(ftmpc_handle* h, int64_t B,
                                 const double* x0, const double* ub, const double* stuck,
                                 const double* xref, int64_t xref_stride,
                                 const double* uref, int64_t uref_stride,
                                 const double* G, double* out_cost, double* out_tviol);

/*
 * Line-search sequential QP towards the reference's NONLINEAR program in its own formulation (spiraling_mpc.py:87-238: the 6-D
 * generalized force as decision, the input hull at every stage, the terminal set, the full terminal cost, RK4 dynamics; IPOPT at
 * :346).  Iterate G = (tau_0 .. tau_{N-1}), started at warmG (NULL: tau_k = D stuck; warmG is assumed inside the hull, as the shifted
 * previous solution is).  Per major iteration: the QP of ftmpc_solve_wrench_batch linearised about G (same routing; Hessian with the
 * quadratic terminal weight, gradient exact), then the trial points G + 2^-j (G_qp - G), j < backtracks, all evaluated in one launch,
 * the first with merit below phi - tol (1 + |phi|) accepted, on the merit
 *     phi(G) = J(G) + sigma * violation(G)      (J and the violation of ftmpc_eval_cost_wrench_batch)
 * (the hull rows hold at G and at G_qp, so they stay out of the merit).  An instance without an acceptable point, or whose QP ends
 * with FTMPC_STATUS_NUMERIC, stops.  After the last iteration, once: u0 = min-norm allocation of tau_0 - D stuck (on an fp32 handle
 * tau_0 is first pulled towards the hull centre by a relative 1e-8, as ftmpc_solve_wrench_batch's fp32 kernel does).  Direct launches on
 * the handle's stream (no graph replay).  Refuses a handle with state_bounds != 0 (FTMPC_ERR_ARG: the wrench kernels have no state rows).
 *   hull_A .. hull_rows, xref .. uref_stride: as ftmpc_solve_wrench_batch;  warmG NULL or [B*N*6] (read only)
 *   sqp_iters >= 0, backtracks >= 1, tol >= 0;  penalty: sigma (<= 0: the library default, 1e5)
 *   out_u0 [B*NT];  out_tau0 NULL or [B*6];  out_G NULL or [B*N*6];  out_X NULL or [B*(N+1)*13] centre states of the rollout under the
 *   returned G (stage 0 = robot_to_center(x0));  out_cost / out_cost0 / out_tviol NULL or [B]: J of the returned G / of the start point,
 *   violation of the returned G;  out_sqp_iters [B] major iterations that made progress;  out_iters [B] interior-point iterations
 *   summed;  status [B] of the last QP;  alloc_status [B] as ftmpc_allocate_batch.  Each output but out_u0 may be NULL.   HOST buffers.
 */
int ftmpc_solve_sqp_wrench_batch(ftmpc_handle* h, int64_t B,
                                 const double* x0, const double* ub, const double* stuck,
                                 const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                 const double* xref, int64_t xref_stride,
                                 const double* uref, int64_t uref_stride,
                                 const double* warmG, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                 double* out_u0, double* out_tau0, double* out_G, double* out_X,
                                 double* out_cost, double* out_cost0, double* out_tviol,
                                 int32_t* out_sqp_iters, int32_t* out_iters, int32_t* status, int32_t* alloc_status);

/* Number of instances of the LAST ftmpc_solve_wrench_batch / ftmpc_simulate_wrench_batch step on this handle that the one-wave fp32
 * kernel handed over to the float64 kernel (its active-set polish did not settle, or hull and terminal rows were active together);
 * 0 where the float64 kernel solved the whole batch anyway.  Blocks until that step's kernels have finished. */
int ftmpc_last_handed_over(ftmpc_handle* h, int64_t* count);

/*
 * Batched thruster allocation: the reference's second stage,
 * ControlAllocator.get_physical_input (ft_mpc/controllers/tools/control_allocator.py:27-40,65-94):
 *     min |u|^2   s.t.  D u = tau,  0 <= u <= ub
 * with the handle's D (6 x NT).  The thruster-space MPC step does not call it (its QP allocates
 * inside); it serves callers that hold a generalized force, as the reference's controller does.
 * HOST buffers.
 *   tau     [B*6]    generalized force to realise with the healthy thrusters (the reference passes
 *                    u_des, i.e. the controller output with the faulty wrench already removed)
 *   ub      [B*NT]   upper bounds, 0 for a broken thruster (u_ub_physical, sys_model.py:237-240)
 *   out_u   [B*NT]   thruster forces
 *   status  NULL or [B]: 0 solved (|D u - tau|_inf <= 1e-8 (1 + |tau|_inf)), 1 iteration cap,
 *                    2 tau not attainable (least-residual u returned; the reference prints and
 *                    exit()s here, control_allocator.py:88-93)
 *   iters   NULL or [B]: Newton steps taken
 */
int ftmpc_allocate_batch(ftmpc_handle* h, int64_t B, const double* tau, const double* ub,
                         double* out_u, int32_t* status, int32_t* iters);

/* Shifts a [B*N*NT] host warm-start buffer by one stage in place, zero-filling the last
 * stage (spiraling_mpc.py:327-329). */
int ftmpc_shift_warm(int64_t B, int32_t N, int32_t NT, double* warmU);

/*
 * T closed-loop steps for B independent vehicles entirely on the device -- the batched form of
 * SimulationEnvironment.run_simulation (ft_mpc/simulation/sim_env.py:77-112) around get_control:
 * per step  u = MPC step (warm-started from the shifted previous solution, spiraling_mpc.py:324-334),
 * x <- RK4 plant step with u (sys_model.py:138-226), x += U(0, noise) per component (sim_env.py:88-91,
 * here from a counter-based generator keyed by `seed` instead of the unseeded global RNG), quaternion
 * renormalised (sim_env.py:93).  HOST buffers; nothing crosses PCIe between steps.
 *   x            [B*13]  in: initial states, out: final states
 *   xref_traj    9 x (T+N) column-major, shared by all vehicles: step t tracks columns t..t+N
 *                (the padded trajectory of assign_trajectory, spiraling_mpc.py:255-286)
 *   uref_traj    NULL (hover) or 6 x (T+N) column-major
 *   noise        amplitudes {position, velocity, orientation, angular velocity} (sim_env.py:25-30: 1e-3 each)
 *   u_hist       NULL or [T*B*NT]: applied thruster commands
 *   not_converged NULL or [T]: number of instances whose IPM status was not 0 at each step
 */
int ftmpc_simulate_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                         const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                         double* u_hist, int32_t* not_converged);

/* The same closed loop with the NONLINEAR program solved at every step (sqp_iters > 0: that many major iterations of the
 * line-search SQP of ftmpc_solve_sqp_batch, started from the shifted previous solution; sqp_iters = 0: ftmpc_simulate_batch). */
int ftmpc_simulate_batch_ex(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                            const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                            int32_t sqp_iters, int32_t backtracks, double tol, double* u_hist, int32_t* not_converged);

/* The same closed loop in the reference's TWO-STAGE structure (ftmpc_solve_wrench_batch at every step: generalized-force MPC with
 * the input hull -- and the terminal set when the handle's config has one -- then the min-norm allocation): the wrench warm start
 * is the previous solution shifted by one stage with its last stage repeated.  The hull tables are those of
 * ftmpc_solve_wrench_batch and stay fixed over the run (faults that start mid-run: ftmpc_simulate_wrench_faults_batch).
 * State bounds of the handle apply at every step, as in ftmpc_solve_wrench_batch.
 *   alloc_failed  NULL or [T]: number of instances whose allocation status was not 0 at each step */
int ftmpc_simulate_wrench_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                double* u_hist, int32_t* not_converged, int32_t* alloc_failed);

/* ftmpc_simulate_wrench_batch with the NONLINEAR program solved at every step: sqp_iters > 0 major iterations of
 * ftmpc_solve_sqp_wrench_batch (backtracks, tol, penalty as there), started from the previous wrench solution shifted by one stage with
 * its last stage repeated; not_converged counts the status of each instance's last QP.  sqp_iters = 0: ftmpc_simulate_wrench_batch.
 * A handle with state_bounds != 0 is refused for sqp_iters > 0 only (FTMPC_ERR_ARG: the SQP has no state rows). */
int ftmpc_simulate_wrench_batch_ex(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                   const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                   const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                   int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                   double* u_hist, int32_t* not_converged, int32_t* alloc_failed);

/*
 * Thruster faults that start mid-run: a schedule of up to E = n_events fault events per vehicle for the closed loops above.
 * Event e of vehicle b carries the FULL pattern after the event (ub / stuck as BrokenThruster / SystemModel.set_fault leave them,
 * sys_model.py:237-250), an onset step and a detection step detect >= onset:
 *   - onset[b*E+e] = -1 marks an unused slot; used slots come first and are non-decreasing in onset and in detect.  An onset >= T
 *     never fires.
 *   - at loop step t the PLANT integrates with the pattern of the last event with onset <= t (none: the call's ub / stuck), applying
 *     (ub > 0 ? u : 0) + stuck as always: between onset and detection the controller may command a thruster that is dead in the plant.
 *   - at loop step t the CONTROLLER solves with the pattern of the last event with detect <= t (none: the call's ub / stuck); on the
 *     wrench form that includes the event's hull table number hull_set[b*E+e] (indexing the call's hull_A) and offsets
 *     hull_b[(b*E+e)*hull_rows ..].  The switch happens before step t's solve.
 *   - when the controller's pattern changes at a step t > 0 the shifted warm start is repaired: thruster form (one QP or SQP) U
 *     clipped elementwise to [0, ub_new]; wrench form (one QP or SQP) every stage of G pulled towards the new hull centre
 *     D (ub_new/2 + stuck_new) by the smallest factor that leaves every new facet a relative margin of 1e-8 (the tau_0 rule of
 *     ftmpc_solve_sqp_wrench_batch, applied per stage; a stage that keeps the margin is not moved).  The wrench SQP needs this: its
 *     warm start must lie inside the hull.
 * All buffers are HOST buffers, staged once per call.  A NULL schedule or n_events = 0 is exactly the loop without one.
 */
#define FTMPC_MAX_FAULT_EVENTS 8
typedef struct ftmpc_fault_schedule {
    int32_t struct_size;      /* sizeof(ftmpc_fault_schedule) */
    int32_t n_events;         /* E, 0 <= E <= FTMPC_MAX_FAULT_EVENTS */
    const int32_t* onset;     /* [B*E] */
    const int32_t* detect;    /* NULL (detect = onset) or [B*E] */
    const double* ub;         /* [B*E*NT] >= 0, finite */
    const double* stuck;      /* [B*E*NT] finite */
    const int32_t* hull_set;  /* wrench form: NULL exactly when the call's hull_set is NULL (one table), else [B*E] in [0, n_sets) */
    const double* hull_b;     /* wrench form: [B*E*hull_rows] */
} ftmpc_fault_schedule;

/* ftmpc_simulate_batch_ex with the fault schedule `faults` (NULL: none) and
 *   x_hist  NULL or [T*B*13]: the state after each step, after noise and renormalisation (x_hist[T-1] is the returned x).
 * u_hist keeps its meaning: what the controller commanded. */
int ftmpc_simulate_faults_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                double* u_hist, double* x_hist, int32_t* not_converged);

/* ftmpc_simulate_wrench_batch_ex with the fault schedule `faults` (NULL: none; its hull_b is required when n_events > 0) and x_hist as
 * ftmpc_simulate_faults_batch.  State bounds of the handle: as ftmpc_simulate_wrench_batch_ex. */
int ftmpc_simulate_wrench_faults_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                       const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                       const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                       int32_t sqp_iters, int32_t backtracks, double tol, double penalty, const ftmpc_fault_schedule* faults,
                                       double* u_hist, double* x_hist, int32_t* not_converged, int32_t* alloc_failed);

/*
 * Per-vehicle outcomes of a fault campaign, reduced on the device while the closed loop runs, so that a caller who wants to know
 * which vehicles recovered, when, and at what cost needs neither x_hist nor u_hist (3.3 GB at B = 65 536, T = 300, NT = 8; the
 * records below are 84 bytes per vehicle).  Per loop step t, with x_{t+1} the state after the step (after noise and
 * renormalisation), e = robot_to_center(x_{t+1})[0:9] - xref_traj[:, t+1] (spiral_model.py:91-109) and ep, ev, ew the Euclidean
 * norms of e[0:3], e[3:6], e[6:9]:
 *   err_int        [B*3]  sum_t dt ep^2, sum_t dt ev^2, sum_t dt ew^2, added in step order
 *   err_max        [B*3]  max_t ep, ev, ew
 *   impulse        [B*2]  sum_t dt sum_i a_i  and  sum_t dt sum_i c_i, with c_i = ub_i > 0 ? u_i : 0 what was commanded of a live
 *                         thruster and a_i = c_i + stuck_i what the plant applied (sys_model.py:198-208); ub / stuck are the PLANT's
 *                         pattern of step t (under a fault schedule: of the last event with onset <= t)
 *   settle_step    [B]    smallest s in [0, T] with ep <= tol_pos, ev <= tol_vel and ew <= tol_rate at every step t >= s (the last
 *                         step outside the band + 1): 0 inside throughout, T not settled at the end
 *   tset_step      [B]    first step t with term_A e <= term_b on all term_rows rows of the handle's config, -1 never.  The rows of
 *                         the config whether or not terminal_set is on; asked for with term_rows = 0: FTMPC_ERR_ARG
 *   unsolved       [B]    number of steps whose solve status (the SQP's last QP where an SQP ran) was not 0
 *   first_unsolved [B]    the first such step, -1 none
 *   alloc_failed   [B]    wrench form: number of steps whose allocation status was not 0.  Thruster form: FTMPC_ERR_ARG if non-NULL
 *   status_hist    [T*B]  a history, not a record: the solve status of every instance at every step
 * Each output is NULL (not wanted) or a HOST buffer of that size.  With every output NULL nothing is added to the loop's launches.
 * index0 / index_total: this call's vehicles are [index0, index0 + B) of a campaign of index_total vehicles.  The measurement noise
 * of vehicle b at step t, component i is drawn at counter (t * index_total + index0 + b) * 13 + i, so slices of a campaign run as
 * separate calls (on other handles, devices or processes) draw exactly what the same vehicles draw in one call over the whole
 * campaign.  0 / 0 means 0 / B: the call is the campaign, the counter of the entries without this struct.
 * FTMPC_ERR_ARG, the message naming the field: a struct_size other than sizeof(ftmpc_outcomes); index0 < 0; index_total != 0 with
 * index0 + B > index_total; settle_step with a tolerance that is not positive and finite.
 */
typedef struct ftmpc_outcomes {
    int32_t struct_size;      /* sizeof(ftmpc_outcomes) */
    int32_t reserved;
    int64_t index0, index_total;
    double tol_pos, tol_vel, tol_rate;   /* settle band; read only when settle_step is asked for */
    double* err_int;
    double* err_max;
    double* impulse;
    int32_t* settle_step;
    int32_t* tset_step;
    int32_t* unsolved;
    int32_t* first_unsolved;
    int32_t* alloc_failed;
    int32_t* status_hist;
} ftmpc_outcomes;

/* ftmpc_simulate_faults_batch with the outcomes `out` (NULL: exactly ftmpc_simulate_faults_batch). */
int ftmpc_simulate_outcomes_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                  const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                  int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                  double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out);

/* ftmpc_simulate_wrench_faults_batch with the outcomes `out` (NULL: exactly ftmpc_simulate_wrench_faults_batch). */
int ftmpc_simulate_wrench_outcomes_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                         const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                         const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                         int32_t sqp_iters, int32_t backtracks, double tol, double penalty, const ftmpc_fault_schedule* faults,
                                         double* u_hist, double* x_hist, int32_t* not_converged, int32_t* alloc_failed,
                                         const ftmpc_outcomes* out);

/*
 * Plant dispersion: the plant that the closed loop integrates, per vehicle, while the CONTROLLER keeps the nominal model of the
 * handle's config everywhere (linearisation, cost, hulls, allocation, robot_to_center, the reference of the outcomes).  Vehicle b has
 * a plant mass m_b, a plant inertia J_b (3 x 3, symmetric positive definite), a plant allocation matrix D_b (6 x NT), a constant
 * disturbance force f_b in the inertial frame and a constant disturbance torque t_b in the body frame.  With
 * a_i = (ub_i > 0 ? u_i : 0) + stuck_i, exactly as without this struct and taken from the plant's pattern of that step under a fault
 * schedule:
 *   [F; tau] = D_b a
 *   p' = v
 *   v' = (Rot(q)^T F + f_b) / m_b
 *   q' = 1/2 Omega(w) q
 *   w' = J_b^-1 (tau + t_b - w x J_b w)
 * RK4 over dt holds a, f_b and t_b constant.  The noise, its counter, the renormalisation, u_hist, x_hist and not_converged are those
 * of the entries without this struct.  An array that is NULL takes the handle's value for every vehicle: cfg.mass, cfg.J, cfg.D,
 * zero force, zero torque.  `impulse` of ftmpc_outcomes keeps its meaning of thruster force a_i: a gain error of a thruster lives in
 * D_b (a scaled column), not in a.  All arrays are HOST buffers, vehicle-major, so a shard of a campaign is a pointer offset.
 * plant = NULL, or a struct whose five arrays are all NULL, launches exactly the kernels of the _outcomes_ entries.
 * FTMPC_ERR_ARG, the message naming the field and the first offending vehicle: a struct_size other than sizeof(ftmpc_plant_model); a
 * mass that is not finite or not positive; a J that is not finite, not symmetric to 1e-12 of its largest entry or not positive
 * definite (leading minors); a non-finite entry of D, force or torque.
 */
typedef struct ftmpc_plant_model {
    int32_t struct_size;   /* sizeof(ftmpc_plant_model) */
    int32_t reserved;
    const double* mass;    /* NULL or [B]        > 0, finite */
    const double* J;       /* NULL or [B*9]      row-major, symmetric positive definite */
    const double* D;       /* NULL or [B*6*NT]   row-major 6 x NT per vehicle, row stride NT */
    const double* force;   /* NULL or [B*3]      inertial frame */
    const double* torque;  /* NULL or [B*3]      body frame */
} ftmpc_plant_model;

/* ftmpc_simulate_outcomes_batch with the plant model `plant` (NULL: exactly ftmpc_simulate_outcomes_batch). */
int ftmpc_simulate_plant_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                               const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                               int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                               double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                               const ftmpc_plant_model* plant);

/* ftmpc_simulate_wrench_outcomes_batch with the plant model `plant` (NULL: exactly ftmpc_simulate_wrench_outcomes_batch). */
int ftmpc_simulate_wrench_plant_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                      const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                      const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                      int32_t sqp_iters, int32_t backtracks, double tol, double penalty, const ftmpc_fault_schedule* faults,
                                      double* u_hist, double* x_hist, int32_t* not_converged, int32_t* alloc_failed,
                                      const ftmpc_outcomes* out, const ftmpc_plant_model* plant);

/*
 * Reference missions and the closed-loop cost.  A mission is K reference tables and, per vehicle, a table number and a start column:
 * table k is xref [9 x C] column-major (orbit-centre [p, v, omega], exactly the columns of xref_traj) and optionally uref [6 x C].
 * Vehicle b has table[b] in [0, K) and offset[b] >= 0; at loop step t its solve tracks the columns offset[b] + t .. offset[b] + t + N
 * of its table, for xref and uref alike, and every outcome and tset_step take
 *   e = robot_to_center(x_{t+1})[0:9] - column offset[b] + t + 1   of its table.
 * offset[b] + T + N <= C is required: a table does not wrap around.  Everything else in the loop (warm-start shift, fault events and
 * warm-start repair, plant or dispersed plant, noise counter, histories) is as without the struct.  The tables are shared by the
 * vehicles and uploaded once per call; a kernel gathers every vehicle's window [9 (N+1)] (and [6 (N+1)] with uref) before each solve
 * into buffers of the call: 120 (N+1) bytes per vehicle, 2.5 KB at N = 20, 165 MB at B = 65 536.
 * cost [B*3], accumulated in step order and not multiplied by dt (the controller's stage cost is not), with Q, R, P, D and f_virt of
 * the handle's config (a dispersed plant's D_b stays on the plant side):
 *   cost[b][0] = sum_t e_{t+1}' diag(Q) e_{t+1}
 *   cost[b][1] = sum_t w_t' diag(R) w_t,   w_t = D a_t - [Rot(q_t)^T uref_t[0:3]; uref_t[3:6]] - [f_virt; 0]
 *                a_i = (ub_i > 0 ? u_i : 0) + stuck_i from the PLANT's pattern of step t (the a_i of `impulse`), q_t the quaternion of
 *                the state step t started from (the call's x for t = 0, else the state after step t-1's noise and renormalisation),
 *                uref_t column offset[b] + t (zero without uref), rotated as ftmpc_eval_cost_batch rotates ur
 *   cost[b][2] = V(e_T), the terminal cost of the last step's error as ftmpc_eval_cost_batch defines V for the handle: e' P e, plus
 *                V_nq(e) when terminal_cost_terms != 0.  Zero for T = 0.
 * n_tables = 0: every vehicle tracks the call's xref_traj / uref_traj and the struct only asks for cost.  mission = NULL, or
 * n_tables = 0 with cost = NULL, launches exactly the kernels of the _plant_ entries and returns their bits.
 * FTMPC_ERR_ARG, the message naming the field and, where there is one, the first offending vehicle: a struct_size other than
 * sizeof(ftmpc_mission); n_tables < 0; with n_tables > 0: xref NULL, n_cols < T + N, the call's xref_traj or uref_traj not NULL, a
 * table[b] outside [0, K), an offset[b] < 0 or with offset[b] + T + N > n_cols, a non-finite table entry; with n_tables = 0: the
 * call's xref_traj NULL, table or offset not NULL.
 */
typedef struct ftmpc_mission {
    int32_t struct_size;      /* sizeof(ftmpc_mission) */
    int32_t n_tables;         /* K >= 0.  0: every vehicle tracks the call's xref_traj / uref_traj (the struct then only asks for cost) */
    int64_t n_cols;           /* C, columns of every table */
    const double* xref;       /* [K][9*C] */
    const double* uref;       /* NULL (hover on every table) or [K][6*C] */
    const int32_t* table;     /* NULL (table 0) or [B] */
    const int32_t* offset;    /* NULL (0) or [B] */
    double* cost;             /* NULL or [B*3], output */
} ftmpc_mission;

/* ftmpc_simulate_plant_batch with the mission `mission` (NULL: exactly ftmpc_simulate_plant_batch).  With n_tables > 0 xref_traj and
 * uref_traj must be NULL. */
int ftmpc_simulate_mission_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                 const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                 int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                 double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                 const ftmpc_plant_model* plant, const ftmpc_mission* mission);

/* ftmpc_simulate_wrench_plant_batch with the mission `mission` (NULL: exactly ftmpc_simulate_wrench_plant_batch). */
int ftmpc_simulate_wrench_mission_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                        const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                        const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                        int32_t sqp_iters, int32_t backtracks, double tol, double penalty, const ftmpc_fault_schedule* faults,
                                        double* u_hist, double* x_hist, int32_t* not_converged, int32_t* alloc_failed,
                                        const ftmpc_outcomes* out, const ftmpc_plant_model* plant, const ftmpc_mission* mission);

/*
 * Pulsed (PWM) thrusters and valve lag in the plant.  Without the struct every loop applies a_i = (ub_i > 0 ? u_i : 0) + stuck_i as a
 * force held constant over dt: an ideal proportional thruster.  With it the plant's step of loop step t is cut into S = substeps
 * sub-steps of h = dt / S (substeps = 0 is read as 1), each one RK4 step of length h of the right-hand side the plant kernels use
 * (m_b, J_b, D_b, f_b, t_b of the call's ftmpc_plant_model where given, the config's where not), under the force the valves deliver in
 * that sub-step.  ub_i / stuck_i are the PLANT's pattern of the step (under a fault schedule: of the last event with onset <= t), u_i
 * the command.  The parameters are uniform over the call.
 *   mode 0, proportional: the target of every sub-step j is g_ij = ub_i > 0 ? u_i : 0, unclipped as the plant kernels apply it.
 *   mode 1, PWM: duty d_i = ub_i > 0 ? min(max(u_i / ub_i, 0), 1) : 0, ticks k_i = floor(d_i S + 0.5), then k_i = 0 where k_i < min_on
 *     (the dead band: nothing rounds up); the on-window starts at tick s_i = 0 (align 0, leading), (S - k_i) / 2 in integer division
 *     (1, centred) or S - k_i (2, trailing); g_ij = ub_i for s_i <= j < s_i + k_i, else 0.  S is the PWM clock: on-times are whole
 *     ticks of h, and a pulse does not cross a step boundary.
 *   valve lag: every thruster has a valve state a_i (N), from `state` or 0 at entry, carried from sub-step to sub-step and from step
 *     to step.  With E_x = exp(-h / tau_x), K_x = -expm1(-h / tau_x) tau_x / h for x in {on, off} (E = K = 0 for tau_x = 0, no lag),
 *     computed on the host once per call: in sub-step j the pair (E, K) is the on-pair where g_ij > a_i, else the off-pair; the mean
 *     force of the sub-step is m_ij = g_ij + (a_i - g_ij) K, then a_i = g_ij + (a_i - g_ij) E.
 *   A jammed-open valve has no lag and no modulation: the thrust of the sub-step is m_ij + stuck_i, and [F; tau] = D_b (m_j + stuck)
 *   (plus t_b on the torque) is held over the sub-step.  After the S sub-steps the step ends as without the struct: the noise is added
 *   once at the same counter, the quaternion renormalised once; u_hist (the command), x_hist and not_converged keep their meaning.
 * The controller is not told: ftmpc_outcomes.impulse and ftmpc_mission.cost[1] stay command-level a_i = (ub_i > 0 ? u_i : 0) + stuck_i.
 * What the valves delivered comes back here.  Each output is NULL or a host buffer:
 *   delivered [B]          sum_t sum_j h sum_i (m_ij + stuck_i), N s, added in step and sub-step order
 *   pulses [B]             PWM only: the number of (step, thruster) pairs with k_i > 0 (valve wear)
 *   applied_hist [T*B*NT]  per step (1/S) sum_j (m_ij + stuck_i); summed over thrusters and steps, times dt, it gives delivered
 *   ticks_hist [T*B*NT]    PWM only: k_i
 *   state [B*NT]           in/out: the valve states, read at entry (finite, >= 0) and written at exit, so that a campaign continues
 *                          across calls; NULL starts at 0 and returns nothing.  Under PWM a state stays within [0, ub_i].  In
 *                          proportional mode the target is the unclipped command, so a command below 0 on a live thruster (solver
 *                          round-off) leaves a negative state, which the next call would refuse: clamp the returned states at 0
 *                          before handing them on (a valve does not deliver negative thrust)
 * actuator = NULL, or mode = 0 with substeps <= 1, both tau 0 and every output (state included) NULL, launches exactly the kernels of
 * the _mission_ entries and returns their bits.
 * FTMPC_ERR_ARG, the message naming ftmpc_actuator.<field> and, where there is one, the first offending vehicle, the call's x
 * untouched: a struct_size other than sizeof(ftmpc_actuator); mode outside {0, 1}; substeps outside [0, 64]; min_on < 0 or > S; align
 * outside {0, 1, 2}; a tau negative or not finite; mode = 0 with min_on != 0, align != 0, pulses or ticks_hist; a state entry negative
 * or not finite.
 */
typedef struct ftmpc_actuator {
    int32_t struct_size;      /* sizeof(ftmpc_actuator) */
    int32_t mode;             /* 0 proportional, 1 PWM */
    int32_t substeps;         /* S in [1, 64]; 0 is read as 1 */
    int32_t min_on;           /* ticks, 0 <= min_on <= S (PWM) */
    int32_t align;            /* 0 leading, 1 centred, 2 trailing (PWM) */
    int32_t reserved;         /* 0 */
    double tau_on, tau_off;   /* s, >= 0; 0: no lag */
    double* delivered;        /* NULL or [B], output */
    int32_t* pulses;          /* NULL or [B], output (PWM) */
    double* applied_hist;     /* NULL or [T*B*NT], output */
    int32_t* ticks_hist;      /* NULL or [T*B*NT], output (PWM) */
    double* state;            /* NULL or [B*NT], in/out */
} ftmpc_actuator;

/* ftmpc_simulate_mission_batch with the actuator `actuator` (NULL: exactly ftmpc_simulate_mission_batch). */
int ftmpc_simulate_actuator_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                  const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                  int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                  double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                  const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator);

/* ftmpc_simulate_wrench_mission_batch with the actuator `actuator` (NULL: exactly ftmpc_simulate_wrench_mission_batch). */
int ftmpc_simulate_wrench_actuator_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                         const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                         const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                         int32_t sqp_iters, int32_t backtracks, double tol, double penalty, const ftmpc_fault_schedule* faults,
                                         double* u_hist, double* x_hist, int32_t* not_converged, int32_t* alloc_failed,
                                         const ftmpc_outcomes* out, const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                         const ftmpc_actuator* actuator);

/* Navigation errors and command latency in the on-device closed loops.  Without this struct one buffer is both the plant's state
 * and the x0 of every solve, and the command solved from x_t acts over step t.  With it the plant keeps the TRUTH x_t in a buffer of
 * the call; the call's noise / seed keep acting on the truth (process noise); the outcome, mission-cost and actuator kernels read
 * the truth; x_hist and the returned x are the truth.  The controller is handed a measurement, and its command acts `latency` steps
 * later.  The parameters are uniform over the call, bias and pending are per vehicle.
 *   measurement y_t, formed before the solve of loop step t.  g = index0 + b is the vehicle's campaign number (ftmpc_outcomes), the
 *     channels are j = 0..11 (position, velocity, attitude, rate: 3 each), c = ((step0 + t) index_total + g) 12 + j the counter:
 *       u1 = u01(seed, 2c), u2 = u01(seed, 2c + 1) (the splitmix counter function of the process noise),
 *       z_j = sqrt(-2 log(1 - u1)) cos(2 pi u2)
 *       y_p = p + bias[b][0:3] + sigma[0] z_{0:3}         y_v = v + bias[b][3:6] + sigma[1] z_{3:6}
 *       theta = bias[b][6:9] + sigma[2] z_{6:9}, a body-frame rotation vector (rad):  y_q = cos(|theta|/2) q + s Omega(theta) q,
 *         s = sin(|theta|/2) / |theta| (0.5 below |theta| = 1e-8), Omega the operator of q' = 1/2 Omega(w) q; then y_q / |y_q|
 *       y_w = w + bias[b][9:12] + sigma[3] z_{9:12}
 *     bias NULL is zero; sigma[k] == 0 draws nothing for its group.
 *   latency d in [0, 8]: the plant applies a_t = u_{t-d} at step t; for t < d it applies row t of pending [B][d][NT] (NULL: zeros,
 *     so only `stuck` acts).  On return pending holds the d commands computed but not yet applied, oldest first.  u_hist[t],
 *     ftmpc_outcomes.impulse, ftmpc_mission.cost[1] and the actuator all see a_t, the command the plant applied in step t.
 *   predict = 1: from x^ = y_t, for j = 0..d-1 one RK4 step of dt of the CONTROLLER's model -- the config's mass, J and D, under
 *     gen = D ((ub_c > 0 ? a_{t+j} : 0) + stuck_c) with the controller's pattern of step t (after a detected fault event) -- and the
 *     quaternion renormalised after each step.  The solve of step t takes x0 = x^ and the reference window starting at column
 *     t + d: the trajectory arguments are then [9, T + N + L] and [6, T + N + L], L = predict ? d : 0, and under a mission
 *     offset + T + N + L <= n_cols.  Outcomes and cost keep column t + 1 of xref and column t of uref.  predict = 0: the solve takes
 *     y_t and the window at t.
 *   outputs (NULL or host buffers): meas_hist [T*B*13] the y_t, pred_hist [T*B*13] the x^_t.
 * sensor = NULL, or latency = 0, predict = 0, all sigma zero and bias, pending and both histories NULL, launches exactly the kernels
 * of the _actuator_ entries and returns their bits.
 * Continued runs: a run of T steps equals two runs of T / 2 with pending and step0 handed over, bit for bit where the solves do not
 * depend on the handle's history.  The queue and the counters travel in the struct; the solver's warm start stays on the handle:
 * every call with a non-trivial sensor keeps the warm start its last step shifted, the x it returned and step0 + T, and a call
 * whose step0 (> 0), B, form and x are exactly these warm-starts its first solve from what was kept (and repairs it at a fault
 * event of its step 0, as a later step would).  Any other call starts cold, as every call without a sensor does.
 * FTMPC_ERR_ARG, the message naming ftmpc_sensor.<field> and, for an array, the first offending vehicle, the call's x untouched: a
 * struct_size other than sizeof(ftmpc_sensor); latency outside [0, 8]; predict outside {0, 1}; a sigma negative or not finite; a
 * bias or pending entry not finite; pending given with latency = 0; pred_hist given with predict = 0; step0 < 0.
 */
#define FTMPC_MAX_LATENCY 8
typedef struct ftmpc_sensor {
    int32_t struct_size;      /* sizeof(ftmpc_sensor) */
    int32_t latency;          /* d, control periods, 0..FTMPC_MAX_LATENCY */
    int32_t predict;          /* 0: the solve takes y_t; 1: y_t propagated over the d queued commands */
    int32_t reserved;         /* 0 */
    uint64_t seed;            /* of the sensor noise (the call's seed is the process noise's) */
    int64_t step0;            /* number of the call's first step in the campaign (>= 0): a continued run draws on */
    double sigma[4];          /* standard deviations: position (m), velocity (m/s), attitude (rad), rate (rad/s) */
    const double* bias;       /* NULL (zero) or [B*12] */
    double* pending;          /* NULL (zeros; nothing returned) or [B*d*NT], in/out */
    double* meas_hist;        /* NULL or [T*B*13], output */
    double* pred_hist;        /* NULL or [T*B*13], output (predict = 1) */
} ftmpc_sensor;

/* ftmpc_simulate_actuator_batch with the sensor `sensor` (NULL: exactly ftmpc_simulate_actuator_batch). */
int ftmpc_simulate_sensor_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                const ftmpc_sensor* sensor);

/* ftmpc_simulate_wrench_actuator_batch with the sensor `sensor` (NULL: exactly ftmpc_simulate_wrench_actuator_batch). */
int ftmpc_simulate_wrench_sensor_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                       const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                       const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                       int32_t sqp_iters, int32_t backtracks, double tol, double penalty, const ftmpc_fault_schedule* faults,
                                       double* u_hist, double* x_hist, int32_t* not_converged, int32_t* alloc_failed,
                                       const ftmpc_outcomes* out, const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                       const ftmpc_actuator* actuator, const ftmpc_sensor* sensor);

/* A navigation filter between the sensor and the controller in the on-device closed loops: a multiplicative (error-state) extended
 * Kalman filter per vehicle (ftmpc_filter_kernel).  With it the solve of step t no longer reads the raw sample y_t but the filter's
 * estimate, and the measurement may come at a lower rate than the control.  The parameters are uniform over the call; xhat, cov
 * and the outputs are per vehicle.
 *   state: the mean x^ [13] in the layout of x, and the covariance P (12 x 12, symmetric) over the error coordinates
 *     delta = (dp, dv, dtheta, dw) of the retraction  x [+] delta = (p + dp, v + dv, rotate(q, dtheta), w + dw),  rotate the closed
 *     form of the sensor's attitude error (body-frame rotation vector, renormalised).  P travels packed: 78 doubles, the upper
 *     triangle row-major.
 *   residual y [-] x^ (12): differences for position, velocity and rate; for the attitude the theta with rotate(q^, theta) = y_q:
 *     c = q^ . y_q, s = Xi(q^)' y_q with Omega(theta) q = Xi(q) theta; c < 0 flips y_q; theta = 2 atan2(|s|, c) / |s| s, and
 *     theta = 2 s below |s| = 1e-8.
 *   measurement update (H = I, R = diag(meas_sigma[g]^2) by group): twelve sequential scalar updates in channel order j = 0..11 on
 *     d = 0:  sj = P_jj + R_j,  k = P[:, j] / sj,  d += k (r_j - d_j),  P -= sj k k';  then x^ <- x^ [+] d.  The covariance is not
 *     reset.  Exact for a diagonal R, no inverse; only the packed triangle is updated, so P stays symmetric by construction.
 *   time update with a_t, the command the plant applies in step t, under the controller's pattern of step t and the config's mass,
 *     J and D (the model of the sensor's prediction):  gen = D ((ub_c > 0 ? a_t : 0) + stuck_c),  Phi = I + dt A(x^_{t|t}, gen),
 *     P <- Phi P Phi' + diag(proc_sigma[g]^2),  then x^ <- one RK4 step of the model, renormalised.  A is the Jacobian of the error
 *     dynamics under the retraction; its non-zero blocks are (p, v) = I, (theta, w) = I, (v, theta) = -M [F/m]x with M(q) the
 *     body-to-inertial matrix of the model, (theta, theta) = -[w]x and (w, w) = J^-1 ([J w]x - [w]x J).
 *   per loop step t (campaign step c = step0 + t; step0 is the sensor's, 0 without one):
 *     1. ftmpc_sense_kernel forms y_t (without its prediction);
 *     2. on the first step of a call that was not handed xhat: x^ = y_t, P = diag(p0[g]^2), no update.  Otherwise the update runs
 *        when c % every == 0; when it does not, nothing is drawn from y_t.  est_hist[t] = x^_{t|t}; err_sq accumulates; when the
 *        sensor predicts, x^_{t|t} is propagated over the d queued commands exactly as the sensor propagates y_t (that is what
 *        pred_hist then holds); the result is the x0 of the solve;
 *     3. solve, command queue and plant step as without the filter;
 *     4. the time update.
 *   A handed-over xhat / cov are the priors x^_{t|t-1}, P_{t|t-1} of the call's first step (cov NULL: diag(p0[g]^2)); on return they
 *   hold the priors of step T, so that a continued run (with the sensor's pending and step0) is the whole run bit for bit.
 * estimator = NULL launches exactly the kernels of the _sensor_ entries and returns their bits.  A non-NULL estimator with a trivial
 * or NULL sensor still keeps the truth in a buffer of the call (and the handle's warm start for a continued run): then y_t = x_t and
 * nothing is drawn.  The filter is told neither the plant's dispersion nor the actuator.
 * FTMPC_ERR_ARG, the message naming ftmpc_estimator.<field> and, for an array, the first offending vehicle, the call's x untouched:
 * a struct_size other than sizeof(ftmpc_estimator); every < 1; a p0 or proc_sigma negative or not finite; a meas_sigma not finite
 * and > 0; cov without xhat; an xhat or cov entry not finite; a diagonal entry of cov below zero.
 */
typedef struct ftmpc_estimator {
    int32_t struct_size;      /* sizeof(ftmpc_estimator) */
    int32_t every;            /* >= 1: the update runs on campaign steps c with c % every == 0 */
    double p0[4];             /* initial standard deviations: position (m), velocity (m/s), attitude (rad), rate (rad/s) */
    double proc_sigma[4];     /* process noise standard deviations per step, by group */
    double meas_sigma[4];     /* measurement noise standard deviations by group, > 0 */
    double* xhat;             /* NULL or [B*13], in/out: the prior mean */
    double* cov;              /* NULL or [B*78], in/out: the prior covariance, packed; requires xhat */
    double* est_hist;         /* NULL or [T*B*13], output: x^_{t|t} */
    double* err_sq;           /* NULL or [B*4], output: per vehicle the sums over the call's steps, against the truth, of
                                 |p^ - p|^2, |v^ - v|^2, |x_t [-] x^|_theta^2, |w^ - w|^2 */
} ftmpc_estimator;

/* ftmpc_simulate_sensor_batch with the filter `estimator` (NULL: exactly ftmpc_simulate_sensor_batch). */
int ftmpc_simulate_estimator_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                   const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                   int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                   double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                   const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                   const ftmpc_sensor* sensor, const ftmpc_estimator* estimator);

/* ftmpc_simulate_wrench_sensor_batch with the filter `estimator` (NULL: exactly ftmpc_simulate_wrench_sensor_batch). */
int ftmpc_simulate_wrench_estimator_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                          const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                          int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                          uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                          const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist, int32_t* not_converged,
                                          int32_t* alloc_failed, const ftmpc_outcomes* out, const ftmpc_plant_model* plant,
                                          const ftmpc_mission* mission, const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                          const ftmpc_estimator* estimator);

/* Thruster fault diagnosis in the on-device closed loop (thruster form: one QP, or the thruster SQP, per step).  Without this struct
 * the controller learns of a fault at the step the schedule's `detect` names.  With it the controller finds the fault itself: per
 * vehicle a bank of one-sided CUSUM tests, one per hypothesis "thruster i is stuck at level l" (a dead thruster is level 0), driven by
 * a parity residual: the measurement against an open-loop prediction of the controller's model from the last used measurement.  When
 * a statistic crosses the threshold the controller's pattern switches on the device, before that step's solve, exactly as a
 * schedule event with detect = t switches it, the repair of the warm start included.  The parameters are uniform over the call; the
 * state and the outputs are per vehicle.
 *   NT thrusters, L = n_levels, H = NT L hypotheses, thruster i at level l has index i L + l; (ub_c, stuck_c) is the controller's
 *   pattern; c = step0 + t the campaign step (step0 the sensor's, 0 without one); K = max_detect.
 *   state per vehicle: xt [13] the prediction from the last used measurement, n the model steps since, acc [NT] the sum over those
 *   steps of the effective command, llr [H] the statistics.
 *   per loop step t:
 *     1. ftmpc_sense_kernel forms y_t (a trivial or NULL sensor: the truth, kept in a buffer of the call as under an estimator);
 *     2. phase 0, before the filter's phase 0 and the solve.  On the first step of a call that was not handed `state`: xt = y_t,
 *        n = 0, acc = 0, llr = 0 and no test.  Otherwise, when c % every == 0, n >= 1 and fewer than K detections have been made:
 *          r = y_t [-] xt (the filter's residual);  rho_v = M(q~)' r[3:6] with q~ the quaternion of xt and M the model's
 *          body-to-inertial matrix;  r_w = r[9:12];  s_v = resid_sigma[0]^2 + n drift_sigma[0]^2, s_w with index 1;
 *          for every thruster i with ub_c,i > 0 and every level l:  delta = n levels[l] - acc_i,  a_v = (dt / m) D[0:3, i] delta,
 *          a_w = dt J^-1 D[3:6, i] delta,  z = (a_v . rho_v - a_v . a_v / 2) / s_v + (a_w . r_w - a_w . a_w / 2) / s_w,
 *          llr = max(0, llr + z);  the statistics of a thruster with ub_c,i == 0 are 0.
 *        If the largest statistic exceeds `threshold`, its hypothesis (a tie: the lowest index) is detected: detect_step[k] = c,
 *        detect_thruster[k] = i, detect_level[k] = l with k the vehicle's detection count; the controller's pattern becomes
 *        ub_c,i = 0, stuck_c,i = levels[l]; when t > 0, or the handle resumes a warm start, the shifted warm start U is clipped
 *        elementwise to [0, ub_new]; all H statistics of the vehicle are set to 0.  llr_hist[t] holds the statistics after the
 *        max(0, .) and before a detection's reset (on a step without a test: the carried values).  Whenever c % every == 0, test or
 *        not: xt = y_t, n = 0, acc = 0.
 *     3. filter phase 0 (when an estimator is given), solve, command queue and plant step as without the struct: they see the new
 *        pattern in the step of the detection;
 *     4. phase 1, after the plant step, with a_t the command the plant applied in step t:  c_i = ub_c,i > 0 ? a_t,i : 0,
 *        gen = D (c + stuck_c),  xt <- one RK4 step of the model, renormalised (the filter's step),  acc_i += c_i,  n += 1.
 * With a fault schedule the schedule moves the PLANT only: its `detect` must be NULL and is not consulted.  Without one the plant
 * keeps the call's ub / stuck whatever the diagnosis decides.
 * Limits: the signature is first order in dt (one rotation per test, the gyroscopic coupling of the difference neglected); a dead
 * thruster that is not commanded has no signature, and neither has a thruster stuck at the level it is commanded at (stuck on while the
 * controller saturates it); a fault that starts inside a window of every > 1 steps shows only a part of its signature in that window's
 * test; a detection is never withdrawn; position and attitude are not used; the diagnosis is told neither the plant dispersion nor the
 * actuator (resid_sigma / drift_sigma have to cover them).  (ftmpc_probe below lifts the first and the fourth of these: it pulses
 * thrusters that have been quiet, and with reinstate tests a detected thruster for "healthy after all".)
 * A continued run (state, llr and the detect arrays handed over, the returned ub / stuck as the call's pattern, the sensor's
 * pending / step0, the filter's xhat / cov, the schedule shifted) is the whole run bit for bit.
 * FTMPC_ERR_ARG, the message naming ftmpc_diagnosis.<field> and, for an array, the first offending vehicle, the call's x untouched:
 * a struct_size other than sizeof(ftmpc_diagnosis); every < 1, or different from a given estimator's every; n_levels outside [1, 4];
 * max_detect outside [1, FTMPC_MAX_FAULT_EVENTS]; a level negative, not finite or not above the one before; a resid_sigma not
 * finite and > 0; a drift_sigma negative or not finite; a threshold not finite and > 0; llr or a detect array without state; state
 * without the three detect arrays; a non-finite state or llr entry; n < 0; a handed detect entry out of range, or a used slot after
 * an unused one; a fault schedule with detect != NULL; a sensor with predict = 1 and no estimator (the sense kernel would predict
 * with the old pattern before the diagnosis runs).
 */
typedef struct ftmpc_diagnosis {
    int32_t struct_size;       /* sizeof(ftmpc_diagnosis) */
    int32_t every;             /* >= 1: the test runs on campaign steps c with c % every == 0 */
    int32_t n_levels;          /* L, 1..4 */
    int32_t max_detect;        /* K, 1..FTMPC_MAX_FAULT_EVENTS */
    double levels[4];          /* N, finite, >= 0, strictly increasing */
    double resid_sigma[2];     /* > 0: velocity (m/s), rate (rad/s) */
    double drift_sigma[2];     /* >= 0, per model step */
    double threshold;          /* > 0 */
    double* state;             /* NULL or [B*(14+NT)] in/out: xt[13], n, acc[NT] */
    double* llr;               /* NULL or [B*H] in/out; requires state */
    int32_t* detect_step;      /* NULL or [B*max_detect] in/out, -1 = unused; a handed state requires all three */
    int32_t* detect_thruster;
    int32_t* detect_level;
    double* ub;                /* NULL or [B*NT] out: the controller's pattern after the last step */
    double* stuck;
    double* llr_hist;          /* NULL or [T*B*H] out */
} ftmpc_diagnosis;

/* ftmpc_simulate_estimator_batch with the diagnosis `diagnosis` (NULL: exactly ftmpc_simulate_estimator_batch).  The wrench form has
 * its own entry, ftmpc_simulate_wrench_diagnosis_batch below: it needs no hull table per hypothesis, only new offsets. */
int ftmpc_simulate_diagnosis_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                   const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                   int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                   double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                   const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                   const ftmpc_sensor* sensor, const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis);

/* The offsets of the input hull for other patterns on the SAME normals.  The hull {D u : 0 <= u_i <= ub_i, dead or stuck thrusters at
 * stuck_i} is a zonotope whose facet normals are the directions orthogonal to five independent generators, so the normals of a
 * pattern with fewer live thrusters are among those of the pattern it started from; only the offsets change.  For row r of vehicle
 * b's table hull_A[hull_set[b]] (hull_set NULL: table 0), with D the handle's config's:
 *   c_i = sum_g a_g D[g, i],   b_r = sum_i (c_i (ub_i / 2 + stuck_i) + |c_i| ub_i / 2)     (g and i ascending)
 * A row that is no longer a facet of the new pattern stays a supporting half-space, so the set is described exactly.  A row whose six
 * entries are exactly 0 is padding: b_r = 1.  out_flat[b] (NULL: not asked for) is 1 when a non-padding row has no width,
 *   w_r = sum_i |c_i| ub_i <= 1e-9 |a_r|_1 max|D| max_i ub_i,
 * i.e. the live thrusters no longer span R^6 and the two-stage form does not exist for the pattern, else 0.
 * The caller's contract: a vehicle's table holds the facet normals of an index set that contains the pattern's live thrusters (the
 * table of the pattern the vehicle started from).  Host buffers: ub, stuck [B*NT], hull_A [n_sets*hull_rows*6], hull_set NULL or [B],
 * out_b [B*hull_rows], out_flat NULL or [B].  ftmpc_hull_offsets_kernel, a lane per vehicle; the closed loop below runs the same
 * kernel, so both give the same bits. */
int ftmpc_hull_offsets_batch(ftmpc_handle* h, int64_t B, const double* ub, const double* stuck, const double* hull_A, int32_t n_sets,
                             const int32_t* hull_set, int32_t hull_rows, double* out_b, int32_t* out_flat);

/* ftmpc_simulate_wrench_estimator_batch with the diagnosis `diagnosis` (NULL: exactly that entry, kernel for kernel).  The loop of
 * ftmpc_diagnosis above on the two-stage form.  Per step: sense; diagnosis phase 0 (as on the thruster form: it switches ub_c /
 * stuck_c and records the detection); the hull step; filter phase 0; solve, allocation, command queue and plant step; diagnosis
 * phase 1; filter phase 1.  The hull step, for the vehicles that switched in this step:
 *   - ftmpc_hull_offsets_kernel evaluates the offsets of the new pattern on the vehicle's table and the flat criterion;
 *   - not flat: the controller's hull_b becomes the new offsets, hull_set[b] does not change, and when t > 0, or the handle resumes a
 *     warm start, every stage of the shifted warm start G is pulled towards the new hull centre as at a detected schedule event;
 *   - flat: the detection stands (detect arrays and the controller's pattern as phase 0 left them), hull_b and the warm start are
 *     left untouched, and no_hull_step[b] takes the campaign step c if it was -1.
 * The caller's contract for the table: a vehicle's table must hold the facet normals of its STARTING index set (the live thrusters
 * of the call's ub), which is what hull tables built from the call's pattern give; every later pattern has its normals among them.
 * out_hull_b: NULL or [B*hull_rows], the controller's offsets after the last step.  no_hull_step: NULL or [B], in/out, -1 = none; for a
 * continued run hand back both (out_hull_b as the next call's hull_b) with the diagnosis' own carry-over.
 * With a fault schedule the schedule moves the PLANT only: its detect, hull_set and hull_b must be NULL.
 * FTMPC_ERR_ARG, the call's x untouched: the refusals of ftmpc_simulate_diagnosis_batch, and with a diagnosis a schedule whose
 * hull_set or hull_b is set (the message names the field) and a no_hull_step entry below -1 (it names the vehicle). */
int ftmpc_simulate_wrench_diagnosis_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                          const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                          int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                          uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                          const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist, int32_t* not_converged,
                                          int32_t* alloc_failed, const ftmpc_outcomes* out, const ftmpc_plant_model* plant,
                                          const ftmpc_mission* mission, const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                          const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                          int32_t* no_hull_step);

/* On-device disturbance estimation and offset-free control (thruster form with one QP per step: this entry; the two-stage wrench form
 * with one QP or the wrench SQP per step: ftmpc_simulate_wrench_disturbance_batch below).  The filter of ftmpc_estimator is
 * augmented by six states per vehicle: f^ [3], a constant force in the inertial frame (N), and t^ [3], a constant torque in the body
 * frame (N m): the frames and units of ftmpc_plant_model.force / .torque.  The estimate is given to every consumer of the
 * controller's model: the filter's own prediction, the diagnosis' prediction and, compensate = 1, the linearisation the QP is built
 * from, which removes the steady tracking offset a constant disturbance leaves under the nominal MPC (it has no integral action).
 * The parameters are uniform over the call; the state and the outputs are per vehicle.
 *   error coordinates (dp, dv, dtheta, dw, df, dt), 18 in all; the covariance travels in three pieces: P_xx = ftmpc_estimator.cov
 *   (78 packed), P_xd = cross (12 x 6, row-major, 72) and P_dd = cov (packed upper triangle, row-major, 21).
 *   the model with the estimate, the plant's own equation (ftmpc_plant_model) with the config's m, J and D:
 *     v' = (Rot(q)^T F + f^) / m,   w' = J^-1 (tau + t^ - w x J w),   f^ and t^ held over the step.
 *   measurement update, when the estimator's update runs, H = [I 0] and the estimator's R: its twelve sequential scalar updates
 *     carried over all 18 coordinates:  s_j = P_jj + R_j,  k = P[:, j] / s_j (18 entries),  delta += k (r_j - delta_j),
 *     P -= s_j k k';  then x^ <- x^ [+] delta[0:12], f^ += delta[12:15], t^ += delta[15:18].
 *   time update, with a_t and gen as in the estimator:  Phi = [[Phi_xx, Phi_xd], [0, I]], Phi_xx the estimator's (its G block from
 *     F / m), Phi_xd with two non-zero blocks (v, f) = (dt / m) I and (w, t) = dt J^-1,
 *     P <- Phi P Phi' + diag(estimator.proc_sigma[g]^2, proc_sigma[0]^2 x 3, proc_sigma[1]^2 x 3);  x^ <- one RK4 step of the
 *     model with the estimate, renormalised;  f^ and t^ unchanged.
 *   per loop step t (campaign step c = step0 + t):
 *     1. ftmpc_sense_kernel forms y_t; the diagnosis' phase 0 (test, decision, re-anchor) as without the struct;
 *     2. filter phase 0 (ftmpc_filter_dist_kernel<0>, <1>).  On the first step of a call that was not handed xhat: x^ = y_t,
 *        P_xx = diag(estimator.p0[g]^2), P_xd = 0, P_dd = diag(p0[0]^2 x 3, p0[1]^2 x 3), f^ / t^ the handed values or 0, no update.
 *        Otherwise the update runs when c % every == 0.  est_hist[t] = x^_{t|t}, force_hist[t] = f^_{t|t}, torque_hist[t] = t^_{t|t};
 *        when the sensor predicts, x^_{t|t} is propagated over the d queued commands with the model with the estimate (pred_hist);
 *        the result is the x0 of the solve;
 *     3. the solve.  compensate = 1: the linearise kernel's DIST instantiation rolls the orbit-centre model out under tau + t^ and
 *        f^ / m (d^_{t|t}); the cost's R .* (gen - ur - f_virt) keeps the commanded gen.  compensate = 0: the plain instantiation,
 *        so the controller stays nominal (the A/B switch of a campaign).  Command queue and plant step as without the struct;
 *     4. the diagnosis' phase 1 with the model with the estimate d^_{t|t} (ftmpc_diagnose_dist_kernel); the filter's time update
 *        (ftmpc_filter_dist_kernel<2>, <3>).
 * A handed force / torque / cross / cov are the priors of the call's first step; on return they hold the priors of step T, so that a
 * continued run (with the estimator's xhat / cov, the sensor's pending / step0 and the diagnosis' carry-over) is the whole run bit for
 * bit.  disturbance = NULL launches exactly the kernels of ftmpc_simulate_diagnosis_batch and returns its bits.
 * Not served: the thruster-form SQP loop (ftmpc_cost_kernel does not know the estimate; the wrench form's SQP does, see
 * ftmpc_simulate_wrench_disturbance_batch), m / J / D (a gain or centre-of-mass error shows up as a command-dependent part of (f^, t^)), per-vehicle filter
 * parameters, ftmpc_multi_upload / _step.  Known limit: an undetected stuck thruster is a constant body wrench, so a slow t^ absorbs
 * its torque signature over time; proc_sigma has to be small against the CUSUM's detection time.
 * FTMPC_ERR_ARG, the message naming ftmpc_disturbance.<field> and, for an array, the first offending vehicle, the call's x untouched:
 * a struct_size other than sizeof(ftmpc_disturbance); no estimator; sqp_iters > 0; compensate outside {0, 1}; a p0 or proc_sigma
 * negative or not finite; cross without force, torque or the estimator's xhat; cov without cross; a force, torque, cross or cov entry
 * not finite; a diagonal entry of cov below zero.
 */
typedef struct ftmpc_disturbance {
    int32_t struct_size;   /* sizeof(ftmpc_disturbance) */
    int32_t compensate;    /* 0 / 1 */
    double p0[2];          /* initial standard deviations: force (N), torque (N m), >= 0 */
    double proc_sigma[2];  /* per step, >= 0 */
    double* force;         /* NULL (start at 0) or [B*3] in/out */
    double* torque;        /* NULL or [B*3] in/out */
    double* cross;         /* NULL or [B*72] in/out; requires force, torque and estimator->xhat */
    double* cov;           /* NULL or [B*21] in/out; requires cross */
    double* force_hist;    /* NULL or [T*B*3] out: f^_{t|t} */
    double* torque_hist;   /* NULL or [T*B*3] out */
} ftmpc_disturbance;

/* ftmpc_simulate_diagnosis_batch with the disturbance estimate `disturbance` (NULL: exactly ftmpc_simulate_diagnosis_batch). */
int ftmpc_simulate_disturbance_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                     const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                     int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                     double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                     const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                     const ftmpc_sensor* sensor, const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                     const ftmpc_disturbance* disturbance);

/* The disturbance estimate on the two-stage wrench form: ftmpc_simulate_wrench_diagnosis_batch with `disturbance` (NULL: exactly that
 * entry's kernels and bits; ftmpc_simulate_wrench_diagnosis_batch IS this entry with NULL).  The filter and the diagnosis work on the
 * applied thruster commands, so they are the thruster form's (ftmpc_filter_dist_kernel, ftmpc_diagnose_dist_kernel); the hull rows,
 * the terminal set and the allocation constrain and allocate the COMMANDED wrench and stay nominal.  sqp_iters >= 0 is served: under
 * compensate = 1 the wrench SQP takes d^_{t|t} in every linearisation (the linearise kernel's DIST instantiations about the iterate)
 * AND in every launch of its cost / merit kernel (ftmpc_cost_wrench_kernel<1>: the start point, the line-search trials, the final
 * rollout), which agree term for term.  Per loop step:
 *   1. sense;  2. the diagnosis' phase 0;  3. hull offsets and hull switch (under a diagnosis);  4. ftmpc_filter_dist_kernel<0>, <1>;
 *   5. the solve (one wrench QP, or the wrench SQP) with d^_{t|t} when compensate = 1;  6. the allocation of the commanded
 *   tau_0 - D stuck;  7. the command queue;  8. the plant step;  9. ftmpc_diagnose_dist_kernel;  10. ftmpc_filter_dist_kernel<2>, <3>.
 * FTMPC_ERR_ARG with the call's x untouched: what ftmpc_simulate_disturbance_batch refuses except sqp_iters > 0, what
 * ftmpc_simulate_wrench_diagnosis_batch refuses (state bounds with sqp_iters > 0 among it).  The thruster-form SQP loop stays refused
 * by ftmpc_simulate_disturbance_batch (ftmpc_cost_kernel does not know the estimate). */
int ftmpc_simulate_wrench_disturbance_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                            const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                            int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                            uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                            const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist, int32_t* not_converged,
                                            int32_t* alloc_failed, const ftmpc_outcomes* out, const ftmpc_plant_model* plant,
                                            const ftmpc_mission* mission, const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                            const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                            int32_t* no_hull_step, const ftmpc_disturbance* disturbance);

/* On-device estimation of the velocity and rate sensor bias.  The filter of ftmpc_estimator is augmented by six states per vehicle:
 * b_v^ [3], a constant bias of the velocity measurement (m/s), and b_w^ [3], a constant bias of the rate measurement (rad/s): the
 * channels 3..5 and 9..11 of ftmpc_sensor.bias.  Position tells the filter what the velocity is and attitude what the rate is, so both
 * are observable from the kinematics alone; a constant position or attitude bias is not, and stays in the estimate.  The parameters
 * are uniform over the call; the state and the outputs are per vehicle.
 *   the filter (its definition): error coordinates (dp, dv, dtheta, dw, db_v, db_w), 18 in all;  y_v = v + b_v + n, y_w = w + b_w + n,
 *     H = [I_12, HB], HB [12 x 6] with HB[3+r, r] = HB[9+r, 3+r] = 1;  Phi = diag(Phi_xx, I_6) with the estimator's Phi_xx, the mean
 *     takes the estimator's RK4 step and b^ stays;  Q = diag(estimator.proc_sigma[g]^2, proc_sigma[0]^2 x 3, proc_sigma[1]^2 x 3), the
 *     initial covariance likewise with p0;  the residual is the estimator's y [-] x~ with x~ = x^ with v^ + b_v^ and w^ + b_w^;  the
 *     update is the estimator's twelve sequential scalar updates in channel order, each over all 18 coordinates with row h_j of H.
 *   the form the device runs (exactly equivalent) and the arrays of this struct carry: the MEASURED coordinates
 *     m = (dp, dv + db_v, dtheta, dw + db_w) with b unchanged, P^m = T P T', T = [[I, HB], [0, I]].  There H = [I 0];
 *     Phi^m = [[Phi_xx, E], [0, I]] with E = (I - Phi_xx) HB, non-zero in (p, b_v) = -dt I, (theta, b_w) = -dt I, (w, b_w) = I - W;
 *     Q^m = T Q T' (the v and w diagonals of Q_xx gain proc_sigma[0]^2, proc_sigma[1]^2; Q_xb = HB diag(q_b^2); Q_bb = diag(q_b^2));
 *     after the twelve updates delta_x = delta_m - HB delta_b, x^ <- (x^ [+] delta_m) with HB delta_b taken off v^ and w^,
 *     b^ += delta_b.  The covariance travels in three pieces: P_mm = ftmpc_estimator.cov (78 packed), P_mb = cross (12 x 6, row-major,
 *     72) and P_bb = cov (packed upper triangle, row-major, 21), so that a continued run rounds nowhere on the way out or in.
 *   priors: with cross handed, ftmpc_estimator.cov (diag(estimator.p0[g]^2) when NULL) is P_mm as it stands and cov, when NULL, is
 *     diag(p0[0]^2 x 3, p0[1]^2 x 3).  Without cross the bias prior is independent of the state error: ftmpc_estimator.cov (or
 *     diag(estimator.p0[g]^2)) is the covariance of (dp, dv, dtheta, dw) itself, P_bb = diag(p0^2), and the pieces are T P T':
 *     the v and w diagonals of P_mm gain p0[0]^2 and p0[1]^2, P_mb = HB diag(p0^2).  On return ftmpc_estimator.cov is P_mm.
 *   per loop step: as ftmpc_simulate_diagnosis_batch with ftmpc_filter_bias_kernel<0>, <1> in place of ftmpc_filter_kernel<0> and
 *     <2>, <3> in place of <1>.  On the first step of a call that was not handed xhat: x^ = y_t with b^ (the handed values or 0) taken
 *     off its velocity and rate, no update.  est_hist[t] = x^_{t|t}, bias_hist[t] = b^_{t|t}; err_sq as the estimator's; when the
 *     sensor predicts, x^_{t|t} is propagated over the queued commands with the plain model (the bias does not enter the dynamics).
 *     The estimate reaches the solve through x0 alone, so sqp_iters >= 0 is served on both forms.  The diagnosis kernels are
 *     untouched: they read the raw y_t, and a constant bias cancels in their re-anchored residual.
 * A handed bias / cross / cov are the priors of the call's first step; on return they hold the priors of step T, so that a continued
 * run (with the estimator's xhat / cov, the sensor's pending / step0 and the diagnosis' carry-over) is the whole run bit for bit.
 * Not served: a position or attitude bias, the bias states together with the disturbance states (24 states), per-vehicle filter
 * parameters, ftmpc_multi_upload / _step.
 * FTMPC_ERR_ARG, the message naming ftmpc_bias_estimate.<field> and, for an array, the first offending vehicle, the call's x
 * untouched: a struct_size other than sizeof(ftmpc_bias_estimate); no estimator; a non-NULL disturbance in the same call; a p0 or
 * proc_sigma negative or not finite; cross without bias or the estimator's xhat; cov without cross; a bias, cross or cov entry not
 * finite; a diagonal entry of cov below zero.
 */
typedef struct ftmpc_bias_estimate {
    int32_t struct_size;   /* sizeof(ftmpc_bias_estimate) */
    int32_t reserved;      /* 0 */
    double p0[2];          /* initial standard deviations: velocity bias (m/s), rate bias (rad/s), >= 0 */
    double proc_sigma[2];  /* per step, >= 0 */
    double* bias;          /* NULL (start at 0) or [B*6] in/out: b_v^, b_w^ */
    double* cross;         /* NULL or [B*72] in/out; requires bias and estimator->xhat */
    double* cov;           /* NULL or [B*21] in/out; requires cross */
    double* bias_hist;     /* NULL or [T*B*6] out: b^_{t|t} */
} ftmpc_bias_estimate;

/* ftmpc_simulate_disturbance_batch with the bias estimate `bias_estimate` (NULL: exactly ftmpc_simulate_disturbance_batch, which IS
 * this entry with NULL). */
int ftmpc_simulate_bias_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                              const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                              int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                              double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                              const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                              const ftmpc_sensor* sensor, const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                              const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate);

/* The bias estimate on the two-stage wrench form: ftmpc_simulate_wrench_disturbance_batch with `bias_estimate` (NULL: exactly that
 * entry's kernels and bits).  The filter works on the applied thruster commands, so it is the thruster form's. */
int ftmpc_simulate_wrench_bias_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                     const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                     int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                     uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                     const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist, int32_t* not_converged,
                                     int32_t* alloc_failed, const ftmpc_outcomes* out, const ftmpc_plant_model* plant,
                                     const ftmpc_mission* mission, const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                     const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                     int32_t* no_hull_step, const ftmpc_disturbance* disturbance,
                                     const ftmpc_bias_estimate* bias_estimate);

/* Measurement dropouts, outliers and a gated filter.  The fix a vehicle navigates by drops out for stretches and sometimes returns a
 * wild sample; per vehicle and step the device decides whether y_t is available, whether it carries an outlier, and which channels of
 * it the filter accepts.  The parameters are uniform over the call; the state, the counters and the histories are per vehicle.
 *   notation: campaign step c = step0 + t (step0 the sensor's, 0 without one); vehicle number g = index0 + b and index_total as in
 *     ftmpc_outcomes; counter k = c * index_total + g; u_s = u01(seed, 32 k + s), the splitmix counter function of the plant noise
 *     and the sensor, under this struct's own seed.
 *   per loop step, right after ftmpc_sense_kernel has formed y_t (the truth when the sensor is trivial) and before the diagnosis' and
 *     the filter's phase 0 (ftmpc_outage_kernel):
 *     init step (the first step of a call that was not handed ftmpc_estimator.xhat): available, run = 0, no outlier is drawn and
 *       y_t is untouched, whatever the chain or the window say.
 *     otherwise lost = run_prev > 0 ? !(u_0 < p_recover) : (u_0 < p_loss), and inside the window (from <= c < to) lost regardless.
 *     a lost step: run = run_prev + 1, lost_steps += 1, longest = max(longest, run); y_t stays as the sense kernel left it and
 *       nobody reads it.
 *     an available step: run = 0; for each group k (position, velocity, attitude, rate) with p_outlier[k] > 0 an outlier is drawn
 *       when u_{1+k} < p_outlier[k]; its three channels j = 3k .. 3k+2 get e_j = outlier_sigma[k] sqrt(-2 log(1 - u_{8+2j}))
 *       cos(2 pi u_{9+2j}), added to y_t for position, velocity and rate, and y_q <- rotate(y_q, e_{6:9}) for attitude (the
 *       sensor's closed form, renormalised); outliers[b][k] += 1.
 *     meas_hist[t] is y_t after this step, on lost steps too; ftmpc_sensor.meas_hist stays the sense kernel's sample.
 *   the filter (ftmpc_filter_gated_kernel in place of ftmpc_filter_kernel<0>): the measurement update of step c runs for a vehicle
 *     when !init && c % every == 0 && available; otherwise the solve starts from the propagated estimate, as between two updates.
 *     Inside the update, at channel j, e = r_j - d_j and s_j = P_jj + R_j; with gate > 0 and e e > (gate gate) s_j the channel is
 *     rejected: d and P stay as they are, rejected[b][j / 3] += 1 and bit j of gate_hist[t] is set; otherwise the channel is
 *     processed as ftmpc_filter_kernel<0> does.  The time update, est_hist, err_sq and the queue prediction are unchanged.
 *   the diagnosis, when the call has one (ftmpc_diagnose_gated_kernel in place of ftmpc_diagnose_kernel<0>): on a step where the
 *     vehicle is lost phase 0 does nothing for it: no test, no re-anchor; xt, n, acc and llr carry over and llr_hist[t] holds the
 *     carried values.  Phase 1 is unchanged, so n keeps counting and the first test after reacquisition covers the whole outage (the
 *     n >= 1 window of the signature).  The first step of a call without ftmpc_diagnosis.state anchors on y_t whatever the
 *     availability.  On the wrench form the hull step runs off `switched` and is unchanged.
 * A handed state / rejected / outliers are the values at the call's first step; on return they hold those of step T, so that a
 * continued run (with the sensor's pending / step0, the estimator's xhat / cov and the diagnosis' carry-over) is the whole run bit
 * for bit; without them the chain starts available and the counters at zero.  outage == NULL, or a trivial struct (p_loss = 0, every
 * p_outlier = 0, gate = 0, window and every array NULL), launches exactly the kernels of the _bias_ entries and returns their bits.
 * Limits: outliers reach the diagnosis ungated (the gate lives in the filter alone); ftmpc_filter_dist_kernel and
 * ftmpc_filter_bias_kernel have no gated form, so ftmpc_disturbance and ftmpc_bias_estimate are refused; the parameters are uniform
 * over the call; the whole 12-channel measurement is lost or present (no per-group availability); ftmpc_multi_upload / _step take
 * no outage.
 * FTMPC_ERR_ARG, the message naming ftmpc_outage.<field> and, for an array, the first offending vehicle, the call's x untouched: a
 * struct_size other than sizeof(ftmpc_outage); reserved != 0; no estimator; a non-NULL disturbance or bias_estimate in the same call;
 * p_loss outside [0, 1); p_recover outside (0, 1]; a p_outlier outside [0, 1]; an outlier_sigma or gate negative or not finite; a
 * negative state, rejected or outliers entry.
 */
typedef struct ftmpc_outage {
    int32_t struct_size, reserved;      /* sizeof(ftmpc_outage), 0 */
    uint64_t seed;                      /* its own stream */
    double p_loss;                      /* P(lost at c | available at c-1), in [0, 1) */
    double p_recover;                   /* P(available at c | lost at c-1), in (0, 1] */
    double p_outlier[4];                /* per group (position, velocity, attitude, rate), in [0, 1] */
    double outlier_sigma[4];            /* >= 0, the group's units */
    double gate;                        /* 0: no gate; > 0: in standard deviations of the scalar innovation */
    const int32_t* window;              /* NULL or [B*2]: a scripted outage [from, to) in campaign steps; to <= from: none */
    int32_t* state;                     /* NULL or [B*3] in/out: run (length of the current outage, 0 = available), lost_steps, longest */
    int32_t* rejected;                  /* NULL or [B*4] in/out: gated channel-steps per group */
    int32_t* outliers;                  /* NULL or [B*4] in/out: outlier draws per group */
    int32_t* avail_hist;                /* NULL or [T*B] out: 1 available, 0 lost */
    int32_t* outlier_hist;              /* NULL or [T*B] out: bit k = group k carried an outlier */
    int32_t* gate_hist;                 /* NULL or [T*B] out: bit j = channel j was rejected */
    double* meas_hist;                  /* NULL or [T*B*13] out: y_t as the filter and the diagnosis saw it */
} ftmpc_outage;

/* ftmpc_simulate_bias_batch with the outage `outage` (NULL: exactly ftmpc_simulate_bias_batch, which IS this entry with NULL). */
int ftmpc_simulate_outage_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                const ftmpc_sensor* sensor, const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate,
                                const ftmpc_outage* outage);

/* The outage on the two-stage wrench form: ftmpc_simulate_wrench_bias_batch with `outage` (NULL: exactly that entry's kernels and
 * bits).  The three kernels are the thruster form's. */
int ftmpc_simulate_wrench_outage_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                       const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                       int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                       uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                       const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist, int32_t* not_converged,
                                       int32_t* alloc_failed, const ftmpc_outcomes* out, const ftmpc_plant_model* plant,
                                       const ftmpc_mission* mission, const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                       const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                       int32_t* no_hull_step, const ftmpc_disturbance* disturbance,
                                       const ftmpc_bias_estimate* bias_estimate, const ftmpc_outage* outage);

/* A disturbance that varies over the run.  ftmpc_plant_model.force / .torque are one constant wrench per vehicle for the whole call;
 * here the wrench the plant integrates under is rewritten on the device before every plant step: a Gauss-Markov process, a periodic
 * term and a kick on top of that constant.  The parameters sigma, tau and period are uniform over the call; the amplitudes, the
 * phase, the kick, its window, the process state and the outputs are per vehicle.
 *   notation: campaign step c = step0 + t (step0 this struct's own; a sensor in the same call has to carry the same value);
 *     vehicle number g = index0 + b and index_total as in ftmpc_outcomes; counter k = c * index_total + g; u_s = u01(seed, 32 k + s),
 *     the splitmix counter function of the plant noise and the sensor, under this struct's own seed; the Gaussian of the slot pair
 *     (s, s + 1) is sqrt(-2 log(1 - u_s)) cos(6.283185307179586 u_{s+1}).
 *   per loop step, after the step's solve and right before the plant step (ftmpc_environment_kernel), the wrench held over plant
 *     step t (zero-order hold, as the constant one is) is  w_c = base + g_c + p_c + k_c,  six components: force in the inertial frame
 *     [0:3] (N), torque in the body frame [3:6] (N m), the frames and units of ftmpc_plant_model.
 *     base: plant.force / plant.torque of the call, zero where they are NULL (or the call has no plant model).
 *     g_c: six independent first-order Gauss-Markov processes, exactly discretised: with phi_a = exp(-dt / tau[a]), a = 0 for the
 *       force and 1 for the torque, g_{c+1,j} = phi_a g_{c,j} + sigma[a] sqrt(1 - phi_a^2) n_{c,j}, n_{c,j} the Gaussian of the
 *       slots 2j, 2j+1 of counter k; phi and the innovation scale are computed on the host once per call.  With `state` handed
 *       over, g of the call's first step is that state; otherwise it is a stationary draw, sigma[a] times the Gaussian of the slots
 *       16+2j, 17+2j of that step's counter.  On return `state` holds g of step step0 + T, so that a continued run (with step0
 *       moved on) is the whole run bit for bit.  A non-NULL state always counts as handed over: a caller who wants the end state of
 *       a run that starts stationary makes that draw itself (ft_mpc_amd.environments.stationary restates it).  sigma[a] = 0 switches the process off: tau[a] is not looked at, nothing is drawn
 *       and phi_a = 0.
 *     p_c = amp sin(6.283185307179586 (c dt / period) + phase_b), amp the vehicle's amp_force / amp_torque (a NULL array: zero).
 *     k_c = kick_b while from_b <= c < to_b (window, in campaign steps); to <= from: no kick.
 *   the plant: ftmpc_plant_step_var_kernel (with an actuator: ftmpc_plant_step_act_kernel) reads w_c where it read the constant
 *     wrench; neither kernel changes.  A call without a plant model gets the nominal mass, J and D, as a plant model with every
 *     array NULL would.
 *   est_err_sq, in step order: [b][0] += |f^ - w_c[0:3]|^2, [b][1] += |t^ - w_c[3:6]|^2, with (f^, t^) the disturbance estimate
 *     the step's solve saw (what ftmpc_disturbance.force_hist[t] / torque_hist[t] record).  A handed array is continued.
 * environment == NULL, or a trivial struct (both sigma zero, every array NULL and no output), launches exactly the kernels of the
 * _outage_ entries and returns their bits.
 * Limits: sigma, tau and period are uniform over the call; the force is in the inertial frame only (no body-frame force such as a
 * leaking valve's, no inertial torque); one kick per vehicle; neither the controller nor the disturbance filter is told the
 * process's tau (the filter's model stays a random walk with proc_sigma); ftmpc_multi_upload / _step take no environment.
 * FTMPC_ERR_ARG, the message naming ftmpc_environment.<field> and, for an array, the first offending vehicle, the call's x
 * untouched: a struct_size other than sizeof(ftmpc_environment); reserved != 0; step0 < 0; a sensor in the call whose step0
 * differs; a sigma that is negative or not finite; sigma[a] > 0 with a tau[a] that is not positive and finite; an amplitude array
 * given with a period that is not positive and finite; a non-finite entry of any array; kick without window; est_err_sq without a
 * disturbance estimate (ftmpc_disturbance) in the call, or with a negative entry.
 */
typedef struct ftmpc_environment {
    int32_t struct_size, reserved;      /* sizeof(ftmpc_environment), 0 */
    uint64_t seed;                      /* its own stream */
    int64_t step0;                      /* campaign step of the call's first loop step, >= 0 */
    double sigma[2];                    /* stationary standard deviation of the Gauss-Markov force (N) and torque (N m); 0: off */
    double tau[2];                      /* its correlation time (s), > 0 where sigma > 0 */
    double period;                      /* of the periodic term (s), > 0 where an amplitude is given */
    const double* amp_force;            /* NULL or [B*3]: amplitude of the periodic force (N, inertial frame) */
    const double* amp_torque;           /* NULL or [B*3]: amplitude of the periodic torque (N m, body frame) */
    const double* phase;                /* NULL (0) or [B]: rad */
    const double* kick;                 /* NULL or [B*6]: force, then torque; needs window */
    const int32_t* window;              /* NULL or [B*2]: the kick acts while from <= c < to, in campaign steps; to <= from: none */
    double* state;                      /* NULL or [B*6] in/out: g of the call's first step; on return g of step step0 + T */
    double* wrench_hist;                /* NULL or [T*B*6] out: w_c of every step */
    double* est_err_sq;                 /* NULL or [B*2] in/out: summed squared error of f^ and of t^ against w_c; needs a disturbance */
} ftmpc_environment;

/* ftmpc_simulate_outage_batch with the environment `environment` (NULL: exactly ftmpc_simulate_outage_batch, which IS this entry
 * with NULL). */
int ftmpc_simulate_environment_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                     const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                     int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                     double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                     const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                     const ftmpc_sensor* sensor, const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                     const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate,
                                     const ftmpc_outage* outage, const ftmpc_environment* environment);

/* The environment on the two-stage wrench form: ftmpc_simulate_wrench_outage_batch with `environment` (NULL: exactly that entry's
 * kernels and bits).  The kernel is the thruster form's. */
int ftmpc_simulate_wrench_environment_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                            const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                            int32_t hull_rows, const double* xref_traj, const double* uref_traj,
                                            const double noise[4], uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol,
                                            double penalty, const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                            int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                            const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                            const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                            const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                            int32_t* no_hull_step, const ftmpc_disturbance* disturbance,
                                            const ftmpc_bias_estimate* bias_estimate, const ftmpc_outage* outage,
                                            const ftmpc_environment* environment);

/* Three safeguards for the diagnosis' decision rule (ftmpc_diagnosis), as an opt-in: a consistency gate, confirmation and level
 * revision.  The plain rule switches the controller's pattern on the first test whose largest statistic crosses the threshold and
 * never looks back; a short unmodelled push is then taken for a stuck thruster, a fault that starts inside a window is named at
 * the neighbour, and a wrong level stays wrong.  The parameters are uniform over the call; lead, the counters and fit_hist are per
 * vehicle.  A test happens under exactly the plain rule's condition (c % every == 0, n >= 1, fewer than max_detect entries, and
 * the vehicle available when the call has an outage); rho_v, r_w, s_v, s_w, a_v(h), a_w(h) and z_h are ftmpc_diagnosis'.
 *   fit: q_0 = |rho_v|^2 / s_v + |r_w|^2 / s_w and, for hypothesis h, q_h = q_0 - 2 z_h, the normalised energy left once h's
 *     signature is subtracted (under h chi-square with 6 degrees of freedom).  With consist > 0, h is counted in this test only if
 *     q_h <= consist^2: llr_h = max(0, llr_h + z_h); a statistic that is not counted keeps its value.  The test is void, and adds 1
 *     to voided[b], when q_0 > consist^2 and no eligible hypothesis was counted.  consist = 0: every eligible hypothesis is counted
 *     and no test is void.  (ft_mpc_amd.diagnosis.consist_for(p) gives the square root of the chi-square(6) quantile.)
 *   eligible: (i, l) with ub_c,i > 0, delta = n levels[l] - acc_i, as in the plain rule.  With revise also (i, l) of a thruster
 *     with ub_c,i == 0 that stands in the vehicle's own detection list (of this call, or carried in through
 *     ftmpc_diagnosis.detect_*), delta = n (levels[l] - stuck_c,i); the hypothesis at its current level has delta = 0 and z = 0
 *     and stays where it is.  A thruster that is off in the call's pattern but not in the list stays the caller's: it is never
 *     revised and its statistics are 0.
 *   confirmation: the leader is the largest statistic strictly above the threshold (the lowest index on a tie).  The same leader
 *     as lead[b][0] gives run + 1, another one lead = h, run = 1, none lead = -1, run = 0.  The decision is taken when
 *     run >= persist; until then the statistics keep accumulating.  persist = 1 is the plain rule.
 *   decision: for a live thruster the plain rule's (a detection entry, ub_c,i = 0, stuck_c,i = levels[l], every statistic 0).
 *     For a revision the entry (c, i, l), which uses a slot of max_detect, stuck_c,i = levels[l], ub_c,i stays 0, revised[b] += 1,
 *     every statistic 0.  Either resets lead and run and flags the vehicle as switched, so the warm-start repair, the hull offsets
 *     (wrench form) and the linearisation follow as after any detection.
 * Re-anchoring, the model's step, llr_hist and an outage's carry-over of a lost vehicle (lead and the counters included) are
 * unchanged.  ftmpc_diagnose_iso_kernel runs in place of the call's phase-0 diagnosis kernel.
 * isolation == NULL, or a trivial struct (consist = 0, persist = 1, revise = 0, every array NULL), launches exactly the kernels
 * of the _environment_ entries and returns their bits.
 * Limits: this rule alone never withdraws a detection back to healthy (a thruster the controller no longer commands has no
 * signature; a reinstating ftmpc_probe pulses it and adds that hypothesis); consist and persist are uniform over the call; the innovation gate of the filters is ftmpc_outage's, not this one.
 * FTMPC_ERR_ARG, the message naming ftmpc_isolation.<field> and, for an array, the first offending vehicle, the call's x
 * untouched: a struct_size other than sizeof(ftmpc_isolation); reserved != 0; a non-trivial struct without an ftmpc_diagnosis in
 * the call; consist negative or not finite; persist < 1; revise outside {0, 1}; a lead entry with a hypothesis outside
 * [-1, NT * n_levels) or a negative run; lead without ftmpc_diagnosis.state; a negative voided or revised entry.
 */
typedef struct ftmpc_isolation {
    int32_t struct_size, reserved;      /* sizeof(ftmpc_isolation), 0 */
    double consist;                     /* the gate on q_h (its square root); 0: no gate */
    int32_t persist;                    /* consecutive tests with the same leader before the decision, >= 1 */
    int32_t revise;                     /* 1: the level of a detected thruster is tested on, 0: not */
    int32_t* lead;                      /* NULL or [B*2] in/out: the leader (-1: none) and its run length; needs diagnosis.state */
    int32_t* voided;                    /* NULL or [B] in/out: void tests */
    int32_t* revised;                   /* NULL or [B] in/out: revisions */
    double* fit_hist;                   /* NULL or [T*B*2] out: q_0 and the smallest q_h over the eligible hypotheses of a tested step;
                                           -1, -1 on a step without a test or without an eligible hypothesis */
} ftmpc_isolation;

/* ftmpc_simulate_environment_batch with the decision rule `isolation` (NULL: exactly ftmpc_simulate_environment_batch, which IS
 * this entry with NULL). */
int ftmpc_simulate_isolation_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                   const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                   int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                   double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                   const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                   const ftmpc_sensor* sensor, const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                   const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate,
                                   const ftmpc_outage* outage, const ftmpc_environment* environment,
                                   const ftmpc_isolation* isolation);

/* The decision rule on the two-stage wrench form: ftmpc_simulate_wrench_environment_batch with `isolation` (NULL: exactly that
 * entry's kernels and bits).  The kernel is the thruster form's; a revision recomputes the hull offsets as any detection does. */
int ftmpc_simulate_wrench_isolation_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                          const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                          int32_t hull_rows, const double* xref_traj, const double* uref_traj,
                                          const double noise[4], uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol,
                                          double penalty, const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                          int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                          const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                          const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                          const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                          int32_t* no_hull_step, const ftmpc_disturbance* disturbance,
                                          const ftmpc_bias_estimate* bias_estimate, const ftmpc_outage* outage,
                                          const ftmpc_environment* environment, const ftmpc_isolation* isolation);

/* Probe pulses, as an opt-in: the diagnosis (ftmpc_diagnosis) is passive, it sees only what the controller commands.  A dead
 * thruster that is not commanded has no signature, and a thruster the controller was told to leave alone can never clear itself.
 * With this struct the loop briefly fires a thruster that has been quiet, after the step's solve (on the wrench form after the
 * allocation and its alloc_failed count) and before the command enters the latency ring; everything downstream (the ring, the
 * plant step, u_hist, the filters' time update, the diagnosis' phase 1, the outcomes) sees the pulsed command as it sees any
 * command.  The parameters are uniform over the call; the counters are per vehicle and thruster.  With (ub_c, stuck_c) the
 * controller's pattern of the step, u the solve's command and K = max_detect, NT, L, H of ftmpc_diagnosis:
 *   listed: thruster i is off (ub_c,i == 0) and the newest entry for i in the vehicle's detection list has a level below
 *     n_levels (see the reinstatement below).
 *   probeable: live (ub_c,i > 0), or listed when reinstate = 1.
 *   idle counter: e_i = ub_c,i > 0 ? u_i : 0;  idle_i = (probeable and e_i < quiet) ? idle_i + 1 : 0.  A NaN command compares
 *     false: its counter resets.
 *   candidate: the probeable thruster with the largest idle_i among those with idle_i >= idle_steps and, with max_pulses > 0,
 *     pulses_i < max_pulses; the lowest index on a tie.  At most one thruster per vehicle and step.
 *   pulse: on a live candidate u_i = min(u_i + amp, ub_c,i), on a listed one u_i = amp; then pulses_i += 1,
 *     impulse += (u_i,new - e_i) dt, idle_i = 0 and thruster_hist[t] = i.  Without a candidate nothing changes and
 *     thruster_hist[t] = -1.  (ftmpc_probe_kernel<0>; ft_mpc_amd.probes.step restates it.)
 * reinstate = 1 adds the hypothesis "this listed thruster is healthy after all" to the decision rule.  After the plant step
 * pacc_i += a_t,i for the listed thrusters (ftmpc_probe_kernel<1>; the model's c_i is 0 for a thruster that is off), and the
 * call's phase-0 diagnosis kernel is replaced by ftmpc_diagnose_probe_kernel: the test of ftmpc_isolation (the call's struct, or
 * the trivial rule when there is none; the availability word when the call has an outage) with NT further hypotheses, index
 * H + i, for the listed thrusters: delta = pacc_i - n stuck_c,i, a_v, a_w, z and q from delta exactly as for a level hypothesis,
 * the statistic in health[i] (0 for a thruster that is not listed).  The gate counts it like any other hypothesis and it
 * competes for the leader like any other; on a tie the lower index wins, so a level hypothesis beats it: with levels[0] = 0 and
 * no pulse yet "dead" is read before "healthy".  Confirmation is unchanged (lead may hold H + i).  The decision for H + i: the
 * detection entry (c, i, n_levels), which uses a slot of max_detect; ub_c,i = restore_ub, stuck_c,i = 0; reinstated[b] += 1;
 * every statistic (llr and health), lead and run reset; the vehicle flagged as switched, so the warm-start repair, the hull
 * offsets and switch (wrench form) and the linearisation follow as after any detection.  Any decision resets health; pacc is
 * set to 0 wherever the diagnosis re-anchors.  In that kernel a level revision (ftmpc_isolation.revise) looks at `listed` as
 * defined here: a thruster that is off behind a reinstatement entry is the caller's.  With reinstate = 0 the phase-0 kernels are
 * the ones the call launches without the struct, and pacc and health do not move.
 * probe == NULL launches exactly the kernels of the _isolation_ entries and returns their bits.
 * Limits: the pulse is not wrench-neutral, the controller sees its effect as a disturbance and corrects it on the next step; a
 * thruster stuck at the level it is commanded at still has no signature; the parameters are uniform over the call; under a PWM
 * actuator (ftmpc_actuator) a pulse below the minimum on-time is swallowed by the valve; the multi-GPU drivers have no probe.
 * A continued run (every in/out array handed over, with the diagnosis' and the isolation's) is the whole run bit for bit.
 * FTMPC_ERR_ARG, the message naming ftmpc_probe.<field> and, for an array, the first offending vehicle, the call's x untouched:
 * a struct_size other than sizeof(ftmpc_probe); reserved != 0; a probe without an ftmpc_diagnosis in the call; amp not finite
 * and > 0; quiet outside [0, amp); idle_steps < 1; max_pulses < 0; reinstate outside {0, 1}; restore_ub not finite and > 0 under
 * reinstate; a negative idle, pulses or reinstated entry; a negative or non-finite impulse, pacc or health entry; pacc or health
 * without ftmpc_diagnosis.state.  Under a reinstating probe a carried ftmpc_diagnosis.detect_level entry may equal n_levels and
 * ftmpc_isolation.lead may name H + i; both stay refused without one.
 */
typedef struct ftmpc_probe {
    int32_t struct_size, reserved;      /* sizeof(ftmpc_probe), 0 */
    double amp;                         /* the pulse, N: finite, > 0 */
    double quiet;                       /* a command below it counts as idle, N: 0 <= quiet < amp */
    int32_t idle_steps;                 /* >= 1: idle steps before a thruster is pulsed */
    int32_t max_pulses;                 /* per thruster and vehicle, counted with what `pulses` carries in; 0: no cap */
    int32_t reinstate;                  /* 1: listed thrusters are pulsed and tested for "healthy", 0: not */
    double restore_ub;                  /* the bound a reinstated thruster gets, N: finite, > 0 under reinstate */
    int32_t* idle;                      /* NULL or [B*NT] in/out (NULL: from 0) */
    int32_t* pulses;                    /* NULL or [B*NT] in/out */
    double* impulse;                    /* NULL or [B] in/out, N s: what the pulses added to the commands */
    double* pacc;                       /* NULL or [B*NT] in/out; needs diagnosis.state */
    double* health;                     /* NULL or [B*NT] in/out; needs diagnosis.state */
    int32_t* reinstated;                /* NULL or [B] in/out: reinstatements */
    int32_t* thruster_hist;             /* NULL or [T*B] out: the pulsed thruster of the step, or -1 */
} ftmpc_probe;

/* ftmpc_simulate_isolation_batch with the probe `probe` (NULL: exactly ftmpc_simulate_isolation_batch, which IS this entry with
 * NULL). */
int ftmpc_simulate_probe_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                               const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                               int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                               double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                               const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                               const ftmpc_sensor* sensor, const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                               const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate,
                               const ftmpc_outage* outage, const ftmpc_environment* environment,
                               const ftmpc_isolation* isolation, const ftmpc_probe* probe);

/* The probe on the two-stage wrench form: ftmpc_simulate_wrench_isolation_batch with `probe` (NULL: exactly that entry's kernels
 * and bits).  The kernels are the thruster form's; a reinstatement recomputes the hull offsets as any detection does (the
 * reinstated thruster lies inside the starting index set of the hull tables). */
int ftmpc_simulate_wrench_probe_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                      const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                      int32_t hull_rows, const double* xref_traj, const double* uref_traj,
                                      const double noise[4], uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol,
                                      double penalty, const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                      int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                      const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                      const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                      const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                      int32_t* no_hull_step, const ftmpc_disturbance* disturbance,
                                      const ftmpc_bias_estimate* bias_estimate, const ftmpc_outage* outage,
                                      const ftmpc_environment* environment, const ftmpc_isolation* isolation,
                                      const ftmpc_probe* probe);

/* The wrench-form cost, QP step and SQP under a given estimate dist [B*6]: per vehicle f^ [3] (inertial, N), then t^ [3] (body, N m).
 * Each is its plain entry (ftmpc_eval_cost_wrench_batch, ftmpc_solve_wrench_batch, ftmpc_solve_sqp_wrench_batch) with `dist` inserted
 * after G / warmG; the rollout of the cost and of the linearisation sees tau + t^ at every RK4 stage and f^ / m added to the inertial
 * acceleration, the R .* (tau - ur - f_virt) term keeps the commanded wrench, the terminal-set violation, the terminal cost and out_X
 * are those of the disturbed rollout.  With dist all zero each returns the bits of its plain entry.  dist NULL or with a non-finite
 * entry: FTMPC_ERR_ARG. */
int ftmpc_eval_cost_wrench_disturbance_batch(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                                             const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride,
                                             const double* G, const double* dist, double* out_cost, double* out_tviol);
int ftmpc_solve_wrench_disturbance_batch(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                                         const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                         int32_t hull_rows, const double* xref, int64_t xref_stride, const double* uref,
                                         int64_t uref_stride, double* warmG, const double* dist, double* out_u0, double* out_tau0,
                                         double* out_G, int32_t* status, int32_t* iters, int32_t* alloc_status);
int ftmpc_solve_sqp_wrench_disturbance_batch(ftmpc_handle* h, int64_t B, const double* x0, const double* ub, const double* stuck,
                                             const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                             int32_t hull_rows, const double* xref, int64_t xref_stride, const double* uref,
                                             int64_t uref_stride, const double* warmG, const double* dist, int32_t sqp_iters,
                                             int32_t backtracks, double tol, double penalty, double* out_u0, double* out_tau0,
                                             double* out_G, double* out_X, double* out_cost, double* out_cost0, double* out_tviol,
                                             int32_t* out_sqp_iters, int32_t* out_iters, int32_t* status, int32_t* alloc_status);

/* Per-kernel device timing of the LAST solve call, measured with hipEvents on the launch
 * stream when enabled.  ms[slot] is the duration of kernel slot `slot` (0 when that kernel was
 * not launched), for slot < min(n_slots, FTMPC_KERNEL_SLOTS); ftmpc_kernel_name(slot) is the kernel's name as it appears
 * in rocprofv3 traces:  0 linearise, 1..3 condense+IPM fp32 (one wave per instance) for n <= 128 / 144 / 160,
 * 4 condense+IPM fp64, dense (workgroup per instance, general n), 5 condense+IPM fp32, workgroup per instance, for
 * 160 < N*NT: ftmpc_solve_wsw32_kernel (Newton systems through the 6N-variable wrench-space form, one wave per instance:
 * N <= 16 with N*NT <= 256, N <= 21 with N*NT <= 384), ftmpc_solve_ws32_kernel (the same form on a workgroup per instance:
 * kernel_select = FTMPC_KERNEL_WORKGROUP) or, with kernel_select = FTMPC_KERNEL_DENSE and N*NT <= 240, the dense
 * ftmpc_solve_wg32_kernel<15> (the slot reports all three names), 6 IPM fp64 on one wave per instance by the
 * Riccati recursion (ftmpc_solve_ric64_kernel, N <= 40: the box QP, the state bounds, and the terminal set where N * NT > 256 or
 * kernel_select = FTMPC_KERNEL_RICCATI) or condense+IPM fp64 through the wrench-space form (ftmpc_solve_ws64_kernel, 6 N <= 256). */
#define FTMPC_KERNEL_SLOTS 7
int ftmpc_set_profiling(ftmpc_handle* h, int32_t enabled);
int ftmpc_last_kernel_ms(ftmpc_handle* h, float* ms, int32_t n_slots);
const char* ftmpc_kernel_name(int32_t slot);
/* the ONE kernel slot `slot` launches on this handle (slot 5 names three kernels above, slot 6 two; which of them runs is the
 * handle's routing: its shape, terminal_set / state_bounds and kernel_select) */
const char* ftmpc_routed_kernel_name(const ftmpc_handle* h, int32_t slot);

/*
 * Test hook: runs the build for instance `inst` of a host batch and returns the condensed
 * QP the solve kernel sees (active thrusters only):  n = N*na,  H [n*n] row-major,
 * g [n], lo [n], hi [n] (bounds on d = U - Ubar), all as double.  *n_out receives n.
 * H_cap is the capacity of H in elements (>= n*n).
 * The dump is the BOX QP: the rows of the terminal set are not part of it.  On a terminal-set handle whose thruster form runs on
 * ftmpc_solve_ric64_kernel (N * NT > 256, or kernel_select = FTMPC_KERNEL_RICCATI) it comes from the dense float64 kernel's box mode --
 * the same H, g, lo, hi as a handle without the set dumps -- and the first call allocates that kernel's per-workgroup slots, which
 * ftmpc_create leaves out for such a handle beyond N * NT = 256.
 */
int ftmpc_debug_build_qp(ftmpc_handle* h, int64_t B,
                         const double* x0, const double* ub, const double* stuck,
                         const double* xref, int64_t xref_stride,
                         const double* uref, int64_t uref_stride,
                         const double* warmU, int64_t inst,
                         double* H, int64_t H_cap, double* g, double* lo, double* hi,
                         int32_t* n_out);

/*
 * Test hook: runs the linearisation alone on a host batch -- the kernel the handle's lin_split_max picks for B, with the
 * parameters (work lists included) a solve would give it -- and copies the records back:
 * rec_out [B * N * 152] doubles, the layout of csrc/ftmpc_common.h (REC_*), stage k of instance b at (b * N + k) * 152.
 */
int ftmpc_debug_records(ftmpc_handle* h, int64_t B,
                        const double* x0, const double* ub, const double* stuck,
                        const double* xref, int64_t xref_stride,
                        const double* uref, int64_t uref_stride,
                        const double* warmU, double* rec_out);

/* Test hook: ftmpc_debug_records through the linearise kernel's DIST instantiation (the one a loop with
 * ftmpc_disturbance.compensate = 1 launches) with the estimated disturbance dist [B*6]: per vehicle f^ [3] (inertial, N), then
 * t^ [3] (body, N m).  With dist all zero the records are the bits of ftmpc_debug_records. */
int ftmpc_debug_records_disturbance(ftmpc_handle* h, int64_t B,
                                    const double* x0, const double* ub, const double* stuck,
                                    const double* xref, int64_t xref_stride,
                                    const double* uref, int64_t uref_stride,
                                    const double* warmU, const double* dist, double* rec_out);

/*
 * Test hook: the float64 reference gradient of the fp32 solve kernels (csrc/ftmpc_solve.hip, struct_grad_at) alone.  Linearises
 * the host batch as ftmpc_debug_records does, then evaluates, per instance b with na active thrusters and n = N * na variables,
 *     g = 2 Bbar' Wbar (e_bar + Bbar d) + 2 Da' R (ut_bar + Da d)          (without the 2 rho (u_bar + d) term)
 * at the caller's d: d [B * N * NT] floats, instance b's n values first at b * N * NT, stage-major over the active thrusters in
 * ascending order; g_out [B * N * NT] doubles in the same layout (the rest zero).
 * form 0: the sweeps as float64 MFMA chains; form 1: as row-per-lane vector FMAs.  Both exchange through LDS, which limits the
 * hook to fp32 handles with N <= 21 and NT <= 8.  The launch has fewer workgroups than instances.
 */
int ftmpc_debug_struct_grad(ftmpc_handle* h, int64_t B,
                            const double* x0, const double* ub, const double* stuck,
                            const double* xref, int64_t xref_stride,
                            const double* uref, int64_t uref_stride,
                            const double* warmU, const float* d, int32_t form, double* g_out);

/*
 * The batch axis across the GPUs of one node from ONE process.  The reference
 * never couples instances (one controller object per vehicle, spiraling_mpc.py:288-317), so device g owns
 * the contiguous range [B g / G, B (g+1) / G) (ftmpc_multi_shard_bounds); one host thread + one handle + one
 * stream set per device, no collective, nothing on xGMI: every device reads its slice of the caller's arrays
 * and writes its slice of the caller's outputs.
 *   device_ids  NULL (devices 0..n_devices-1) or n_devices ordinals; an ordinal may repeat (several handles
 *               on one GPU);  n_devices <= 0: every visible device.
 * ftmpc_multi_solve_batch has the contract of ftmpc_solve_batch (host buffers, pinned staging per device).
 * ftmpc_multi_upload keeps the shards RESIDENT in each device's HBM; ftmpc_multi_step then runs `steps` MPC
 * steps over them on every device at once (keep_U != 0: the whole-horizon solution is kept too) and returns
 * when all devices are idle; ftmpc_multi_download gathers u0 [B*NT], U [B*N*NT] (needs keep_U), status, iters
 * (each may be NULL) on the host.
 */
typedef struct ftmpc_multi ftmpc_multi;
int ftmpc_multi_create(const ftmpc_config* cfg, const int32_t* device_ids, int32_t n_devices, ftmpc_multi** out);
int ftmpc_multi_destroy(ftmpc_multi* m);
const char* ftmpc_multi_last_error(const ftmpc_multi* m); /* m may be NULL: last create error */
int32_t ftmpc_multi_device_count(const ftmpc_multi* m);
/* host cores the worker thread of device slot `slot` is bound to: the cores nearest its GPU (sysfs local_cpulist of the PCI
 * function) that the process may use; 0 when the two sets do not meet and the affinity was left alone */
int32_t ftmpc_multi_worker_cpus(const ftmpc_multi* m, int32_t slot);
int ftmpc_multi_shard_bounds(const ftmpc_multi* m, int64_t B, int32_t slot, int64_t* lo, int64_t* hi);
int ftmpc_multi_solve_batch(ftmpc_multi* m, int64_t B,
                            const double* x0, const double* ub, const double* stuck,
                            const double* xref, int64_t xref_stride,
                            const double* uref, int64_t uref_stride,
                            double* warmU,
                            double* out_u0, double* out_U,
                            int32_t* status, int32_t* iters);
int ftmpc_multi_upload(ftmpc_multi* m, int64_t B,
                       const double* x0, const double* ub, const double* stuck,
                       const double* xref, int64_t xref_stride,
                       const double* uref, int64_t uref_stride,
                       const double* warmU);
int ftmpc_multi_step(ftmpc_multi* m, int32_t steps, int32_t keep_U);
int ftmpc_multi_download(ftmpc_multi* m, double* out_u0, double* out_U, int32_t* status, int32_t* iters);
/* The closed loops on the multi-GPU driver: ftmpc_simulate_outcomes_batch / ftmpc_simulate_wrench_outcomes_batch with device slot g
 * running the vehicles [lo, hi) of ftmpc_multi_shard_bounds as the slice index0 = lo of a campaign of index_total = B, so the result is
 * what one handle computes for the whole batch wherever a vehicle's solve does not depend on its batch.  Every per-vehicle input
 * (x, ub, stuck, the call's hull_set / hull_b, the schedule's arrays) is read at the shard's offset; hull_A, the reference
 * trajectories, the noise amplitudes and the seed are shared.  Per-vehicle outputs land at the shard's offset, the [T, B, ..]
 * histories row by row, not_converged [T] / alloc_failed [T] are summed over the slots.  `out` may be NULL; its index0 / index_total
 * must be 0 / 0 or 0 / B (the driver sets them per slot).  More slots than vehicles (B > 0): FTMPC_ERR_ARG.  A failing slot fails the
 * call with its message. */
int ftmpc_multi_simulate_outcomes_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                        const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                        int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                        double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out);
int ftmpc_multi_simulate_wrench_outcomes_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                               const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                               int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                               uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                               const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                               int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out);
/* The two entries above with the plant model `plant` (ftmpc_plant_model; NULL: exactly the entries above).  Every array of the struct
 * is read at the shard's offset: mass + lo, J + 9 lo, D + 6 NT lo, force + 3 lo, torque + 3 lo.  A refusal names the vehicle by its
 * number in the whole batch. */
int ftmpc_multi_simulate_plant_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                     const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                     int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                     double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                     const ftmpc_plant_model* plant);
int ftmpc_multi_simulate_wrench_plant_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                            const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                            int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                            uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                            const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                            int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                            const ftmpc_plant_model* plant);
/* The two entries above with the mission `mission` (ftmpc_mission; NULL: exactly the entries above).  The mission is checked once over
 * the whole batch, so a refusal names the vehicle by its number in the caller's arrays; the tables are shared, table + lo, offset + lo
 * and cost + 3 lo are read or written per shard. */
int ftmpc_multi_simulate_mission_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                       const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                       int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                       double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                       const ftmpc_plant_model* plant, const ftmpc_mission* mission);
int ftmpc_multi_simulate_wrench_mission_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                              const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                              int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                              uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                              const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                              int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                              const ftmpc_plant_model* plant, const ftmpc_mission* mission);
/* The two entries above with the actuator `actuator` (ftmpc_actuator; NULL: exactly the entries above).  The struct is checked once
 * over the whole batch, so a refusal names the vehicle by its number in the caller's arrays; delivered + lo, pulses + lo and
 * state + lo NT are read and written per shard, the two histories are copied row by row from the shard's staging as u_hist is. */
int ftmpc_multi_simulate_actuator_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                        const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                        int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                        double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                        const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator);
int ftmpc_multi_simulate_wrench_actuator_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                               const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                               int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                               uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                               const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                               int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                               const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                               const ftmpc_actuator* actuator);
/* The two entries above with the sensor `sensor` (ftmpc_sensor; NULL: exactly the entries above).  The struct is checked once over
 * the whole batch, so a refusal names the vehicle by its number in the caller's arrays; bias + 12 lo and pending + lo d NT are read
 * (and pending written) per shard, the two histories are copied row by row from the shard's staging as u_hist is.
 * ftmpc_multi_upload / _step take no sensor. */
int ftmpc_multi_simulate_sensor_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                      const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                      int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                      double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                      const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                      const ftmpc_sensor* sensor);
int ftmpc_multi_simulate_wrench_sensor_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                             const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                             int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                             uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                             const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                             int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                             const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                             const ftmpc_actuator* actuator, const ftmpc_sensor* sensor);
/* The two entries above with the filter `estimator` (ftmpc_estimator; NULL: exactly the entries above).  The struct is checked once
 * over the whole batch, so a refusal names the vehicle by its number in the caller's arrays; xhat + 13 lo, cov + 78 lo and
 * err_sq + 4 lo are read and written per shard, est_hist is copied row by row from the shard's staging as meas_hist is.
 * ftmpc_multi_upload / _step take no estimator. */
int ftmpc_multi_simulate_estimator_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                         const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                         int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                         double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                         const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                         const ftmpc_sensor* sensor, const ftmpc_estimator* estimator);
int ftmpc_multi_simulate_wrench_estimator_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                                const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                                int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                                uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                                const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                                int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                                const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                                const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                                const ftmpc_estimator* estimator);
/* ftmpc_multi_simulate_estimator_batch with the diagnosis `diagnosis` (ftmpc_diagnosis; NULL: exactly that entry).  The struct is
 * checked once over the whole batch, so a refusal names the vehicle by its number in the caller's arrays; state + (14 + NT) lo,
 * llr + H lo, the detect arrays + max_detect lo and ub / stuck + NT lo are read and written per shard, llr_hist is copied row by row
 * from the shard's staging as est_hist is.  ftmpc_multi_upload / _step take no diagnosis. */
int ftmpc_multi_simulate_diagnosis_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                         const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                         int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                         double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                         const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                         const ftmpc_sensor* sensor, const ftmpc_estimator* estimator,
                                         const ftmpc_diagnosis* diagnosis);
/* ftmpc_multi_simulate_wrench_estimator_batch with the diagnosis `diagnosis` (NULL: exactly that entry) as
 * ftmpc_simulate_wrench_diagnosis_batch runs it.  The struct and no_hull_step are checked once over the whole batch; per shard the
 * diagnosis' arrays as in ftmpc_multi_simulate_diagnosis_batch, out_hull_b + hull_rows lo and no_hull_step + lo.
 * ftmpc_multi_upload / _step take no diagnosis. */
int ftmpc_multi_simulate_wrench_diagnosis_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                                const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                                int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                                uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                                const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                                int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                                const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                                const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                                const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                                int32_t* no_hull_step);
/* ftmpc_multi_simulate_diagnosis_batch with the disturbance estimate `disturbance` (ftmpc_disturbance; NULL: exactly that entry).
 * The struct is checked once over the whole batch, so a refusal names the vehicle by its number in the caller's arrays; force /
 * torque + 3 lo, cross + 72 lo and cov + 21 lo are read and written per shard, force_hist / torque_hist are copied row by row from
 * the shard's staging as llr_hist is.  ftmpc_multi_upload / _step take no disturbance. */
int ftmpc_multi_simulate_disturbance_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                           const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                           int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                           double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                           const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                           const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                           const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                           const ftmpc_disturbance* disturbance);
/* ftmpc_multi_simulate_wrench_diagnosis_batch with the disturbance estimate `disturbance` (NULL: exactly that entry) as
 * ftmpc_simulate_wrench_disturbance_batch runs it (sqp_iters >= 0).  The struct is checked once over the whole batch; the shards read
 * and write its arrays by pointer offset and the two histories are scattered as in ftmpc_multi_simulate_disturbance_batch. */
int ftmpc_multi_simulate_wrench_disturbance_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                                  const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                                  int32_t hull_rows, const double* xref_traj, const double* uref_traj,
                                                  const double noise[4], uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol,
                                                  double penalty, const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                                  int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                                  const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                                  const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                                  const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                                  int32_t* no_hull_step, const ftmpc_disturbance* disturbance);
/* ftmpc_multi_simulate_disturbance_batch with the bias estimate `bias_estimate` (ftmpc_bias_estimate; NULL: exactly that entry).
 * The struct is checked once over the whole batch, so a refusal names the vehicle by its number in the caller's arrays; bias + 6 lo,
 * cross + 72 lo and cov + 21 lo are read and written per shard, bias_hist is copied row by row from the shard's staging.  The
 * two-stage wrench form has no multi-GPU bias entry; ftmpc_multi_upload / _step take no bias estimate. */
int ftmpc_multi_simulate_bias_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                    const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                    int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                    double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                    const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                    const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                    const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                    const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate);
/* ftmpc_multi_simulate_bias_batch with the outage `outage` (ftmpc_outage; NULL: exactly that entry).  The struct is checked once
 * over the whole batch, so a refusal names the vehicle by its number in the caller's arrays; window + 2 lo, state + 3 lo,
 * rejected + 4 lo and outliers + 4 lo are read and written per shard, the four histories are copied row by row from the shard's
 * staging.  The two-stage wrench form has no multi-GPU bias entry to extend, so it has no multi-GPU outage entry either. */
int ftmpc_multi_simulate_outage_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                      const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                      int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                      double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                      const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                      const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                      const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                      const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate,
                                      const ftmpc_outage* outage);
/* ftmpc_multi_simulate_outage_batch with the environment `environment` (ftmpc_environment; NULL: exactly that entry).  The struct
 * is checked once over the whole batch, so a refusal names the vehicle by its number in the caller's arrays; amp_force + 3 lo,
 * amp_torque + 3 lo, phase + lo, kick + 6 lo, window + 2 lo, state + 6 lo and est_err_sq + 2 lo are read and written per shard,
 * wrench_hist is copied row by row from the shard's staging; the shard's index0 keys its draws, so the bits are the single handle's.
 * The two-stage wrench form has no multi-GPU outage entry to extend, so it has no multi-GPU environment entry either. */
int ftmpc_multi_simulate_environment_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                           const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                           int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                           double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                           const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                           const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                           const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                           const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate,
                                           const ftmpc_outage* outage, const ftmpc_environment* environment);
/* ftmpc_multi_simulate_environment_batch with the decision rule `isolation` (ftmpc_isolation; NULL: exactly that entry).  The
 * struct is checked once over the whole batch, so a refusal names the vehicle by its number in the caller's arrays; lead + 2 lo,
 * voided + lo and revised + lo are read and written per shard, fit_hist is copied row by row from the shard's staging.  The
 * two-stage wrench form has no multi-GPU environment entry to extend, so it has no multi-GPU isolation entry either. */
int ftmpc_multi_simulate_isolation_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                         const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                         int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                         double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                         const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                         const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                         const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                         const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate,
                                         const ftmpc_outage* outage, const ftmpc_environment* environment,
                                         const ftmpc_isolation* isolation);
/* per-kernel device timing of device slot `slot` (see ftmpc_set_profiling / ftmpc_last_kernel_ms) */
int ftmpc_multi_set_profiling(ftmpc_multi* m, int32_t enabled);
int ftmpc_multi_last_kernel_ms(ftmpc_multi* m, int32_t slot, float* ms, int32_t n_slots);
const char* ftmpc_multi_routed_kernel_name(const ftmpc_multi* m, int32_t slot); /* ftmpc_routed_kernel_name of the device handles */

/* Library/ABI version: major*10000 + minor*100 + patch. */
int32_t ftmpc_version(void);
/* Hash of the kernel and host sources this binary was built from (csrc/Makefile): two builds of the same sources -- the
 * shipped one and the `plain` diagnostic build with the asm-side wait states as written -- report the same string. */
const char* ftmpc_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* FTMPC_H */
