"""Batched front-end of the HIP MPC QP-step path (numpy in / numpy out, or device pointers).

`BatchedMPC.solve` is the batched form of SpiralingController.get_control
(reference: ft_mpc/controllers/spiraling_mpc.py:288-317): B robot states + fault scenarios in,
B thruster command vectors out.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .models.sys_model import allocation_matrix_16, allocation_matrix_8

F_MAX = 3.4  # sys_model.py:60


@dataclass
class MPCConfig:
    """Problem constants; defaults are the reference's (see include/ftmpc.h ftmpc_config)."""
    N: int = 20
    NT: int = 8
    dt: float = 0.1
    mass: float = 16.8
    J: np.ndarray = field(default_factory=lambda: np.diag([0.2, 0.3, 0.25]))
    D: np.ndarray = None
    Q: np.ndarray = field(default_factory=lambda: np.array([1, 1, 1, 1, 1, 1, 2, 2, 2], float))
    R: np.ndarray = field(default_factory=lambda: np.array([0.1, 0.1, 0.1, 0.01, 0.01, 0.01]))
    P: np.ndarray = None
    r: np.ndarray = None
    f_virt: np.ndarray = field(default_factory=lambda: np.array([0.0, 3.5, 0.0]))
    rho: float = 0.05
    max_iters: int = 0            # <= 0: library default (30)
    mu_stop: float = 0.0          # <= 0: library default (1e-11 for f32, 1e-13 for f64)
    device_id: int = 0
    dtype: str = "f32"            # arithmetic of the KKT/IPM solve: "f32" | "f64" (N*NT > 240 always runs f64)
    # terminal set  term_A (c_N[0:9] - xref_N) <= term_b  (config/terminal.yaml term_set; spiraling_mpc.py:199-202):
    # a TerminalSet / (A, b) pair, or True for the shipped config/terminal.yaml.  Needs dtype "f64".
    terminal_set: object = None
    # False: the rows above are carried in the config (for the tset_step outcome of `simulate`) but are NOT added to the QP
    terminal_set_active: bool = True
    # non-quadratic part of the terminal cost (config/terminal.yaml `cost` beyond e'P e; spiraling_mpc.py:196): a
    # TerminalIngredients object, or True for the shipped config/terminal.yaml.  Every QP then carries its exact
    # gradient at the linearisation point and eval_cost includes it (see BatchedMPC.solve_sqp).
    terminal_cost: object = None
    # implementation switches (include/ftmpc.h ftmpc_config; diagnostics and A/B runs): "auto" | "dense" (Newton systems
    # always in the thruster variables, never through the wrench-space form) | "workgroup" (the wrench-space form on a
    # workgroup per instance, kernel 8, where "auto" gives the instance one wave, kernel 10), the batch size up to which the linearisation
    # is split by tangent direction (0: library default, < 0: never) and the staging ranges of the host-buffer entry
    kernel_select: str = "auto"
    lin_split_max: int = 0
    stage_chunks: int = 0
    # state bounds  xlb <= c_k <= xub  on the 13 orbit-centre states [p, v, omega, q] of the stages 1 .. N-1: the reference's optional
    # controller params "xub" / "xlb" (spiraling_mpc.py:129-130,179-185; None = no bounds, +-inf = no row for that component)
    xlb: np.ndarray = None
    xub: np.ndarray = None


def _ptr(a, ct=C.c_double):
    return None if a is None else a.ctypes.data_as(C.POINTER(ct))


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


class BatchedMPC:
    """One handle == one GPU.  Not re-entrant (like the reference controller, which keeps its
    warm start in `self.optimal_solution`); use one instance per host thread / GPU."""

    @staticmethod
    def make_c_config(lib, cfg):
        """MPCConfig -> the C struct of include/ftmpc.h (defaults from ftmpc_default_config)."""
        c = _lib.ftmpc_config()
        rc = lib.ftmpc_default_config(C.byref(c), cfg.N, cfg.NT)
        if rc != 0:
            raise _lib.FtmpcError(rc, "bad N/NT")
        c.dt, c.mass, c.rho, c.mu_stop = cfg.dt, cfg.mass, cfg.rho, cfg.mu_stop
        c.max_iters, c.device_id = cfg.max_iters, cfg.device_id
        if cfg.dtype not in ("f32", "f64"):
            raise ValueError("dtype must be 'f32' or 'f64'")
        c.dtype = 1 if cfg.dtype == "f64" else 0
        if cfg.kernel_select not in ("auto", "dense", "workgroup", "riccati"):
            raise ValueError("kernel_select must be 'auto', 'dense', 'workgroup' or 'riccati'")
        c.kernel_select = {"auto": _lib.KERNEL_AUTO, "dense": _lib.KERNEL_DENSE, "workgroup": _lib.KERNEL_WORKGROUP,
                           "riccati": _lib.KERNEL_RICCATI}[cfg.kernel_select]
        c.lin_split_max, c.stage_chunks = int(cfg.lin_split_max), int(cfg.stage_chunks)
        c.J[:] = list(_f64(cfg.J, 9))
        D = cfg.D
        if D is None:
            D = allocation_matrix_16() if cfg.NT == 16 else (allocation_matrix_8() if cfg.NT == 8 else None)
        if D is None:
            raise ValueError("MPCConfig.D (6 x NT) is required for NT not in (8, 16)")
        D = _f64(D, (6, cfg.NT))
        flat = np.zeros(6 * _lib.MAX_NT)
        flat[:6 * cfg.NT] = D.reshape(-1)
        c.D[:] = list(flat)
        c.Q[:] = list(_f64(cfg.Q, 9))
        c.R[:] = list(_f64(cfg.R, 6))
        if cfg.P is not None:
            c.P[:] = list(_f64(cfg.P, 81))
        if cfg.r is not None:
            c.r[:] = list(_f64(cfg.r, 3))
        c.f_virt[:] = list(_f64(cfg.f_virt, 3))
        if cfg.xlb is not None or cfg.xub is not None:      # (as the reference: one given, the other defaults to no bound)
            NOB = 1e300
            lo = np.full(13, -np.inf) if cfg.xlb is None else _f64(cfg.xlb, 13)
            hi = np.full(13, np.inf) if cfg.xub is None else _f64(cfg.xub, 13)
            c.state_bounds = 1
            c.xlb[:] = list(np.clip(lo, -NOB, NOB))
            c.xub[:] = list(np.clip(hi, -NOB, NOB))
        ts = cfg.terminal_set
        if ts is not None and ts is not False:
            if ts is True:
                from .controllers.tools.terminal_ingredients import load_terminal
                ts = load_terminal().term_set
            A, b = (ts.A, ts.b) if hasattr(ts, "A") else ts
            A = _f64(A).reshape(-1, 9)
            b = _f64(b).reshape(-1)
            if A.shape[0] != b.size or A.shape[0] > _lib.MAX_TERM_ROWS:
                raise ValueError(f"terminal set must have at most {_lib.MAX_TERM_ROWS} rows of 9 coefficients")
            c.terminal_set, c.term_rows = (1 if cfg.terminal_set_active else 0), A.shape[0]
            flatA = np.zeros(_lib.MAX_TERM_ROWS * 9)
            flatA[:A.size] = A.reshape(-1)
            flatb = np.zeros(_lib.MAX_TERM_ROWS)
            flatb[:b.size] = b
            c.term_A[:] = list(flatA)
            c.term_b[:] = list(flatb)
        tc = cfg.terminal_cost
        if tc is not None and tc is not False:
            if tc is True:
                from .controllers.tools.terminal_ingredients import load_terminal
                tc = load_terminal()
            t = tc.device_tables(_lib.MAX_TCOST, _lib.MAX_TCOST)
            c.terminal_cost_terms, c.tc_npoly, c.tc_nroot = 1, len(t["poly_coef"]), len(t["root_coef"])

            def put(dst, src, n):
                a = np.zeros(n, dtype=np.asarray(src).dtype if np.asarray(src).size else float)
                a[:np.asarray(src).size] = np.asarray(src).reshape(-1)
                dst[:] = list(a)
            put(c.tc_poly_coef, t["poly_coef"], _lib.MAX_TCOST)
            put(c.tc_poly_exp, t["poly_exp"].astype(int), _lib.MAX_TCOST * 9)
            put(c.tc_root_coef, t["root_coef"], _lib.MAX_TCOST)
            put(c.tc_root_eps, t["root_eps"], _lib.MAX_TCOST)
            put(c.tc_root_pow, t["root_pow"], _lib.MAX_TCOST)
            put(c.tc_root_exp, t["root_exp"].astype(int), _lib.MAX_TCOST * 9)
            c.tc_const = float(t["const"])
            if cfg.P is None:
                c.P[:] = list(_f64(tc.P, 81))
        return c

    def __init__(self, cfg: MPCConfig | None = None, **kw):
        cfg = cfg or MPCConfig(**kw)
        self.cfg = cfg
        self.lib = _lib.load_library()
        c = self.make_c_config(self.lib, cfg)
        self.D = np.array(list(c.D))[:6 * cfg.NT].reshape(6, cfg.NT)     # the struct packs D at row stride NT
        self.r = np.array(list(c.r))
        self.P = np.array(list(c.P)).reshape(9, 9)
        self._c = c
        self._h = C.c_void_p()
        rc = self.lib.ftmpc_create(C.byref(c), C.byref(self._h))
        if rc != 0:
            msg = self.lib.ftmpc_last_error(None).decode()
            raise _lib.FtmpcError(rc, msg)

    # -- lifetime -----------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.ftmpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise _lib.FtmpcError(rc, self.lib.ftmpc_last_error(self._h).decode())

    def reserve(self, max_batch: int):
        self._check(self.lib.ftmpc_reserve(self._h, int(max_batch)))

    def kernel_name(self, slot: int) -> str:
        return self.lib.ftmpc_kernel_name(int(slot)).decode()

    # -- host-buffer path ---------------------------------------------------------------
    def _refs(self, B, xref, uref):
        N = self.cfg.N
        xref = _f64(xref)
        xs = 0 if xref.size == 9 * (N + 1) else xref.size // B
        us = 0
        if uref is not None:
            uref = _f64(uref)
            us = 0 if uref.size == 6 * (N + 1) else uref.size // B
        return xref, xs, uref, us

    def solve(self, x0, ub, stuck, xref, uref=None, warmU=None, return_U=False, relinearize=0):
        """x0 [B,13], ub/stuck [B,NT], xref 9x(N+1) column-major flat (shared) or [B, 9(N+1)],
        uref likewise with 6 rows or None (hover), warmU [B,N,NT] or None (updated in place).
        relinearize=k runs k further QP steps, each linearised about the previous solution (sequential
        QP towards the reference's nonlinear program; iterations accumulate).
        Returns dict(u0 [B,NT], U [B,N,NT]|None, status [B], iters [B])."""
        if relinearize > 0:
            out = self.solve(x0, ub, stuck, xref, uref=uref, warmU=warmU, return_U=True)
            W = np.ascontiguousarray(out["U"])
            iters = out["iters"].copy()
            for _ in range(int(relinearize)):
                out = self.solve(x0, ub, stuck, xref, uref=uref, warmU=W, return_U=True)   # W <- U* in place
                iters += out["iters"]
            if warmU is not None:
                warmU[...] = W.reshape(warmU.shape)
            out["iters"] = iters
            if not return_U:
                out["U"] = None
            return out
        N, NT = self.cfg.N, self.cfg.NT
        x0 = _f64(x0).reshape(-1, 13)
        B = x0.shape[0]
        ub = _f64(ub, (B, NT))
        stuck = _f64(stuck, (B, NT))
        xref, xs, uref, us = self._refs(B, xref, uref)
        if warmU is not None and not (isinstance(warmU, np.ndarray) and warmU.dtype == np.float64
                                      and warmU.flags.c_contiguous and warmU.size == B * N * NT):
            raise ValueError("warmU must be a C-contiguous float64 array of B*N*NT (updated in place)")
        u0 = np.empty((B, NT))
        U = np.empty((B, N, NT)) if return_U else None
        status = np.empty(B, np.int32)
        iters = np.empty(B, np.int32)
        self._check(self.lib.ftmpc_solve_batch(self._h, B, _ptr(x0), _ptr(ub), _ptr(stuck), _ptr(xref), xs,
                                               _ptr(uref), us, _ptr(warmU), _ptr(u0), _ptr(U),
                                               _ptr(status, C.c_int32), _ptr(iters, C.c_int32)))
        return dict(u0=u0, U=U, status=status, iters=iters)

    # -- towards the reference's nonlinear program: sequential QP with a line search on the true cost -----------
    def eval_cost(self, x0, ub, stuck, xref, U, uref=None):
        """Cost of the NONLINEAR program (nonlinear rollout, full terminal cost when MPCConfig.terminal_cost is set)
        for thruster sequences U [B,N,NT] -> [B]   (include/ftmpc.h ftmpc_eval_cost_batch)."""
        N, NT = self.cfg.N, self.cfg.NT
        x0 = _f64(x0).reshape(-1, 13)
        B = x0.shape[0]
        ub = _f64(ub, (B, NT))
        stuck = _f64(stuck, (B, NT))
        U = _f64(U, (B, N, NT))
        xref, xs, uref, us = self._refs(B, xref, uref)
        J = np.empty(B)
        self._check(self.lib.ftmpc_eval_cost_batch(self._h, B, _ptr(x0), _ptr(ub), _ptr(stuck), _ptr(xref), xs, _ptr(uref), us,
                                                   _ptr(U), _ptr(J)))
        return J

    def solve_sqp(self, x0, ub, stuck, xref, uref=None, warmU=None, sqp_iters=10, tol=1e-9, backtracks=8):
        """Globalised sequential QP towards the reference's NLP (spiraling_mpc.py:87-238: nonlinear dynamics, full
        terminal cost) in thruster space.  Each major iteration solves the QP linearised about the current U (Hessian
        2 (B'QB + R + rho I) with the quadratic terminal weight P, gradient exact -- including the non-quadratic terminal
        terms when MPCConfig.terminal_cost is set), then backtracks alpha = 1, 1/2, ... along U_qp - U on the TRUE cost
        (eval_cost) until it decreases; an instance stops when no step decreases its cost by more than tol (1 + |J|).
        Plain re-linearisation (`solve(relinearize=k)`) has no such safeguard and oscillates on the smoothed |.|^(1/4)
        terms of the terminal cost.  Returns dict(u0, U, cost [B], cost0 [B] (at the start point), sqp_iters [B],
        iters [B] (IPM iterations summed), status [B] of the last QP)."""
        N, NT = self.cfg.N, self.cfg.NT
        x0 = _f64(x0).reshape(-1, 13)
        B = x0.shape[0]
        ub = _f64(ub, (B, NT))
        stuck = _f64(stuck, (B, NT))
        U = np.zeros((B, N, NT)) if warmU is None else np.clip(_f64(warmU, (B, N, NT)), 0.0, ub[:, None, :])
        J = self.eval_cost(x0, ub, stuck, xref, U, uref)
        J0 = J.copy()
        active = np.ones(B, bool)
        n_major = np.zeros(B, np.int32)
        ipm = np.zeros(B, np.int32)
        status = np.zeros(B, np.int32)
        for _ in range(int(sqp_iters)):
            if not active.any():
                break
            W = U.copy()                      # solve() overwrites its warm-start buffer with the QP solution
            out = self.solve(x0, ub, stuck, xref, uref=uref, warmU=W, return_U=True)     # W <- U_qp
            ipm += np.where(active, out["iters"], 0)
            status = np.where(active, out["status"], status)
            step = np.clip(out["U"], 0.0, ub[:, None, :]) - U      # the fp32 kernels return ub rounded to float32
            alpha = np.ones(B)
            todo = active & (out["status"] != 2)
            improved = np.zeros(B, bool)
            for _bt in range(int(backtracks)):
                if not todo.any():
                    break
                Jt = self.eval_cost(x0, ub, stuck, xref, U + alpha[:, None, None] * step, uref)
                ok = todo & (Jt < J - tol * (1.0 + np.abs(J)))
                U[ok] += alpha[ok, None, None] * step[ok]
                J[ok] = Jt[ok]
                improved |= ok
                todo &= ~ok
                alpha[todo] *= 0.5
            n_major += improved.astype(np.int32)
            active &= improved
        return dict(u0=U[:, 0, :].copy(), U=U, cost=J, cost0=J0, sqp_iters=n_major, iters=ipm, status=status)

    def solve_sqp_device(self, x0, ub, stuck, xref, uref=None, warmU=None, sqp_iters=10, tol=1e-9, backtracks=8):
        """The same line-search SQP with the whole loop on the device (include/ftmpc.h ftmpc_solve_sqp_batch): inputs go up
        once, results come down once; every instance runs `sqp_iters` QP steps and `backtracks` cost evaluations per step
        (a stopped instance's are discarded).  Same return dict as solve_sqp."""
        N, NT = self.cfg.N, self.cfg.NT
        x0 = _f64(x0).reshape(-1, 13)
        B = x0.shape[0]
        ub = _f64(ub, (B, NT))
        stuck = _f64(stuck, (B, NT))
        xref, xs, uref, us = self._refs(B, xref, uref)
        W = None if warmU is None else _f64(warmU, (B, N, NT))
        u0, U = np.empty((B, NT)), np.empty((B, N, NT))
        J, J0 = np.empty(B), np.empty(B)
        nmaj, ipm, st = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32)
        self._check(self.lib.ftmpc_solve_sqp_batch(self._h, B, _ptr(x0), _ptr(ub), _ptr(stuck), _ptr(xref), xs, _ptr(uref), us, _ptr(W),
                                                   int(sqp_iters), int(backtracks), float(tol), _ptr(u0), _ptr(U), _ptr(J), _ptr(J0),
                                                   _ptr(nmaj, C.c_int32), _ptr(ipm, C.c_int32), _ptr(st, C.c_int32)))
        return dict(u0=u0, U=U, cost=J, cost0=J0, sqp_iters=nmaj, iters=ipm, status=st)

    # -- the reference's two-stage structure: 6-D generalized-force QP with the input hull, then allocation ----
    def solve_wrench(self, x0, ub, stuck, xref, uref=None, warmG=None, return_G=False, hull=None, dist=None):
        """One MPC step in generalized-force space (reference: spiraling_mpc.py:87-238 with the per-stage hull rows
        :133-137,175-177) followed by the min-norm allocation (control_allocator.py:65-94).
        x0 [B,13], ub/stuck [B,NT]; warmG [B,N,6] or None (in/out: total wrenches, already shifted);
        hull: dict from controllers.tools.input_bounds.hull_tables (built here when None).
        dist [B,6] or None: the estimated disturbance per vehicle (f^ inertial in N, t^ body in N m) the linearisation rolls the
        model out under (ftmpc_solve_wrench_disturbance_batch; the hull, the allocation and the cost's R term keep the commanded wrench).
        Returns dict(u0 [B,NT], tau0 [B,6], G [B,N,6]|None, status [B], iters [B], alloc_status [B]); instances whose
        healthy thrusters do not span R^6 have no hull: status 3, u0 = tau0 = NaN (use `solve` for them)."""
        from .controllers.tools.input_bounds import hull_tables
        N, NT = self.cfg.N, self.cfg.NT
        x0 = _f64(x0).reshape(-1, 13)
        B = x0.shape[0]
        ub = _f64(ub, (B, NT))
        stuck = _f64(stuck, (B, NT))
        if hull is None:
            hull = hull_tables(self.D, ub, stuck)
        ok = ~np.asarray(hull["degenerate"], bool)
        u0 = np.full((B, NT), np.nan)
        tau0 = np.full((B, 6), np.nan)
        G = np.full((B, N, 6), np.nan) if return_G else None
        status = np.full(B, 3, np.int32)
        iters = np.zeros(B, np.int32)
        ast = np.zeros(B, np.int32)
        if not ok.any():
            return dict(u0=u0, tau0=tau0, G=G, status=status, iters=iters, alloc_status=ast)
        sel = np.flatnonzero(ok)
        full = sel.size == B
        take = (lambda a: a) if full else (lambda a: np.ascontiguousarray(a[sel]))
        xref, xs, uref, us = self._refs(B, xref, uref)
        if xs:
            xref = take(xref.reshape(B, -1))
        if uref is not None and us:
            uref = take(uref.reshape(B, -1))
        W = None
        if warmG is not None:
            if not (isinstance(warmG, np.ndarray) and warmG.dtype == np.float64 and warmG.flags.c_contiguous and warmG.size == B * N * 6):
                raise ValueError("warmG must be a C-contiguous float64 array of B*N*6 (updated in place)")
            W = warmG.reshape(B, N, 6) if full else np.ascontiguousarray(warmG.reshape(B, N, 6)[sel])
        b = sel.size
        A = np.ascontiguousarray(hull["A"], dtype=np.float64)
        hs = np.ascontiguousarray(take(hull["set"]), dtype=np.int32)
        hb = np.ascontiguousarray(take(hull["b"]), dtype=np.float64)
        o_u0, o_t0 = np.empty((b, NT)), np.empty((b, 6))
        o_G = np.empty((b, N, 6)) if return_G else None
        o_st, o_it, o_as = np.empty(b, np.int32), np.empty(b, np.int32), np.empty(b, np.int32)
        if dist is not None:
            self._check(self.lib.ftmpc_solve_wrench_disturbance_batch(
                self._h, b, _ptr(take(x0)), _ptr(take(ub)), _ptr(take(stuck)), _ptr(A), A.shape[0], _ptr(hs, C.c_int32), _ptr(hb),
                int(hull["rows"]), _ptr(xref), xs, _ptr(uref), us, _ptr(W), _ptr(take(_f64(dist, (B, 6)))), _ptr(o_u0), _ptr(o_t0),
                _ptr(o_G), _ptr(o_st, C.c_int32), _ptr(o_it, C.c_int32), _ptr(o_as, C.c_int32)))
        else:
            self._check(self.lib.ftmpc_solve_wrench_batch(
                self._h, b, _ptr(take(x0)), _ptr(take(ub)), _ptr(take(stuck)), _ptr(A), A.shape[0], _ptr(hs, C.c_int32), _ptr(hb),
                int(hull["rows"]), _ptr(xref), xs, _ptr(uref), us, _ptr(W), _ptr(o_u0), _ptr(o_t0), _ptr(o_G),
                _ptr(o_st, C.c_int32), _ptr(o_it, C.c_int32), _ptr(o_as, C.c_int32)))
        u0[sel], tau0[sel], status[sel], iters[sel], ast[sel] = o_u0, o_t0, o_st, o_it, o_as
        if return_G:
            G[sel] = o_G
        if warmG is not None and not full:
            warmG.reshape(B, N, 6)[sel] = W
        return dict(u0=u0, tau0=tau0, G=G, status=status, iters=iters, alloc_status=ast)

    # -- the reference's nonlinear program in its own formulation: line-search SQP over the wrench sequences --------------
    def eval_cost_wrench(self, x0, xref, G, uref=None, return_tviol=False, dist=None):
        """Cost of the NONLINEAR program in the generalized-force formulation for total-wrench sequences G [B,N,6] -> [B]
        (include/ftmpc.h ftmpc_eval_cost_wrench_batch: nonlinear rollout, no rho term, full terminal cost when
        MPCConfig.terminal_cost is set).  return_tviol: (cost, terminal-set violation sum_r max(0, A e_N - b)) instead.
        dist [B,6] or None: the rollout runs under the estimated disturbance (f^ inertial, t^ body) per vehicle
        (ftmpc_eval_cost_wrench_disturbance_batch); the R term keeps the commanded G."""
        N = self.cfg.N
        x0 = _f64(x0).reshape(-1, 13)
        B = x0.shape[0]
        G = _f64(G, (B, N, 6))
        xref, xs, uref, us = self._refs(B, xref, uref)
        J, V = np.empty(B), np.empty(B)
        if dist is not None:
            self._check(self.lib.ftmpc_eval_cost_wrench_disturbance_batch(self._h, B, _ptr(x0), None, None, _ptr(xref), xs, _ptr(uref), us,
                                                                          _ptr(G), _ptr(_f64(dist, (B, 6))), _ptr(J), _ptr(V)))
        else:
            self._check(self.lib.ftmpc_eval_cost_wrench_batch(self._h, B, _ptr(x0), None, None, _ptr(xref), xs, _ptr(uref), us, _ptr(G),
                                                              _ptr(J), _ptr(V)))
        return (J, V) if return_tviol else J

    def solve_sqp_wrench(self, x0, ub, stuck, xref, uref=None, warmG=None, hull=None, sqp_iters=10, backtracks=8, tol=1e-9,
                         penalty=0.0, return_X=False, dist=None):
        """Line-search SQP towards the reference's NLP in its own formulation (spiraling_mpc.py:87-238: generalized-force decision,
        input hull at every stage, terminal set and full terminal cost when configured, RK4 dynamics), entirely on the device
        (include/ftmpc.h ftmpc_solve_sqp_wrench_batch): each major iteration solves the wrench QP of solve_wrench linearised about
        the current G, then backtracks along G_qp - G on the merit J + penalty * terminal-set violation (penalty <= 0: the library
        default); u0 is the min-norm allocation of the final tau_0.  warmG [B,N,6] or None (tau_k = D stuck; read only); hull as
        solve_wrench.  dist [B,6] or None: every linearisation and every cost / merit evaluation runs under the estimated disturbance
        (f^ inertial, t^ body) per vehicle (ftmpc_solve_sqp_wrench_disturbance_batch), so X, cost, cost0 and tviol are the disturbed
        program's.  Returns dict(u0 [B,NT], tau0 [B,6], G [B,N,6], X [B,N+1,13] | None (centre states under G), cost [B],
        cost0 [B] (at the start point), tviol [B], sqp_iters [B], iters [B] (IPM iterations summed), status [B] of the last QP,
        alloc_status [B]); instances whose healthy thrusters do not span R^6 have no hull: status 3, NaN outputs."""
        from .controllers.tools.input_bounds import hull_tables
        N, NT = self.cfg.N, self.cfg.NT
        x0 = _f64(x0).reshape(-1, 13)
        B = x0.shape[0]
        ub = _f64(ub, (B, NT))
        stuck = _f64(stuck, (B, NT))
        if hull is None:
            hull = hull_tables(self.D, ub, stuck)
        ok = ~np.asarray(hull["degenerate"], bool)
        nan = lambda *shape: np.full((B,) + shape, np.nan)
        out = dict(u0=nan(NT), tau0=nan(6), G=nan(N, 6), X=nan(N + 1, 13) if return_X else None, cost=nan(), cost0=nan(), tviol=nan(),
                   sqp_iters=np.zeros(B, np.int32), iters=np.zeros(B, np.int32), status=np.full(B, 3, np.int32),
                   alloc_status=np.zeros(B, np.int32))
        if not ok.any():
            return out
        sel = np.flatnonzero(ok)
        full = sel.size == B
        take = (lambda a: a) if full else (lambda a: np.ascontiguousarray(a[sel]))
        xref, xs, uref, us = self._refs(B, xref, uref)
        if xs:
            xref = take(xref.reshape(B, -1))
        if uref is not None and us:
            uref = take(uref.reshape(B, -1))
        W = None if warmG is None else take(_f64(warmG, (B, N, 6)))
        b = sel.size
        A = np.ascontiguousarray(hull["A"], dtype=np.float64)
        hs = np.ascontiguousarray(take(hull["set"]), dtype=np.int32)
        hb = np.ascontiguousarray(take(hull["b"]), dtype=np.float64)
        o = dict(u0=np.empty((b, NT)), tau0=np.empty((b, 6)), G=np.empty((b, N, 6)), X=np.empty((b, N + 1, 13)) if return_X else None,
                 cost=np.empty(b), cost0=np.empty(b), tviol=np.empty(b), sqp_iters=np.empty(b, np.int32), iters=np.empty(b, np.int32),
                 status=np.empty(b, np.int32), alloc_status=np.empty(b, np.int32))
        ip = lambda a: _ptr(a, C.c_int32)
        head = (self._h, b, _ptr(take(x0)), _ptr(take(ub)), _ptr(take(stuck)), _ptr(A), A.shape[0], ip(hs), _ptr(hb), int(hull["rows"]),
                _ptr(xref), xs, _ptr(uref), us, _ptr(W))
        tail = (int(sqp_iters), int(backtracks), float(tol), float(penalty),
                _ptr(o["u0"]), _ptr(o["tau0"]), _ptr(o["G"]), _ptr(o["X"]), _ptr(o["cost"]), _ptr(o["cost0"]), _ptr(o["tviol"]),
                ip(o["sqp_iters"]), ip(o["iters"]), ip(o["status"]), ip(o["alloc_status"]))
        if dist is not None:
            self._check(self.lib.ftmpc_solve_sqp_wrench_disturbance_batch(*head, _ptr(take(_f64(dist, (B, 6)))), *tail))
        else:
            self._check(self.lib.ftmpc_solve_sqp_wrench_batch(*head, *tail))
        for k, v in o.items():
            if v is not None:
                out[k][sel] = v
        return out

    # -- closed loop on the device (SimulationEnvironment.run_simulation, batched) ------------
    def simulate(self, x0, ub, stuck, xref_traj, T, uref_traj=None, noise=(1e-3, 1e-3, 1e-3, 1e-3), seed=0,
                 return_inputs=False, sqp_iters=0, backtracks=8, tol=1e-9, formulation="thruster", hull=None, penalty=0.0,
                 faults=None, detect_delay=0, return_states=False, outcomes=None, return_status=False, index0=0, index_total=None,
                 plant=None, mission=None, actuator=None, sensor=None, estimator=None, diagnosis=None, disturbance=None,
                 bias_estimate=None, outage=None, environment=None, isolation=None, probe=None):
        """T closed-loop steps (MPC step -> plant RK4 -> noise -> renormalise) without host round trips.
        sqp_iters > 0: every step solves the nonlinear program by that many major iterations of the line-search SQP
        (solve_sqp_device) instead of one QP step.  formulation="wrench": every step is the reference's two-stage structure
        (solve_wrench: generalized-force MPC with the input hull, then allocation); every vehicle's healthy thrusters must span R^6;
        with sqp_iters > 0 every step runs that many major iterations of solve_sqp_wrench (merit weight `penalty`) instead.
        xref_traj: 9 x (T+N) (column t..t+N is the window of step t), uref_traj: 6 x (T+N) or None.
        faults: thruster faults that start mid-run (include/ftmpc.h, ftmpc_fault_schedule): dict(onset [B,E] int (-1: unused slot),
        ub [B,E,NT], stuck [B,E,NT]) -- the full pattern after each event; a leading B may be left out (broadcast).  The plant switches
        at the onset step, the controller detect_delay steps later (int, [B] or [B,E]) and repairs its warm start then.  On the wrench
        form the hull tables are built over all patterns together (hull None, or ft_mpc_amd.faults.fault_hull_tables of the same
        schedule built beforehand).  return_states: also x_hist [T,B,13], the state after each step.
        outcomes: per-vehicle results reduced on the device while the loop runs (include/ftmpc.h, ftmpc_outcomes), so that a campaign
        needs neither history: True for err_int [B,3], err_max [B,3], impulse [B,2] (delivered, commanded), unsolved [B],
        first_unsolved [B], tset_step [B] (when the config has terminal rows) and, wrench form, alloc_failed [B]; a
        dict(tol_pos=, tol_vel=, tol_rate=) adds settle_step [B] for that band (a key fields=[names] asks for exactly those).
        return_status: also status_hist [T,B], the solve status of every vehicle at every step.  index0 / index_total: the call's
        vehicles are [index0, index0 + B) of a campaign of index_total; the noise is then what the same vehicles draw in one call over
        the whole campaign (default: the call is the campaign).
        plant: the plant the loop integrates, per vehicle (include/ftmpc.h, ftmpc_plant_model; ft_mpc_amd.dispersion.sample draws one):
        a dict with any of mass [B], J [B,3,3], D [B,6,NT], force [B,3] (inertial frame), torque [B,3] (body frame); a key that is
        missing takes the config's value (zero for the disturbances).  The controller keeps the nominal model.
        mission: what each vehicle is asked to fly (include/ftmpc.h, ftmpc_mission; ft_mpc_amd.missions builds one): a dict with
        tables [K,9,C], optionally utables [K,6,C], table [B] int (default 0) and offset [B] int (default 0); at step t vehicle b tracks
        the columns offset[b] + t .. offset[b] + t + N of its table (offset[b] + T + N <= C), and its outcomes are measured against
        them.  xref_traj (and uref_traj) must then be None.  outcomes=dict(cost=True, ..), or "cost" among its fields, adds
        outcomes["cost"] [B,3]: the realised sum of e'Qe, of ut'R ut and the terminal cost of the last error; outcomes=True does not.
        actuator: how the plant's thrusters turn a command into force (include/ftmpc.h, ftmpc_actuator; ft_mpc_amd.actuators restates it
        in NumPy): a dict with mode="pwm" | "proportional", substeps (S in [1, 64]: the plant's step becomes S RK4 steps of dt / S, and
        S is the PWM clock), min_on=0 (ticks; shorter pulses are not produced), align="leading" | "centred" | "trailing", tau_on=0.0,
        tau_off=0.0 (s; time constants of rising and falling thrust), state=None ([B,NT] valve states to start from, finite and >= 0,
        e.g. those a previous call returned; in proportional mode a command below 0 leaves a negative state: clamp at 0 before
        handing it on) and fields=(...) among delivered [B] (N s), pulses [B], applied [T,B,NT], ticks [T,B,NT] and state
        [B,NT]; they come back as out["actuator"].  The controller is not told, and the impulse and cost outcomes stay command-level.
        sensor: what the controller knows about the state and when its command takes effect (include/ftmpc.h, ftmpc_sensor;
        ft_mpc_amd.sensors restates it in NumPy): a dict with sigma=(4,) (standard deviations of position, velocity, attitude (rad)
        and rate), bias=None ([B,12], e.g. sensors.sample_bias), seed=0, step0=0 (number of the call's first step, for a continued
        run), latency=0 (d in [0, 8]: the command solved at step t acts at t + d), predict=False (propagate the measurement over the
        d waiting commands and solve for the window d columns later: xref_traj / uref_traj then have T + N + d columns, a mission
        needs offset + T + N + d <= C), pending=None ([B,d,NT] commands applied in the first d steps; default zeros) and fields=(...)
        among meas [T,B,13], pred [T,B,13] and pending [B,d,NT] (the commands not yet applied at the end); they come back as
        out["sensor"].  x, x_hist and the outcomes are the truth; u is the command the plant applied in each step.
        estimator: a navigation filter between the sensor and the solve (include/ftmpc.h, ftmpc_estimator; ft_mpc_amd.estimators
        restates it in NumPy), an error-state extended Kalman filter per vehicle: a dict with every=1 (the measurement update runs on
        the campaign steps c = step0 + t with c % every == 0), p0=(4,), proc_sigma=(4,), meas_sigma=(4,) (standard deviations by
        group: position, velocity, attitude, rate), xhat=None ([B,13]) and cov=None ([B,78] packed or [B,12,12]; needs xhat), the
        priors of the call's first step (default: the first measurement and diag(p0^2)), and fields=(...) among est [T,B,13] (the
        estimate each solve started from, before the sensor's prediction), err_sq [B,4] (summed squared errors against the truth by
        group), xhat [B,13] and cov [B,78] (the priors of step T, to hand to a continued run); they come back as out["estimator"].
        With a predicting sensor the field pred of the sensor holds the estimate propagated over the queue.
        diagnosis: the controller finds thruster faults itself (include/ftmpc.h, ftmpc_diagnosis; ft_mpc_amd.diagnosis restates it in
        NumPy): a bank of CUSUM tests per vehicle, one per hypothesis "thruster i stuck at level l", on
        the measurement against the model's open-loop prediction.  A dict with every=1, levels=(0.0, F_MAX), resid_sigma=(2,)
        (velocity, rate; diagnosis.default_sigma), drift_sigma=(0, 0), threshold, max_detect=2, state=None ([B,14+NT]), llr=None
        ([B,NT*L]), detect=None ((step, thruster, level), each [B,max_detect]) -- what a previous call returned, for a continued run --
        and fields=(...) among detect, pattern, llr_hist, state (default: all).  They come back as out["diagnosis"]: step, thruster,
        level [B,max_detect] (-1: unused), ub, stuck [B,NT] (the controller's pattern after the last step), llr_hist [T,B,NT*L],
        state, llr.  With `faults` the schedule then moves the plant only and detect_delay is not used.  A call without state that
        asks for detect or state starts from xt = x0, n = 0, which the first step's re-anchor replaces by the first measurement
        when step0 % every == 0.
        On formulation="wrench" the diagnosis is opt-in, rebuild_hull=True in the dict (ftmpc_simulate_wrench_diagnosis_batch): after a
        detection the device recomputes the offsets of the vehicle's hull rows for the new pattern (the normals of the pattern it
        started from stay; input_bounds.hull_offsets restates it), so `hull` must be the tables of the call's pattern (the default).
        out["diagnosis"] gains hull_b [B,rows], the controller's offsets after the last step, and no_hull [B], the step of the first
        detection that left a pattern without a hull (-1: none; the offsets then stay as they were); hand both back as
        diagnosis["hull_b"] / diagnosis["no_hull"] for a continued run.  With `faults` no event hull tables are built.
        disturbance: the estimator's filter augmented by a constant force f^ (inertial frame, N) and torque t^ (body frame, N m) per
        vehicle, the frames and units of plant["force"] / plant["torque"], and the estimate given to every consumer of the
        controller's model (include/ftmpc.h, ftmpc_disturbance; ft_mpc_amd.disturbances restates it in NumPy; thruster formulation,
        sqp_iters = 0, needs `estimator`; with the opt-in key wrench=True: formulation="wrench" with sqp_iters >= 0,
        ftmpc_simulate_wrench_disturbance_batch, the hulls, the allocation and the terminal set staying nominal): a dict with p0=(2,), proc_sigma=(2,) (standard deviations of force and torque: initial, and
        per step), compensate=True (the linearisation the QP is built from uses the estimate too, which removes the steady offset of
        a constant disturbance; False: only the filter and the diagnosis do, the controller stays nominal), force=None, torque=None
        ([B,3], the estimates to start from; default 0), cross=None ([B,72] or [B,12,6]; needs force, torque and estimator["xhat"])
        and cov=None ([B,21] packed or [B,6,6]; needs cross) -- what a previous call returned, for a continued run -- and
        fields=(...) among force_hist, torque_hist [T,B,3] (the estimates each solve saw) and state (force, torque [B,3], cross
        [B,72], cov [B,21]: the priors of step T); they come back as out["disturbance"].
        bias_estimate: the estimator's filter augmented by a constant bias of the velocity measurement b_v^ (m/s) and of the rate
        measurement b_w^ (rad/s) per vehicle, the channels 3..5 and 9..11 of sensor["bias"] (include/ftmpc.h, ftmpc_bias_estimate;
        ft_mpc_amd.biases restates it in NumPy; both formulations, sqp_iters >= 0, needs `estimator`, not together with
        `disturbance`): a dict with p0=(2,), proc_sigma=(2,) (standard deviations of the velocity and the rate bias: initial, and per
        step), bias=None ([B,6], the estimates to start from; default 0), cross=None ([B,72] or [B,12,6]; needs bias and
        estimator["xhat"]) and cov=None ([B,21] packed or [B,6,6]; needs cross) -- what a previous call returned, for a continued
        run: the pieces travel in the measured coordinates of ft_mpc_amd.biases, and estimator["cov"] is then P_mm -- and
        fields=(...) among bias_hist [T,B,6] (the estimates of each step) and state (bias [B,6], cross [B,72], cov [B,21]: the
        priors of step T); they come back as out["bias_estimate"].
        outage: measurement dropouts, outliers and an innovation gate in the estimator's filter, decided per vehicle on the device
        (include/ftmpc.h, ftmpc_outage; ft_mpc_amd.outages restates it in NumPy; both formulations, needs `estimator`, not together
        with `disturbance` or `bias_estimate`): a dict with seed=0, p_loss=0.0 and p_recover=1.0 (the availability chain:
        outages.chain_params converts a loss fraction and a mean outage length), p_outlier=0.0 and outlier_sigma=0.0 (one value or 4,
        by group: position, velocity, attitude, rate), gate=0.0 (standard deviations of the scalar innovation; 0: no gate), window=None
        ([B,2] int: a scripted outage [from, to) in campaign steps), state=None ([B,3]: run, lost_steps, longest), rejected=None
        ([B,4]) and outliers=None ([B,4]) -- what a previous call returned, for a continued run -- and fields=(...) among avail,
        outlier, gate [T,B] int, meas [T,B,13] (y_t as the filter and the diagnosis saw it), state, rejected, outliers; they come
        back as out["outage"].  A lost vehicle's filter propagates and its diagnosis waits; outliers reach the diagnosis ungated.
        environment: a disturbance wrench that varies over the run, drawn per vehicle on the device and handed to the plant before every
        plant step (include/ftmpc.h, ftmpc_environment; ft_mpc_amd.environments restates it in NumPy; both formulations): on top of
        plant["force"] / ["torque"], a Gauss-Markov process (sigma=0.0 and tau=1.0, one value or 2: force in N, torque in N m; s), a
        periodic term (amp_force=None, amp_torque=None [B,3], phase=None [B] rad, period=1.0 s) and a kick (kick=None [B,6] while
        window [B,2] int holds: from <= c < to in campaign steps c = step0 + t); seed=0, step0=0 (the sensor's, where the call has
        one), state=None ([B,6]: what a previous call returned, for a continued run; without it the process starts from a stationary
        draw), est_err_sq=None ([B,2], continued likewise; needs `disturbance`) and fields=(...) among wrench [T,B,6] (the wrench of
        every plant step), state, est_err_sq (summed squared error of the disturbance estimate against the wrench, force and
        torque); they come back as out["environment"].  environments.sample draws a campaign's amplitudes, phases and kicks.
        isolation: three safeguards for the diagnosis' decision rule (include/ftmpc.h, ftmpc_isolation; ft_mpc_amd.diagnosis.replay
        with isolation= restates them in NumPy; both formulations; needs `diagnosis`): consist=0.0 (the gate on the fit q_h of a
        hypothesis, in standard deviations: diagnosis.consist_for(p); 0: no gate), persist=1 (tests in a row with the same leader
        before the decision), revise=False (the level of a detected thruster is tested on and may be revised), lead=None ([B,2] int:
        leader and run, what a previous call returned; needs diagnosis['state']), voided=None ([B]) and revised=None ([B]),
        continued likewise, and fields=(...) among lead, voided, revised, fit [T,B,2] (q_0 and the smallest q_h of every tested
        step, else -1); they come back as out["isolation"].
        probe: test pulses for thrusters that have been quiet (include/ftmpc.h, ftmpc_probe; ft_mpc_amd.probes restates the step
        in NumPy; both formulations; needs `diagnosis`): amp (the pulse, N), quiet=0.0 (a command below it counts as idle),
        idle_steps (idle steps before a pulse), max_pulses=0 (per thruster and vehicle; 0: no cap), reinstate=False (a detected
        thruster is pulsed too and tested for "healthy after all": the entry (c, i, n_levels), ub_c,i = restore_ub), restore_ub,
        the carried idle / pulses [B,NT], impulse [B], pacc / health [B,NT] (these two need the diagnosis' state), reinstated [B]
        and fields=(...) among thruster_hist [T,B], idle, pulses, impulse, pacc, health, reinstated; they come back as out["probe"].
        Returns dict(x [B,13] final states, u [T,B,NT]|None (commanded), not_converged [T][, alloc_failed [T]][, x_hist][, outcomes]
        [, status_hist][, actuator][, sensor][, estimator][, diagnosis][, disturbance][, bias_estimate][, outage][, environment][, isolation][, probe])."""
        return _simulate(self, False, x0, ub, stuck, xref_traj, T, uref_traj, noise, seed, return_inputs, sqp_iters, backtracks, tol,
                         formulation, hull, penalty, faults, detect_delay, return_states, outcomes, return_status, index0, index_total,
                         plant, mission, actuator, sensor, estimator, diagnosis, disturbance, bias_estimate, outage, environment,
                         isolation, probe)

    def hull_offsets(self, ub, stuck, hull):
        """Offsets of the patterns ub / stuck [B,NT] on the normals of `hull` (a dict from input_bounds.hull_tables: A, set [B], rows),
        on the device (ftmpc_hull_offsets_batch; input_bounds.hull_offsets restates it).  Returns dict(b [B,rows], flat [B] bool)."""
        NT = self.cfg.NT
        ub = _f64(ub).reshape(-1, NT)
        B = ub.shape[0]
        stuck = _f64(stuck, (B, NT))
        A = np.ascontiguousarray(hull["A"], dtype=np.float64).reshape(-1, int(hull["rows"]), 6)
        hs = np.ascontiguousarray(hull["set"], dtype=np.int32).reshape(-1)
        if hs.shape != (B,):
            raise ValueError(f"hull['set'] must have shape {(B,)}")
        b = np.empty((B, A.shape[1]))
        flat = np.empty(B, np.int32)
        self._check(self.lib.ftmpc_hull_offsets_batch(self._h, B, _ptr(ub), _ptr(stuck), _ptr(A), A.shape[0], _ptr(hs, C.c_int32),
                                                      A.shape[1], _ptr(b), _ptr(flat, C.c_int32)))
        return dict(b=b, flat=flat.astype(bool))

    def sqp_graph_launches(self) -> int:
        """Calls of solve_sqp_device on this handle that were replayed from the recorded hipGraph (ftmpc_sqp_graph_launches)."""
        return int(self.lib.ftmpc_sqp_graph_launches(self._h))

    def last_handed_over(self) -> int:
        """Instances of the last two-stage step that the one-wave fp32 kernel handed to the float64 kernel (ftmpc_last_handed_over)."""
        c = C.c_int64(0)
        self._check(self.lib.ftmpc_last_handed_over(self._h, C.byref(c)))
        return int(c.value)

    # -- standalone thruster allocation (ControlAllocator.get_physical_input, batched) ---------
    def allocate(self, tau, ub):
        """min |u|^2 s.t. D u = tau, 0 <= u <= ub for B generalized forces tau [B,6] (reference:
        controllers/tools/control_allocator.py:27-40,65-94).  Returns dict(u [B,NT], status [B], iters [B]);
        status 2 = tau not attainable with these bounds (the reference exit()s there)."""
        NT = self.cfg.NT
        tau = _f64(tau).reshape(-1, 6)
        B = tau.shape[0]
        ub = _f64(ub, (B, NT))
        u = np.empty((B, NT))
        status = np.zeros(B, np.int32)
        iters = np.zeros(B, np.int32)
        self._check(self.lib.ftmpc_allocate_batch(self._h, B, _ptr(tau), _ptr(ub), _ptr(u), _ptr(status, C.c_int32),
                                                  _ptr(iters, C.c_int32)))
        return dict(u=u, status=status, iters=iters)

    # -- device-pointer path (HBM-resident inputs; used by bench.py with torch tensors) --
    def solve_device(self, B, x0, ub, stuck, xref, xref_stride, uref, uref_stride, warmU, out_u0, out_U,
                     status, iters, stream=0):
        """All buffer arguments are integer device addresses (e.g. torch.Tensor.data_ptr())."""
        vp = lambda p: C.c_void_p(int(p)) if p else None
        self._check(self.lib.ftmpc_solve_batch_device(self._h, int(B), vp(x0), vp(ub), vp(stuck), vp(xref),
                                                      int(xref_stride), vp(uref), int(uref_stride), vp(warmU),
                                                      vp(out_u0), vp(out_U), vp(status), vp(iters), vp(stream)))

    def set_profiling(self, on: bool):
        self._check(self.lib.ftmpc_set_profiling(self._h, 1 if on else 0))

    def last_kernel_ms(self):
        """{kernel name: device ms} of the last profiled solve (kernels that were launched)."""
        ms = (C.c_float * _lib.KERNEL_SLOTS)()
        self._check(self.lib.ftmpc_last_kernel_ms(self._h, ms, _lib.KERNEL_SLOTS))
        return {self.lib.ftmpc_routed_kernel_name(self._h, k).decode(): float(ms[k]) for k in range(_lib.KERNEL_SLOTS) if ms[k] > 0}

    # -- test hook ----------------------------------------------------------------------
    def debug_build_qp(self, x0, ub, stuck, xref, inst, uref=None, warmU=None):
        N, NT = self.cfg.N, self.cfg.NT
        x0 = _f64(x0).reshape(-1, 13)
        B = x0.shape[0]
        ub = _f64(ub, (B, NT))
        stuck = _f64(stuck, (B, NT))
        xref, xs, uref, us = self._refs(B, xref, uref)
        warm = None if warmU is None else _f64(warmU)
        nmax = N * NT
        H = np.zeros(nmax * nmax)
        g = np.zeros(nmax)
        lo = np.zeros(nmax)
        hi = np.zeros(nmax)
        n = C.c_int32(0)
        self._check(self.lib.ftmpc_debug_build_qp(self._h, B, _ptr(x0), _ptr(ub), _ptr(stuck), _ptr(xref), xs,
                                                  _ptr(uref), us, _ptr(warm), int(inst), _ptr(H), H.size,
                                                  _ptr(g), _ptr(lo), _ptr(hi), C.byref(n)))
        n = n.value
        return H[:n * n].reshape(n, n).copy(), g[:n].copy(), lo[:n].copy(), hi[:n].copy()

    def debug_records(self, x0, ub, stuck, xref, uref=None, warmU=None):
        """The linearisation records [B, N, 152] (csrc/ftmpc_common.h REC_*) of a host batch, from the kernel this handle's
        lin_split_max picks for B."""
        N, NT = self.cfg.N, self.cfg.NT
        x0 = _f64(x0).reshape(-1, 13)
        B = x0.shape[0]
        ub = _f64(ub, (B, NT))
        stuck = _f64(stuck, (B, NT))
        xref, xs, uref, us = self._refs(B, xref, uref)
        warm = None if warmU is None else _f64(warmU, (B, N, NT))
        rec = np.zeros((B, N, 152))
        self._check(self.lib.ftmpc_debug_records(self._h, B, _ptr(x0), _ptr(ub), _ptr(stuck), _ptr(xref), xs,
                                                 _ptr(uref), us, _ptr(warm), _ptr(rec)))
        return rec

    def debug_records_disturbance(self, x0, ub, stuck, xref, dist, uref=None, warmU=None):
        """debug_records through the linearise kernel's instantiation with the estimated disturbance dist [B,6] = (f^ inertial,
        t^ body): what a loop with disturbance["compensate"] launches (ftmpc_debug_records_disturbance)."""
        N, NT = self.cfg.N, self.cfg.NT
        x0 = _f64(x0).reshape(-1, 13)
        B = x0.shape[0]
        ub = _f64(ub, (B, NT))
        stuck = _f64(stuck, (B, NT))
        dist = _f64(dist, (B, 6))
        xref, xs, uref, us = self._refs(B, xref, uref)
        warm = None if warmU is None else _f64(warmU, (B, N, NT))
        rec = np.zeros((B, N, 152))
        self._check(self.lib.ftmpc_debug_records_disturbance(self._h, B, _ptr(x0), _ptr(ub), _ptr(stuck), _ptr(xref), xs,
                                                             _ptr(uref), us, _ptr(warm), _ptr(dist), _ptr(rec)))
        return rec

    def debug_struct_grad(self, x0, ub, stuck, xref, d, form, uref=None, warmU=None):
        """The float64 reference gradient of the fp32 solve kernels at `d` [B, N*NT] (float32; an instance's n = N*na values
        first, stage-major over its active thrusters), without the 2 rho (ubar + d) term: [B, N*NT] float64 in the same layout.
        form 0: the MFMA chains, 1: the vector FMAs.  fp32 handles with N <= 21, NT <= 8."""
        N, NT = self.cfg.N, self.cfg.NT
        x0 = _f64(x0).reshape(-1, 13)
        B = x0.shape[0]
        ub = _f64(ub, (B, NT))
        stuck = _f64(stuck, (B, NT))
        xref, xs, uref, us = self._refs(B, xref, uref)
        warm = None if warmU is None else _f64(warmU, (B, N, NT))
        d = np.ascontiguousarray(d, dtype=np.float32).reshape(B, N * NT)
        g = np.zeros((B, N * NT))
        self._check(self.lib.ftmpc_debug_struct_grad(self._h, B, _ptr(x0), _ptr(ub), _ptr(stuck), _ptr(xref), xs,
                                                     _ptr(uref), us, _ptr(warm), _ptr(d, C.c_float), int(form), _ptr(g)))
        return g


OUTCOME_FIELDS = (("err_int", 3, np.float64), ("err_max", 3, np.float64), ("impulse", 2, np.float64), ("settle_step", 0, np.int32),
                  ("tset_step", 0, np.int32), ("unsolved", 0, np.int32), ("first_unsolved", 0, np.int32), ("alloc_failed", 0, np.int32))


def _outcome_request(obj, B, T, wrench, outcomes, return_status, index0, index_total):
    """The ftmpc_outcomes struct of a simulate call and the arrays it points into: (struct, dict of outcome arrays | None,
    status_hist | None)."""
    oc = _lib.ftmpc_outcomes(struct_size=C.sizeof(_lib.ftmpc_outcomes), index0=int(index0),
                             index_total=0 if index_total is None else int(index_total))
    arrays = None
    if outcomes is not None and outcomes is not False:
        spec = {} if outcomes is True else dict(outcomes)
        names = spec.pop("fields", None)
        tols = [spec.pop(k, None) for k in ("tol_pos", "tol_vel", "tol_rate")]
        if spec:
            raise ValueError(f"outcomes: unknown keys {sorted(spec)}")
        if any(t is not None for t in tols) and not all(t is not None for t in tols):
            raise ValueError("outcomes: tol_pos, tol_vel and tol_rate come together")
        if tols[0] is not None:
            oc.tol_pos, oc.tol_vel, oc.tol_rate = (float(t) for t in tols)
        if names is None:
            names = [n for n, _, _ in OUTCOME_FIELDS
                     if not (n == "settle_step" and tols[0] is None) and not (n == "tset_step" and obj._c.term_rows == 0)
                     and not (n == "alloc_failed" and not wrench)]
        arrays = {}
        for n, w, dt in OUTCOME_FIELDS:
            if n in names:
                arrays[n] = np.zeros((B, w) if w else (B,), dt)
                setattr(oc, n, _ptr(arrays[n], C.c_double if dt is np.float64 else C.c_int32))
        if len(arrays) != len(names):
            raise ValueError(f"outcomes: fields must be among {[n for n, _, _ in OUTCOME_FIELDS]}")
    sh = None
    if return_status:
        sh = np.zeros((T, B), np.int32)
        oc.status_hist = _ptr(sh, C.c_int32)
    return oc, arrays, sh


PLANT_FIELDS = (("mass", ()), ("J", (3, 3)), ("D", (6, None)), ("force", (3,)), ("torque", (3,)))      # None: NT


def _plant_request(plant, B, NT):
    """The ftmpc_plant_model struct of a simulate call and the arrays it points into (kept alive by the caller)."""
    spec = dict(plant)
    pm = _lib.ftmpc_plant_model(struct_size=C.sizeof(_lib.ftmpc_plant_model))
    keep = []
    for name, tail in PLANT_FIELDS:
        a = spec.pop(name, None)
        if a is None:
            continue
        shape = (B,) + tuple(NT if d is None else d for d in tail)
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != shape:
            raise ValueError(f"plant[{name!r}] must have shape {shape}, not {a.shape}")
        keep.append(a)
        setattr(pm, name, _ptr(a))
    if spec:
        raise ValueError(f"plant: unknown keys {sorted(spec)}")
    return pm, keep


def _mission_request(mission, B, T, N, want_cost):
    """The ftmpc_mission struct of a simulate call, the arrays it points into (kept alive by the caller) and the cost array | None.
    mission None: the struct only asks for cost (n_tables = 0)."""
    ms = _lib.ftmpc_mission(struct_size=C.sizeof(_lib.ftmpc_mission))
    keep = []
    if mission is not None:
        spec = dict(mission)
        tables = spec.pop("tables", None)
        if tables is None:
            raise ValueError("mission: needs tables [K,9,C]")
        tables = _f64(tables)
        if tables.ndim != 3 or tables.shape[0] < 1 or tables.shape[1] != 9:
            raise ValueError(f"mission['tables'] must have shape [K,9,C] with K >= 1, not {tables.shape}")
        K, _, Cn = tables.shape
        xt = np.ascontiguousarray(tables.transpose(0, 2, 1))      # [K][C][9]: every table column-major
        keep.append(xt)
        ms.n_tables, ms.n_cols, ms.xref = K, Cn, _ptr(xt)
        ut = spec.pop("utables", None)
        if ut is not None:
            ut = _f64(ut)
            if ut.shape != (K, 6, Cn):
                raise ValueError(f"mission['utables'] must have shape {(K, 6, Cn)}, not {ut.shape}")
            ut = np.ascontiguousarray(ut.transpose(0, 2, 1))
            keep.append(ut)
            ms.uref = _ptr(ut)
        for name in ("table", "offset"):
            a = spec.pop(name, None)
            if a is None:
                continue
            a = np.asarray(a)
            if a.shape != (B,) or not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"mission[{name!r}] must be {B} integers, not {a.dtype} {a.shape}")
            a = np.ascontiguousarray(a, dtype=np.int32)
            keep.append(a)
            setattr(ms, name, _ptr(a, C.c_int32))
        if spec:
            raise ValueError(f"mission: unknown keys {sorted(spec)}")
    cost = None
    if want_cost:
        cost = np.zeros((B, 3))
        ms.cost = _ptr(cost)
    return ms, keep, cost


ACTUATOR_MODES = {"proportional": 0, "pwm": 1}
ACTUATOR_ALIGN = {"leading": 0, "centred": 1, "trailing": 2}
ACTUATOR_FIELDS = ("delivered", "pulses", "applied", "ticks", "state")


def _actuator_request(actuator, B, T, NT):
    """The ftmpc_actuator struct of a simulate call, the arrays it points into (kept alive by the caller) and the dict of outputs."""
    spec = dict(actuator)
    mode = spec.pop("mode", "proportional")
    if mode not in ACTUATOR_MODES:
        raise ValueError(f"actuator['mode'] must be one of {sorted(ACTUATOR_MODES)}, not {mode!r}")
    align = spec.pop("align", "leading")
    if align not in ACTUATOR_ALIGN:
        raise ValueError(f"actuator['align'] must be one of {sorted(ACTUATOR_ALIGN)}, not {align!r}")
    S = int(spec.pop("substeps", 1))
    if not 1 <= S <= 64:
        raise ValueError(f"actuator['substeps'] must be in [1, 64], not {S}")
    min_on = int(spec.pop("min_on", 0))
    if not 0 <= min_on <= S:
        raise ValueError(f"actuator['min_on'] must be in [0, substeps = {S}], not {min_on}")
    taus = [float(spec.pop(k, 0.0)) for k in ("tau_on", "tau_off")]
    if not all(np.isfinite(t) and t >= 0 for t in taus):
        raise ValueError("actuator: tau_on and tau_off must be finite and >= 0")
    fields = tuple(spec.pop("fields", ()))
    if any(f not in ACTUATOR_FIELDS for f in fields):
        raise ValueError(f"actuator['fields'] must be among {list(ACTUATOR_FIELDS)}")
    if mode == "proportional":
        if min_on != 0 or align != "leading":
            raise ValueError("actuator: min_on and align belong to mode='pwm'")
        if "pulses" in fields or "ticks" in fields:
            raise ValueError("actuator: the fields pulses and ticks belong to mode='pwm'")
    state = spec.pop("state", None)
    if spec:
        raise ValueError(f"actuator: unknown keys {sorted(spec)}")
    ac = _lib.ftmpc_actuator(struct_size=C.sizeof(_lib.ftmpc_actuator), mode=ACTUATOR_MODES[mode], substeps=S, min_on=min_on,
                             align=ACTUATOR_ALIGN[align], tau_on=taus[0], tau_off=taus[1])
    out = {}
    if state is not None or "state" in fields:
        st = np.zeros((B, NT)) if state is None else np.array(state, dtype=np.float64)      # a copy: the call writes into it
        if st.shape != (B, NT):
            raise ValueError(f"actuator['state'] must have shape {(B, NT)}, not {st.shape}")
        if not (np.isfinite(st).all() and (st >= 0).all()):
            raise ValueError("actuator['state'] must be finite and >= 0")
        st = np.ascontiguousarray(st)
        ac.state = _ptr(st)
        if "state" in fields:
            out["state"] = st
        else:
            out["_state"] = st
    if "delivered" in fields:
        out["delivered"] = np.zeros(B)
        ac.delivered = _ptr(out["delivered"])
    if "pulses" in fields:
        out["pulses"] = np.zeros(B, np.int32)
        ac.pulses = _ptr(out["pulses"], C.c_int32)
    if "applied" in fields:
        out["applied"] = np.zeros((T, B, NT))
        ac.applied_hist = _ptr(out["applied"])
    if "ticks" in fields:
        out["ticks"] = np.zeros((T, B, NT), np.int32)
        ac.ticks_hist = _ptr(out["ticks"], C.c_int32)
    keep = list(out.values())
    out.pop("_state", None)
    return ac, keep, out


def _sensor_request(sensor, B, T, NT):
    """The ftmpc_sensor struct of a simulate call, the arrays it points into (kept alive by the caller), the dict of outputs and L, the
    columns the reference gains (the latency of a predicting sensor)."""
    from .sensors import request
    r = request(sensor, B, T, NT)
    se = _lib.ftmpc_sensor(struct_size=C.sizeof(_lib.ftmpc_sensor), latency=r["latency"], predict=int(r["predict"]),
                           seed=r["seed"] & ((1 << 64) - 1), step0=r["step0"])
    for k in range(4):
        se.sigma[k] = float(r["sigma"][k])
    keep, out = [], {}
    if r["bias"] is not None:
        keep.append(r["bias"])
        se.bias = _ptr(r["bias"])
    if r["pending"] is not None or "pending" in r["fields"]:
        pend = np.ascontiguousarray(r["pending"]) if r["pending"] is not None else np.zeros((B, r["latency"], NT))
        keep.append(pend)
        se.pending = _ptr(pend)
        if "pending" in r["fields"]:
            out["pending"] = pend
    if "meas" in r["fields"]:
        out["meas"] = np.zeros((T, B, 13))
        se.meas_hist = _ptr(out["meas"])
    if "pred" in r["fields"]:
        out["pred"] = np.zeros((T, B, 13))
        se.pred_hist = _ptr(out["pred"])
    return se, keep, out, (r["latency"] if r["predict"] else 0)


def _estimator_request(estimator, B, T):
    """The ftmpc_estimator struct of a simulate call, the arrays it points into (kept alive by the caller) and the dict of outputs."""
    from .estimators import NP, request
    r = request(estimator, B, T)
    es = _lib.ftmpc_estimator(struct_size=C.sizeof(_lib.ftmpc_estimator), every=r["every"])
    for k in range(4):
        es.p0[k], es.proc_sigma[k], es.meas_sigma[k] = float(r["p0"][k]), float(r["proc_sigma"][k]), float(r["meas_sigma"][k])
    keep, out = [], {}
    # xhat / cov are in/out: asked back without being handed over, they start as the library's defaults would (the first measurement
    # cannot be staged here, so xhat then comes back through a buffer the call fills from its first step on)
    if r["xhat"] is not None:
        keep.append(r["xhat"])
        es.xhat = _ptr(r["xhat"])
        if "xhat" in r["fields"]:
            out["xhat"] = r["xhat"]
        cov = r["cov"]
        if cov is None and "cov" in r["fields"]:
            cov = np.zeros((B, NP))
            cov[:, np.cumsum([0] + [12 - i for i in range(11)])] = np.repeat(r["p0"] ** 2, 3)[None, :]
        if cov is not None:
            keep.append(cov)
            es.cov = _ptr(cov)
            if "cov" in r["fields"]:
                out["cov"] = cov
    elif "xhat" in r["fields"] or "cov" in r["fields"]:
        raise ValueError("estimator: the fields xhat and cov need estimator['xhat'] (e.g. the first measurement) to be handed in")
    if "est" in r["fields"]:
        out["est"] = np.zeros((T, B, 13))
        es.est_hist = _ptr(out["est"])
    if "err_sq" in r["fields"]:
        out["err_sq"] = np.zeros((B, 4))
        es.err_sq = _ptr(out["err_sq"])
    return es, keep, out


def _diagnosis_request(diagnosis, x0, B, T, NT, estimator, sensor, reinstating=False):
    """The ftmpc_diagnosis struct of a simulate call, the arrays it points into (kept alive by the caller) and the dict of outputs."""
    from .diagnosis import request
    r = request(diagnosis, B, T, NT, estimator, sensor, F_MAX, reinstating)
    L, K = r["levels"].size, r["max_detect"]
    dg = _lib.ftmpc_diagnosis(struct_size=C.sizeof(_lib.ftmpc_diagnosis), every=r["every"], n_levels=L, max_detect=K,
                              threshold=r["threshold"])
    for k in range(L):
        dg.levels[k] = float(r["levels"][k])
    for k in range(2):
        dg.resid_sigma[k], dg.drift_sigma[k] = float(r["resid_sigma"][k]), float(r["drift_sigma"][k])
    keep, out = [], {}
    state, llr, det = r["state"], r["llr"], r["detect"]
    if state is None and ("detect" in r["fields"] or "state" in r["fields"]):
        # state, llr and the detect arrays are in/out: asked back without being handed over, the run starts from xt = x0, n = 0
        state = np.zeros((B, 14 + NT))
        state[:, 0:13] = x0
        det = tuple(np.full((B, K), -1, np.int32) for _ in range(3))
    if state is not None:
        if llr is None and "state" in r["fields"]:      # (not handed over and not asked back: filled on the device, nothing staged)
            llr = np.zeros((B, NT * L))
        keep += [state, llr, *det]
        dg.state, dg.llr = _ptr(state), _ptr(llr)
        dg.detect_step, dg.detect_thruster, dg.detect_level = (_ptr(a, C.c_int32) for a in det)
        if "detect" in r["fields"]:
            out["step"], out["thruster"], out["level"] = det
        if "state" in r["fields"]:
            out["state"], out["llr"] = state, llr
    if "pattern" in r["fields"]:
        out["ub"], out["stuck"] = np.zeros((B, NT)), np.zeros((B, NT))
        dg.ub, dg.stuck = _ptr(out["ub"]), _ptr(out["stuck"])
    if "llr_hist" in r["fields"]:
        out["llr_hist"] = np.zeros((T, B, NT * L))
        dg.llr_hist = _ptr(out["llr_hist"])
    return dg, keep, out


def _disturbance_request(disturbance, B, T, estimator, sqp_iters, formulation):
    """The ftmpc_disturbance struct of a simulate call, the arrays it points into (kept alive by the caller) and the dict of outputs."""
    from .disturbances import NC, NDD, request
    r = request(disturbance, B, T, estimator, sqp_iters, formulation)
    db = _lib.ftmpc_disturbance(struct_size=C.sizeof(_lib.ftmpc_disturbance), compensate=int(r["compensate"]))
    for k in range(2):
        db.p0[k], db.proc_sigma[k] = float(r["p0"][k]), float(r["proc_sigma"][k])
    keep, out = [], {}
    force, torque, cross, cov = r["force"], r["torque"], r["cross"], r["cov"]
    if "state" in r["fields"]:
        # in/out: asked back without being handed over, they start as the library's defaults would; cross and cov need the
        # estimator's xhat (without it the first step initialises the filter on the device and nothing is staged)
        force = np.zeros((B, 3)) if force is None else force
        torque = np.zeros((B, 3)) if torque is None else torque
        if estimator.get("xhat") is not None:
            cross = np.zeros((B, NC)) if cross is None else cross
            if cov is None:
                cov = np.zeros((B, NDD))
                cov[:, np.cumsum([0, 6, 5, 4, 3, 2])] = np.repeat(r["p0"] ** 2, 3)[None, :]
        elif cross is not None or cov is not None:
            raise ValueError("disturbance['cross'] requires estimator['xhat']")
        out["force"], out["torque"] = force, torque
        if cross is not None:
            out["cross"], out["cov"] = cross, cov
    keep += [force, torque, cross, cov]
    db.force, db.torque, db.cross, db.cov = _ptr(force), _ptr(torque), _ptr(cross), _ptr(cov)
    if "force_hist" in r["fields"]:
        out["force_hist"] = np.zeros((T, B, 3))
        db.force_hist = _ptr(out["force_hist"])
    if "torque_hist" in r["fields"]:
        out["torque_hist"] = np.zeros((T, B, 3))
        db.torque_hist = _ptr(out["torque_hist"])
    return db, keep, out


def _bias_request(bias_estimate, B, T, estimator, disturbance, es, ekeep):
    """The ftmpc_bias_estimate struct of a simulate call, the arrays it points into (kept alive by the caller) and the dict of outputs."""
    from .biases import NC, NDD, request
    from .estimators import NP
    r = request(bias_estimate, B, T, estimator, disturbance)
    be = _lib.ftmpc_bias_estimate(struct_size=C.sizeof(_lib.ftmpc_bias_estimate))
    for k in range(2):
        be.p0[k], be.proc_sigma[k] = float(r["p0"][k]), float(r["proc_sigma"][k])
    keep, out = [], {}
    bias, cross, cov = r["bias"], r["cross"], r["cov"]
    if "state" in r["fields"]:
        # in/out: asked back without being handed over, they start as the library's defaults would; cross and cov need the
        # estimator's xhat (without it the first step initialises the filter on the device and nothing is staged)
        bias = np.zeros((B, 6)) if bias is None else bias
        if estimator.get("xhat") is not None:
            pb = np.repeat(r["p0"] ** 2, 3)
            if cross is None:
                # the pieces in measured coordinates the library forms when no cross is handed (ft_mpc_amd.biases.prior): the
                # estimator's covariance gains p0^2 on its velocity and rate diagonals and is handed over as P_mm
                covx = next((a for a in ekeep if a.shape == (B, NP)), None)
                if covx is None:
                    covx = np.zeros((B, NP))
                    covx[:, np.cumsum([0] + [12 - i for i in range(11)])] = np.repeat(np.array(list(es.p0)) ** 2, 3)[None, :]
                    keep.append(covx)
                    es.cov = _ptr(covx)
                tri = np.cumsum([0] + [12 - i for i in range(11)])
                covx[:, tri[3:6]] += pb[None, 0:3]
                covx[:, tri[9:12]] += pb[None, 3:6]
                cross = np.zeros((B, 12, 6))
                cross[:, np.arange(3, 6), np.arange(0, 3)] = pb[None, 0:3]
                cross[:, np.arange(9, 12), np.arange(3, 6)] = pb[None, 3:6]
                cross = cross.reshape(B, NC)
            if cov is None:
                cov = np.zeros((B, NDD))
                cov[:, np.cumsum([0, 6, 5, 4, 3, 2])] = pb[None, :]
        elif cross is not None or cov is not None:
            raise ValueError("bias_estimate['cross'] requires estimator['xhat']")
        out["bias"] = bias
        if cross is not None:
            out["cross"], out["cov"] = cross, cov
    keep += [bias, cross, cov]
    be.bias, be.cross, be.cov = _ptr(bias), _ptr(cross), _ptr(cov)
    if "bias_hist" in r["fields"]:
        out["bias_hist"] = np.zeros((T, B, 6))
        be.bias_hist = _ptr(out["bias_hist"])
    return be, keep, out


def _outage_request(outage, B, T, estimator, disturbance, bias_estimate):
    """The ftmpc_outage struct of a simulate call, the arrays it points into (kept alive by the caller) and the dict of outputs."""
    from .outages import request
    r = request(outage, B, T, estimator, disturbance, bias_estimate)
    og = _lib.ftmpc_outage(struct_size=C.sizeof(_lib.ftmpc_outage), seed=r["seed"] & ((1 << 64) - 1), p_loss=r["p_loss"],
                           p_recover=r["p_recover"], gate=r["gate"])
    for k in range(4):
        og.p_outlier[k], og.outlier_sigma[k] = float(r["p_outlier"][k]), float(r["outlier_sigma"][k])
    keep, out = [], {}
    if r["window"] is not None:
        keep.append(r["window"])
        og.window = _ptr(r["window"], C.c_int32)
    # state, rejected and outliers are in/out: asked back without being handed over, they start as the library's defaults (zeros)
    for name, width in (("state", 3), ("rejected", 4), ("outliers", 4)):
        a = r[name]
        if a is None and name in r["fields"]:
            a = np.zeros((B, width), np.int32)
        if a is not None:
            keep.append(a)
            setattr(og, name, _ptr(a, C.c_int32))
            if name in r["fields"]:
                out[name] = a
    for name, field in (("avail", "avail_hist"), ("outlier", "outlier_hist"), ("gate", "gate_hist")):
        if name in r["fields"]:
            out[name] = np.zeros((T, B), np.int32)
            setattr(og, field, _ptr(out[name], C.c_int32))
    if "meas" in r["fields"]:
        out["meas"] = np.zeros((T, B, 13))
        og.meas_hist = _ptr(out["meas"])
    return og, keep, out


def _environment_request(environment, B, T, sensor, disturbance, index0, index_total):
    """The ftmpc_environment struct of a simulate call, the arrays it points into (kept alive by the caller) and the dict of outputs."""
    from .environments import request, stationary
    r = request(environment, B, T, sensor, disturbance)
    ev = _lib.ftmpc_environment(struct_size=C.sizeof(_lib.ftmpc_environment), seed=r["seed"] & ((1 << 64) - 1), step0=r["step0"],
                                period=r["period"])
    for a in range(2):
        ev.sigma[a], ev.tau[a] = float(r["sigma"][a]), float(r["tau"][a])
    keep, out = [], {}
    for name in ("amp_force", "amp_torque", "phase", "kick"):
        if r[name] is not None:
            keep.append(r[name])
            setattr(ev, name, _ptr(r[name]))
    if r["window"] is not None:
        keep.append(r["window"])
        ev.window = _ptr(r["window"], C.c_int32)
    # state and est_err_sq are in/out.  At the ABI a state pointer means "handed over", so a state asked back from a run that starts
    # stationary needs the stationary draw made here (environments.stationary restates the library's) and handed over
    for name, width in (("state", 6), ("est_err_sq", 2)):
        a = r[name]
        if a is None and name in r["fields"]:
            a = (stationary(B, r["sigma"], r["seed"], r["step0"], index0, index_total) if name == "state" else np.zeros((B, width)))
        if a is not None:
            keep.append(a)
            setattr(ev, name, _ptr(a))
            if name in r["fields"]:
                out[name] = a
    if "wrench" in r["fields"]:
        out["wrench"] = np.zeros((T, B, 6))
        ev.wrench_hist = _ptr(out["wrench"])
    return ev, keep, out


def _isolation_request(isolation, B, T, NT, diagnosis, reinstating=False):
    """The ftmpc_isolation struct of a simulate call, the arrays it points into (kept alive by the caller) and the dict of outputs."""
    from .diagnosis import isolation_request
    r = isolation_request(isolation, B, NT, diagnosis, reinstating)
    iso = _lib.ftmpc_isolation(struct_size=C.sizeof(_lib.ftmpc_isolation), consist=r["consist"], persist=r["persist"],
                               revise=int(r["revise"]))
    keep, out = [], {}
    # lead, voided and revised are in/out: asked back without being handed over, they start as the library's defaults
    for name, shape in (("lead", (B, 2)), ("voided", (B,)), ("revised", (B,))):
        a = r[name]
        if a is None and name in r["fields"]:
            a = np.zeros(shape, np.int32)
            if name == "lead":
                a[:, 0] = -1
        if a is not None:
            keep.append(a)
            setattr(iso, name, _ptr(a, C.c_int32))
            if name in r["fields"]:
                out[name] = a
    if "fit" in r["fields"]:
        out["fit"] = np.zeros((T, B, 2))
        iso.fit_hist = _ptr(out["fit"])
    return iso, keep, out


def _probe_request(probe, B, T, NT, diagnosis):
    """The ftmpc_probe struct of a simulate call, the arrays it points into (kept alive by the caller) and the dict of outputs."""
    from .probes import request
    r = request(probe, B, T, NT, diagnosis)
    pb = _lib.ftmpc_probe(struct_size=C.sizeof(_lib.ftmpc_probe), amp=r["amp"], quiet=r["quiet"], idle_steps=r["idle_steps"],
                          max_pulses=r["max_pulses"], reinstate=int(r["reinstate"]), restore_ub=r["restore_ub"])
    keep, out = [], {}
    # the carried arrays are in/out: asked back without being handed over, they start from 0 as the library's do
    for name, dtype, shape in (("idle", np.int32, (B, NT)), ("pulses", np.int32, (B, NT)), ("impulse", np.float64, (B,)),
                               ("pacc", np.float64, (B, NT)), ("health", np.float64, (B, NT)), ("reinstated", np.int32, (B,))):
        a = r[name]
        if a is None and name in r["fields"]:
            a = np.zeros(shape, dtype)
        if a is not None:
            keep.append(a)
            setattr(pb, name, _ptr(a, C.c_int32 if dtype is np.int32 else C.c_double))
            if name in r["fields"]:
                out[name] = a
    if "thruster_hist" in r["fields"]:
        out["thruster_hist"] = np.full((T, B), -1, np.int32)
        pb.thruster_hist = _ptr(out["thruster_hist"], C.c_int32)
    return pb, keep, out


def _simulate(self, multi, x0, ub, stuck, xref_traj, T, uref_traj, noise, seed, return_inputs, sqp_iters, backtracks, tol, formulation,
              hull, penalty, faults, detect_delay, return_states, outcomes, return_status, index0, index_total, plant=None, mission=None,
              actuator=None, sensor=None, estimator=None, diagnosis=None, disturbance=None, bias_estimate=None, outage=None, environment=None,
              isolation=None, probe=None):
    """BatchedMPC.simulate (multi False) and MultiGPUMPC.simulate (multi True: the ftmpc_multi_* entries on the driver's handle)."""
    N, NT = self.cfg.N, self.cfg.NT
    x = _f64(x0).reshape(-1, 13).copy()
    B = x.shape[0]
    ub = _f64(ub, (B, NT))
    stuck = _f64(stuck, (B, NT))
    # `cost` is an outcome by name, but lives in the mission struct (ftmpc_outcomes is full): taken out of the request here
    want_cost = False
    if isinstance(outcomes, dict):
        outcomes = dict(outcomes)
        want_cost = bool(outcomes.pop("cost", False))
        if outcomes.get("fields") is not None and "cost" in outcomes["fields"]:
            want_cost = True
            outcomes["fields"] = [n for n in outcomes["fields"] if n != "cost"]
    ms, mkeep, cost = None, None, None
    if mission is not None and (xref_traj is not None or uref_traj is not None):
        raise ValueError("with a mission xref_traj and uref_traj must be None (the mission's tables are the reference)")
    if mission is not None or want_cost:
        ms, mkeep, cost = _mission_request(mission, B, T, N, want_cost)
    se, skeep, sout, L = _sensor_request(sensor, B, T, NT) if sensor is not None else (None, None, None, 0)
    es, ekeep, eout = _estimator_request(estimator, B, T) if estimator is not None else (None, None, None)
    if probe is not None and multi:
        raise ValueError("probe: the probe on MultiGPUMPC is not built (use BatchedMPC)")
    reinstating = probe is not None and bool(probe.get("reinstate", False))      # widens the detect level and the leader's range
    rebuild, d_hb, d_nh = False, None, None
    if diagnosis is not None:     # the wrench form's keys are taken out here: ft_mpc_amd.diagnosis.request knows the common ones
        diagnosis = dict(diagnosis)
        rebuild = bool(diagnosis.pop("rebuild_hull", False))
        d_hb, d_nh = diagnosis.pop("hull_b", None), diagnosis.pop("no_hull", None)
        if formulation == "wrench" and not rebuild:
            raise ValueError("diagnosis: thruster formulation only, unless diagnosis['rebuild_hull'] is True (the wrench form then "
                             "recomputes the hull offsets of the new pattern on the device after a detection)")
        if formulation != "wrench" and (rebuild or d_hb is not None or d_nh is not None):
            raise ValueError("diagnosis['rebuild_hull'], ['hull_b'] and ['no_hull'] belong to formulation='wrench' (the thruster "
                             "formulation has no hull)")
        if formulation == "wrench":
            d_nh = np.full(B, -1, np.int32) if d_nh is None else np.array(d_nh, dtype=np.int32)      # (a copy: the call writes into it)
            if d_nh.shape != (B,) or (d_nh < -1).any():
                raise ValueError(f"diagnosis['no_hull'] must have shape {(B,)} and no entry below -1")
    dg, dkeep, dout = (_diagnosis_request(diagnosis, x, B, T, NT, estimator, sensor, reinstating) if diagnosis is not None
                       else (None, None, None))
    db, bkeep, bout = (_disturbance_request(disturbance, B, T, estimator, sqp_iters, formulation) if disturbance is not None
                       else (None, None, None))
    if bias_estimate is not None and multi and formulation == "wrench":
        raise ValueError("bias_estimate: the two-stage wrench form on MultiGPUMPC is not built (use BatchedMPC, or the thruster formulation)")
    be, bekeep, beout = (_bias_request(bias_estimate, B, T, estimator, disturbance, es, ekeep) if bias_estimate is not None
                         else (None, None, None))
    if outage is not None and multi and formulation == "wrench":
        raise ValueError("outage: the two-stage wrench form on MultiGPUMPC is not built (use BatchedMPC, or the thruster formulation)")
    og, ogkeep, ogout = (_outage_request(outage, B, T, estimator, disturbance, bias_estimate) if outage is not None
                         else (None, None, None))
    if environment is not None and multi and formulation == "wrench":
        raise ValueError("environment: the two-stage wrench form on MultiGPUMPC is not built (use BatchedMPC, or the thruster formulation)")
    ev, evkeep, evout = (_environment_request(environment, B, T, sensor, disturbance, index0, index_total) if environment is not None
                         else (None, None, None))
    if isolation is not None and multi and formulation == "wrench":
        raise ValueError("isolation: the two-stage wrench form on MultiGPUMPC is not built (use BatchedMPC, or the thruster formulation)")
    iso, isokeep, isoout = (None, None, None)
    if isolation is not None:
        # lead needs a state at the ABI: asked back (or handed over) on a run whose diagnosis carries no state, the call is refused here
        iso, isokeep, isoout = _isolation_request(isolation, B, T, NT, diagnosis, reinstating)
        if iso.lead and dg is not None and not dg.state:
            raise ValueError("isolation['lead'] (handed over or among fields) needs the diagnosis' state: put 'state' into "
                             "diagnosis['fields'] or hand diagnosis['state'] over")
    pr, prkeep, prout = (None, None, None)
    if probe is not None:
        # pacc and health need a state at the ABI, as the isolation's lead does
        pr, prkeep, prout = _probe_request(probe, B, T, NT, diagnosis)
        if (pr.pacc or pr.health) and dg is not None and not dg.state:
            raise ValueError("probe['pacc'] and probe['health'] (handed over or among fields) need the diagnosis' state: put 'state' "
                             "into diagnosis['fields'] or hand diagnosis['state'] over")
    if L and mission is not None and mission.get("tables") is not None:
        off = np.asarray(0 if mission.get("offset") is None else mission["offset"])
        if int(off.max()) + T + N + L > np.shape(mission["tables"])[-1]:
            raise ValueError(f"mission: offset + T + N + L = {int(off.max()) + T + N + L} is beyond the tables' "
                             f"{np.shape(mission['tables'])[-1]} columns (L = {L}: the sensor predicts over its latency)")
    xr = None
    if mission is None:
        xr = _f64(xref_traj)
        if xr.shape != (9, T + N + L):
            raise ValueError(f"xref_traj must be 9 x (T+N) = 9 x {T + N}" if not L else
                             f"xref_traj must be 9 x (T+N+L) = 9 x {T + N + L} (L = {L}: the sensor predicts over its latency)")
        xr = np.ascontiguousarray(xr.reshape(-1, order="F"))
    ur = None
    if uref_traj is not None:
        ur = _f64(uref_traj)
        if ur.shape != (6, T + N + L):
            raise ValueError("uref_traj must be 6 x (T+N)" if not L else f"uref_traj must be 6 x (T+N+L) = 6 x {T + N + L}")
        ur = np.ascontiguousarray(ur.reshape(-1, order="F"))
    nz = _f64(noise, 4)
    uh = np.empty((T, B, NT)) if return_inputs else None
    xh = np.empty((T, B, 13)) if return_states else None
    bad = np.zeros(T, np.int32)
    ext = faults is not None or return_states      # the entries with a fault schedule and x_hist
    sched, keep, fh = None, None, None
    if faults is not None:
        from .faults import fault_hull_tables, normalize_schedule
        onset, detect, eub, est = normalize_schedule(faults, B, NT, T, detect_delay)
        keep = [onset, detect, eub, est]
        sched = _lib.ftmpc_fault_schedule(struct_size=C.sizeof(_lib.ftmpc_fault_schedule), n_events=onset.shape[1],
                                          onset=_ptr(onset, C.c_int32), detect=_ptr(detect, C.c_int32), ub=_ptr(eub), stuck=_ptr(est))
        if dg is not None:      # the schedule moves the plant only: the diagnosis detects
            sched.detect = None
        if formulation == "wrench" and dg is None:
            if hull is not None and ("ev_set" not in hull or np.shape(hull["ev_set"]) != onset.shape):
                raise ValueError("with faults `hull` must be None or ft_mpc_amd.faults.fault_hull_tables of the same schedule")
            fh = fault_hull_tables(self.D, ub, stuck, eub, est, onset) if hull is None else hull
            hull = fh
            evs, evb = fh["ev_set"], np.ascontiguousarray(fh["ev_b"], dtype=np.float64)
            keep += [evs, evb]
            sched.hull_set, sched.hull_b = _ptr(evs, C.c_int32), _ptr(evb)
    sp = C.byref(sched) if sched is not None else None
    if formulation not in ("thruster", "wrench"):
        raise ValueError("formulation must be 'thruster' or 'wrench'")
    # the entries with outcomes: asked for, a slice of a campaign, the multi-GPU driver (which has no others), or a plant model (whose
    # entries take the outcomes struct too)
    pm, pkeep = _plant_request(plant, B, NT) if plant is not None else (None, None)
    ac, akeep, aout = _actuator_request(actuator, B, T, NT) if actuator is not None else (None, None, None)
    new = (multi or (outcomes is not None and outcomes is not False) or return_status or index0 != 0 or index_total is not None
           or pm is not None or ms is not None or ac is not None or se is not None or es is not None or dg is not None
           or db is not None or be is not None or og is not None or environment is not None
           or isolation is not None or probe is not None)
    oc, orec, sh = _outcome_request(self, B, T, formulation == "wrench", outcomes, return_status, index0, index_total) if new else (None,) * 3

    if cost is not None:
        orec = {} if orec is None else orec
        orec["cost"] = cost
    def result(out):
        if return_states:
            out["x_hist"] = xh
        if orec is not None:
            out["outcomes"] = orec
        if sh is not None:
            out["status_hist"] = sh
        if aout is not None:
            out["actuator"] = aout
        if sout is not None:
            out["sensor"] = sout
        if eout is not None:
            out["estimator"] = eout
        if dout is not None:
            out["diagnosis"] = dout
        if bout is not None:
            out["disturbance"] = bout
        if beout is not None:
            out["bias_estimate"] = beout
        if ogout is not None:
            out["outage"] = ogout
        if evout is not None:
            out["environment"] = evout
        if isoout is not None:
            out["isolation"] = isoout
        if prout is not None:
            out["probe"] = prout
        return out
    # One argument list, built once: the lead-in of the form, then the feature structs in the order every entry takes them.  The entry
    # is the narrowest one that carries every feature present, so that each ABI level keeps being exercised from here.
    ref = lambda st: C.byref(st) if st is not None else None
    wrench = formulation == "wrench"
    lead = [self._h, B, int(T), _ptr(x), _ptr(ub), _ptr(stuck)]
    sqp = [int(sqp_iters), int(backtracks), float(tol)]
    counts = [_ptr(bad, C.c_int32)]
    out = dict(x=x, u=uh, not_converged=bad)
    dgx = []      # what the wrench form's entries take behind the diagnosis
    if wrench:
        from .controllers.tools.input_bounds import hull_tables
        if hull is None:
            hull = hull_tables(self.D, ub, stuck)
        if np.asarray(hull["degenerate"], bool).any():
            raise ValueError("a vehicle's healthy thrusters do not span R^6: no input hull (use the thruster formulation)")
        A = np.ascontiguousarray(hull["A"], dtype=np.float64)
        hs = np.ascontiguousarray(hull["set"], dtype=np.int32)
        hb = np.ascontiguousarray(hull["b"], dtype=np.float64)
        abad = np.zeros(T, np.int32)
        if dg is not None:
            if d_hb is not None:      # a continued run: the offsets the previous call returned
                hb = np.array(d_hb, dtype=np.float64)
                if hb.shape != (B, int(hull["rows"])) or not np.isfinite(hb).all():
                    raise ValueError(f"diagnosis['hull_b'] must be finite with shape {(B, int(hull['rows']))}")
            dout["hull_b"], dout["no_hull"] = np.empty((B, int(hull["rows"]))), d_nh
        lead += [_ptr(A), A.shape[0], _ptr(hs, C.c_int32), _ptr(hb), int(hull["rows"])]
        sqp += [float(penalty)]
        counts += [_ptr(abad, C.c_int32)]
        out["alloc_failed"] = abad
        dgx = [_ptr(dout["hull_b"]), _ptr(d_nh, C.c_int32)] if dg is not None else [None, None]
    lead += [_ptr(xr), _ptr(ur), _ptr(nz), C.c_uint64(int(seed))]
    form = "wrench_" if wrench else ""
    # (name of the entry, the feature is present, what the entry appends to the narrower one's arguments)
    tail = [("outcomes", new, [ref(oc)]), ("plant", pm is not None, [ref(pm)]), ("mission", ms is not None, [ref(ms)]),
            ("actuator", ac is not None, [ref(ac)]), ("sensor", se is not None, [ref(se)]), ("estimator", es is not None, [ref(es)]),
            ("diagnosis", dg is not None, [ref(dg)] + dgx), ("disturbance", db is not None, [ref(db)]),
            ("bias", be is not None, [ref(be)]), ("outage", og is not None, [ref(og)]),
            ("environment", ev is not None, [ref(ev)]), ("isolation", iso is not None, [ref(iso)]),
            ("probe", pr is not None, [ref(pr)])]
    last = max((i for i, (_, present, _) in enumerate(tail) if present), default=-1)
    if last >= 0:
        name = tail[last][0]
        # (the wrench form's bias, outage, environment and isolation entries exist on the single handle only: the multi-GPU request
        # has been refused above)
        pre = ("ftmpc_simulate_" if (not multi or (wrench and name in ("bias", "outage", "environment", "isolation")))
               else "ftmpc_multi_simulate_")
        args = lead + sqp + [sp, _ptr(uh), _ptr(xh)] + counts + [a for _, _, extra in tail[:last + 1] for a in extra]
        self._check(getattr(self.lib, pre + form + name + "_batch")(*args))
        return result(out)
    if ext:
        self._check(getattr(self.lib, "ftmpc_simulate_" + form + "faults_batch")(*lead, *sqp, sp, _ptr(uh), _ptr(xh), *counts))
        if return_states:
            out["x_hist"] = xh
        return out
    if wrench and not sqp_iters:
        self._check(self.lib.ftmpc_simulate_wrench_batch(*lead, _ptr(uh), *counts))
        return out
    self._check(getattr(self.lib, "ftmpc_simulate_" + form + "batch_ex")(*lead, *sqp, _ptr(uh), *counts))
    return out


def make_synthetic_batch(B, N, NT, nfault, seed, f_max=F_MAX, omega_des=(0.0, 0.0, 0.6)):
    """Seeded random-pose / random-fault batch of BASELINE.md section 4:
    p~U(-2,2)^3, v~U(-.5,.5)^3, q uniform on S^3, omega~omega_des+U(-.2,.2)^3, hover reference,
    `nfault` distinct broken thrusters per instance with iid U(0,1) intensities.
    Returns (x0 [B,13], ub [B,NT], stuck [B,NT], xref 9x(N+1))."""
    rng = np.random.default_rng(seed)
    od = np.asarray(omega_des, float)
    x0 = np.zeros((B, 13))
    x0[:, 0:3] = rng.uniform(-2, 2, (B, 3))
    x0[:, 3:6] = rng.uniform(-0.5, 0.5, (B, 3))
    q = rng.standard_normal((B, 4))
    x0[:, 6:10] = q / np.linalg.norm(q, axis=1, keepdims=True)
    x0[:, 10:13] = od + rng.uniform(-0.2, 0.2, (B, 3))
    ub = np.full((B, NT), f_max)
    stuck = np.zeros((B, NT))
    if nfault > 0:
        keys = rng.random((B, NT))
        idx = np.argsort(keys, axis=1)[:, :nfault]
        inten = rng.uniform(0, 1, (B, nfault))
        rows = np.arange(B)[:, None]
        ub[rows, idx] = 0.0
        stuck[rows, idx] = inten * f_max
    xref = np.zeros((9, N + 1))
    xref[6:9, :] = od.reshape(3, 1)
    return x0, ub, stuck, xref
