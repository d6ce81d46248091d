"""GPU: a non-finite vehicle must not touch the rest of its batch (tests/poisoned.py builds the batches; tests/test_poisoned_host.py
fixes the oracle's verdicts on them).

include/ftmpc.h promises FTMPC_STATUS_NUMERIC and the linearisation point for an instance that meets a non-finite value.  Every other
GPU test feeds finite data, where `0 * residue` is 0 whatever a neighbour left behind in LDS, in the per-block scratch tiles, in the
global gradient slot or in a lane next door.  Each family below is reached as tests/test_gpu_other_vehicle.py reaches it (same
kernel_select / dtype / shape, the named kernel seen in last_kernel_ms) and held to four things:

  a  isolation    every output of every healthy instance of the poisoned launch has the BITS of the clean twin's, and the twin's
                  healthy instances all have status 0 (their accuracy is held elsewhere and not repeated here);
  b  verdict      a NaN / Inf instance comes back with status 2 (never 0), finite outputs inside [0, ub], zero on broken thrusters
                  and equal to the linearisation point: zeros cold, clip(warm start) warm (at the precision of the build: the fp32
                  kernels carry it in float32; wrench form: the warm wrenches, D stuck cold -- include/ftmpc.h);
  c  overflow     x[0] = 1e30 (fp32 handle) / 1e200 (float64 handle) is finite as the entry receives it: finite outputs inside their
                  bounds, a documented status, and status 0 only within the family's tolerance of the C oracle where that reports 0
                  (what each family answered: DESIGN.md section 2);
  d  persistence  after the poisoned launch the clean twin on the SAME handle has the bits of a fresh handle (asserted on that second
                  launch, so warm start, scratch tiles, gradient slot and staging are all crossed); the kernels that pull work through
                  a cursor get one case of more than twice their grid, so that waves take a healthy instance right after a poisoned one.

Before any of these ran, every loop bound, every barrier-skipping branch and every memory index of the kernels was read for
dependence on floating-point data ("poisoned instances": none found).  Each test prints what it measured."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))

from ft_mpc_amd.controllers.tools.terminal_ingredients import load_terminal
from oracle import c_oracle as co
from oracle import qp_oracle as qo
from oracle import refmath as rm
import poisoned as po
import wrench_state_rows as ws
import other_vehicle as ov

pytestmark = pytest.mark.gpu
F_MAX = rm.F_MAX
NO_STUCK = tuple(k for k in po.POISONS if k != "nan_stuck")      # vehicles without a broken thruster have no stuck entry to poison

_handles = {}


def _handle(factory, tag="used", **kw):
    """one handle per configuration, tag and session (tag "fresh": the handle no poisoned launch ever touched)"""
    key = repr((tag, sorted((k, np.asarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v)) for k, v in kw.items())))
    if key not in _handles:
        _handles[key] = factory(**kw)
    return _handles[key]


@pytest.fixture(scope="module", autouse=True)
def _close_the_handles_of_this_module():
    """Some seventy handles (a used and a fresh one per configuration, grown to 4101 instances by the cursor cases): closed when
    the module is done, not at the end of the session, so that the modules after this one find the device memory they found before."""
    yield
    for m in _handles.values():
        m.close()
    _handles.clear()


def _term():
    t = load_terminal().term_set
    return t.A, t.b.reshape(-1)


def _inside_the_terminal_set(B, N, NT, seed):
    """other_vehicle.near_terminal_set on the default vehicle, at half the set's boundary: every twin reaches the set"""
    return ov.near_terminal_set(qo.QPConfig(N=N, NT=NT), B, 2, seed, *_term(), scale=0.5)


def _spanning(batch, D):
    """the first half of `batch` (drawn at twice the size) whose healthy thrusters span R^6: the wrench form has no hull for the others"""
    from ft_mpc_amd.controllers.tools.input_bounds import hull_tables
    x0, ub, stuck, xref = batch
    keep = np.flatnonzero(~hull_tables(D, ub, stuck)["degenerate"])[:x0.shape[0] // 2]
    assert keep.size == x0.shape[0] // 2
    return x0[keep], ub[keep], stuck[keep], xref


def _bits(a, b, rows, what):
    for k in a:
        if a[k] is None:
            assert b[k] is None
            continue
        assert po.same_bits(a[k][rows], b[k][rows]), (what, k, np.flatnonzero([not po.same_bits(a[k][i], b[k][i]) for i in np.flatnonzero(rows)])[:8])


def _all(B):
    return np.ones(B, bool)


def _profiled(mpc, kernel, call):
    if kernel is None:
        return call()
    mpc.set_profiling(True)
    out = call()
    ms = mpc.last_kernel_ms()
    mpc.set_profiling(False)
    assert any(kernel in k for k in ms), (kernel, ms)
    return out


def _grid(per_cu):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * per_cu


def _in_box(U, ub, dtype):
    """0 <= U <= ub (an fp32 kernel returns ub rounded to float32), exactly zero on broken thrusters"""
    hi = np.maximum(ub, np.float32(ub).astype(np.float64)) if dtype == "f32" else ub
    hi = hi[:, None, :] if U.ndim == 3 else hi
    dead = np.broadcast_to(hi == 0, U.shape)
    return bool(np.isfinite(U).all() and (U >= 0).all() and (U <= hi).all() and (U[dead] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# thruster form: ftmpc_solve_batch on every solve kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _thruster_family(factory, kernel, N, NT, nf, B, seed, dtype, tol_u0, tol_U, polish, batch=None, where=None, oracle=True, **hkw):
    used, fresh = _handle(factory, N=N, NT=NT, dtype=dtype, **hkw), _handle(factory, "fresh", N=N, NT=NT, dtype=dtype, **hkw)
    q = qo.QPConfig(N=N, NT=NT)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, nf, seed) if batch is None else batch
    xr = np.ascontiguousarray(xref.reshape(-1, order="F"))
    where = po.every_third(B) if where is None else where
    xp, sp, kind = po.poison(x0, ub, stuck, where, dtype, po.POISONS if nf else NO_STUCK)
    h, bad, ovf = po.healthy(kind), po.nonfinite(kind), po.overflow(kind)
    report = []
    for warm in (False, True):
        W = None
        if warm:      # near the twin's solution, some entries outside [0, ub] (the clip), broken thrusters not zero (the mask)
            rng = np.random.default_rng(seed + 17)
            W = np.ascontiguousarray(0.9 * cold["U"] + 0.05 * F_MAX * rng.uniform(-1.5, 1.5, (B, N, NT)))
        solve = lambda m, a, s: m.solve(a, ub, s, xr, warmU=None if W is None else W.copy(), return_U=True)
        out = _profiled(used, kernel, lambda: solve(used, xp, sp))      # the poisoned launch
        again = solve(used, x0, stuck)                                   # d: the clean twin on the handle the poison went through ...
        twin = solve(fresh, x0, stuck)                                   # ... against the handle it never touched
        if not warm:
            cold = twin
        _bits(again, twin, _all(B), "persistence")
        assert (twin["status"] == 0).all(), twin["status"]
        _bits(out, twin, h, "isolation")                                 # a
        # b: the verdict on NaN / Inf, and the linearisation point
        assert (out["status"][bad] == 2).all(), list(zip(kind[bad], out["status"][bad]))
        lin = np.zeros((B, N, NT)) if W is None else np.where(ub[:, None, :] > 0, np.clip(W, 0.0, ub[:, None, :]), 0.0)
        if dtype == "f32":
            lin = np.float32(lin).astype(np.float64)
        assert _in_box(out["U"][bad], ub[bad], dtype) and _in_box(out["u0"][bad], ub[bad], dtype)
        assert np.array_equal(out["U"][bad], lin[bad]) and np.array_equal(out["u0"][bad], lin[bad][:, 0])
        # c: the overflow poison
        assert _in_box(out["U"][ovf], ub[ovf], dtype) and _in_box(out["u0"][ovf], ub[ovf], dtype)
        assert np.isin(out["status"][ovf], (0, 1, 2)).all()
        if oracle:
            with np.errstate(all="ignore"):
                ref = co.solve_batch(q, xp[ovf], ub[ovf], sp[ovf], xref, warmU=None if W is None else W[ovf].copy(), max_iters=60,
                                     mu_stop=1e-13, polish=polish)
            both = (out["status"][ovf] == 0) & (ref["status"] == 0)
            e0 = np.abs(out["u0"][ovf] - ref["u0"])[both].max(initial=0.0) / F_MAX
            eU = np.abs(out["U"][ovf] - ref["U"])[both].max(initial=0.0) / F_MAX
            report.append(f"{'warm' if warm else 'cold'}: overflow status {out['status'][ovf].tolist()} (oracle {ref['status'].tolist()}), "
                          f"u0 within {e0:.1e}, U within {eU:.1e} f_max where both solve")
            assert e0 <= tol_u0 and eU <= tol_U, (e0, eU)
        else:      # (rows the C oracle does not have: the documented verdict at these magnitudes, include/ftmpc.h)
            assert (out["status"][ovf] != 0).all(), out["status"][ovf]
    print(f"poisoned {kernel} N={N} NT={NT} faults={nf} B={B} {dtype}: {int(bad.sum())} NaN/Inf -> status 2; " + "; ".join(report))


@pytest.mark.parametrize("N,nf,B", [(20, 2, 24), (20, 1, 24), (20, 0, 24), (3, 2, 24), (23, 2, 24)])
def test_kernel_2(gpu_mpc_factory, N, nf, B):
    """ftmpc_solve_f32_kernel<8>, <9>, <10>; gradient storage in LDS (N <= 21) and in the global slot (N = 23).  Dropping
    `if (status == 2) u = ubar[v]` fails b; a tile, a parked factor or the gradient slot read before it is written fails a or d."""
    nb = -(-N * (8 - nf) // 16)
    _thruster_family(gpu_mpc_factory, f"ftmpc_solve_f32_kernel<{max(nb, 8)}>", N, 8, nf, B, 100 + N + nf, "f32", 1e-4, 1e-4, True)


@pytest.mark.parametrize("N,nf", [(11, 0), (11, 2), (17, 2)])
def test_kernel_10(gpu_mpc_factory, N, nf):
    """ftmpc_solve_wsw32_kernel<6> and <8>: Sblk is zeroed once per wave, before the instance loop."""
    _thruster_family(gpu_mpc_factory, "ftmpc_solve_wsw32_kernel", N, 16, nf, 24, 200 + N + nf, "f32", 1e-4, 1e-4, True)


@pytest.mark.parametrize("sel,nf,kernel", [("workgroup", 2, "ftmpc_solve_ws32_kernel"), ("workgroup", 0, "ftmpc_solve_ws32_kernel"),
                                           ("dense", 2, "ftmpc_solve_f32_kernel<10>"), ("dense", 0, "ftmpc_solve_wg32_kernel")])
def test_kernels_8_and_7(gpu_mpc_factory, sel, nf, kernel):
    """The four-wave fp32 kernels: their exits are taken on wg_reduce results and on s_flag behind a barrier, NaN included."""
    _thruster_family(gpu_mpc_factory, kernel, 11, 16, nf, 24, 300 + nf, "f32", 1e-4, 1e-4, True, kernel_select=sel)


@pytest.mark.parametrize("N,NT", [(3, 8), (17, 16), (25, 16)])
def test_kernel_12(gpu_mpc_factory, N, NT):
    """ftmpc_solve_ric64_kernel<4>, <6>, <10>."""
    _thruster_family(gpu_mpc_factory, "ftmpc_solve_ric64_kernel", N, NT, 2, 24, 400 + N, "f64", 1e-7, 1e-6, True, max_iters=40)


@pytest.mark.parametrize("sel,kernel", [("dense", "ftmpc_solve_f64_kernel"), ("workgroup", "ftmpc_solve_ws64_kernel")])
@pytest.mark.parametrize("N", [5, 7])
def test_kernels_3_and_9(gpu_mpc_factory, N, sel, kernel):
    """The dense float64 kernel (MODE 0) and the float64 wrench-space kernel: gm = fmax(gm, fabs(grad)) drops a NaN, so the
    start barrier parameter stays finite; the NaN must then reach mu through the first step and end the instance with status 2."""
    _thruster_family(gpu_mpc_factory, kernel, N, 16, 2, 24, 500 + N, "f64", 1e-7, 1e-6, False, max_iters=40, kernel_select=sel)


def test_kernel_12_with_state_bounds(gpu_mpc_factory):
    """<6, true>: rpn = fmax(rpn, fabs(residual)) drops a NaN residual; the verdict must come from mu.  The batch is a plain one
    (|v| <= 0.5 against the bound 0.9), not other_vehicle.near_state_bounds, so that every twin ends with status 0: the state rows are
    in the program but not active on the healthy instances, so this holds the instantiation, not active rows."""
    xlb, xub = ws.bounds()
    _thruster_family(gpu_mpc_factory, "ftmpc_solve_ric64_kernel", 5, 16, 2, 24, 6, "f64", 1e-7, 1e-6, True, oracle=False, max_iters=60,
                     xlb=xlb, xub=xub)


@pytest.mark.parametrize("sel,kernel", [("riccati", "ftmpc_solve_ric64_kernel"), ("auto", "ftmpc_solve_f64_kernel")])
def test_kernels_12_and_3_with_the_terminal_set(gpu_mpc_factory, sel, kernel):
    """Kernel 12's terminal-set instantiation and the dense kernel's MODE 2, vehicles inside the set (half its boundary)."""
    N, NT, B = 5, 16, 24
    _thruster_family(gpu_mpc_factory, kernel, N, NT, 2, B, 41, "f64", 1e-7, 1e-6, True, oracle=False,
                     batch=_inside_the_terminal_set(B, N, NT, 41), max_iters=60, terminal_set=True, kernel_select=sel)


CURSOR = [  # (id, handle keywords, kernel, N, NT, faults, workgroups or waves per CU of the persistent grid at most)
    ("kernel-2", dict(dtype="f32"), "ftmpc_solve_f32_kernel<8>", 3, 8, 2, 8),
    ("kernel-10", dict(dtype="f32"), "ftmpc_solve_wsw32_kernel", 11, 16, 2, 4),
    ("kernel-8", dict(dtype="f32", kernel_select="workgroup"), "ftmpc_solve_ws32_kernel", 11, 16, 2, 2),
    ("kernel-7", dict(dtype="f32", kernel_select="dense"), "ftmpc_solve_wg32_kernel", 11, 16, 0, 1),
    ("kernel-12", dict(dtype="f64", max_iters=40), "ftmpc_solve_ric64_kernel", 3, 8, 2, 8),
    ("kernel-9", dict(dtype="f64", max_iters=40, kernel_select="workgroup"), "ftmpc_solve_ws64_kernel", 5, 16, 2, 2),
    ("kernel-3", dict(dtype="f64", max_iters=40, kernel_select="dense"), "ftmpc_solve_f64_kernel", 5, 16, 2, 2),
]


@pytest.mark.parametrize("hkw,kernel,N,NT,nf,per_cu", [c[1:] for c in CURSOR], ids=[c[0] for c in CURSOR])
def test_a_healthy_instance_right_after_a_poisoned_one(gpu_mpc_factory, hkw, kernel, N, NT, nf, per_cu):
    """More than twice the persistent grid (ftmpc_capi.hip: num_cu * blocks_per_cu, at most `per_cu` per CU), every third instance
    poisoned: every wave or workgroup solves a healthy instance directly after a poisoned one, at the shortest horizon that reaches
    the instantiation.  a, b (cold) and d."""
    B = 2 * _grid(per_cu) + 5
    used, fresh = _handle(gpu_mpc_factory, N=N, NT=NT, **hkw), _handle(gpu_mpc_factory, "fresh", N=N, NT=NT, **hkw)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, nf, 900 + N)
    xr = np.ascontiguousarray(xref.reshape(-1, order="F"))
    xp, sp, kind = po.poison(x0, ub, stuck, po.every_third(B), hkw["dtype"], po.POISONS if nf else NO_STUCK)
    out = _profiled(used, kernel, lambda: used.solve(xp, ub, sp, xr, return_U=True))
    again = used.solve(x0, ub, stuck, xr, return_U=True)
    twin = fresh.solve(x0, ub, stuck, xr, return_U=True)
    _bits(again, twin, _all(B), "persistence")
    _bits(out, twin, po.healthy(kind), "isolation")
    bad, ovf = po.nonfinite(kind), po.overflow(kind)
    assert (out["status"][bad] == 2).all() and (out["U"][bad] == 0).all() and (out["u0"][bad] == 0).all()
    assert _in_box(out["U"][ovf], ub[ovf], hkw["dtype"]) and np.isin(out["status"][ovf], (1, 2)).all()      # (never "solved": include/ftmpc.h)
    print(f"poisoned {kernel} B={B}: {int((~po.healthy(kind)).sum())} poisoned, twin status {np.bincount(twin['status']).tolist()}")


# ---------------------------------------------------------------------------------------------------------------------------
# lane-per-instance kernels: linearise records, the condensed QP, the cost kernels, the allocator
# ---------------------------------------------------------------------------------------------------------------------------
def _where(B):
    return po.wave_lanes(B) if B > 64 else po.every_third(B)


@pytest.mark.parametrize("B", [16, 24, 65, 130])
@pytest.mark.parametrize("N,NT", [(3, 8), (2, 16)])
def test_linearise_records(gpu_mpc_factory, N, NT, B):
    """The full-record kernel, the direction-split kernel <double, 1> and the shares kernel <double, 2> (lin_split_max = 16: B = 16 one
    direction per block, B = 24 four shares, B = 65 two shares, B = 130 the full-record kernel): the healthy instances' records have the
    twin's bits from all three, poisoned lanes 0, 31, 63 and the last lane of the partial wave (every third below a wave); the poison
    reaches the poisoned instance's record (a kernel that never read x0 would pass otherwise); the twin on the same handle afterwards
    has the bits of the launch before."""
    hs = [_handle(gpu_mpc_factory, N=N, NT=NT, lin_split_max=-1), _handle(gpu_mpc_factory, N=N, NT=NT),
          _handle(gpu_mpc_factory, N=N, NT=NT, lin_split_max=16)]
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, 2, 700 + B)
    xr = np.ascontiguousarray(xref.reshape(-1, order="F"))
    rng = np.random.default_rng(B)
    W = np.ascontiguousarray(rng.uniform(-0.1, 1.1, (B, N, NT)) * F_MAX)
    xp, sp, kind = po.poison(x0, ub, stuck, _where(B), "f64")
    h = po.healthy(kind)
    for warm in (None, W):
        kw = dict(xref=xr, warmU=None if warm is None else warm.copy())
        clean = hs[0].debug_records(x0, ub, stuck, **kw)
        assert np.isfinite(clean).all()
        for m in hs:
            before = m.debug_records(x0, ub, stuck, **kw)
            rec = m.debug_records(xp, ub, sp, **kw)
            after = m.debug_records(x0, ub, stuck, **kw)
            assert po.same_bits(before, clean) and po.same_bits(after, clean)
            assert po.same_bits(rec[h], clean[h]), np.argwhere(rec[h] != clean[h])[:8]
            for b in np.flatnonzero(po.nonfinite(kind)):
                assert not np.isfinite(rec[b]).all(), (b, kind[b])
            if po.overflow(kind).any():
                assert not po.same_bits(rec[po.overflow(kind)], clean[po.overflow(kind)])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_build_of_the_neighbours_of_a_poisoned_instance(gpu_mpc_factory, dtype):
    """H, g and the box of the healthy instances next to a poisoned one (the test hook solves the batch and dumps one instance's QP)."""
    N, NT, B = 20, 8, 12
    mpc = _handle(gpu_mpc_factory, N=N, NT=NT, dtype=dtype)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, 2, 1)
    xr = np.ascontiguousarray(xref.reshape(-1, order="F"))
    xp, sp, kind = po.poison(x0, ub, stuck, po.every_third(B), dtype)
    for inst in (0, 2, 5, 11):
        assert kind[inst] == ""
        clean = mpc.debug_build_qp(x0, ub, stuck, xr, inst)
        got = mpc.debug_build_qp(xp, ub, sp, xr, inst)
        after = mpc.debug_build_qp(x0, ub, stuck, xr, inst)
        for a, b, c in zip(clean, got, after):
            assert np.isfinite(a).all() and po.same_bits(a, b) and po.same_bits(a, c), inst


def test_cost_kernel(gpu_mpc_factory):
    """ftmpc_eval_cost_batch: the healthy lanes keep their bits; a NaN / Inf vehicle's cost is not finite (include/ftmpc.h), the overflow
    vehicle's is +Inf or beyond 1e50."""
    N, NT, B = 6, 8, 65
    mpc = _handle(gpu_mpc_factory, N=N, NT=NT)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, 2, 61)
    xr = np.ascontiguousarray(xref.reshape(-1, order="F"))
    U = np.random.default_rng(1).uniform(0, F_MAX, (B, N, NT)) * (ub[:, None, :] > 0)
    for dtype in ("f32", "f64"):
        xp, sp, kind = po.poison(x0, ub, stuck, po.wave_lanes(B), dtype, po.POISONS[2:] + po.POISONS[:2])
        clean = mpc.eval_cost(x0, ub, stuck, xr, U)
        J = mpc.eval_cost(xp, ub, sp, xr, U)
        after = mpc.eval_cost(x0, ub, stuck, xr, U)
        assert np.isfinite(clean).all() and po.same_bits(clean, after)
        assert po.same_bits(J[po.healthy(kind)], clean[po.healthy(kind)])
        assert not np.isfinite(J[po.nonfinite(kind)]).any(), J[po.nonfinite(kind)]
        assert not (J[po.overflow(kind)] < 1e50).any(), J[po.overflow(kind)]


def test_cost_wrench_kernel(gpu_mpc_factory):
    """ftmpc_eval_cost_wrench_batch with the terminal set: cost as above; the violation sums max(0, .), which drops a NaN row: it is
    never NaN and >= 0 for every vehicle (+Inf for an infinite error; include/ftmpc.h says so), and the healthy lanes keep the bits of both."""
    N, NT, B = 6, 16, 65
    mpc = _handle(gpu_mpc_factory, N=N, NT=NT, dtype="f64", terminal_set=True)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, 2, 62)
    xr = np.ascontiguousarray(xref.reshape(-1, order="F"))
    q = qo.QPConfig(N=N, NT=NT)
    G = ((ub / 2 + stuck) @ q.D.T)[:, None, :] + np.random.default_rng(N).uniform(-1.0, 1.0, (B, N, 6))
    xp, _, kind = po.poison(x0, ub, stuck, po.wave_lanes(B), "f64", NO_STUCK)      # (the entry takes no stuck)
    clean = mpc.eval_cost_wrench(x0, xr, G, return_tviol=True)
    got = mpc.eval_cost_wrench(xp, xr, G, return_tviol=True)
    after = mpc.eval_cost_wrench(x0, xr, G, return_tviol=True)
    h = po.healthy(kind)
    for c, g, a in zip(clean, got, after):
        assert np.isfinite(c).all() and po.same_bits(c, a) and po.same_bits(g[h], c[h])
    assert not np.isfinite(got[0][po.nonfinite(kind)]).any() and not (got[0][po.overflow(kind)] < 1e50).any()
    assert not np.isnan(got[1]).any() and (got[1] >= 0).all()


def test_allocator_alone(gpu_mpc_factory):
    """ftmpc_allocate_batch, a NaN in one tau entry of lanes 0, 31, 63 and of the partial wave's last lane, in all six of lane 7 and an
    Inf in lane 40: tmax, the residual and the multiplier norm are fmax reductions that drop a NaN, so the stop test must not see a
    zero residual.  Non-zero status, u finite inside
    [0, ub] and zero on broken thrusters; the other lanes keep their bits and their status 0 (a wave leaves the Newton loop lane by
    lane: no lane waits for a NaN lane's cap)."""
    NT, B = 16, 65
    mpc = _handle(gpu_mpc_factory, N=5, NT=NT, dtype="f64")
    _, ub, _, _ = qo.make_batch(B, 5, NT, 2, 63)
    rng = np.random.default_rng(64)
    tau = (rng.uniform(0.1, 0.9, (B, NT)) * ub) @ np.asarray(mpc.D).T      # attainable, inside
    bad = np.concatenate([po.wave_lanes(B), [7, 40]])
    tp = tau.copy()
    for i, b in enumerate(po.wave_lanes(B)):
        tp[b, (2 * i) % 6] = np.nan
    tp[7] = np.nan          # every entry: the fmax residual of such a wrench reads 0
    tp[40, 3] = np.inf
    clean = mpc.allocate(tau, ub)
    got = mpc.allocate(tp, ub)
    after = mpc.allocate(tau, ub)
    assert (clean["status"] == 0).all()
    h = np.ones(B, bool)
    h[bad] = False
    _bits(after, clean, _all(B), "persistence")
    _bits(got, clean, h, "isolation")
    print("allocator on a NaN tau entry: status", got["status"][bad], "iterations", got["iters"][bad], "max u", np.abs(got["u"][bad]).max())
    assert (got["status"][bad] != 0).all(), got["status"][bad]
    assert _in_box(got["u"][bad], ub[bad], "f64")


# ---------------------------------------------------------------------------------------------------------------------------
# wrench form (ftmpc_solve_wrench_batch): kernels 13, 11 and the dense kernel's hull mode, with the allocation behind them
# ---------------------------------------------------------------------------------------------------------------------------
def _wrench_family(factory, kernel, N, NT, B, seed, dtype, batch=None, where=None, **hkw):
    """a, b, d as the thruster form; the linearisation point of the wrench form is the warm wrench sequence, D stuck cold (include/
    ftmpc.h), which a failed QP returns as G (float64 kernels: to rounding of the sum; kernel 11 carries it in float32); tau0 is that
    point pulled into the hull and u0 its allocation.  A NaN stuck entry makes D stuck itself non-finite: the entries come back as 0.
    An overflow instance is never reported solved (status 1 or 2: the documented verdict at 1e30 / 1e200)."""
    used, fresh = _handle(factory, N=N, NT=NT, dtype=dtype, **hkw), _handle(factory, "fresh", N=N, NT=NT, dtype=dtype, **hkw)
    q = qo.QPConfig(N=N, NT=NT)
    x0, ub, stuck, xref = _spanning(qo.make_batch(2 * B, N, NT, 2, seed) if batch is None else batch, used.D)
    xr = np.ascontiguousarray(xref.reshape(-1, order="F"))
    xp, sp, kind = po.poison(x0, ub, stuck, po.every_third(B) if where is None else where, dtype)
    h, bad, ovf = po.healthy(kind), po.nonfinite(kind), po.overflow(kind)
    from ft_mpc_amd.controllers.tools.input_bounds import hull_tables
    hull = hull_tables(used.D, ub, stuck)      # the twin's tables for both (a NaN stuck entry must reach the device, not NumPy's einsum)
    with np.errstate(all="ignore"):
        hull_p = hull_tables(used.D, ub, sp)
    assert not hull["degenerate"].any() and np.array_equal(hull["set"], hull_p["set"])
    eps = 1e-12 if dtype == "f64" else 2e-6
    for warm in (False, True):
        W = None
        if warm:
            W = np.ascontiguousarray(0.9 * cold["G"] + 0.1 * ((ub / 2 + stuck) @ q.D.T)[:, None, :])      # inside the hull
        solve = lambda m, a, s, hl: m.solve_wrench(a, ub, s, xr, warmG=None if W is None else W.copy(), return_G=True, hull=hl)
        out = solve(used, xp, sp, hull_p)      # (the two-stage entry records no kernel times: the family is what the handle routes to)
        again = solve(used, x0, stuck, hull)
        twin = solve(fresh, x0, stuck, hull)
        if not warm:
            cold = twin
        _bits(again, twin, _all(B), "persistence")
        assert (twin["status"] == 0).all() and (twin["alloc_status"] == 0).all(), (twin["status"], twin["alloc_status"])
        _bits(out, twin, h, "isolation")
        assert (out["status"][bad] == 2).all(), list(zip(kind[bad], out["status"][bad]))
        with np.errstate(all="ignore"):
            lin = np.repeat((sp @ q.D.T)[:, None, :], N, axis=1) if W is None else W
        lin = np.where(np.isfinite(lin), lin, 0.0)      # (D stuck of a NaN stuck entry: returned as 0, include/ftmpc.h)
        for k in ("u0", "G", "tau0"):
            assert np.isfinite(out[k][bad | ovf]).all(), (k, kind[~np.isfinite(out[k].reshape(B, -1)).all(axis=1)])
        scale = max(1.0, np.abs(lin[bad]).max())
        assert np.abs(out["G"][bad] - lin[bad]).max() <= eps * scale
        hc = bad & (kind != "nan_stuck")      # (tau0 is G[0] pulled towards the hull centre D (ub / 2 + stuck) by 1e-9 / 1e-8 at most; 0 without one)
        assert np.abs(out["tau0"][hc] - lin[hc][:, 0]).max() <= max(eps, 2e-8) * scale
        ns = kind == "nan_stuck"      # no wrench to allocate: flagged, no thrust
        assert (out["tau0"][ns] == 0).all() and (out["alloc_status"][ns] == 2).all() and (out["u0"][ns] == 0).all()
        assert _in_box(out["u0"][bad | ovf], ub[bad | ovf], "f64")
        assert np.isin(out["status"][ovf], (1, 2)).all(), out["status"][ovf]      # (the documented verdict: never "solved" at 1e30 / 1e200)
        print(f"poisoned wrench {kernel} N={N} NT={NT} {dtype} {'warm' if warm else 'cold'}: NaN/Inf status {out['status'][bad].tolist()}, "
              f"allocation {out['alloc_status'][bad].tolist()}, max u0 {np.abs(out['u0'][bad]).max():.2e}; overflow status "
              f"{out['status'][ovf].tolist()} allocation {out['alloc_status'][ovf].tolist()}")


@pytest.mark.parametrize("N", [5, 25])
def test_kernel_13(gpu_mpc_factory, N):
    _wrench_family(gpu_mpc_factory, "ftmpc_solve_ricw64_kernel", N, 16, 24, 800 + N, "f64", max_iters=40)


def test_kernel_13_with_the_terminal_set(gpu_mpc_factory):
    N, NT, B = 5, 16, 24
    _wrench_family(gpu_mpc_factory, "ftmpc_solve_ricw64_kernel", N, NT, B, 41, "f64", batch=_inside_the_terminal_set(2 * B, N, NT, 41),
                   max_iters=60, terminal_set=True)


def test_kernel_13_with_state_bounds(gpu_mpc_factory):
    """<6, false, true>.  As test_kernel_12_with_state_bounds: a plain batch, so that every twin ends with status 0 -- the state rows are in
    the program, not active on the healthy instances."""
    xlb, xub = ws.bounds()
    _wrench_family(gpu_mpc_factory, "ftmpc_solve_ricw64_kernel", 5, 16, 24, 6, "f64", max_iters=60, xlb=xlb, xub=xub)


@pytest.mark.parametrize("hkw,kernel", [(dict(dtype="f32", max_iters=40), "ftmpc_solve_hull32_kernel"),
                                        (dict(dtype="f64", max_iters=40, kernel_select="dense"), "ftmpc_solve_f64_kernel")],
                         ids=["kernel-11", "kernel-3-mode-1"])
def test_kernels_11_and_3_two_stage(gpu_mpc_factory, hkw, kernel):
    """Kernel 11 with its hand-over list and the allocation behind it, and the dense float64 kernel's hull mode."""
    hkw = dict(hkw)
    _wrench_family(gpu_mpc_factory, kernel, 5, 16, 24, 805, hkw.pop("dtype"), **hkw)


WRENCH_CURSOR = [  # (id, handle keywords, N, waves per CU of the persistent grid at most: kernel 11 one per SIMD, kernel 13 two)
    ("kernel-11", dict(dtype="f32", max_iters=40), 3, 4),
    ("kernel-13", dict(dtype="f64", max_iters=40), 3, 8),
]


@pytest.mark.parametrize("hkw,N,per_cu", [c[1:] for c in WRENCH_CURSOR], ids=[c[0] for c in WRENCH_CURSOR])
def test_two_stage_a_healthy_instance_right_after_a_poisoned_one(gpu_mpc_factory, hkw, N, per_cu):
    """ftmpc_solve_hull32_kernel (with its hand-over list and kernel 13 behind it) and ftmpc_solve_ricw64_kernel at more than twice
    their persistent grids (ftmpc_capi.hip: grid_hull, grid_ricw = num_cu * blocks_per_cu), every third instance poisoned, N = 3: every
    wave solves a healthy instance directly after a poisoned one, so the wave's LDS, its slot of hull_slot / ricw_slot and the allocation
    behind it are crossed inside one launch.  a, b (cold) and d."""
    from ft_mpc_amd.controllers.tools.input_bounds import hull_tables
    NT, B = 16, 2 * _grid(per_cu) + 5
    used, fresh = _handle(gpu_mpc_factory, N=N, NT=NT, **hkw), _handle(gpu_mpc_factory, "fresh", N=N, NT=NT, **hkw)
    q = qo.QPConfig(N=N, NT=NT)
    x0, ub, stuck, xref = _spanning(qo.make_batch(2 * B, N, NT, 2, 950 + per_cu), used.D)
    xr = np.ascontiguousarray(xref.reshape(-1, order="F"))
    xp, sp, kind = po.poison(x0, ub, stuck, po.every_third(B), hkw["dtype"])
    h, bad, ovf, ns = po.healthy(kind), po.nonfinite(kind), po.overflow(kind), kind == "nan_stuck"
    hull = hull_tables(used.D, ub, stuck)
    with np.errstate(all="ignore"):
        hull_p = hull_tables(used.D, ub, sp)
    solve = lambda m, a, s, hl: m.solve_wrench(a, ub, s, xr, return_G=True, hull=hl)
    out = solve(used, xp, sp, hull_p)
    handed = used.last_handed_over()
    again, twin = solve(used, x0, stuck, hull), solve(fresh, x0, stuck, hull)
    _bits(again, twin, _all(B), "persistence")
    _bits(out, twin, h, "isolation")
    assert (out["status"][bad] == 2).all() and np.isin(out["status"][ovf], (1, 2)).all()
    with np.errstate(all="ignore"):
        lin = np.repeat((sp @ q.D.T)[:, None, :], N, axis=1)
    lin = np.where(np.isfinite(lin), lin, 0.0)
    for k in ("u0", "G", "tau0"):
        assert np.isfinite(out[k][bad | ovf]).all(), k
    assert np.abs(out["G"][bad] - lin[bad]).max() <= (1e-12 if hkw["dtype"] == "f64" else 2e-6) * max(1.0, np.abs(lin[bad]).max())
    assert _in_box(out["u0"][bad | ovf], ub[bad | ovf], "f64")
    assert (out["tau0"][ns] == 0).all() and (out["alloc_status"][ns] == 2).all() and (out["u0"][ns] == 0).all()
    print(f"poisoned two-stage {hkw['dtype']} B={B}: {int((~h).sum())} poisoned, handed over {handed}, twin status "
          f"{np.bincount(twin['status']).tolist()}, allocation {np.bincount(twin['alloc_status']).tolist()}")


# ---------------------------------------------------------------------------------------------------------------------------
# the two SQPs, few major iterations
# ---------------------------------------------------------------------------------------------------------------------------
def test_thruster_sqp(gpu_mpc_factory):
    """ftmpc_solve_sqp_batch, two major iterations: a NaN / Inf vehicle's first QP ends with status 2, so no line search opens for it:
    U stays the start point (zeros), sqp_iters 0, cost and cost0 not finite (include/ftmpc.h)."""
    N, NT, B = 6, 8, 24
    used, fresh = _handle(gpu_mpc_factory, N=N, NT=NT), _handle(gpu_mpc_factory, "fresh", N=N, NT=NT)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, 2, 71)
    xr = np.ascontiguousarray(xref.reshape(-1, order="F"))
    xp, sp, kind = po.poison(x0, ub, stuck, po.every_third(B), "f32")
    run = lambda m, a, s: m.solve_sqp_device(a, ub, s, xr, sqp_iters=2, backtracks=4)
    out, again, twin = run(used, xp, sp), run(used, x0, stuck), run(fresh, x0, stuck)
    _bits(again, twin, _all(B), "persistence")
    _bits(out, twin, po.healthy(kind), "isolation")
    assert np.isin(twin["status"], (0,)).all() and np.isfinite(twin["cost"]).all()
    bad, ovf = po.nonfinite(kind), po.overflow(kind)
    assert (out["status"][bad] == 2).all() and (out["sqp_iters"][bad] == 0).all()
    assert (out["U"][bad] == 0).all() and (out["u0"][bad] == 0).all()
    assert not np.isfinite(out["cost"][bad]).any() and not np.isfinite(out["cost0"][bad]).any()
    assert _in_box(out["U"][ovf], ub[ovf], "f64") and np.isin(out["status"][ovf], (1, 2)).all()
    print("thruster SQP: overflow status", out["status"][ovf], "major iterations", out["sqp_iters"][ovf], "cost", out["cost"][ovf])


def test_wrench_sqp(gpu_mpc_factory):
    """ftmpc_solve_sqp_wrench_batch, two major iterations, float64: as above with G = D stuck (the start point; 0 where a NaN stuck
    entry makes D stuck itself NaN), tau0 and u0 finite."""
    from ft_mpc_amd.controllers.tools.input_bounds import hull_tables
    N, NT, B = 5, 16, 24
    kw = dict(N=N, NT=NT, dtype="f64", max_iters=40)
    used, fresh = _handle(gpu_mpc_factory, **kw), _handle(gpu_mpc_factory, "fresh", **kw)
    x0, ub, stuck, xref = _spanning(qo.make_batch(2 * B, N, NT, 2, 72), used.D)
    xr = np.ascontiguousarray(xref.reshape(-1, order="F"))
    xp, sp, kind = po.poison(x0, ub, stuck, po.every_third(B), "f64")
    hull = hull_tables(used.D, ub, stuck)
    with np.errstate(all="ignore"):
        hull_p = hull_tables(used.D, ub, sp)
    run = lambda m, a, s, hl: m.solve_sqp_wrench(a, ub, s, xr, hull=hl, sqp_iters=2, backtracks=4)
    out, again, twin = run(used, xp, sp, hull_p), run(used, x0, stuck, hull), run(fresh, x0, stuck, hull)
    _bits(again, twin, _all(B), "persistence")
    _bits(out, twin, po.healthy(kind), "isolation")
    assert (twin["status"] == 0).all() and (twin["alloc_status"] == 0).all() and np.isfinite(twin["cost"]).all()
    bad, ovf = po.nonfinite(kind), po.overflow(kind)
    assert (out["status"][bad] == 2).all() and (out["sqp_iters"][bad] == 0).all()
    assert not np.isfinite(out["cost"][bad & (kind != "nan_stuck")]).any()      # (the wrench cost does not read stuck)
    for k in ("u0", "G", "tau0"):
        assert np.isfinite(out[k][bad | ovf]).all(), (k, kind[~np.isfinite(out[k].reshape(B, -1)).all(axis=1)])
    assert _in_box(out["u0"][bad | ovf], ub[bad | ovf], "f64")
    assert (out["alloc_status"][kind == "nan_stuck"] == 2).all() and (out["u0"][kind == "nan_stuck"] == 0).all()
    assert np.isin(out["status"][ovf], (1, 2)).all(), out["status"][ovf]
    print("wrench SQP: NaN/Inf allocation", out["alloc_status"][bad], "overflow status", out["status"][ovf], "major", out["sqp_iters"][ovf])


# ---------------------------------------------------------------------------------------------------------------------------
# closed loops: the campaign counters on a lost vehicle
# ---------------------------------------------------------------------------------------------------------------------------
SIGMA = (1e-2, 5e-3, 1e-2, 5e-3)


def _hover(N, T):
    xr = np.zeros((9, T + N))
    xr[8] = 0.6
    return xr


@pytest.mark.parametrize("form,dtype,est", [("thruster", "f64", True), ("wrench", "f64", False)], ids=["thruster-estimator", "two-stage"])
def test_closed_loop_counters(gpu_mpc_factory, form, dtype, est):
    """Six steps, B = 65 (a partial wave), vehicles 0, 31 and 64 poisoned at t = 0 (NaN position, NaN quaternion, NaN rate: the state
    stays non-finite through the plant).  Healthy vehicles: every history and outcome has the twin's bits; not_converged[t] is the
    twin's plus exactly 3, unsolved is T for the three, status_hist non-zero for them at every step."""
    N, NT, B, T = 5, 16, 65, 6
    kw = dict(N=N, NT=NT, dtype=dtype, max_iters=40)
    used, fresh = _handle(gpu_mpc_factory, **kw), _handle(gpu_mpc_factory, "fresh", **kw)
    x0, ub, stuck, _ = _spanning(qo.make_batch(2 * B, N, NT, 2, 81), used.D)
    x0[:, 0:6] *= 0.1
    where = np.array([0, 31, 64])
    xp, sp, kind = po.poison(x0, ub, stuck, where, dtype, po.POISONS[:3])
    h = po.healthy(kind)
    extra = dict(sensor=dict(sigma=SIGMA, seed=77, fields=("meas",)),
                 estimator=dict(every=1, p0=SIGMA, proc_sigma=tuple(0.1 * s for s in SIGMA), meas_sigma=SIGMA, fields=("est", "err_sq"))) if est else {}
    hull = None
    if form == "wrench":
        from ft_mpc_amd.controllers.tools.input_bounds import hull_tables
        hull = hull_tables(used.D, ub, stuck)
    run = lambda m, a, s: m.simulate(a, ub, s, _hover(N, T), T, seed=5, return_inputs=True, return_states=True, outcomes=True,
                                     return_status=True, formulation=form, hull=hull, **extra)
    out, again, twin = run(used, xp, sp), run(used, x0, stuck), run(fresh, x0, stuck)

    def per_vehicle(o):      # every per-vehicle array of the result, vehicle axis first
        d = dict(x=o["x"], u=o["u"].transpose(1, 0, 2), x_hist=o["x_hist"].transpose(1, 0, 2), status_hist=o["status_hist"].T)
        d.update({"outcomes/" + k: v for k, v in o["outcomes"].items()})
        for grp in ("sensor", "estimator"):
            for k, v in (o.get(grp) or {}).items():
                d[grp + "/" + k] = v.transpose(1, 0, 2) if v.ndim == 3 else v
        return d

    a, b, c = per_vehicle(out), per_vehicle(again), per_vehicle(twin)
    _bits(b, c, _all(B), "persistence")
    assert np.array_equal(again["not_converged"], twin["not_converged"])
    _bits(a, c, h, "isolation")
    assert np.isfinite(twin["x"]).all()
    print(f"{form} loop: not_converged {out['not_converged'].tolist()} (twin {twin['not_converged'].tolist()}), unsolved "
          f"{out['outcomes']['unsolved'][where].tolist()}, status of the three {out['status_hist'][:, where].T.tolist()}")
    assert np.array_equal(out["not_converged"], twin["not_converged"] + 3)
    assert (out["outcomes"]["unsolved"][where] == T).all() and (out["outcomes"]["first_unsolved"][where] == 0).all()
    assert (out["status_hist"][:, where] != 0).all()
