"""GPU: the float64 reference gradient of the fp32 solve kernels (csrc/ftmpc_solve.hip, struct_grad_at) in its two forms --
the sweeps as float64 MFMA chains and as row-per-lane vector FMAs -- through the test hook `BatchedMPC.debug_struct_grad`,
and whole solves through `ftmpc_solve_f32_kernel<8>` on both sides of the horizon at which the vector form is routed.

a. The hook, both forms, against numpy float64 from `oracle/qp_oracle.build_qp`: g + H d without the 2 rho (ubar + d) term.
   The tolerance is measured: the MFMA form's own worst error against that reference over all inputs of this file; the
   vector form may have at most twice that (the same number of float64 roundings in another order).  The error of an
   instance is max |g - g_ref| / max |g_ref|.  The test prints both errors and whether the two forms agree bit for bit.
   Both forms keep Da in fp32 as the solve kernel does, which is what separates them from numpy (about 1e-7); against each
   other they must agree to float64 rounding (1e-11, reasoned at the assertion).
   A batch of 130 holds 13 distinct instances ten times over (the reference is the slow part), so the launch's 44 waves
   take three instances each, always different ones, and equal instances must give equal bits wherever they ran.
b. Whole solves: N = 4 (the hand-on path, N a multiple of four), 5 (the scalar tail), 21 (the last horizon with the
   sweeps in LDS), 22 (the first that keeps the MFMA form), two faults, B = 24, against the C oracle at mu 1e-13 with the
   bounds of test_horizons_not_multiple_of_four; and B = 130 solved twice on one handle, expecting equal bits.
"""
import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import qp_oracle as qo
from oracle import refmath as rm

pytestmark = pytest.mark.gpu
F_MAX = rm.F_MAX
TOL_U = 1e-4
NT = 8
HORIZONS = (1, 3, 4, 5, 8, 20, 21)
FAULTS = (0, 2, 3)
BATCHES = (1, 2, 130)
DISTINCT = 13

_handles = {}
_results = {}


def _handle(factory, N):
    if N not in _handles:
        _handles[N] = factory(N=N, NT=NT)
    return _handles[N]


def _reference(cfg, qp, d):
    """g + H d of one instance without the rho terms (the caller of struct_grad_at adds 2 rho (ubar + d)); ubar = 0 here."""
    dd = d[:qp["n"]].astype(np.float64)
    return qp["g"] + qp["H"] @ dd - 2.0 * cfg.rho * dd


def _run(factory):
    """Every case of part a, once: {(N, nfault, B, dkind): (err_mfma, err_vec, equal_bits, difference of the two forms)}."""
    if _results:
        return _results
    for N in HORIZONS:
        mpc = _handle(factory, N)
        cfg = qo.QPConfig(N=N, NT=NT)
        for nfault in FAULTS:
            x0, ub, stuck, xref = qo.make_batch(DISTINCT, N, NT, nfault, 8100 + 10 * N + nfault)
            rng = np.random.default_rng(8200 + 10 * N + nfault)
            na = NT - nfault
            drand = np.zeros((DISTINCT, N * NT), dtype=np.float32)
            drand[:, :N * na] = (rng.uniform(0.0, 1.0, (DISTINCT, N * na)) * F_MAX).astype(np.float32)      # inside the box [0, ub]
            qps = [qo.build_qp(cfg, x0[b], ub[b], stuck[b], xref) for b in range(DISTINCT)]
            assert all(qp["n"] == N * na for qp in qps)
            for dkind, d13 in (("zero", np.zeros_like(drand)), ("random", drand)):
                ref = np.array([_reference(cfg, qps[b], d13[b]) for b in range(DISTINCT)])
                scale = np.abs(ref).max(axis=1)
                for B in BATCHES:
                    idx = np.arange(B) % DISTINCT
                    args = dict(x0=x0[idx], ub=ub[idx], stuck=stuck[idx], xref=np.ascontiguousarray(xref.reshape(-1, order="F")))
                    g0 = mpc.debug_struct_grad(d=d13[idx], form=0, **args)
                    g1 = mpc.debug_struct_grad(d=d13[idx], form=1, **args)
                    assert (g0[:, N * na:] == 0).all() and (g1[:, N * na:] == 0).all()
                    for g in (g0, g1):      # equal instances, equal bits, whatever the wave solved before
                        for b in range(DISTINCT, B):
                            assert np.array_equal(g[b], g[b % DISTINCT]), (N, nfault, B, dkind, b)
                    e0 = (np.abs(g0[:, :N * na] - ref[idx]).max(axis=1) / scale[idx]).max()
                    e1 = (np.abs(g1[:, :N * na] - ref[idx]).max(axis=1) / scale[idx]).max()
                    e01 = (np.abs(g1[:, :N * na] - g0[:, :N * na]).max(axis=1) / scale[idx]).max()
                    _results[(N, nfault, B, dkind)] = (e0, e1, bool(np.array_equal(g0, g1)), e01)
    return _results


@pytest.mark.parametrize("N", HORIZONS)
def test_vector_form_within_twice_the_mfma_forms_error(gpu_mpc_factory, N):
    res = _run(gpu_mpc_factory)
    worst_mfma = max(v[0] for v in res.values())
    # (sanity of hook and reference: the kernels keep Da in fp32 -- 6e-8 per entry, entering g = .. Da' .. Da d twice -- and
    # everything else in float64, so both forms sit a few 1e-7 from numpy; an fp32 evaluation or a wrong layout is far above)
    assert 0.0 < worst_mfma < 1e-6, worst_mfma
    for (n_, nfault, B, dkind), (e0, e1, same, e01) in sorted(res.items()):
        if n_ != N:
            continue
        print(f"N={N} faults={nfault} B={B} d={dkind}: mfma {e0:.3e}  vector {e1:.3e}  worst mfma {worst_mfma:.3e}  "
              f"forms differ by {e01:.3e}  equal bits: {same}")
        assert e1 <= 2.0 * worst_mfma, (N, nfault, B, dkind, e0, e1, worst_mfma)
        # The two forms against each other, where the fp32 Da cancels: the same float64 roundings in another order.  2 N stages of
        # dot products of at most 19 terms at 1.1e-16 give 9e-14 at N = 21, times the growth of the sweeps (products of the A_k,
        # of order 1 to 10 at these horizons): 1e-11 leaves two orders for that and is four orders below the figure above.
        assert e01 <= 1e-11, (N, nfault, B, dkind, e01)


@pytest.mark.parametrize("N", [4, 5, 21, 22])
def test_whole_solves_around_the_routing_seam(gpu_mpc_factory, N):
    nfault, B = 2, 24
    mpc = _handle(gpu_mpc_factory, N)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, nfault, 8300 + N)
    out = mpc.solve(x0, ub, stuck, xref.reshape(-1, order="F"), return_U=True)
    assert (out["status"] == 0).all(), out["status"]
    ref = co.solve_batch(qo.QPConfig(N=N, NT=NT), x0, ub, stuck, xref, nthreads=4, max_iters=60, mu_stop=1e-13)
    assert (ref["status"] == 0).all()
    eu0 = np.abs(out["u0"] - ref["u0"]).max() / F_MAX
    eU = np.abs(out["U"] - ref["U"]).max() / F_MAX
    print(f"N={N}: u0 {eu0:.3e} f_max, U {eU:.3e} f_max")
    assert eu0 <= 1e-4
    assert eU <= TOL_U


@pytest.mark.parametrize("N", [4, 5, 21, 22])
def test_a_batch_solved_twice_gives_the_same_bits(gpu_mpc_factory, N):
    nfault, B = 2, 130
    mpc = _handle(gpu_mpc_factory, N)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, nfault, 8400 + N)
    a = mpc.solve(x0, ub, stuck, xref.reshape(-1, order="F"), return_U=True)
    b = mpc.solve(x0, ub, stuck, xref.reshape(-1, order="F"), return_U=True)
    assert (a["status"] == 0).all(), a["status"]
    for k in ("u0", "U", "status", "iters"):
        assert np.array_equal(a[k], b[k]), k
