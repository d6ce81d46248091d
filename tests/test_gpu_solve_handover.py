"""Kernel 2 (ftmpc_solve_f32_kernel) hands work from one instance to the next inside a persistent wave: the next work-list number
is pulled while the current instance is solved, the handle's constants are staged once per wave, the float64 gradient exchanges
its lanes' data through LDS at short horizons and through the global slot beyond.  The small shapes at which that can go wrong,
each against the C oracle (float64, converged to mu 1e-13) at the fp32 tolerance of tests/test_gpu_parity.py: 1e-4 f_max on u0
and on the whole horizon.

Stage storage of the gradient sweeps: 9 (N + 1) doubles behind the vectors in LDS while (N + 1) * 72 <= 1632 bytes (the NB = 8
instantiation), i.e. N <= 21; N = 22 is the first horizon on the global-slot instantiation, N = 24 the first multiple of four."""
import os

import numpy as np
import pytest

import ft_mpc_amd
from oracle import c_oracle as co
from oracle import qp_oracle as qo
from oracle import refmath as rm

pytestmark = pytest.mark.gpu
F_MAX = rm.F_MAX
TOL = 1e-4
N, NT = 20, 8
# the persistent grid of the NB = 8 instantiation (ftmpc_capi.hip: grid[v] = num_cu * blocks_per_cu, launched as min(B, grid)):
# two waves per SIMD, four SIMDs per CU
WAVES_PER_CU = 8


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _oracle(cfg, x0, ub, stuck, xref, warmU=None):
    ref = co.solve_batch(cfg, x0, ub, stuck, xref, warmU=warmU, nthreads=_threads(), max_iters=60, mu_stop=1e-13)
    assert (ref["status"] == 0).all(), np.flatnonzero(ref["status"])
    return ref


def _check(out, ref, ub, rows=None):
    rows = slice(None) if rows is None else rows
    assert (out["status"][rows] == 0).all(), np.bincount(out["status"][rows])
    e0 = np.abs(out["u0"][rows] - ref["u0"][rows]).max() / F_MAX
    eU = np.abs(out["U"][rows] - ref["U"][rows]).max() / F_MAX
    print(f"max |u0 - oracle| = {e0:.2e} f_max, max |U - oracle| = {eU:.2e} f_max")
    assert e0 <= TOL and eU <= TOL
    assert (out["u0"][ub == 0] == 0).all()


def _same_bits(a, b):
    for k in ("u0", "U", "status", "iters"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("B", [1, 2])
def test_last_instance_of_a_wave_has_no_successor(gpu_mpc_factory, B):
    mpc = gpu_mpc_factory(N=N, NT=NT)
    x0, ub, stuck, xref = ft_mpc_amd.make_synthetic_batch(B, N, NT, 2, 5100 + B)
    out = mpc.solve(x0, ub, stuck, xref.reshape(-1, order="F"), return_U=True)
    _check(out, _oracle(qo.QPConfig(N=N, NT=NT), x0, ub, stuck, xref), ub)


def test_several_instances_per_wave(gpu_mpc_factory):
    """A batch of three times the persistent grid plus five: waves take three and more instances in a row."""
    import torch
    grid = torch.cuda.get_device_properties(0).multi_processor_count * WAVES_PER_CU
    B = 3 * grid + 5
    mpc = gpu_mpc_factory(N=N, NT=NT)
    x0, ub, stuck, xref = ft_mpc_amd.make_synthetic_batch(B, N, NT, 2, 5200)
    xr = xref.reshape(-1, order="F")
    out = mpc.solve(x0, ub, stuck, xr, return_U=True)
    _check(out, _oracle(qo.QPConfig(N=N, NT=NT), x0, ub, stuck, xref), ub)
    _same_bits(out, mpc.solve(x0, ub, stuck, xr, return_U=True))


def test_mixed_fault_counts_and_failed_vehicles_between_instances(gpu_mpc_factory):
    """0, 1, 2 and 3 broken thrusters interleaved (work lists of NB = 8, 9 and 10 with gaps) and every fifth vehicle with no
    thruster left: those take the early `continue` of the kernel between two solved instances."""
    B = 60
    x0, ub, stuck, xref = ft_mpc_amd.make_synthetic_batch(B, N, NT, 3, 5300)
    rng = np.random.default_rng(5301)
    for b in range(B):
        k = b % 5
        if k == 4:
            ub[b] = 0.0
            stuck[b] = rng.uniform(0, 1, NT) * F_MAX
        else:      # keep k of the three broken thrusters broken
            idx = np.flatnonzero(ub[b] == 0)[k:]
            ub[b, idx] = F_MAX
            stuck[b, idx] = 0.0
    dead = (ub == 0).all(axis=1)
    assert dead.sum() == B // 5 and sorted(set((ub[~dead] == 0).sum(axis=1))) == [0, 1, 2, 3]
    mpc = gpu_mpc_factory(N=N, NT=NT)
    out = mpc.solve(x0, ub, stuck, xref.reshape(-1, order="F"), return_U=True)
    assert (out["u0"][dead] == 0).all() and (out["U"][dead] == 0).all()
    assert (out["status"][dead] == 0).all() and (out["iters"][dead] == 0).all()
    live = np.flatnonzero(~dead)
    ref = _oracle(qo.QPConfig(N=N, NT=NT), x0[live], ub[live], stuck[live], xref)
    _check({k: v[live] for k, v in out.items()}, ref, ub[live])


def test_no_stale_state_between_launches(gpu_mpc_factory):
    mpc = gpu_mpc_factory(N=N, NT=NT)
    A = ft_mpc_amd.make_synthetic_batch(100, N, NT, 2, 5400)
    Bb = ft_mpc_amd.make_synthetic_batch(37, N, NT, 2, 5401)
    run = lambda t: mpc.solve(t[0], t[1], t[2], t[3].reshape(-1, order="F"), return_U=True)
    first = run(A)
    second = run(Bb)
    third = run(A)
    assert (first["status"] == 0).all() and (second["status"] == 0).all()
    _same_bits(first, third)


def test_each_handle_solves_with_its_own_constants(gpu_mpc_factory):
    B = 48
    x0, ub, stuck, xref = ft_mpc_amd.make_synthetic_batch(B, N, NT, 2, 5500)
    xr = xref.reshape(-1, order="F")
    kw1 = dict()
    kw2 = dict(Q=np.array([2.0, 1.5, 1.0, 0.5, 1.0, 2.0, 1.0, 3.0, 2.0]), R=np.array([0.2, 0.05, 0.1, 0.02, 0.01, 0.03]), rho=0.08)
    m1 = gpu_mpc_factory(N=N, NT=NT, **kw1)
    m2 = gpu_mpc_factory(N=N, NT=NT, **kw2)
    o1 = m1.solve(x0, ub, stuck, xr, return_U=True)
    o2 = m2.solve(x0, ub, stuck, xr, return_U=True)
    o1b = m1.solve(x0, ub, stuck, xr, return_U=True)
    _check(o1, _oracle(qo.QPConfig(N=N, NT=NT, **kw1), x0, ub, stuck, xref), ub)
    _check(o2, _oracle(qo.QPConfig(N=N, NT=NT, **kw2), x0, ub, stuck, xref), ub)
    _same_bits(o1, o1b)
    # each result is within TOL of its own oracle: more than 2 TOL apart, they are the solutions of different problems
    assert np.abs(o1["u0"] - o2["u0"]).max() / F_MAX > 2 * TOL


def test_warm_start(gpu_mpc_factory):
    B = 130
    x0, ub, stuck, xref = ft_mpc_amd.make_synthetic_batch(B, N, NT, 2, 5600)
    W = np.ascontiguousarray(np.random.default_rng(5601).uniform(0, 0.3, (B, N, NT)) * ub[:, None, :])
    W0 = W.copy()
    mpc = gpu_mpc_factory(N=N, NT=NT)
    out = mpc.solve(x0, ub, stuck, xref.reshape(-1, order="F"), warmU=W, return_U=True)
    _check(out, _oracle(qo.QPConfig(N=N, NT=NT), x0, ub, stuck, xref, warmU=W0), ub)
    assert np.array_equal(W, out["U"])      # (the warm-start buffer takes the solution)


@pytest.mark.parametrize("Nh", [24, 22])
def test_gradient_storage_in_the_global_slot(gpu_mpc_factory, Nh):
    """Three faults: n = 5 N <= 128, the NB = 8 instantiation, with the stage storage of the float64 sweeps beyond the LDS room
    (N > 21).  N = 22 runs the sweeps' tail for horizons that are no multiple of four."""
    B = 64
    x0, ub, stuck, xref = ft_mpc_amd.make_synthetic_batch(B, Nh, NT, 3, 5700 + Nh)
    mpc = gpu_mpc_factory(N=Nh, NT=NT)
    out = mpc.solve(x0, ub, stuck, xref.reshape(-1, order="F"), return_U=True)
    _check(out, _oracle(qo.QPConfig(N=Nh, NT=NT), x0, ub, stuck, xref), ub)
