"""GPU: the full-record linearise kernel, whose tangents run by direction group with the exact-zero terms left out
(csrc/ftmpc_tangent.h), writes the record values of the split kernel, which keeps the generic 13-direction loop.

Records through `BatchedMPC.debug_records` on a pair of handles, lin_split_max = -1 (full-record kernel at every batch size)
against the default (split kernel at these sizes), compared with np.array_equal.  Shapes: a single stage (no hand-over between
stages), two and three stages (the flush hand-over), one lane and one lane past a full wave.  Every batch starts with
instances at rest in the identity attitude (w0 = 0, q0 = (0, 0, 0, 1): the blocks with exact zeros in them) and mixes 0, 1 and
2 faults and one vehicle with no healthy thruster.  Equality is value equality; each comparison prints how many words differ
in their bits (the sign of a zero is the one place a left-out `+ 0` can show).
"""
import numpy as np
import pytest

from oracle import qp_oracle as qo
from oracle import refmath as rm

pytestmark = pytest.mark.gpu

_handles = {}
_batches = {}


def _pair(factory, **kw):
    key = repr(sorted(kw.items()))
    if key not in _handles:
        _handles[key] = (factory(lin_split_max=-1, **kw), factory(**kw))
    return _handles[key]


def _batch(B, N, NT):
    if (B, N, NT) in _batches:
        return _batches[(B, N, NT)]
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, 2, 9100 + 17 * B + N)
    rng = np.random.default_rng(9200 + B + N)
    for b in range(B):
        broken = np.flatnonzero(ub[b] == 0)
        heal = broken[:2 - (b % 3)]            # b % 3 faults stay
        ub[b, heal], stuck[b, heal] = rm.F_MAX, 0.0
    # at rest in the identity attitude: x = [p, v, q = (x, y, z, w), omega]
    for b in range(min(B, 3)):
        x0[b, 6:10] = (0.0, 0.0, 0.0, 1.0)
        x0[b, 10:13] = 0.0
    if B > 1:
        dead = B // 2
        ub[dead] = 0.0
        stuck[dead] = rng.uniform(0, 1, NT) * rm.F_MAX
    traj = rm.circle_trajectory(0.1, 10, radius=0.65, s_per_circle=40.0)
    xr_all, ur_all = rm.assign_trajectory(traj, N)
    xw = np.zeros((B, 9 * (N + 1)))
    uw = np.zeros((B, 6 * (N + 1)))
    for b in range(B):
        xb, ubb = rm.trajectory_window(xr_all, ur_all, 0.1 * (b % 37), N)
        xw[b], uw[b] = xb.reshape(-1, order="F"), ubb.reshape(-1, order="F")
    W = np.ascontiguousarray(rng.uniform(-0.1, 1.1, (B, N, NT)) * rm.F_MAX)
    d = dict(x0=x0, ub=ub, stuck=stuck, xref=np.ascontiguousarray(xref.reshape(-1, order="F")), xw=xw, uw=uw, W=W)
    _batches[(B, N, NT)] = d
    return d


def _inputs(d, warm):
    if warm:
        return dict(x0=d["x0"], ub=d["ub"], stuck=d["stuck"], xref=d["xw"], uref=d["uw"], warmU=d["W"].copy())
    return dict(x0=d["x0"], ub=d["ub"], stuck=d["stuck"], xref=d["xref"])


def _same(ra, rb, what):
    bits = int((ra.view(np.uint64) != rb.view(np.uint64)).sum())
    print(f"{what}: {ra.size} words, {int((ra != rb).sum())} differ in value, {bits} in bits")
    assert np.isfinite(ra).all()
    assert np.array_equal(ra, rb), np.argwhere(ra != rb)[:8]


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm_uref"])
@pytest.mark.parametrize("N,NT", [(1, 8), (2, 8), (3, 16)])
@pytest.mark.parametrize("B", [1, 65])
def test_group_kernel_writes_the_generic_kernels_records(gpu_mpc_factory, B, N, NT, warm):
    full, split = _pair(gpu_mpc_factory, N=N, NT=NT)
    d = _batch(B, N, NT)
    ra = full.debug_records(**_inputs(d, warm))
    rb = split.debug_records(**_inputs(d, warm))
    assert ra.shape == (B, N, 152)
    assert full.lib.ftmpc_version() == 540
    _same(ra, rb, f"B={B} N={N} NT={NT} warm={warm}")


def test_group_kernel_with_a_disturbance_estimate(gpu_mpc_factory):
    """The DIST instantiations: a non-zero estimate (f^ inertial, t^ body) per instance."""
    B, N, NT = 65, 2, 8
    full, split = _pair(gpu_mpc_factory, N=N, NT=NT)
    d = _batch(B, N, NT)
    rng = np.random.default_rng(9300)
    dist = np.concatenate([rng.normal(size=(B, 3)) * 0.5, rng.normal(size=(B, 3)) * 0.05], axis=1)
    for warm in (False, True):
        ra = full.debug_records_disturbance(dist=dist, **_inputs(d, warm))
        rb = split.debug_records_disturbance(dist=dist, **_inputs(d, warm))
        _same(ra, rb, f"DIST warm={warm}")
        assert not np.array_equal(ra, full.debug_records(**_inputs(d, warm)))      # the estimate reached the kernel


def test_solve_on_the_two_kernels_agrees(gpu_mpc_factory):
    B, N, NT = 24, 4, 8
    full, split = _pair(gpu_mpc_factory, N=N, NT=NT)
    d = _batch(B, N, NT)
    for warm in (False, True):
        a = full.solve(return_U=True, **_inputs(d, warm))
        b = split.solve(return_U=True, **_inputs(d, warm))
        for k in ("u0", "U", "status", "iters"):
            assert np.array_equal(a[k], b[k]), (k, warm)
