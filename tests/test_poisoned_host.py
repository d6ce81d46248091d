"""CPU: what tests/poisoned.py builds and what the C oracle answers on it (the reference of test_gpu_poisoned_instances.py).

oracle/qp_oracle.py:solve_instance returns a finite vector on a NaN instance without any flag and is NOT a reference for poisoned
instances; oracle/c_oracle.py:solve_batch (max_iters 60, mu_stop 1e-13) is: status 2 after one iteration with the cold
linearisation point (all zero) on every NaN / Inf poison.  Its verdict on the overflow poisons is recorded here per shape:
x[0] = 1e30 (what an fp32 handle is given) converges to a bang-bang solution, x[0] = 1e200 (float64 handle) stops at max_iters."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))

from oracle import c_oracle as co
from oracle import qp_oracle as qo
from oracle import refmath as rm
import poisoned as po

# the oracle's (status, iterations within) on the overflow poison of every shape of po.SHAPES (measured: 15 or 16 iterations at 1e30)
OVERFLOW_VERDICT = {"f32": (0, 16), "f64": (1, 60)}


def _solve(q, x0, ub, stuck, xref):
    with np.errstate(all="ignore"):
        return co.solve_batch(q, x0, ub, stuck, xref, max_iters=60, mu_stop=1e-13, nthreads=4)


@pytest.mark.parametrize("place", ["every_third", "wave_lanes"])
def test_the_twin_differs_only_in_the_poisoned_rows(place):
    N, NT, nf = 5, 16, 2
    B = 24 if place == "every_third" else 65
    where = po.every_third(B) if place == "every_third" else po.wave_lanes(B)
    if place == "wave_lanes":
        assert where.tolist() == [0, 31, 63, 64]
    x0, ub, stuck, _ = qo.make_batch(B, N, NT, nf, 6)
    keep = x0.copy(), stuck.copy()
    for dtype in ("f32", "f64"):
        xp, sp, kind = po.poison(x0, ub, stuck, where, dtype)
        assert po.same_bits(x0, keep[0]) and po.same_bits(stuck, keep[1])      # the twin is left as it was
        h = po.healthy(kind)
        assert sorted(np.flatnonzero(~h)) == sorted(where)
        assert po.same_bits(xp[h], x0[h]) and po.same_bits(sp[h], stuck[h])
        assert [kind[b] for b in where] == [po.POISONS[i % 6] for i in range(len(where))]
        for b in where:
            dx, ds = np.flatnonzero(xp[b] != x0[b]), np.flatnonzero(sp[b] != stuck[b])
            assert dx.size + ds.size == 1, (b, dx, ds)      # one entry per poisoned instance ...
            if kind[b] == "nan_stuck":
                assert ub[b, ds[0]] == 0 and np.isnan(sp[b, ds[0]])      # ... of a broken thruster
            elif kind[b] == "overflow":
                assert dx[0] == 0 and xp[b, 0] == po.OVERFLOW[dtype] and np.isfinite(np.float32(xp[b, 0]) if dtype == "f32" else xp[b, 0])
            else:
                assert dx[0] == {"nan_pos": 0, "nan_quat": 6, "nan_rate": 10, "inf_pos": 0}[kind[b]]
                assert not np.isfinite(xp[b, dx[0]])
        assert (po.nonfinite(kind) | po.overflow(kind) | h).all() and (po.nonfinite(kind) & po.overflow(kind)).sum() == 0


@pytest.mark.parametrize("shape", po.SHAPES, ids=lambda s: f"N{s[0]}-NT{s[1]}")
def test_oracle_verdicts(shape):
    N, NT, nf, B, seed = shape
    q = qo.QPConfig(N=N, NT=NT)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, nf, seed)
    twin = _solve(q, x0, ub, stuck, xref)
    assert (twin["status"] == 0).all(), twin["status"]
    for dtype in ("f32", "f64"):
        xp, sp, kind = po.poison(x0, ub, stuck, po.every_third(B), dtype)
        assert set(kind) == set(po.POISONS) | {""}
        out = _solve(q, xp, ub, sp, xref)
        h, bad, ovf = po.healthy(kind), po.nonfinite(kind), po.overflow(kind)
        for k in ("u0", "U", "status", "iters"):      # the oracle solves instance by instance: the healthy ones keep their bits
            assert po.same_bits(out[k][h], twin[k][h]), k
        assert (out["status"][bad] == 2).all(), list(zip(kind[bad], out["status"][bad]))
        assert (out["iters"][bad] == 1).all()
        assert (out["U"][bad] == 0).all() and (out["u0"][bad] == 0).all()      # the cold linearisation point
        st, it = OVERFLOW_VERDICT[dtype]
        print(f"N={N} NT={NT} overflow {po.OVERFLOW[dtype]:g}: status {out['status'][ovf]}, iterations {out['iters'][ovf]}, "
              f"|U| up to {np.abs(out['U'][ovf]).max():.3g}")
        assert (out["status"][ovf] == st).all() and (out["iters"][ovf] <= it).all(), (out["status"][ovf], out["iters"][ovf])
        assert np.isfinite(out["U"][ovf]).all() and (out["U"][ovf] >= 0).all() and (out["U"][ovf] <= ub[ovf][:, None, :] + 1e-9).all()


def test_warm_started_poison_returns_the_clipped_warm_start():
    """the linearisation point of a warm start: clip(warm start) to [0, ub], zero on broken thrusters"""
    N, NT, nf, B, seed = po.SHAPES[0]
    q = qo.QPConfig(N=N, NT=NT)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, nf, seed)
    W = np.random.default_rng(2).uniform(-0.5, rm.F_MAX + 0.5, (B, N, NT))
    xp, sp, kind = po.poison(x0, ub, stuck, po.every_third(B), "f64")
    with np.errstate(all="ignore"):
        out = co.solve_batch(q, xp, ub, sp, xref, warmU=W.copy(), max_iters=60, mu_stop=1e-13)
    bad = po.nonfinite(kind)
    assert (out["status"][bad] == 2).all()
    assert np.array_equal(out["U"][bad], np.clip(W, 0.0, ub[:, None, :])[bad])
