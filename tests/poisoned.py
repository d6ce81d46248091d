"""Poisoned batches and their clean twins (helper of test_poisoned_host.py and test_gpu_poisoned_instances.py; not a test module).

A vehicle of a fault campaign that diverges ends with a huge, Inf or NaN state.  include/ftmpc.h promises FTMPC_STATUS_NUMERIC and
the linearisation point for it; what the suite must hold besides is that such an instance does not touch the rest of its batch:
padding tiles, identity blocks and parked factors are multiplied by exact zeros, and 0 * residue is 0 only for a finite residue.

`poison` takes a healthy batch (the CLEAN TWIN: same shape, ub and fault pattern) and returns the poisoned copy, one poison per
poisoned instance, cycled in the order of POISONS:

  nan_pos    NaN in x[0]       position: reaches the gradient, not the Hessian
  nan_quat   NaN in x[6]       quaternion: Hessian and gradient
  nan_rate   NaN in x[10]      rate
  nan_stuck  NaN in the stuck entry of the first broken thruster (needs a fault)
  inf_pos    +Inf in x[0]
  overflow   x[0] = 1e30 on an fp32 handle, 1e200 on a float64 one: finite as the entry receives it

Placement: `every_third(B)` for the persistent one-wave and workgroup kernels (a wave takes a healthy instance after a poisoned one),
`wave_lanes(B)` for the lane-per-instance kernels (lanes 0, 31 and 63 of the first wave and the last lane of a partial last wave)."""
import numpy as np

POISONS = ("nan_pos", "nan_quat", "nan_rate", "nan_stuck", "inf_pos", "overflow")
NONFINITE = POISONS[:5]
OVERFLOW = {"f32": 1e30, "f64": 1e200}

# (N, NT, faults, B, seed) of qo.make_batch: the shapes of test_gpu_poisoned_instances.py whose verdicts test_poisoned_host.py fixes
# on the C oracle (every healthy instance converges there in 60 iterations)
SHAPES = ((20, 8, 2, 24, 1), (3, 8, 2, 24, 3), (23, 8, 2, 24, 4), (11, 16, 2, 24, 5), (5, 16, 2, 24, 6))


def every_third(B):
    return np.arange(1, B, 3)


def wave_lanes(B):
    """lanes 0, 31 and 63 of the first wave and the last lane of the partial last wave"""
    assert B > 64 and B % 64 != 0, B
    return np.array([0, 31, 63, B - 1])


def poison(x0, ub, stuck, where, dtype="f32", kinds=POISONS):
    """(x0_p, stuck_p, kind): the poisoned copies and kind[b] = the name of instance b's poison ("" for a healthy one)"""
    x0p, stp = np.array(x0, float), np.array(stuck, float)
    kind = np.full(x0p.shape[0], "", dtype=object)
    for i, b in enumerate(where):
        k = kinds[i % len(kinds)]
        kind[b] = k
        if k == "nan_pos":
            x0p[b, 0] = np.nan
        elif k == "nan_quat":
            x0p[b, 6] = np.nan
        elif k == "nan_rate":
            x0p[b, 10] = np.nan
        elif k == "nan_stuck":
            broken = np.flatnonzero(np.asarray(ub)[b] == 0)
            assert broken.size, ("nan_stuck needs a broken thruster", b)
            stp[b, broken[0]] = np.nan
        elif k == "inf_pos":
            x0p[b, 0] = np.inf
        elif k == "overflow":
            x0p[b, 0] = OVERFLOW[dtype]
        else:
            raise ValueError(k)
    return x0p, stp, kind


def healthy(kind):
    return kind == ""


def nonfinite(kind):
    return np.isin(kind, NONFINITE)


def overflow(kind):
    return kind == "overflow"


def same_bits(a, b):
    """bitwise equality of two arrays (NaN payloads and the sign of zero included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
