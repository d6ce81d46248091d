"""GPU: the full-record linearise kernel (`ftmpc_linearize_kernel<double, 0>`, forced through lin_split_max < 0) writes the
same record bits as the direction-split kernel (`<double, 1>`, the default at these batch sizes), and both agree with the
oracle's linearisation.

The records come back through the test hook `BatchedMPC.debug_records`; a solve on the same two handles must also agree
in every output bit.  The batches put a lone lane, a full wave, one real lane in the last wave and a partial last wave
through the full-record kernel's cooperative write-out.

Tolerance against the oracle: what test_build_matches_oracle uses, 2e-5 of the block's scale (both sides are float64
here, so the figures are near 1e-12; the comparison is there so that a mistake shared by both kernels cannot pass).
"""
import numpy as np
import pytest

from oracle import qp_oracle as qo
from oracle import refmath as rm

pytestmark = pytest.mark.gpu

REC = dict(APW=0, APQ=9, AVW=21, AVQ=30, AWW=42, AQW=51, AQQ=63, BPF=79, BPT=88, BVF=97, BVT=106, BWT=115, BQT=124, WE=136,
           RUT=145, USED=151)
# record block -> (matrix, rows, columns) of the oracle's A (13 x 13) / Bg (13 x 6); centre state [p, v, w, q], wrench [F, tau]
BLOCKS = dict(APW=("A", (0, 3), (6, 9)), APQ=("A", (0, 3), (9, 13)), AVW=("A", (3, 6), (6, 9)), AVQ=("A", (3, 6), (9, 13)),
              AWW=("A", (6, 9), (6, 9)), AQW=("A", (9, 13), (6, 9)), AQQ=("A", (9, 13), (9, 13)),
              BPF=("B", (0, 3), (0, 3)), BPT=("B", (0, 3), (3, 6)), BVF=("B", (3, 6), (0, 3)), BVT=("B", (3, 6), (3, 6)),
              BWT=("B", (6, 9), (3, 6)), BQT=("B", (9, 13), (3, 6)))
TOL = 2e-5

_handles = {}
_batches = {}


def _pair(factory, **kw):
    """(full-record handle, direction-split handle) of one configuration, made once per session."""
    key = repr(sorted((k, np.asarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v)) for k, v in kw.items()))
    if key not in _handles:
        _handles[key] = (factory(lin_split_max=-1, **kw), factory(**kw))
    return _handles[key]


def _batch(B, N, NT):
    """0, 1 and 2 faults mixed over the batch and one failed vehicle (no healthy thruster); the warm inputs with it."""
    if (B, N, NT) in _batches:
        return _batches[(B, N, NT)]
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, 2, 7000 + 131 * B + N)
    rng = np.random.default_rng(7100 + B + N)
    for b in range(B):
        broken = np.flatnonzero(ub[b] == 0)
        heal = broken[:2 - (b % 3)] if B > 1 else broken[:0]       # b % 3 faults stay
        ub[b, heal], stuck[b, heal] = rm.F_MAX, 0.0
    if B > 1:
        dead = B // 2
        ub[dead] = 0.0
        stuck[dead] = rng.uniform(0, 1, NT) * rm.F_MAX
    traj = rm.circle_trajectory(0.1, 10, radius=0.65, s_per_circle=40.0)
    xr_all, ur_all = rm.assign_trajectory(traj, N)
    xw = np.zeros((B, 9 * (N + 1)))
    uw = np.zeros((B, 6 * (N + 1)))
    for b in range(B):      # every instance its own window of the trajectory: per-instance reference strides
        xb, ubb = rm.trajectory_window(xr_all, ur_all, 0.1 * (b % 37), N)
        xw[b], uw[b] = xb.reshape(-1, order="F"), ubb.reshape(-1, order="F")
    W = np.ascontiguousarray(rng.uniform(-0.1, 1.1, (B, N, NT)) * rm.F_MAX)      # (some entries outside [0, ub]: the clip)
    out = dict(x0=x0, ub=ub, stuck=stuck, xref=np.ascontiguousarray(xref.reshape(-1, order="F")), xw=xw, uw=uw, W=W)
    _batches[(B, N, NT)] = out
    return out


def _inputs(d, warm):
    if warm:
        return dict(x0=d["x0"], ub=d["ub"], stuck=d["stuck"], xref=d["xw"], uref=d["uw"], warmU=d["W"].copy())
    return dict(x0=d["x0"], ub=d["ub"], stuck=d["stuck"], xref=d["xref"])


def _check_against_oracle(rec, mpc, d, warm, N, NT, insts, terminal_we=True, cfg=None, tol=TOL):
    """cfg: the QPConfig equal to the handle's constants (None: the default vehicle); tol: of each block's scale"""
    cfg = qo.QPConfig(N=N, NT=NT) if cfg is None else cfg
    fv = np.concatenate([cfg.f_virt, np.zeros(3)])
    for b in insts:
        ub, stuck = d["ub"][b], d["stuck"][b]
        cbar, A, Bg, Ubar = qo.linearize(cfg, d["x0"][b], ub, stuck, d["W"][b] if warm else None)
        xr = (d["xw"][b] if warm else d["xref"]).reshape(9, N + 1, order="F")
        ur = d["uw"][b].reshape(6, N + 1, order="F") if warm else None
        for k in range(N):
            r = rec[b, k]
            for name, (m, (r0, r1), (c0, c1)) in BLOCKS.items():
                ref = (A if m == "A" else Bg)[k][r0:r1, c0:c1]
                got = r[REC[name]:REC[name] + ref.size].reshape(ref.shape)
                assert np.abs(got - ref).max() <= tol * max(1.0, np.abs(ref).max()), (b, k, name)
            e = cbar[k + 1][0:9] - xr[:, k + 1]
            if k + 1 < N or terminal_we:
                we = cfg.Q * e if k + 1 < N else mpc.P @ e
                assert np.abs(r[REC["WE"]:REC["WE"] + 9] - we).max() <= tol * max(1.0, np.abs(we).max()), (b, k, "WE")
            u_r = np.zeros(6) if ur is None else np.concatenate([rm.rot(cbar[k][9:13]).T @ ur[0:3, k], ur[3:6, k]])
            rut = cfg.R * (cfg.D @ (Ubar[k] + stuck) - u_r - fv)
            assert np.abs(r[REC["RUT"]:REC["RUT"] + 6] - rut).max() <= tol * max(1.0, np.abs(rut).max()), (b, k, "RUT")
            assert r[REC["USED"]] == 0.0


def _compare(factory, B, N, NT, warm, terminal_we=True, **kw):
    full, split = _pair(factory, N=N, NT=NT, **kw)
    d = _batch(B, N, NT)
    ra = full.debug_records(**_inputs(d, warm))
    rb = split.debug_records(**_inputs(d, warm))
    assert ra.shape == (B, N, 152)
    assert np.array_equal(ra, rb), np.argwhere(ra != rb)[:8]
    a = full.solve(return_U=True, **_inputs(d, warm))
    b = split.solve(return_U=True, **_inputs(d, warm))
    for k in ("u0", "U", "status", "iters"):
        assert np.array_equal(a[k], b[k]), k
    _check_against_oracle(ra, full, d, warm, N, NT, sorted({0, B // 2, min(B - 1, 63), B - 1}), terminal_we)


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("N,NT", [(20, 8), (7, 8), (15, 16)])
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_full_record_kernel_writes_the_split_kernels_records(gpu_mpc_factory, B, N, NT, warm):
    _compare(gpu_mpc_factory, B, N, NT, warm)


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_records_with_the_terminal_cost_terms(gpu_mpc_factory, warm):
    """config/terminal.yaml's cost: the last stage's W e carries the gradient of the non-quadratic terms (the tcost path);
    that word is compared between the kernels only, the oracle's linearisation has no such term."""
    _compare(gpu_mpc_factory, 65, 20, 8, warm, terminal_we=False, terminal_cost=True)


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_records_and_solve_with_state_bounds(gpu_mpc_factory, warm):
    """State bounds: the kernel also writes the linearisation trajectory (out_cbar) the state rows are built from; it
    reaches the comparison through the solve's outputs."""
    _compare(gpu_mpc_factory, 130, 20, 8, warm, dtype="f64", xlb=np.full(13, -5.0), xub=np.full(13, 5.0))
