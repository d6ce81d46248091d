"""CPU: the host side of the per-vehicle campaign outcomes (include/ftmpc.h, ftmpc_outcomes; ft_mpc_amd/outcomes.py): the four
entries are exported, the ctypes struct has the layout gcc gives the header, the NumPy reductions give hand values on a history
written out by hand, and the campaign-wide noise counter makes slices of a campaign draw what the whole draws."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from oracle import closed_loop as cl

ROOT = Path(__file__).resolve().parents[1]
NEW = ("ftmpc_simulate_outcomes_batch", "ftmpc_simulate_wrench_outcomes_batch", "ftmpc_multi_simulate_outcomes_batch",
       "ftmpc_multi_simulate_wrench_outcomes_batch")


def test_library_exports_the_outcome_entries():
    from ft_mpc_amd import _lib
    _lib.build_library()
    lib = _lib.load_library()
    for n in NEW:
        assert n in _lib.SYMBOLS and getattr(lib, n) is not None
    assert lib.ftmpc_version() >= 500
    # the last argument of each is the struct
    assert lib.ftmpc_simulate_outcomes_batch.argtypes[:-1] == lib.ftmpc_simulate_faults_batch.argtypes
    assert lib.ftmpc_simulate_wrench_outcomes_batch.argtypes[:-1] == lib.ftmpc_simulate_wrench_faults_batch.argtypes


def test_outcomes_struct_layout_matches_the_header(tmp_path):
    from ft_mpc_amd import _lib
    fields = [f for f, _ in _lib.ftmpc_outcomes._fields_]
    src = tmp_path / "layout.c"
    body = "".join(f'printf("{f} %zu\\n", offsetof(ftmpc_outcomes, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftmpc.h"\nint main(void){printf("sizeof %zu\\n", sizeof(ftmpc_outcomes));'
                   + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.ftmpc_outcomes) == 120
    for f in fields:
        assert int(got[f]) == getattr(_lib.ftmpc_outcomes, f).offset, f


def test_outcomes_from_history_on_a_hand_written_history():
    """2 vehicles, 3 steps, 2 thrusters, dt = 0.1, identity attitude, r = (0, 0.5, 0), omega = (0, 0, 0.6) throughout, so
    robot_to_center adds (0, 0.5, 0) to the position and omega x r = (-0.3, 0, 0) to the velocity; the reference is the origin at
    rest, rotating at 0.6.  The states below are written so that the centre error is e = (a, 0, 0 | 0, 0, 0 | 0, 0, 0):
      vehicle 0: a = 0.05, 0.3, 0.05  -- inside the 0.1 band, out again, inside: settle_step 2; in the set |e_0| <= 0.1 at step 0
      vehicle 1: a = 0.5, 0.4, 0.2    -- never inside: settle_step 3 = T, tset_step -1
    vehicle 0 has thruster 1 dead and stuck at 1.0 while the controller still commands 2.0 of it; vehicle 1 is healthy."""
    from ft_mpc_amd import MPCConfig
    from ft_mpc_amd.outcomes import outcomes_from_history, summarize
    T, B = 3, 2
    cfg = MPCConfig(N=5, NT=2, D=np.zeros((6, 2)), r=np.array([0.0, 0.5, 0.0]))
    a = np.array([[0.05, 0.5], [0.3, 0.4], [0.05, 0.2]])
    x_hist = np.zeros((T, B, 13))
    x_hist[..., 0] = a
    x_hist[..., 1] = -0.5
    x_hist[..., 3] = 0.3
    x_hist[..., 9] = 1.0
    x_hist[..., 12] = 0.6
    xref = np.zeros((9, T + 5))
    xref[8] = 0.6
    xref[0, 0] = 123.0        # column 0 is never compared: x_hist[t] goes with column t + 1
    u_hist = np.empty((T, B, 2))
    u_hist[:, 0] = [1.0, 2.0]
    u_hist[:, 1] = [0.5, 0.5]
    ub = np.array([[3.4, 0.0], [3.4, 3.4]])
    stuck = np.array([[0.0, 1.0], [0.0, 0.0]])
    status = np.array([[0, 0], [0, 1], [0, 2]], np.int32)
    A = np.zeros((2, 9))
    A[0, 0], A[1, 0] = 1.0, -1.0
    o = outcomes_from_history(cfg, x_hist, u_hist, status, xref, ub, stuck, tol=(0.1, 0.1, 0.1), term=(A, np.array([0.1, 0.1])),
                              alloc_status_hist=np.array([[0, 2], [0, 0], [1, 2]]))
    np.testing.assert_allclose(o["err_int"], [[0.1 * (0.0025 + 0.09 + 0.0025), 0, 0], [0.1 * (0.25 + 0.16 + 0.04), 0, 0]], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(o["err_max"], [[0.3, 0, 0], [0.5, 0, 0]], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(o["impulse"], [[0.1 * 3 * 2.0, 0.1 * 3 * 1.0], [0.3, 0.3]], rtol=1e-12)      # delivered != commanded
    assert o["settle_step"].tolist() == [2, 3] and o["settle_step"].dtype == np.int32
    assert o["tset_step"].tolist() == [0, -1]
    assert o["unsolved"].tolist() == [0, 2] and o["first_unsolved"].tolist() == [-1, 1]
    assert o["alloc_failed"].tolist() == [1, 2]
    rep = summarize(o, T=T)
    assert rep["vehicles"] == 2 and rep["recovered_fraction"] == 0.5 and rep["tset_fraction"] == 0.5 and rep["unsolved_fraction"] == 0.5


def test_global_noise_counter_makes_slices_equal_the_whole():
    """The plant kernel draws component i of vehicle b at step t at counter (t * index_total + index0 + b) * 13 + i.  A NumPy loop
    with that counter (a contraction standing in for the dynamics) over [0, 40) and [40, 96) gives the rows of the loop over all 96;
    with the counter of the call's own batch, (t * B + b) * 13 + i, it does not."""
    seed, total, T = 77, 96, 5
    rng = np.random.default_rng(3)
    x0 = rng.standard_normal((total, 13))

    def run(x, index0, index_total):
        x = x.copy()
        b = np.arange(x.shape[0], dtype=np.uint64)
        for t in range(T):
            idx = (np.uint64(t) * np.uint64(index_total) + np.uint64(index0) + b)[:, None] * np.uint64(13) + np.arange(13, dtype=np.uint64)
            x = 0.9 * x + 1e-3 * cl.u01(seed, idx)
        return x
    whole = run(x0, 0, total)
    parts = np.concatenate([run(x0[:40], 0, total), run(x0[40:], 40, total)])
    assert np.array_equal(parts, whole)
    local = np.concatenate([run(x0[:40], 0, 40), run(x0[40:], 0, 56)])
    assert not np.array_equal(local[:40], whole[:40]) and not np.array_equal(local[40:], whole[40:])
