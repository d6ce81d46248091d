"""Throughput of the line-search SQP on the reference's own nonlinear program (ftmpc_solve_sqp_wrench_batch: generalized-force
decision, input hull, 72-row terminal set and full terminal cost), N = 15, 16 thrusters, two faults, ten major iterations and eight
backtracks, both handle dtypes, B = 64 / 1 024 / 16 384: NLP solves per second, host clock around the synchronising call (host
buffers in and out, as a caller sees it), best of three after a warm-up.  Optional argument: a comma-separated list of batch sizes."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT + "/fault-tolerant-mpc_amd")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import ft_mpc_amd  # noqa: E402
from ft_mpc_amd.controllers.tools.input_bounds import hull_tables  # noqa: E402
from ft_mpc_amd.controllers.tools.terminal_ingredients import load_terminal  # noqa: E402

N, NT, ITERS, BT = 15, 16, 10, 8
sizes = [int(s) for s in sys.argv[1].split(",")] if len(sys.argv) > 1 else [64, 1024, 16384]
T = load_terminal()
for dt in ("f64", "f32"):
    m = ft_mpc_amd.BatchedMPC(N=N, NT=NT, dtype=dt, max_iters=60, terminal_set=T.term_set, terminal_cost=T)
    for B in sizes:
        x0, ub, stuck, xref = ft_mpc_amd.make_synthetic_batch(B, N, NT, 2, 1213)
        hull = hull_tables(m.D, ub, stuck)
        keep = ~hull["degenerate"]          # (every instance of the timed batch has a hull)
        x0, ub, stuck = x0[keep], ub[keep], stuck[keep]
        hull = hull_tables(m.D, ub, stuck)
        b = x0.shape[0]
        xr = np.ascontiguousarray(xref.reshape(-1, order="F"))
        out = m.solve_sqp_wrench(x0, ub, stuck, xr, hull=hull, sqp_iters=ITERS, backtracks=BT)
        best = 1e9
        for _ in range(3):
            t0 = time.perf_counter()
            m.solve_sqp_wrench(x0, ub, stuck, xr, hull=hull, sqp_iters=ITERS, backtracks=BT)
            best = min(best, time.perf_counter() - t0)
        print(f"{dt} B={b:6d}: {best * 1e3:9.2f} ms  {b / best:10.0f} NLP solves/s  major iterations mean {out['sqp_iters'].mean():.2f}  "
              f"IPM iterations mean {out['iters'].mean():.1f}  cost0/cost median {np.median(out['cost0'] / out['cost']):.1f}  "
              f"inside the terminal set {int((out['tviol'] <= 1e-9).sum())}/{b}  QP status 2 {int((out['status'] == 2).sum())}", flush=True)
    m.close()
