"""Throughput of the two-stage step with STATE BOUNDS on the generalized-force formulation (kernel 13's state-bound instantiation,
ftmpc_solve_ricw64_kernel<6, false, true>) beside the plain kernel 13 on the same batch: N = 15, 16 thrusters, two faults,
|v| <= 0.9, |omega| <= 1.6, float64 handles, B = 16 384 through the host entry (ftmpc_solve_wrench_batch: host buffers in and out, hull
tables built beforehand), host clock around the synchronising call, three runs after a warm-up (best and spread).
Arguments: `plain` times the plain handle only (what a build without the mode can run); a number is the batch size."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT + "/fault-tolerant-mpc_amd")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import ft_mpc_amd  # noqa: E402
from ft_mpc_amd.controllers.tools.input_bounds import hull_tables  # noqa: E402

N, NT = 15, 16
args = sys.argv[1:]
plain_only = "plain" in args
B = next((int(a) for a in args if a.isdigit()), 16384)
xub, xlb = np.full(13, np.inf), np.full(13, -np.inf)
xub[3:6], xlb[3:6] = 0.9, -0.9
xub[6:9], xlb[6:9] = 1.6, -1.6
print("library build", ft_mpc_amd.load_library().ftmpc_build_id().decode())
for name, kw in [("plain", {})] + ([] if plain_only else [("state bounds", dict(xlb=xlb, xub=xub))]):
    m = ft_mpc_amd.BatchedMPC(N=N, NT=NT, dtype="f64", max_iters=60, **kw)
    x0, ub, stuck, xref = ft_mpc_amd.make_synthetic_batch(B, N, NT, 2, 1213)
    hull = hull_tables(m.D, ub, stuck)
    keep = ~hull["degenerate"]          # (every instance of the timed batch has a hull)
    x0, ub, stuck = x0[keep], ub[keep], stuck[keep]
    hull = hull_tables(m.D, ub, stuck)
    b = x0.shape[0]
    xr = np.ascontiguousarray(xref.reshape(-1, order="F"))
    out = m.solve_wrench(x0, ub, stuck, xr, hull=hull)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        m.solve_wrench(x0, ub, stuck, xr, hull=hull)
        ts.append(time.perf_counter() - t0)
    print(f"{name:12s} B={b:6d}: {min(ts) * 1e3:8.2f} ms  {b / min(ts):10.0f} QP-steps/s (three runs: {', '.join(f'{b / t:.0f}' for t in ts)})  "
          f"iterations mean {out['iters'].mean():.2f}  status != 0: {int((out['status'] != 0).sum())}/{b} "
          f"({100.0 * (out['status'] != 0).mean():.2f} %)  allocation failed {int((out['alloc_status'] != 0).sum())}", flush=True)
    m.close()
