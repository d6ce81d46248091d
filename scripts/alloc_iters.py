"""Diagnostic: Newton steps of the allocation kernel on the wrenches the two-stage step hands over."""
import sys, time
import os; ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + '/fault-tolerant-mpc_amd')
import numpy as np
import ft_mpc_amd
from ft_mpc_amd.controllers.tools.input_bounds import hull_tables
from oracle import qp_oracle as qo
N, NT, B = 15, 16, 16384
x0, ub, stuck, xref = qo.make_batch(B, N, NT, 2, 7900)
cfg = qo.QPConfig(N=N, NT=NT)
hull = hull_tables(cfg.D, ub, stuck)
for dt in ("f32", "f64"):
    m = ft_mpc_amd.BatchedMPC(N=N, NT=NT, dtype=dt, max_iters=40)
    out = m.solve_wrench(x0, ub, stuck, xref.reshape(-1, order="F"), hull=hull)
    ok = out["status"] == 0
    taud = out["tau0"][ok] - stuck[ok] @ cfg.D.T
    t0 = time.perf_counter(); a = m.allocate(taud, ub[ok]); t1 = time.perf_counter() - t0
    print(dt, "alloc status", np.bincount(a["status"], minlength=3), "iters: mean %.2f  hist" % a["iters"].mean(), np.bincount(np.minimum(a["iters"], 51))[:52], "%.2f ms" % (t1 * 1e3))
    m.close()
