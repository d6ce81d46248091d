"""Diagnostic: one instance of the hull + terminal-set form on the float64 kernel against the NumPy oracle (objective, feasibility)."""
import sys
import os; ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + '/fault-tolerant-mpc_amd')
import numpy as np
import ft_mpc_amd
from ft_mpc_amd.controllers.tools.input_bounds import hull_tables
from ft_mpc_amd.controllers.tools.terminal_ingredients import load_terminal
from oracle import qp_oracle as qo, refmath as rm
N, NT, B, scale = 15, 16, 8192, 1.0
INST = int(sys.argv[1]) if len(sys.argv) > 1 else 3141
term = load_terminal().term_set
At, bt = term.A, term.b.reshape(-1)
x0, ub, stuck, xref = qo.make_batch(B, N, NT, 2, 9100)
rng = np.random.default_rng(9101); r = rm.spiral_r()
for b in range(B):
    e = rng.standard_normal(9); e *= scale / max((At @ e / bt).max(), 1e-9)
    R = rm.rot(x0[b, 6:10]); w = rm.OMEGA_DES + e[6:9]
    x0[b, 0:3] = e[0:3] - R.T @ r; x0[b, 3:6] = e[3:6] - R.T @ np.cross(w, r); x0[b, 10:13] = w
cfg = qo.QPConfig(N=N, NT=NT)
sl = slice(INST, INST + 1)
with np.errstate(all="ignore"):
    _, T, st, nit, qp = qo.solve_wrench_instance(cfg, x0[INST], ub[INST], stuck[INST], xref, term_set=(At, bt), iters=60)
print("oracle: status %d iters %d, active rows (z > 1e-6): hull %d terminal %d" % (st, nit, (qp["z"][:qp["nhull"]] > 1e-6).sum(), (qp["z"][qp["nhull"]:] > 1e-6).sum()))
H, g, Cm, hv, d_or = qp["H"], qp["g"], qp["C"], qp["h"], qp["d"]
obj = lambda d: 0.5 * d @ H @ d + g @ d
for dt in ("f64", "f32"):
    for mi in (60, 200):
        m = ft_mpc_amd.BatchedMPC(N=N, NT=NT, dtype=dt, max_iters=mi, terminal_set=term)
        out = m.solve_wrench(x0[sl], ub[sl], stuck[sl], xref.reshape(-1, order="F"), return_G=True)
        G = out["G"][0]
        d = (G - (T - d_or.reshape(N, 6))).reshape(-1)      # same linearisation point as the oracle: ubar = T - d
        print("%s max_iters %3d: status %d iters %2d  |G - oracle| %.2e f_max  objective - oracle's %.3e  worst row violation %.2e" %
              (dt, mi, out["status"][0], out["iters"][0], np.abs(G - T).max() / 3.4, obj(d) - obj(d_or), (Cm @ d - hv).max()))
        m.close()
