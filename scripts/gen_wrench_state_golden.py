#!/usr/bin/env python3
"""Writes tests/golden/qp_wrench_state_n15.npz: the first batch of tests/wrench_state_rows.py (N = 15, 16 thrusters, two faults,
|v| <= 0.9, |omega| <= 1.6 on the generalized-force formulation) with the oracle's verdicts -- whole-horizon wrenches, status and
the number of active state rows per instance (oracle/qp_oracle.py:ipm_general with its polish over the rows of the helper)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from oracle import qp_oracle as qo      # noqa: E402
import wrench_state_rows as ws          # noqa: E402


def main():
    N, NT, nf, B, seed = ws.BATCHES[0]
    cfg = qo.QPConfig(N=N, NT=NT)
    x0, ub, stuck, xref = qo.make_batch(B, N, NT, nf, seed)
    xlb, xub = ws.bounds()
    G = np.zeros((B, N, 6))
    status = np.zeros(B, np.int32)
    active = np.zeros(B, np.int32)
    kkt = np.zeros(B)
    with np.errstate(all="ignore"):
        for b in range(B):
            _, G[b], status[b], _, qp = ws.solve_wrench_state_instance(cfg, x0[b], ub[b], stuck[b], xref, xlb, xub)
            if status[b] == 0:
                active[b] = ws.active_state_rows(qp)
                kkt[b] = max(qo.kkt_general(qp["H"], qp["g"], qp["C"], qp["h"], qp["d"], qp["z"]))
    out = ROOT / "tests" / "golden" / "qp_wrench_state_n15.npz"
    np.savez_compressed(out, N=N, NT=NT, x0=x0, ub=ub, stuck=stuck, xref=xref, xlb=xlb, xub=xub, G=G, status=status, active_rows=active, kkt=kkt)
    print(out, "solved", int((status == 0).sum()), "active", int((active > 0).sum()), "kkt max", kkt.max())


if __name__ == "__main__":
    main()
