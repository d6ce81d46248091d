#!/usr/bin/env python3
"""Cost of the disturbance estimate in the on-device closed loop (BatchedMPC.simulate(disturbance=...)), timed with hipEvents.

    python scripts/disturbance_perf.py [--batch 65536] [--N 20] [--steps 20] [--json out.json]
    python scripts/disturbance_perf.py --case wrench64 | wrench32 [--sqp K] [--json profiles/disturbance_wrench64_sqp0.json]

Loop steps: every loop is run twice, T = warm-up + steps and T = warm-up (default 5 + 20 and 5), between two hipEvents recorded on the
idle device around the synchronous library call; the difference over `steps` is the time per loop step without the call's staging and
copies.  Loops: sensor-free with the estimator alone (ftmpc_filter_kernel<0> / <1>), without a filter, with the disturbance estimate
and compensate = 0 (ftmpc_filter_dist_kernel<0..3>, the plain linearise kernel) and with compensate = 1 (the DIST linearise kernel),
and the last two once more with the diagnosis (ftmpc_diagnose_dist_kernel in place of ftmpc_diagnose_kernel<1>).  The filters' own
cost is the difference to the loop without a filter: four launches of the augmented filter against the estimator's two.
Linearise kernel: the library's own hipEvents around the launch (set_profiling, slot 0) over `steps` one-step loops after a warm-up,
plain (compensate = 0) against the DIST instantiation (compensate = 1) on the same states.
--case wrench64 / wrench32: the two-stage wrench form (disturbance["wrench"] = True) at the shape scripts/fault_campaign_perf.py times it
at, N = 15, 16 thrusters, B = 16 384, a float64 / fp32 handle, one wrench QP per step or, --sqp K, K major iterations of the wrench
SQP (the DIST linearisation and ftmpc_cost_wrench_kernel<1> in every launch under compensate = 1).  The hull tables are built once,
outside the timing.  The cost kernel's own time per launch, plain against DIST, comes from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python scripts/disturbance_perf.py --case wrench64 --sqp 2 --steps 5): both instantiations run in it,
the plain one in the loops without compensation."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "fault-tolerant-mpc_amd"))
sys.path.insert(0, str(ROOT))

SIGMA = (1e-2, 5e-3, 1e-2, 5e-3)
WARM = 5


def main():
    import torch

    import ft_mpc_amd
    from ft_mpc_amd import diagnosis as DG
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("thruster", "wrench64", "wrench32"), default="thruster")
    ap.add_argument("--sqp", type=int, default=0, help="major iterations of the wrench SQP per loop step (the wrench cases)")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--N", type=int, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    wrench = a.case != "thruster"
    if a.sqp and not wrench:
        ap.error("--sqp belongs to the wrench cases (the thruster-form SQP loop takes no disturbance estimate)")
    B = a.batch if a.batch is not None else (16384 if wrench else 65536)
    N = a.N if a.N is not None else (15 if wrench else 20)
    NT, K = 16 if wrench else 8, a.steps
    x0, ub, stuck, _ = ft_mpc_amd.make_synthetic_batch(B, N, NT, 1, 77)
    rng = np.random.default_rng(3)
    plant = dict(force=rng.uniform(-0.3, 0.3, (B, 3)), torque=rng.uniform(-0.02, 0.02, (B, 3)))
    if wrench:
        from ft_mpc_amd.controllers.tools.input_bounds import hull_tables
        mpc = ft_mpc_amd.BatchedMPC(N=N, NT=NT, dtype="f64" if a.case == "wrench64" else "f32", max_iters=60)
        hull = hull_tables(mpc.D, ub, stuck)
        form = dict(formulation="wrench", hull=hull, sqp_iters=a.sqp)
    else:
        mpc = ft_mpc_amd.BatchedMPC(N=N, NT=NT, dtype="f32")
        form = {}
    mpc.reserve(B)
    est = dict(every=1, p0=SIGMA, proc_sigma=tuple(0.1 * s for s in SIGMA), meas_sigma=SIGMA, fields=())
    dg = dict(levels=(0.0, 1.7, 3.4), resid_sigma=DG.default_sigma(SIGMA), threshold=18.0, fields=())
    dist = dict(p0=(0.5, 0.05), proc_sigma=(1e-3, 1e-4), fields=())
    if wrench:
        dist["wrench"] = True
        dg["rebuild_hull"] = True

    def xr(T):
        r = np.zeros((9, T + N))
        r[8] = 0.6
        return r

    def timed(T, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        mpc.simulate(x0, ub, stuck, xr(T), T, noise=(1e-3,) * 4, seed=5, plant=plant, **form, **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    loops = dict(no_filter={}, estimator=dict(estimator=est),
                 disturbance_nominal=dict(estimator=est, disturbance=dict(dist, compensate=False)),
                 disturbance_compensated=dict(estimator=est, disturbance=dict(dist, compensate=True)),
                 estimator_diagnosis=dict(estimator=est, diagnosis=dg),
                 disturbance_nominal_diagnosis=dict(estimator=est, diagnosis=dg, disturbance=dict(dist, compensate=False)),
                 disturbance_compensated_diagnosis=dict(estimator=est, diagnosis=dg, disturbance=dict(dist, compensate=True)))
    out = dict(case=a.case, sqp_iters=a.sqp, B=B, N=N, NT=NT, steps=K, warmup=WARM, step_ms={})
    timed(WARM)                                                    # first call: allocations
    for name, kw in loops.items():
        long, short = min(timed(WARM + K, **kw) for _ in range(2)), min(timed(WARM, **kw) for _ in range(2))
        out["step_ms"][name] = (long - short) / K
        print(f"{name:36s} {out['step_ms'][name]:9.4f} ms per loop step")
    s = out["step_ms"]
    out["filter_ms"] = dict(estimator=s["estimator"] - s["no_filter"], disturbance=s["disturbance_nominal"] - s["no_filter"])
    print(f"filter per step: ftmpc_filter_kernel<0> + <1> {out['filter_ms']['estimator']:.4f} ms, "
          f"ftmpc_filter_dist_kernel<0..3> {out['filter_ms']['disturbance']:.4f} ms")
    if not wrench:      # (the library's per-kernel events belong to the thruster path's solve; the wrench cases: see the kernel trace)
        mpc.set_profiling(True)
        lin = {}
        for name, comp in (("plain", False), ("dist", True)):
            ms = []
            for k in range(WARM + K):
                mpc.simulate(x0, ub, stuck, xr(1), 1, noise=(0.0,) * 4, seed=5, estimator=est, disturbance=dict(dist, compensate=comp))
                ms.append(float(mpc.last_kernel_ms()["ftmpc_linearize_kernel"]))
            lin[name] = float(np.mean(ms[WARM:]))
        out["linearize_ms"] = lin
        print(f"linearise kernel: plain {lin['plain']:.4f} ms, with the estimate {lin['dist']:.4f} ms ({K} launches each)")
    s = out["step_ms"]
    out["estimate_ms"] = dict(nominal=s["disturbance_nominal"] - s["estimator"], compensated=s["disturbance_compensated"] - s["estimator"])
    print(f"the estimate per loop step against the loop with the estimator alone: {out['estimate_ms']['nominal']:+.4f} ms with compensate = 0, "
          f"{out['estimate_ms']['compensated']:+.4f} ms with compensate = 1 ({100 * out['estimate_ms']['compensated'] / s['estimator']:+.1f} %)")
    mpc.close()
    if a.json:
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
