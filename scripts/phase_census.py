#!/usr/bin/env python3
"""Diagnostic: instruction census of the fp32 solve kernel (kernel 2) per phase, from the device assembly.

usage: phase_census.py [device .s] [--kernel 8] [--passes 7.98] [--stages 20] [--refines 1.0] [--json out.json]

The stamps build (make -C fault-tolerant-mpc_amd/csrc stamps -> build/csrc_stamps/ftmpc_dev.s) leaves a comment
'; phase_census stamp <i>' right after every stamp site; the instructions between two such comments belong to the phase
of the second one (the phase whose cycles that stamp closes, the same split as scripts/stamps.py).  Without the comments
(the shipped build, build/csrc/ftmpc_dev_final.s) only the whole-kernel counts are printed.

Counts are STATIC (instructions in the text).  Each static region is multiplied by how often it runs per QP: the stage
loop's regions N - 1 times, the peeled terminal stage's once, the interior-point regions once per pass (two solves per
pass: two regions), the float64 gradient `--refines` times split over its two call sites.  Inside the stage loop the
tiles are guarded by run-time branches (X <= Imax), so its static count is the all-tiles upper bound; the PMC run
(SQ_INSTS_VALU, SQ_INSTS_MFMA) gives the dynamic totals to hold the census against.

Pipe cycles per wave: v_mfma_f32_16x16x4_f32 32, v_mfma_f64_16x16x4_f64 64 (fp32 MFMA and VALU share the pipe on gfx950,
scripts/ubench_pipe_share.hip), transcendental VALU 8, every other VALU 4 (wave64 issue on a SIMD of one wave).
"""
import argparse, collections, json, os, re, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHASES = ["prologue", "build:propagate", "build:mfma", "finalize+store", "matvec", "chol", "solves(2)", "elementwise",
          "refine (f64 grad)", "output", "x10", "x11"]
CLASSES = ["mfma", "mfma_f64", "valu_f32", "valu_f64", "dpp", "permlane", "lane_rw", "valu_other", "lds", "vmem",
           "scratch", "s_nop", "s_waitcnt", "salu"]
TRANS = ("v_rsq", "v_rcp", "v_sqrt", "v_exp", "v_log", "v_sin", "v_cos")


def classify(op, line):
    if op.startswith("v_mfma"):
        return "mfma_f64" if "f64" in op else "mfma"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_")):
        return "vmem"
    if op == "s_nop":
        return "s_nop"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_permlane"):
        return "permlane"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane_rw"
    if "_dpp" in op or re.search(r"\b(row_\w+|quad_perm|row_newbcast)\b", line):
        return "dpp"
    if "f64" in op:
        return "valu_f64"
    if "f32" in op:
        return "valu_f32"
    return "valu_other"


def pipe_cycles(op, cls):
    if cls == "mfma":
        return 32
    if cls == "mfma_f64":
        return 64
    if cls in ("valu_f32", "valu_f64", "dpp", "permlane", "lane_rw", "valu_other"):
        return 8 if op.startswith(TRANS) else 4
    return 0


def kernel_lines(asm, nb):
    key = f"ftmpc_solve_f32_kernelILi{nb}E"
    out, on = [], False
    for l in open(asm):
        if not on and re.match(r"^_Z\w*:", l) and key in l:
            on = True
        if on:
            out.append(l.rstrip("\n"))
            if l.startswith(".Lfunc_end"):
                break
    if not out:
        sys.exit(f"{key} not found in {asm}")
    return out


def census(lines):
    """[(phase index or None, Counter of classes, pipe cycles)] per static region, in text order"""
    regions, cur, cyc = [], collections.Counter(), 0
    for l in lines:
        m = re.search(r"phase_census stamp (\d+)", l)
        if m:
            regions.append((int(m.group(1)), cur, cyc))
            cur, cyc = collections.Counter(), 0
            continue
        t = l.strip()
        if not t or t.startswith((";", ".", "//")) or t.endswith(":"):
            continue
        op = t.split()[0]
        if not re.match(r"^(v|s|ds|buffer|global|flat|scratch)_", op):
            continue
        c = classify(op, t)
        cur[c] += 1
        cyc += pipe_cycles(op, c)
    regions.append((None, cur, cyc))
    return regions


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm", nargs="?", default=os.path.join(ROOT, "build", "csrc_stamps", "ftmpc_dev.s"))
    ap.add_argument("--kernel", type=int, default=8, help="NB of the instantiation")
    ap.add_argument("--passes", type=float, default=7.98, help="factorisations per QP (bench: config.ipm_iters_mean)")
    ap.add_argument("--stages", type=int, default=20)
    ap.add_argument("--refines", type=float, default=1.0, help="float64 gradients per QP")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    regions = census(kernel_lines(a.asm, a.kernel))
    seen = collections.Counter()
    per = collections.defaultdict(lambda: [collections.Counter(), 0.0, collections.Counter(), 0])   # dyn counts, dyn cycles, static, regions
    for ph, cnt, cyc in regions:
        occ = seen[ph]
        seen[ph] += 1
        if ph in (1, 2):
            w = (a.stages - 1) if occ == 0 else 1.0
        elif ph in (5, 6, 7):
            w = a.passes
        elif ph == 8:
            w = a.refines / 2.0
        elif ph is None:
            w = 0.0      # behind the last stamp: the instance loop's branch back
        else:
            w = 1.0
        name = PHASES[ph] if ph is not None else "(tail)"
        rec = per[name]
        for k, v in cnt.items():
            rec[0][k] += w * v
            rec[2][k] += v
        rec[1] += w * cyc
        rec[3] += 1
    tot = collections.Counter()
    totc = 0.0
    hdr = "%-18s %4s " % ("phase", "regs") + " ".join("%9s" % c for c in CLASSES) + " %11s" % "pipe cyc"
    print(f"{a.asm}: ftmpc_solve_f32_kernel<{a.kernel}>, per QP (static x runs; {a.passes} passes, {a.stages} stages)")
    print(hdr)
    order = [p for p in PHASES if p in per] + [p for p in per if p not in PHASES]
    for name in order:
        dyn, cyc, st, nreg = per[name]
        tot.update(dyn)
        totc += cyc
        print("%-18s %4d " % (name, nreg) + " ".join("%9.0f" % dyn[c] for c in CLASSES) + " %11.0f" % cyc)
    print("%-18s %4s " % ("total", "") + " ".join("%9.0f" % tot[c] for c in CLASSES) + " %11.0f" % totc)
    valu = sum(tot[c] for c in ("valu_f32", "valu_f64", "dpp", "permlane", "lane_rw", "valu_other"))
    print(f"VALU {valu:.0f}  MFMA {tot['mfma'] + tot['mfma_f64']:.0f}  VALU + 8 MFMA {valu + 8 * (tot['mfma'] + tot['mfma_f64']):.0f}")
    if a.json:
        out = {name: {"dynamic": dict(per[name][0]), "static": dict(per[name][2]), "pipe_cycles": per[name][1]} for name in order}
        out["_args"] = vars(a)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
