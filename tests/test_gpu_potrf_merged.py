"""GPU check of the in-register 16x16 potrf + inverse that reads W = L^-1 from the eliminated columns of the tile
(scripts/test_potrf_merged.hip), against a verbatim copy of the form with a second tile E that it replaced, on the same
matrices in the same run: one wave per matrix, 1, 2 and 130 matrices.  Compiles the diagnostic with hipcc on the GPU box.

The two forms round differently but equally often, so the new form's max|W L - I| and max|W - W64| / max|W64| may be at most
twice the copy's (a step-by-step float32 emulation on the host gave 1.17 at the worst, tests/test_potrf_merged_host.py)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path_factory.mktemp("potrf_merged") / "test_potrf_merged"
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-o", str(exe), str(ROOT / "scripts" / "test_potrf_merged.hip")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("done"), (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    out = []
    for ln in run.stdout.splitlines():
        kv = dict(re.findall(r"(\w+)=(\S+)", ln))
        if "case" in kv:
            out.append(kv)
    return out


@pytest.mark.parametrize("case", ["a", "b", "c"])     # random SPD; plus a diagonal up to 1e8 on some rows; the half tile
@pytest.mark.parametrize("B", [1, 2, 130])
def test_new_form_is_as_accurate_as_the_one_it_replaced(lines, case, B):
    (kv,) = [k for k in lines if k["case"] == case and int(k["B"]) == B]
    print(kv)
    assert float(kv["ref_wl"]) < 1e-4 and float(kv["ref_w"]) < 1e-5          # the copy itself is sane (float32: a few 1e-7)
    assert float(kv["new_wl"]) <= 2.0 * float(kv["ref_wl"])
    assert float(kv["new_w"]) <= 2.0 * float(kv["ref_w"])
    assert float(kv["upper"]) == 0.0                                          # exact zeros above the diagonal
    assert int(kv["dup_mismatch"]) == 0                                       # equal matrices, equal bits, whichever wave
    assert int(kv["pad_rows_wrong"]) == 0                                     # half tile: rows 8..15 of W are rows of I


@pytest.mark.parametrize("B", [1, 2, 130])
@pytest.mark.parametrize("NM", [48, 80])
def test_every_work_slot_runs_once(lines, B, NM):
    (kv,) = [k for k in lines if k["case"] == "d" and int(k["B"]) == B and int(k["NM"]) == NM]
    assert int(kv["count_min"]) == NM and int(kv["count_max"]) == NM
    assert int(kv["acc_mismatch"]) == 0       # the accumulators hold what a plain loop over the same MFMAs gives
    assert int(kv["w_mismatch"]) == 0         # and W is the W of the call without work


def test_a_bad_pivot_shows_in_the_last_diagonal_entry(lines):
    (kv,) = [k for k in lines if k["case"] == "e"]
    assert int(kv["negative_pivot_w1515_finite"]) == 0
    assert int(kv["zero_pivot_w1515_finite"]) == 0
