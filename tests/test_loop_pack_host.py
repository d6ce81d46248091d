"""CPU: the two layout helpers of the closed loop's host layer (csrc/ftmpc_pack.h): pack_kb takes a caller's vehicle-major [B][K] array
to the component-major [K][B] the loop kernels read, unpack_kb takes it back.  Both walk the vehicles 64 at a time, so the sizes here
sit on the tail block and on the block boundary, where a blocked transpose goes wrong.

A stand-alone C++ program with its own main includes the header (which has no HIP include) and writes, for every (B, K), the packed
array, the unpacked packed array and the unpack of the input read as [K][B]; NumPy's transposes are the reference, to the bit."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "fault-tolerant-mpc_amd" / "csrc"
BS = (1, 63, 64, 65, 130)
KS = (1, 3, 21, 78)

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ftmpc_pack.h"
int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const long B = std::atol(argv[1]), K = std::atol(argv[2]);
    const size_t n = (size_t)(B * K);
    std::vector<double> in(n), out(3 * n, -1.0);
    FILE* f = std::fopen(argv[3], "rb");
    if (!f || std::fread(in.data(), sizeof(double), n, f) != n) return 3;
    std::fclose(f);
    ftmpc::pack_kb(in.data(), B, K, out.data());                    // [B][K] -> [K][B]
    ftmpc::unpack_kb(out.data(), B, K, out.data() + n);             // and back
    ftmpc::unpack_kb(in.data(), B, K, out.data() + 2 * n);          // the input read as [K][B] -> [B][K]
    f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
    std::fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("loop_pack")
    src = d / "loop_pack_main.cpp"
    src.write_text(MAIN)
    out = d / "loop_pack"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", str(CSRC), str(src), "-o", str(out)], check=True)
    return out


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", BS)
def test_pack_and_unpack_are_the_transposes(exe, tmp_path, B, K):
    rng = np.random.default_rng(1000 * B + K)
    a = rng.normal(size=B * K)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    a.tofile(fin)
    run = subprocess.run([str(exe), str(B), str(K), str(fin), str(fout)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    packed, back, unpacked = np.fromfile(fout).reshape(3, B * K)
    assert np.array_equal(packed.reshape(K, B), a.reshape(B, K).T)
    assert np.array_equal(back, a)                                       # the round trip
    assert np.array_equal(unpacked.reshape(B, K), a.reshape(K, B).T)
