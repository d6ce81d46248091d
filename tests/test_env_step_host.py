"""CPU: the per-vehicle step of the time-varying disturbance as the kernel runs it (csrc/ftmpc_env.h, the host / device functions
ftmpc_environment_kernel is made of) against ft_mpc_amd.environments.wrench.

A stand-alone C++ program with its own main includes the header and runs ftmpc_env::process once and ftmpc_env::step over 40 steps
of 7 vehicles with every component on: a base wrench, both Gauss-Markov processes from a stationary start, the periodic term with
a phase per vehicle and a kick whose window opens and closes inside the run; the vehicles are a slice [index0, index0 + 7) of a
campaign of 19 and the run starts at campaign step 5.  The program is built with -fsanitize=address,undefined where the toolchain
links them (a plain executable: nothing is preloaded and nothing is loaded into python), else without.
The bound is rtol 1e-12 + atol 1e-12, the one tests/test_gpu_sensors.py holds the device's Gaussian samples to: the two sides differ
by the libm's log / cos / sin / exp alone."""
import subprocess
from pathlib import Path

import numpy as np

from ft_mpc_amd import environments as EV

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "fault-tolerant-mpc_amd" / "csrc"
B, T, STEP0, INDEX0, TOTAL = 7, 40, 5, 3, 19
DT, SEED = 0.1, 0xC0FFEE1234
SIGMA, TAU, PERIOD = (0.4, 0.03), (1.5, 0.7), 2.3
N_IN = 6 + 6 + 1 + 6 + 2            # per vehicle: base, amp, phase, kick, window

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ftmpc_env.h"
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int B = 7, T = 40, NI = 21;
    const long long step0 = 5, index0 = 3, total = 19;
    const unsigned long long seed = 0xC0FFEE1234ull;
    const double sigma[2] = {0.4, 0.03}, tau[2] = {1.5, 0.7};
    std::vector<double> in((size_t)B * NI), out((size_t)T * B * 12);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
    std::fclose(f);
    ftmpc_env::Process p;
    ftmpc_env::process(sigma, tau, 0.1, 2.3, p);
    std::vector<double> g((size_t)B * 6, 0.0);
    for (int t = 0; t < T; ++t)
        for (int b = 0; b < B; ++b) {
            const double* v = in.data() + (size_t)b * NI;
            const long long c = step0 + t;
            const bool kicked = (long long)v[19] <= c && c < (long long)v[20];
            double* o = out.data() + ((size_t)t * B + b) * 12;
            ftmpc_env::step(p, seed, c, (unsigned long long)(c * total + index0 + b), t == 0, true, kicked, v, v + 6, v[12], v + 13,
                            g.data() + (size_t)b * 6, o);
            for (int j = 0; j < 6; ++j) o[6 + j] = g[(size_t)b * 6 + j];
        }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
    std::fclose(f);
    return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "env_step_main.cpp"
    src.write_text(MAIN)
    exe = tmp_path / "env_step"
    base = ["g++", "-std=c++17", "-O1", "-g", "-I", str(CSRC), str(src), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:
        subprocess.run(base, check=True)
    return exe


def test_header_step_is_environments_wrench(tmp_path):
    rng = np.random.default_rng(5)
    base = rng.normal(size=(B, 6)) * np.r_[np.full(3, 0.5), np.full(3, 0.05)]
    amp = rng.normal(size=(B, 6)) * np.r_[np.full(3, 0.3), np.full(3, 0.02)]
    phase = rng.uniform(0, 2 * np.pi, size=B)
    kick = rng.normal(size=(B, 6))
    window = np.stack([STEP0 + rng.integers(0, 20, size=B), STEP0 + rng.integers(10, 50, size=B)], axis=1)
    window[0] = (STEP0 + 9, STEP0 + 9)          # to <= from: none
    window[1] = (0, STEP0 + 4)                  # open before the run starts
    assert N_IN == 21
    rows = np.concatenate([base, amp, phase[:, None], kick, window.astype(np.float64)], axis=1)
    (tmp_path / "in.bin").write_bytes(np.ascontiguousarray(rows).tobytes())
    exe = _build(tmp_path)
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.float64).reshape(T, B, 12)

    g = None
    kicked_steps = 0
    for t in range(T):
        w, g = EV.wrench(STEP0 + t, g, DT, SIGMA, TAU, SEED, base, amp, phase, PERIOD, kick, window, INDEX0, TOTAL)
        np.testing.assert_allclose(got[t, :, 0:6], w, rtol=1e-12, atol=1e-12, err_msg=f"wrench, step {t}")
        np.testing.assert_allclose(got[t, :, 6:12], g, rtol=1e-12, atol=1e-12, err_msg=f"state, step {t}")
        kicked_steps += int(((window[:, 0] <= STEP0 + t) & (STEP0 + t < window[:, 1])).sum())
    # the case exercises what it says: the processes move, some steps are kicked and some are not
    assert 0 < kicked_steps < T * B
    assert np.std(got[:, :, 6]) > 0.1 and np.std(got[:, :, 9]) > 0.005
