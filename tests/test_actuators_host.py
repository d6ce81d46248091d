"""CPU: the host side of the pulsed thrusters and the valve lag (include/ftmpc.h, ftmpc_actuator; ft_mpc_amd/actuators.py): the four
entries are exported, the ctypes struct has the layout gcc gives the header and no earlier struct changed size, ticks / dead band /
alignment windows, the impulse identity without lag, the lag's closed form, one step against oracle.refmath, the refusals Python
raises before any call reaches the library, and the convergence of the PWM plant to the proportional one as the clock gets finer."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import qp_oracle as qo
from oracle import refmath as rm

ROOT = Path(__file__).resolve().parents[1]
NEW = ("ftmpc_simulate_actuator_batch", "ftmpc_simulate_wrench_actuator_batch", "ftmpc_multi_simulate_actuator_batch",
       "ftmpc_multi_simulate_wrench_actuator_batch")
FIELDS = ["struct_size", "mode", "substeps", "min_on", "align", "reserved", "tau_on", "tau_off", "delivered", "pulses", "applied_hist",
          "ticks_hist", "state"]


def test_library_exports_the_actuator_entries():
    from ft_mpc_amd import _lib
    _lib.build_library()
    lib = _lib.load_library()
    header = (ROOT / "include" / "ftmpc.h").read_text()
    for n in NEW:
        assert n in _lib.SYMBOLS and getattr(lib, n) is not None
        assert f"int {n}(" in header
    assert lib.ftmpc_version() >= 530
    assert lib.ftmpc_simulate_actuator_batch.argtypes[:-1] == lib.ftmpc_simulate_mission_batch.argtypes
    assert lib.ftmpc_simulate_wrench_actuator_batch.argtypes[:-1] == lib.ftmpc_simulate_wrench_mission_batch.argtypes
    assert lib.ftmpc_multi_simulate_actuator_batch.argtypes[:-1] == lib.ftmpc_multi_simulate_mission_batch.argtypes
    assert lib.ftmpc_multi_simulate_wrench_actuator_batch.argtypes[:-1] == lib.ftmpc_multi_simulate_wrench_mission_batch.argtypes


def test_actuator_struct_layout_matches_the_header(tmp_path):
    from ft_mpc_amd import _lib
    assert [f for f, _ in _lib.ftmpc_actuator._fields_] == FIELDS
    src = tmp_path / "layout.c"
    body = "".join(f'printf("{f} %zu\\n", offsetof(ftmpc_actuator, {f}));' for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftmpc.h"\nint main(void){printf("sizeof %zu\\n", sizeof(ftmpc_actuator));'
                   + body + 'printf("outcomes %zu\\nplant %zu\\nmission %zu\\n", sizeof(ftmpc_outcomes), sizeof(ftmpc_plant_model), '
                   'sizeof(ftmpc_mission));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.ftmpc_actuator) and int(got["sizeof"]) % 8 == 0
    for f in FIELDS:
        assert int(got[f]) == getattr(_lib.ftmpc_actuator, f).offset, f
    # no existing struct changed
    assert int(got["outcomes"]) == C.sizeof(_lib.ftmpc_outcomes) == 120
    assert int(got["plant"]) == C.sizeof(_lib.ftmpc_plant_model) == 48
    assert int(got["mission"]) == C.sizeof(_lib.ftmpc_mission) == 56


# ---------------------------------------------------------------------------------------------------------------------------
# actuators.py
# ---------------------------------------------------------------------------------------------------------------------------
def test_ticks_ends_dead_band_and_dead_thrusters():
    from ft_mpc_amd.actuators import ticks
    ub = np.array([3.4, 3.4, 0.0, 1.7])
    for S in (1, 5, 8, 64):
        assert np.array_equal(ticks(np.zeros(4), ub, S), [0, 0, 0, 0])
        assert np.array_equal(ticks(ub, ub, S), [S, S, 0, S])
        assert np.array_equal(ticks(2 * ub + 1, ub, S), [S, S, 0, S])          # the duty is clipped; a dead thruster gives 0
        assert np.array_equal(ticks(-np.ones(4), ub, S), [0, 0, 0, 0])
    # S = 8: u / ub = 0.3 -> floor(2.4 + 0.5) = 2, 0.32 -> floor(3.06) = 3
    assert np.array_equal(ticks([0.3 * 3.4, 0.32 * 3.4, 1.0, 0.07 * 1.7], ub, 8), [2, 3, 0, 1])
    # the dead band: k < min_on becomes 0, nothing rounds up; k = min_on stays
    assert np.array_equal(ticks([0.3 * 3.4, 0.32 * 3.4, 1.0, 0.07 * 1.7], ub, 8, min_on=3), [0, 3, 0, 0])
    assert ticks(np.zeros((5, 7, 4)), np.broadcast_to(ub, (5, 7, 4)), 8).dtype == np.int32


@pytest.mark.parametrize("S", [5, 8])
def test_alignment_windows_lie_inside_the_step(S):
    from ft_mpc_amd.actuators import targets
    ub = np.full(S + 1, 3.4)
    k = np.arange(S + 1)              # S - k odd and even
    for align, start in (("leading", np.zeros(S + 1, int)), ("centred", (S - k) // 2), ("trailing", S - k)):
        g = targets(k, ub, S, align)
        assert g.shape == (S, S + 1)
        on = g > 0
        assert np.array_equal(on.sum(axis=0), k)                   # exactly k ticks, none lost past the end of the step
        assert set(np.unique(g)) <= {0.0, 3.4}
        for i in range(1, S + 1):
            j = np.flatnonzero(on[:, i])
            assert j[0] == start[i] and j[-1] == start[i] + k[i] - 1 and 0 <= j[0] and j[-1] < S
            assert np.array_equal(j, np.arange(j[0], j[0] + k[i]))  # one contiguous pulse


def test_impulse_identity_without_lag():
    from ft_mpc_amd.actuators import lag_constants, substep_forces, targets, ticks
    rng = np.random.default_rng(3)
    S, dt = 16, 0.1
    h = dt / S
    ub = np.where(rng.random((40, 8)) < 0.2, 0.0, 3.4)
    u = rng.uniform(0, 3.4, (40, 8))
    consts = lag_constants(h, 0.0, 0.0)
    assert consts == (0.0, 0.0, 0.0, 0.0)                          # tau = 0: E = K = 0
    for align in ("leading", "centred", "trailing"):
        k = ticks(u, ub, S, 2)
        m, a = substep_forces(targets(k, ub, S, align), rng.uniform(0, 3.4, (40, 8)), consts)
        # without lag the valve delivers its target whatever its state was (the sum of k <= 16 equal terms: a few ulp)
        assert np.allclose((h * m).sum(axis=0), k * h * ub, rtol=1e-14, atol=0)
        assert np.array_equal(a, targets(k, ub, S, align)[-1])


def test_lag_closed_form():
    from ft_mpc_amd.actuators import lag_constants, substep_forces
    h, tau_on, tau_off, g, n = 0.1 / 8, 0.02, 0.01, 3.4, 8
    E_on, K_on, E_off, K_off = lag_constants(h, tau_on, tau_off)
    assert E_on == np.exp(-h / tau_on) and E_off == np.exp(-h / tau_off)
    assert abs(K_on - (1 - E_on) * tau_on / h) < 1e-15 and abs(K_off - (1 - E_off) * tau_off / h) < 1e-15
    m, a = substep_forces(np.full((n, 1), g), np.zeros(1), (E_on, K_on, E_off, K_off))
    assert abs(a[0] - g * (1 - E_on ** n)) < 1e-14
    # telescoped: h m_j = g h - tau (a_{j+1} - a_j), so h sum_j m_j = g h n - tau_on a_n  (the valve's state started at 0)
    assert abs(h * m.sum() - (g * h * n - tau_on * a[0])) < 1e-14
    # falling: from a_0 with target 0, a_n = a_0 E_off^n and h sum m = tau_off (a_0 - a_n)
    m, a = substep_forces(np.zeros((n, 1)), np.full(1, g), (E_on, K_on, E_off, K_off))
    assert abs(a[0] - g * E_off ** n) < 1e-14 and abs(h * m.sum() - tau_off * (g - a[0])) < 1e-14


def test_step_proportional_one_substep_is_the_reference_plant():
    from ft_mpc_amd.actuators import step
    x0, ub, stuck, _ = qo.make_batch(6, 10, 8, 2, 5)
    D = rm.allocation_matrix_8()
    rng = np.random.default_rng(9)
    for b in range(6):
        u = rng.uniform(0, 3.4, 8)
        ref = rm.rk4(lambda x: rm.plant_dx_dt(x, u, D, stuck[b], ub[b]), x0[b], 0.1)
        out = step(x0[b], u, ub[b], stuck[b], dict(mode="proportional", substeps=1))
        assert np.abs(out["x"] - ref).max() <= 1e-15
        assert np.array_equal(out["state"], np.where(ub[b] > 0, u, 0.0)) and out["ticks"] is None
        assert np.allclose(out["applied"], np.where(ub[b] > 0, u, 0.0) + stuck[b], rtol=1e-15, atol=0)


def test_min_on_ticks():
    from ft_mpc_amd.actuators import min_on_ticks
    assert min_on_ticks(0.0, 0.1, 16) == 0
    assert min_on_ticks(0.00625, 0.1, 16) == 1 and min_on_ticks(0.007, 0.1, 16) == 2
    assert min_on_ticks(1.0, 0.1, 16) == 16


def test_python_refusals():
    from ft_mpc_amd.actuators import step
    from ft_mpc_amd.batch import _actuator_request
    B, T, NT = 3, 2, 8
    for bad in (dict(mode="bang"), dict(mode="pwm", substeps=0), dict(mode="pwm", substeps=65), dict(mode="pwm", substeps=8, min_on=9),
                dict(mode="pwm", substeps=8, min_on=-1), dict(mode="pwm", substeps=8, align="middle"), dict(mode="pwm", tau_on=-1.0),
                dict(mode="pwm", tau_off=np.inf), dict(mode="proportional", substeps=4, min_on=1),
                dict(mode="proportional", substeps=4, align="centred"), dict(mode="proportional", fields=("pulses",)),
                dict(mode="proportional", fields=("ticks",)), dict(mode="pwm", fields=("thrust",)), dict(mode="pwm", clock=3),
                dict(mode="pwm", state=np.zeros((B, NT + 1))), dict(mode="pwm", state=-np.ones((B, NT))),
                dict(mode="pwm", state=np.full((B, NT), np.nan))):
        with pytest.raises(ValueError):
            _actuator_request(bad, B, T, NT)
    ac, keep, out = _actuator_request(dict(mode="pwm", substeps=8, min_on=2, align="centred", tau_on=0.02, state=np.ones((B, NT)),
                                           fields=("delivered", "pulses", "applied", "ticks", "state")), B, T, NT)
    assert (ac.struct_size, ac.mode, ac.substeps, ac.min_on, ac.align, ac.tau_on, ac.tau_off) == (C.sizeof(type(ac)), 1, 8, 2, 1, 0.02, 0.0)
    assert out["delivered"].shape == (B,) and out["pulses"].dtype == np.int32 and out["applied"].shape == (T, B, NT)
    assert out["ticks"].shape == (T, B, NT) and out["ticks"].dtype == np.int32 and np.array_equal(out["state"], np.ones((B, NT)))
    with pytest.raises(ValueError):
        step(np.zeros(13), np.zeros(8), np.ones(8), np.zeros(8), dict(mode="proportional", substeps=2, min_on=1))


def test_pwm_converges_to_the_proportional_plant():
    """Median over vehicles of max |x_pwm - x_prop| after one step: the finer clock S = 64 must land within half of S = 4's."""
    from ft_mpc_amd.actuators import step
    B = 96
    x0, ub, stuck, _ = qo.make_batch(B, 10, 8, 1, 11)
    u = np.random.default_rng(11).uniform(0, 1, (B, 8)) * ub
    prop = np.array([step(x0[b], u[b], ub[b], stuck[b], dict(mode="proportional"))["x"] for b in range(B)])
    for align in ("leading", "centred", "trailing"):
        med = {}
        for S in (4, 64):
            pwm = np.array([step(x0[b], u[b], ub[b], stuck[b], dict(mode="pwm", substeps=S, align=align))["x"] for b in range(B)])
            med[S] = float(np.median(np.abs(pwm - prop).max(axis=1)))
        print(f"{align}: S = 64 {med[64]:.2e}, S = 4 {med[4]:.2e}")
        assert med[64] < 0.5 * med[4], (align, med)
