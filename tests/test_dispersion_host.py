"""CPU: the host side of the plant dispersion (include/ftmpc.h, ftmpc_plant_model; ft_mpc_amd/dispersion.py): the four entries are
exported, the ctypes struct has the layout gcc gives the header, scale_and_shift against loops written here, sample's shapes, bounds,
slice property and exact nominal values, and dispersion.plant_step against oracle.refmath for nominal parameters."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import refmath as rm

ROOT = Path(__file__).resolve().parents[1]
NEW = ("ftmpc_simulate_plant_batch", "ftmpc_simulate_wrench_plant_batch", "ftmpc_multi_simulate_plant_batch",
       "ftmpc_multi_simulate_wrench_plant_batch")


def test_library_exports_the_plant_entries():
    from ft_mpc_amd import _lib
    _lib.build_library()
    lib = _lib.load_library()
    for n in NEW:
        assert n in _lib.SYMBOLS and getattr(lib, n) is not None
    assert lib.ftmpc_version() >= 510
    # the last argument of each is the struct
    assert lib.ftmpc_simulate_plant_batch.argtypes[:-1] == lib.ftmpc_simulate_outcomes_batch.argtypes
    assert lib.ftmpc_simulate_wrench_plant_batch.argtypes[:-1] == lib.ftmpc_simulate_wrench_outcomes_batch.argtypes
    assert lib.ftmpc_multi_simulate_plant_batch.argtypes[:-1] == lib.ftmpc_multi_simulate_outcomes_batch.argtypes
    assert lib.ftmpc_multi_simulate_wrench_plant_batch.argtypes[:-1] == lib.ftmpc_multi_simulate_wrench_outcomes_batch.argtypes


def test_plant_model_struct_layout_matches_the_header(tmp_path):
    from ft_mpc_amd import _lib
    fields = [f for f, _ in _lib.ftmpc_plant_model._fields_]
    assert fields == ["struct_size", "reserved", "mass", "J", "D", "force", "torque"]
    src = tmp_path / "layout.c"
    body = "".join(f'printf("{f} %zu\\n", offsetof(ftmpc_plant_model, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftmpc.h"\nint main(void){printf("sizeof %zu\\n", sizeof(ftmpc_plant_model));'
                   + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.ftmpc_plant_model) == 48
    for f in fields:
        assert int(got[f]) == getattr(_lib.ftmpc_plant_model, f).offset, f


# ---------------------------------------------------------------------------------------------------------------------------
# scale_and_shift
# ---------------------------------------------------------------------------------------------------------------------------
def test_scale_and_shift_identity_and_column_scaling():
    from ft_mpc_amd.dispersion import scale_and_shift
    D = rm.allocation_matrix_16()
    B = 5
    same = scale_and_shift(D, np.ones((B, 16)), np.zeros((B, 3)))
    assert same.shape == (B, 6, 16) and np.array_equal(same, np.repeat(D[None], B, 0))
    assert np.array_equal(scale_and_shift(D), D[None])
    gain = np.random.default_rng(1).uniform(0.8, 1.2, (B, 16))
    got = scale_and_shift(D, gain=gain)
    for b in range(B):
        for i in range(16):
            assert np.array_equal(got[b, :, i], D[:, i] * gain[b, i])


def test_scale_and_shift_moves_the_torque_rows_to_the_displaced_centre_of_mass():
    from ft_mpc_amd.dispersion import scale_and_shift
    D = rm.allocation_matrix_16()
    rng = np.random.default_rng(2)
    B = 7
    gain = rng.uniform(0.9, 1.1, (B, 16))
    d = rng.uniform(-0.02, 0.02, (B, 3))
    got = scale_and_shift(D, gain, d)
    ref = np.empty((B, 6, 16))
    for b in range(B):
        for i in range(16):
            f = [D[r, i] * gain[b, i] for r in range(3)]
            t = [D[3 + r, i] * gain[b, i] for r in range(3)]
            dxf = [d[b, 1] * f[2] - d[b, 2] * f[1], d[b, 2] * f[0] - d[b, 0] * f[2], d[b, 0] * f[1] - d[b, 1] * f[0]]
            ref[b, 0:3, i] = f
            ref[b, 3:6, i] = [t[r] - dxf[r] for r in range(3)]
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-16)
    assert np.array_equal(got[:, 0:3], ref[:, 0:3])                # the force rows only scale
    assert np.abs(got[:, 3:6] - D[None, 3:6] * gain[:, None, :]).max() > 1e-3      # the shift did something
    # offset alone
    only = scale_and_shift(D, com_offset=d)
    assert np.array_equal(only[:, 0:3], np.repeat(D[None, 0:3], B, 0))
    np.testing.assert_allclose(only[:, 3:6], D[None, 3:6] - np.cross(d[:, :, None], D[None, 0:3], axis=1), rtol=0, atol=1e-16)


# ---------------------------------------------------------------------------------------------------------------------------
# sample
# ---------------------------------------------------------------------------------------------------------------------------
J0 = rm.INERTIA + 0.02 * np.array([[0, 1, -1], [1, 0, 0.5], [-1, 0.5, 0]])
WIDTHS = dict(mass_rel=0.1, inertia_rel=0.1, gain_rel=0.05, com_offset=0.01, force=0.05, torque=0.005)


@pytest.mark.parametrize("NT", [8, 16])
def test_sample_shapes_bounds_and_positive_definite_inertia(NT):
    from ft_mpc_amd.dispersion import sample, scale_and_shift
    D = rm.allocation_matrix_16() if NT == 16 else rm.allocation_matrix_8()
    B = 96
    p = sample(B, NT, D, J0, rm.MASS, seed=7, **WIDTHS)
    assert sorted(p) == ["D", "J", "force", "mass", "torque"]
    assert p["mass"].shape == (B,) and p["J"].shape == (B, 3, 3) and p["D"].shape == (B, 6, NT)
    assert p["force"].shape == (B, 3) and p["torque"].shape == (B, 3)
    assert all(a.dtype == np.float64 for a in p.values())
    assert np.abs(p["mass"] / rm.MASS - 1).max() <= 0.1 and np.abs(p["mass"] / rm.MASS - 1).max() > 0.05
    assert np.abs(p["force"]).max() <= 0.05 and np.abs(p["force"]).max() > 0.025
    assert np.abs(p["torque"]).max() <= 0.005 and np.abs(p["torque"]).max() > 0.0025
    assert np.array_equal(p["J"], np.swapaxes(p["J"], 1, 2))
    assert np.linalg.eigvalsh(p["J"]).min() > 0
    # J_b = S J S with |S_kk - 1| <= 0.1: the diagonal scales by S_kk^2
    s = np.sqrt(np.diagonal(p["J"], axis1=1, axis2=2) / np.diag(J0))
    assert np.abs(s - 1).max() <= 0.1 + 1e-15 and np.abs(s - 1).max() > 0.05
    np.testing.assert_allclose(p["J"], s[:, :, None] * J0[None] * s[:, None, :], rtol=1e-14)
    # the force rows of D_b carry the gain alone, within 5 %; the torque rows are those of scale_and_shift for an offset within 1 cm
    big = np.abs(D[0:3]).argmax(axis=0)
    gain = p["D"][:, big, np.arange(NT)] / D[big, np.arange(NT)]
    assert np.abs(gain - 1).max() <= 0.05 + 1e-15 and np.abs(gain - 1).max() > 0.025
    np.testing.assert_allclose(p["D"][:, 0:3], D[None, 0:3] * gain[:, None, :], rtol=1e-15, atol=1e-17)
    # d_b from the torque rows: t_i' - g_i t_i = -d x (g_i f_i) = skew(g_i f_i) d, linear in d
    for b in range(0, B, 13):
        M = np.concatenate([rm.skew(p["D"][b, 0:3, i]) for i in range(NT)])
        rhs = np.concatenate([p["D"][b, 3:6, i] - D[3:6, i] * gain[b, i] for i in range(NT)])
        d, res = np.linalg.lstsq(M, rhs, rcond=None)[:2]
        assert res.size == 0 or res[0] <= 1e-24
        assert np.abs(d).max() <= 0.01 + 1e-12
        np.testing.assert_allclose(scale_and_shift(D, gain[b:b + 1], d[None])[0], p["D"][b], rtol=0, atol=1e-12)
    # the vehicles differ from each other
    assert len(np.unique(p["mass"])) == B


def test_a_slice_of_a_campaign_draws_what_the_whole_draws():
    from ft_mpc_amd.dispersion import sample
    D = rm.allocation_matrix_8()
    whole = sample(96, 8, D, J0, rm.MASS, seed=11, **WIDTHS)
    part = sample(56, 8, D, J0, rm.MASS, seed=11, index0=40, **WIDTHS)
    for k in whole:
        assert np.array_equal(whole[k][40:96], part[k]), k
    other = sample(56, 8, D, J0, rm.MASS, seed=12, index0=40, **WIDTHS)
    assert not np.array_equal(other["mass"], part["mass"])
    local = sample(56, 8, D, J0, rm.MASS, seed=11, **WIDTHS)          # its own index: other draws
    assert not np.array_equal(local["mass"], part["mass"])


@pytest.mark.parametrize("zero", ["mass_rel", "inertia_rel", "gain_com", "force", "torque"])
def test_a_zero_half_width_returns_the_nominal_value_exactly(zero):
    from ft_mpc_amd.dispersion import sample
    D = rm.allocation_matrix_16()
    w = dict(WIDTHS)
    for k in (("gain_rel", "com_offset") if zero == "gain_com" else (zero,)):
        w[k] = 0.0
    B = 9
    p = sample(B, 16, D, J0, rm.MASS, seed=3, **w)
    nominal = dict(mass_rel=("mass", np.full(B, rm.MASS)), inertia_rel=("J", np.repeat(J0[None], B, 0)),
                   gain_com=("D", np.repeat(D[None], B, 0)), force=("force", np.zeros((B, 3))), torque=("torque", np.zeros((B, 3))))
    key, val = nominal[zero]
    assert np.array_equal(p[key], val)
    for k, (key2, val2) in nominal.items():
        if k != zero:
            assert not np.array_equal(p[key2], val2), key2
    none = sample(B, 16, D, J0, rm.MASS, seed=3)
    for key2, val2 in nominal.values():
        assert np.array_equal(none[key2], val2), key2


# ---------------------------------------------------------------------------------------------------------------------------
# plant_step
# ---------------------------------------------------------------------------------------------------------------------------
def test_plant_step_with_nominal_parameters_is_the_oracles_rk4():
    from ft_mpc_amd import MPCConfig
    from ft_mpc_amd.dispersion import plant_step
    rng = np.random.default_rng(4)
    for NT, D in ((8, rm.allocation_matrix_8()), (16, rm.allocation_matrix_16())):
        cfg = MPCConfig(N=5, NT=NT)
        fs = rm.FaultState(NT).set_fault(2, 0.4).set_fault(5, 0.0)
        for _ in range(5):
            x = rng.standard_normal(13)
            x[6:10] /= np.linalg.norm(x[6:10])
            u = rng.uniform(0, rm.F_MAX, NT)
            ref = rm.rk4(lambda y: rm.plant_dx_dt(y, u, D, fs.stuck, fs.ub), x)
            assert np.abs(plant_step(x, u, fs.ub, fs.stuck, {}, cfg) - ref).max() <= 1e-15
            full = dict(mass=rm.MASS, J=rm.INERTIA, D=D, force=np.zeros(3), torque=np.zeros(3))
            assert np.abs(plant_step(x, u, fs.ub, fs.stuck, full, cfg) - ref).max() <= 1e-15


def test_plant_step_with_dispersed_parameters_follows_the_definition():
    """The definition written out once more with oracle.refmath pieces: plant_dx_dt for m_b, J_b, D_b plus f_b / m_b on the velocity
    rows and J_b^-1 t_b on the rate rows."""
    from ft_mpc_amd import MPCConfig
    from ft_mpc_amd.dispersion import plant_step, sample
    D = rm.allocation_matrix_8()
    cfg = MPCConfig(N=5, NT=8)
    p = sample(4, 8, D, J0, rm.MASS, seed=5, mass_rel=0.2, inertia_rel=0.2, gain_rel=0.1, com_offset=0.02, force=0.05, torque=0.005)
    rng = np.random.default_rng(6)
    fs = rm.FaultState(8).set_fault(1, 0.5)
    for b in range(4):
        x = rng.standard_normal(13)
        x[6:10] /= np.linalg.norm(x[6:10])
        u = rng.uniform(0, rm.F_MAX, 8)

        def f(y):
            dx = rm.plant_dx_dt(y, u, p["D"][b], fs.stuck, fs.ub, p["mass"][b], p["J"][b])
            dx[3:6] += p["force"][b] / p["mass"][b]
            dx[10:13] += np.linalg.solve(p["J"][b], p["torque"][b])
            return dx
        ref = rm.rk4(f, x)
        got = plant_step(x, u, fs.ub, fs.stuck, {k: v[b] for k, v in p.items()}, cfg)
        assert np.abs(got - ref).max() <= 1e-14
        assert np.abs(got - plant_step(x, u, fs.ub, fs.stuck, {}, cfg)).max() > 1e-5
