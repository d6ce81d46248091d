"""CPU: what tests/test_gpu_other_vehicle.py rests on -- the oracle is right on the vehicle of tests/other_vehicle.py, that vehicle's
batches excite every constant, and the batches with terminal-set / state-bound rows meet their conditions on the oracle.

(a) The assertions of test_oracle_qp.py restated with the other vehicle's QPConfig.
(b) One constant put back to its default (J -> diag, J[0][1], r[0], r[2], f_virt[0], f_virt[2], P -> P0, P[0][7], dt, mass) must move
    u0 of the plain solve batches by at least 1e-2 f_max somewhere in the batch: 100 times the loosest GPU tolerance (1e-4 f_max) that is
    to catch a kernel which relies on that default.  Measured: 2.9e-2 (P[0][7] at (20, 8)) .. 0.88 (dt at (20, 8)).  A single entry of R
    moves u0 by less than 1e-4, so R is held where it enters: the word R ut of the float64 records (tolerance 1e-9 of scale) and H, g
    of the float64 build (1e-11 of scale); the changed words must differ by 100 times those.  (R[2] = 0.1 is the default's value; the
    fp32 build's 2e-5 sees the force entries of R by 1.4e-3 .. 1.6e-3 of |H| only, the torque entries by 2e-6 .. 7e-6: not held there.)
(c) The near-terminal-set and near-state-bound batches: the oracle solves at least half of each, at least a quarter has an active
    special row.  Conditions, fixed here by the choice of scale and seed in other_vehicle.TERM / STATE."""
import dataclasses
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))

from ft_mpc_amd.controllers.tools.terminal_ingredients import load_terminal
from oracle import c_oracle as co
from oracle import qp_oracle as qo
from oracle import refmath as rm
import other_vehicle as ov
import wrench_state_rows as ws

F_MAX = rm.F_MAX


# ---- (a) the oracle on this vehicle ----
def test_vehicle_has_no_structural_zero_and_the_selected_groups_only():
    for NT in (8, 16):
        c = ov.constants(NT)
        D0 = rm.allocation_matrix_16() if NT == 16 else rm.allocation_matrix_8()
        assert c["D"].shape == D0.shape and np.abs(c["D"] - D0).max() > 1e-3
        assert np.abs(c["J"] - np.diag(np.diag(c["J"]))).max() > 1e-2
    kw, q = ov.vehicle(5, 8, fields=("J", "QR"))
    assert sorted(kw) == ["J", "N", "NT", "Q", "R", "rho"]
    d = qo.QPConfig(N=5, NT=8)
    assert q.dt == d.dt and q.mass == d.mass and np.array_equal(q.P, d.P) and np.array_equal(q.r, d.r) and np.array_equal(q.D, d.D)
    assert not np.array_equal(q.J, d.J) and q.rho == ov.RHO


def test_linearisation_against_central_differences():
    """A_k, Bg_k of qo.linearize against central differences (step 1e-6) of the RK4 step they linearise: rounding eps |c| / h = 7e-10 for
    |c| <= 3, truncation h^2 |f'''| ~ 1e-12; bound 1e-8 of max(1, |block|) (measured 6e-11)."""
    N, NT = 6, 16
    _, q = ov.vehicle(N, NT)
    x0, ub, stuck, _ = ov.plain_batch(N, NT, 2, 2)
    W = np.random.default_rng(1).uniform(0.0, 1.0, (N, NT)) * F_MAX
    h, worst = 1e-6, 0.0
    for b in range(2):
        cbar, A, Bg, Ubar = qo.linearize(q, x0[b], ub[b], stuck[b], W)
        for k in range(N):
            gen = q.D @ (Ubar[k] + stuck[b])
            step = lambda c, g: rm.rk4(lambda s: rm.centre_dx_dt(s, g, q.r, q.mass, q.J), c, q.dt)
            assert np.abs(step(cbar[k], gen) - cbar[k + 1]).max() <= 1e-13
            for i in range(13):
                d = np.zeros(13)
                d[i] = h
                col = (step(cbar[k] + d, gen) - step(cbar[k] - d, gen)) / (2 * h)
                worst = max(worst, np.abs(col - A[k][:, i]).max() / max(1.0, np.abs(A[k]).max()))
            for i in range(6):
                d = np.zeros(6)
                d[i] = h
                col = (step(cbar[k], gen + d) - step(cbar[k], gen - d)) / (2 * h)
                worst = max(worst, np.abs(col - Bg[k][:, i]).max() / max(1.0, np.abs(Bg[k]).max()))
    print(f"other vehicle: linearisation against central differences within {worst:.2e}")
    assert worst <= 1e-8, worst


@pytest.mark.parametrize("N,NT", ov.SENSITIVITY_SHAPES)
def test_numpy_and_c_build_agree_and_the_port_is_exact(N, NT):
    _, q = ov.vehicle(N, NT)
    x0, ub, stuck, xref = ov.plain_batch(N, NT, 2, 4)
    pol = co.solve_batch(q, x0, ub, stuck, xref, nthreads=4, max_iters=60)
    assert (pol["status"] == 0).all()
    for b in range(4):
        qp = qo.build_qp(q, x0[b], ub[b], stuck[b], xref)
        H, g, lo, hi = co.build_qp(q, x0[b], ub[b], stuck[b], xref)
        assert np.abs(H - qp["H"]).max() < 1e-10 * np.abs(H).max()
        assert np.abs(g - qp["g"]).max() < 1e-10 * max(1, np.abs(g).max())
        assert np.allclose(H, H.T) and np.linalg.eigvalsh(H).min() >= 2 * q.rho * (1 - 1e-9)
        assert np.array_equal(lo, -qp["Ubar"]) and np.array_equal(hi, qp["ub"] - qp["Ubar"])
        _, U, _ = qo.solve_instance(q, x0[b], ub[b], stuck[b], xref, exact=True)
        assert np.abs(pol["U"][b] - U).max() < 1e-9, (b, np.abs(pol["U"][b] - U).max())


def test_wrench_form_passes_the_kkt_certificate():
    N, NT = 11, 16
    _, q = ov.vehicle(N, NT)
    x0, ub, stuck, xref = ov.plain_batch(N, NT, 2, 4)
    for b in range(4):
        tau0, T, st, _, qp = qo.solve_wrench_instance(q, x0[b], ub[b], stuck[b], xref, mu_polish=1e-7)
        assert st == 0 and max(qo.kkt_general(qp["H"], qp["g"], qp["C"], qp["h"], qp["d"], qp["z"])) < 1e-8


# ---- (b) the inputs excite every term ----
def _put_back(q):
    """name -> the QPConfig with that one constant put back to the default's value"""
    P0 = rm.terminal_P_quadratic()
    rep = lambda **k: dataclasses.replace(q, **k)

    def entry(a, idx, sym=False):
        a = np.array(a, float)
        a[idx] = 0.0
        if sym:
            a[idx[::-1]] = 0.0
        return a
    return {"J -> diag": rep(J=np.diag(np.diag(q.J))), "J[0][1] = 0": rep(J=entry(q.J, (0, 1), True)),
            "r[0] = 0": rep(r=entry(q.r, (0,))), "r[2] = 0": rep(r=entry(q.r, (2,))),
            "f_virt[0] = 0": rep(f_virt=entry(q.f_virt, (0,))), "f_virt[2] = 0": rep(f_virt=entry(q.f_virt, (2,))),
            "P -> P0": rep(P=P0), "P[0][7] = 0": rep(P=entry(q.P, (0, 7), True)), "dt = 0.1": rep(dt=rm.DT), "mass = 16.8": rep(mass=rm.MASS)}


@pytest.mark.parametrize("N,NT", ov.SENSITIVITY_SHAPES)
def test_every_constant_moves_u0(N, NT):
    _, q = ov.vehicle(N, NT)
    x0, ub, stuck, xref = ov.plain_batch(N, NT, 2, 8)
    ref = co.solve_batch(q, x0, ub, stuck, xref, nthreads=4, max_iters=60, mu_stop=1e-13)
    assert (ref["status"] == 0).all()
    for name, q1 in _put_back(q).items():
        out = co.solve_batch(q1, x0, ub, stuck, xref, nthreads=4, max_iters=60, mu_stop=1e-13)
        assert (out["status"] == 0).all()
        moved = np.abs(out["u0"] - ref["u0"]).max() / F_MAX
        print(f"other vehicle (N, NT) = ({N}, {NT}): {name:14s} moves u0 by {moved:.2e} f_max")
        assert moved >= 1e-2, (name, moved)


def test_every_entry_of_R_moves_its_record_word_and_the_build():
    N, NT = 20, 8
    _, q = ov.vehicle(N, NT)
    x0, ub, stuck, xref = ov.plain_batch(N, NT, 2, 8)
    fv = np.concatenate([q.f_virt, np.zeros(3)])
    changed = [i for i in range(6) if ov.R_DIAG[i] != rm.R_DIAG[i]]
    assert changed == [0, 1, 3, 4, 5]
    for i in changed:
        R1 = q.R.copy()
        R1[i] = rm.R_DIAG[i]
        q1 = dataclasses.replace(q, R=R1)
        word = hh = gg = np.inf
        for b in range(8):
            ut = q.D @ stuck[b] - fv                           # the cold record: Ubar = 0, no uref
            word = min(word, abs((q.R - R1)[i] * ut[i]) / max(1.0, np.abs(q.R * ut).max()))
            a, c = qo.build_qp(q, x0[b], ub[b], stuck[b], xref), qo.build_qp(q1, x0[b], ub[b], stuck[b], xref)
            hh = min(hh, np.abs(a["H"] - c["H"]).max() / np.abs(a["H"]).max())
            gg = min(gg, np.abs(a["g"] - c["g"]).max() / max(1.0, np.abs(a["g"]).max()))
        print(f"other vehicle: R[{i}] put back moves its record word by {word:.2e}, H by {hh:.2e}, g by {gg:.2e} of scale (least of 8)")
        assert word > 100 * 1e-9 and hh > 100 * 1e-11 and gg > 100 * 1e-11, (i, word, hh, gg)


# ---- (c) reachability conditions of the batches with special rows ----
def _conditions(name, B, solved, active):
    print(f"other vehicle: {name}: the oracle solves {solved} of {B}, special rows active on {active}")
    assert 2 * solved >= B and 4 * active >= B, (name, B, solved, active)


@pytest.mark.parametrize("form", ["wrench", "box"])
def test_terminal_set_batch_meets_its_conditions(form):
    t = ov.TERM
    term = load_terminal().term_set
    At, bt = term.A, term.b.reshape(-1)
    _, q = ov.vehicle(t["N"], t["NT"])
    x0, ub, stuck, xref = ov.near_terminal_set(q, t["B"], t["nf"], t["seed"], At, bt, t["scale"])
    solved = active = 0
    with np.errstate(all="ignore"):
        for b in range(t["B"]):
            if form == "wrench":      # (raises on a flat hull: there is none in this batch)
                _, _, st, _, qp = qo.solve_wrench_instance(q, x0[b], ub[b], stuck[b], xref, term_set=(At, bt), iters=60, mu_polish=1e-7)
            else:
                _, _, st, _, qp = qo.solve_box_terminal_instance(q, x0[b], ub[b], stuck[b], xref, (At, bt), iters=60)
            solved += int(st == 0)
            active += int(st == 0 and (qp["z"][qp["nhull"]:] > 1e-6).any())
    _conditions(f"terminal set, {form} form", t["B"], solved, active)


@pytest.mark.parametrize("shape", ov.STATE)
@pytest.mark.parametrize("form", ["wrench", "box"])
def test_state_bound_batches_meet_their_conditions(form, shape):
    N, NT, nf, B, seed = shape
    xlb, xub = ws.bounds()
    _, q = ov.vehicle(N, NT)
    x0, ub, stuck, xref = ov.near_state_bounds(q, B, nf, seed)
    solved = active = 0
    with np.errstate(all="ignore"):
        for b in range(B):
            if form == "wrench":
                _, _, st, _, qp = ws.solve_wrench_state_instance(q, x0[b], ub[b], stuck[b], xref, xlb, xub)
            else:
                _, _, st, _, qp = qo.solve_box_state_instance(q, x0[b], ub[b], stuck[b], xref, xlb, xub, iters=60)
            solved += int(st == 0)
            active += int(st == 0 and ws.active_state_rows(qp) > 0)
    _conditions(f"state bounds, {form} form, (N, NT) = ({N}, {NT})", B, solved, active)
