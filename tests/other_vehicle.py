"""A controller model WITHOUT the structural zeros and repeated values of the default one (helper of test_other_vehicle_host.py and
test_gpu_other_vehicle.py; not a test module).

ftmpc_default_config's vehicle has a diagonal inertia, r and f_virt along y alone, a terminal weight P of three scalar 2 x 2
couplings repeated on the axes (60 of 81 entries zero) and always dt = 0.1, mass = 16.8.  The kernels take all of these as general
arrays; on the default a dropped or transposed off-diagonal term, a swapped r[0] / r[2] or a P[i][j] read as P[j][i] multiplies a
zero or meets its equal.  `vehicle` gives the keyword arguments of a handle and the equal oracle.qp_oracle.QPConfig with any subset
of the groups FIELDS replaced, so that a failure names its constant:

  dt 0.07, mass 13.1, J = V diag(0.17, 0.33, 0.26) V' (V: the Q factor of a random matrix; cond 1.94), r = (0.11, 0.19, -0.07),
  f_virt = (0.6, 2.9, -0.8), Q / R with nine / six distinct entries and rho 0.04 ("QR"), P = P0 + s .* (S + S') .* s' (P0 the
  default, s = sqrt(diag P0), S Gaussian with standard deviation P_SIGMA: dense, symmetric positive definite), D = the default
  matrix with a gain of +-10 % per thruster and the centre of mass moved by +-2 cm (as _plant of test_gpu_plant_dispersion.py).

The properties the tests rest on are asserted at every call."""
import numpy as np

from oracle import qp_oracle as qo
from oracle import refmath as rm

FIELDS = ("dt", "mass", "J", "r", "f_virt", "P", "QR", "D")
ALL = FIELDS
P_SIGMA = 0.08

DT, MASS, RHO = 0.07, 13.1, 0.04
J_DIAG = (0.17, 0.33, 0.26)
R_VEC = np.array([0.11, 0.19, -0.07])
F_VIRT = np.array([0.6, 2.9, -0.8])
Q_DIAG = np.array([1.3, 0.8, 1.1, 0.9, 1.2, 0.7, 2.2, 1.7, 1.9])
R_DIAG = np.array([0.12, 0.08, 0.1, 0.012, 0.009, 0.011])


def _no_small_entry(a, name):
    a = np.abs(np.asarray(a, float))
    assert a.min() >= 1e-3 * a.max(), (name, a.min(), a.max())


def constants(NT, seed=4242):
    """Every replaced constant of the vehicle: dict(dt, mass, rho, J, r, f_virt, Q, R, P, D).  The draws come in a fixed order from
    one generator, so a group's values do not depend on which groups are asked for."""
    rng = np.random.default_rng(seed)
    V = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    J = V @ np.diag(J_DIAG) @ V.T
    J = 0.5 * (J + J.T)
    P0 = rm.terminal_P_quadratic()
    s = np.sqrt(np.diag(P0))
    for _ in range(64):      # (diag P0 spans a factor 40: a draw may leave an entry between two small axes below 1e-3 of the largest)
        S = P_SIGMA * rng.standard_normal((9, 9))
        P = P0 + s[:, None] * (S + S.T) * s[None, :]
        P = 0.5 * (P + P.T)
        if np.abs(P).min() >= 1e-3 * np.abs(P).max() and np.linalg.eigvalsh(P).min() > 0 and np.linalg.cond(P) <= 200:
            break
    gain = {n: 1 + rng.uniform(-0.1, 0.1, n) for n in (8, 16)}      # (both drawn: the 8-thruster D does not move the shift's draw)
    d = rng.uniform(-0.02, 0.02, 3)
    D0 = rm.allocation_matrix_16() if NT == 16 else rm.allocation_matrix_8()
    D = np.empty((6, NT))
    for i in range(NT):
        f, t = D0[0:3, i] * gain[NT][i], D0[3:6, i] * gain[NT][i]
        D[0:3, i], D[3:6, i] = f, t - np.cross(d, f)
    assert np.linalg.cond(J) <= 3.4
    assert np.array_equal(P, P.T) and np.linalg.eigvalsh(P).min() > 0 and np.linalg.cond(P) <= 200, np.linalg.cond(P)
    for a, name in ((J, "J"), (P, "P"), (R_VEC, "r"), (F_VIRT, "f_virt")):
        _no_small_entry(a, name)
    assert not np.isin(P, P0).any()      # P[i][j] is distinct from every default value (and so from P[j'][i'] of the default)
    assert np.unique(np.triu(P)[np.triu_indices(9)]).size == 45      # ... and from every other entry of its own triangle
    return dict(dt=DT, mass=MASS, rho=RHO, J=J, r=R_VEC.copy(), f_virt=F_VIRT.copy(), Q=Q_DIAG.copy(), R=R_DIAG.copy(), P=P, D=D)


def vehicle(N, NT, fields=ALL, seed=4242):
    """(kw, qcfg): the keyword arguments of gpu_mpc_factory / BatchedMPC and the equal QPConfig, with the groups `fields` replaced.
    r is passed explicitly (the Python layer does not recompute it from the mass)."""
    fields = (fields,) if isinstance(fields, str) else tuple(fields)
    assert set(fields) <= set(FIELDS), fields
    c = constants(NT, seed)
    kw = dict(N=N, NT=NT)
    for f in fields:
        if f == "QR":
            kw.update(Q=c["Q"], R=c["R"], rho=c["rho"])
        else:
            kw[f] = c[f]
    return kw, qo.QPConfig(**kw)


def near_terminal_set(qcfg, B, nf, seed, At, bt, scale=2.0):
    """_near_terminal_set of test_gpu_wrench.py on this vehicle (qcfg.r in place of the default r): random poses / faults whose
    orbit-centre tracking error starts on `scale` times the boundary of the terminal set."""
    x0, ub, stuck, xref = qo.make_batch(B, qcfg.N, qcfg.NT, nf, seed)
    rng = np.random.default_rng(seed + 1)
    r = np.asarray(qcfg.r, float)
    for b in range(B):
        e = rng.standard_normal(9)
        e *= scale / max((At @ e / bt).max(), 1e-9)
        R = rm.rot(x0[b, 6:10])
        w = rm.OMEGA_DES + e[6:9]
        x0[b, 0:3] = e[0:3] - R.T @ r                    # robot_to_center (spiral_model.py:103-109) inverted
        x0[b, 3:6] = e[3:6] - R.T @ np.cross(w, r)
        x0[b, 10:13] = w
    return x0, ub, stuck, xref


def near_state_bounds(qcfg, B, nf, seed, lo=0.85, hi=0.95):
    """Random poses / faults whose orbit-centre velocity points at the reference position with its largest component drawn from
    [lo, hi]: the controller asks for more speed, so a bound |v| <= 0.9 (wrench_state_rows.bounds) is active for the ones below it
    and cannot be met within one step by the ones well above it."""
    x0, ub, stuck, xref = qo.make_batch(B, qcfg.N, qcfg.NT, nf, seed)
    rng = np.random.default_rng(seed + 1)
    r = np.asarray(qcfg.r, float)
    for b in range(B):
        c = rm.robot_to_center(x0[b], r)
        v = -c[0:3] / np.abs(c[0:3]).max() * rng.uniform(lo, hi)
        x0[b, 3:6] = v - rm.rot(x0[b, 6:10]).T @ np.cross(x0[b, 10:13], r)
    return x0, ub, stuck, xref


# ---- the batches of test_gpu_other_vehicle.py whose conditions test_other_vehicle_host.py fixes on the oracle ----
SEED = 555                                  # make_batch(B, N, NT, faults, SEED): the plain solve batches
SENSITIVITY_SHAPES = ((20, 8), (11, 16))    # where every constant must move u0 by 1e-2 f_max (8 instances, two faults)
TERM = dict(N=5, NT=16, nf=2, B=16, seed=9502, scale=2.0)      # near_terminal_set: 14 of 16 reachable, rows active on 6 (wrench) / 8 (box)
STATE = ((5, 8, 2, 16, 5205), (5, 16, 2, 16, 5209))            # near_state_bounds (N, NT, faults, B, seed): 15 / 16 solved, 7 .. 9 active


def plain_batch(N, NT, nf, B):
    return qo.make_batch(B, N, NT, nf, SEED)
