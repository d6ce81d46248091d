"""Plant dispersion of a fault campaign on the host: the per-vehicle plant models that BatchedMPC.simulate(plant=...) integrates
(include/ftmpc.h, ftmpc_plant_model; csrc/ftmpc_sim.hip, ftmpc_plant_step_var_kernel) while the controller keeps the nominal model.

Vehicle b has a plant mass m_b, inertia J_b, allocation matrix D_b, a constant disturbance force f_b (inertial frame) and a constant
disturbance torque t_b (body frame); with a_i = (ub_i > 0 ? u_i : 0) + stuck_i
    [F; tau] = D_b a,   p' = v,   v' = (Rot(q)^T F + f_b) / m_b,   q' = 1/2 Omega(w) q,   w' = J_b^-1 (tau + t_b - w x J_b w)
integrated by RK4 over dt with a, f_b and t_b held constant.

scale_and_shift builds D_b from thruster gain errors and a displaced centre of mass, sample draws a whole campaign's plant models
from a counter-based generator (a slice of a campaign draws what the whole campaign draws for the same vehicles), plant_step is the
NumPy restatement of one plant step.

Not covered: a MISALIGNED thruster.  Its force direction changes and with it the lever arm's torque, which needs the thruster
positions; the allocation matrix D does not determine them.  Callers who have the geometry build D_b themselves and pass it as
plant["D"]."""
from __future__ import annotations

import numpy as np

_M = (1 << 64) - 1
# draw of vehicle v, component c: counter v * STRIDE + c (the same for every B and NT, so a slice draws the whole campaign's values)
STRIDE = 32
C_MASS, C_INERTIA, C_COM, C_FORCE, C_TORQUE, C_GAIN = 0, 1, 4, 7, 10, 16       # 1, 3, 3, 3, 3, NT <= 16 components
# component 13 is reserved for missions.phase_offsets (a vehicle's start column); 14 and 15 are free.  Nothing else may draw from a
# component that is taken: two quantities drawn from one counter with one seed are the same number.
C_PHASE = 13


def u01(seed, idx):
    """Uniform in [0, 1) from splitmix64 of (seed, idx): the construction of the library's measurement noise (csrc/ftmpc_sim.hip)."""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & _M) + np.uint64(0x9E3779B97F4A7C15) * (idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _pm1(seed, vehicles, comp, n):
    """[len(vehicles), n] uniform in [-1, 1): components comp .. comp + n - 1 of every vehicle."""
    idx = vehicles[:, None] * np.uint64(STRIDE) + (np.uint64(comp) + np.arange(n, dtype=np.uint64))[None, :]
    return 2.0 * u01(seed, idx) - 1.0


def scale_and_shift(D, gain=None, com_offset=None):
    """D_b [B,6,NT] from the nominal D [6,NT] (or [B,6,NT]): column i scaled by gain[b, i] (a thruster that delivers gain times what
    is commanded of it), then the torque rows moved to a centre of mass displaced by d_b = com_offset[b] (body frame):
    t_i' = t_i - d_b x f_i, with f_i / t_i the force / torque rows of column i.  gain [B,NT] or None (1), com_offset [B,3] or None (0);
    B comes from whichever is given (1 when neither is)."""
    D = np.asarray(D, dtype=np.float64)
    B = next((np.shape(a)[0] for a in (gain, com_offset) if a is not None), D.shape[0] if D.ndim == 3 else 1)
    out = np.broadcast_to(D, (B,) + D.shape[-2:]).copy()
    if gain is not None:
        out *= np.asarray(gain, dtype=np.float64).reshape(B, 1, -1)
    if com_offset is not None:
        d = np.asarray(com_offset, dtype=np.float64).reshape(B, 3, 1)
        out[:, 3:6, :] -= np.cross(d, out[:, 0:3, :], axis=1)
    return out


def sample(B, NT, D, J, mass, seed, index0=0, mass_rel=0.0, inertia_rel=0.0, gain_rel=0.0, com_offset=0.0, force=0.0, torque=0.0):
    """A `plant` dict for BatchedMPC.simulate with uniform dispersions of the given half-widths about the nominal D [6,NT], J [3,3] and
    mass, for the vehicles [index0, index0 + B) of a campaign:
      mass   m_b = mass (1 + mass_rel u)
      J      J_b = S J S, S = diag(1 + inertia_rel u_k): symmetric positive definite whenever J is and inertia_rel < 1
      D      scale_and_shift(D, 1 + gain_rel u_i, com_offset u_k)           (com_offset in metres)
      force  f_b = force u_k (N, inertial frame),   torque  t_b = torque u_k (N m, body frame)
    with every u uniform in [-1, 1), keyed by (seed, index0 + b, component) alone: sample(B=96)[40:96] is sample(B=56, index0=40) bit
    for bit.  A half-width of zero gives that field's nominal value exactly."""
    if NT > 16:
        raise ValueError("NT must be at most 16")
    D = np.asarray(D, dtype=np.float64).reshape(6, NT)
    J = np.asarray(J, dtype=np.float64).reshape(3, 3)
    v = np.uint64(int(index0)) + np.arange(B, dtype=np.uint64)
    S = 1.0 + float(inertia_rel) * _pm1(seed, v, C_INERTIA, 3)
    return dict(
        mass=float(mass) * (1.0 + float(mass_rel) * _pm1(seed, v, C_MASS, 1)[:, 0]),
        J=J[None] * (S[:, :, None] * S[:, None, :]),      # (S_i S_j) J_ij: symmetric to the bit when J is
        D=scale_and_shift(D, 1.0 + float(gain_rel) * _pm1(seed, v, C_GAIN, NT), float(com_offset) * _pm1(seed, v, C_COM, 3)),
        force=float(force) * _pm1(seed, v, C_FORCE, 3),
        torque=float(torque) * _pm1(seed, v, C_TORQUE, 3),
    )


def _rot(q):
    x, y, z, w = q
    return np.array([[x * x - y * y - z * z + w * w, 2 * (x * y + z * w), 2 * (x * z - y * w)],
                     [2 * (x * y - z * w), -x * x + y * y - z * z + w * w, 2 * (y * z + x * w)],
                     [2 * (x * z + y * w), 2 * (y * z - x * w), -x * x - y * y + z * z + w * w]])


def _omega(w):
    wx, wy, wz = w
    return np.array([[0.0, wz, -wy, wx], [-wz, 0.0, wx, wy], [wy, -wx, 0.0, wz], [-wx, -wy, -wz, 0.0]])


def plant_step(x, u, ub, stuck, plant_b, cfg):
    """One plant step of ONE vehicle on the host: x [13] -> RK4 over cfg.dt of the dispersed dynamics above under the command u [NT]
    with the plant's pattern ub / stuck; no noise, no renormalisation (the loop adds both afterwards).  plant_b: dict with any of
    mass, J [3,3], D [6,NT], force [3], torque [3] of that vehicle (a row of the `plant` dict); what is missing is cfg's (an MPCConfig
    or BatchedMPC.cfg; cfg.D None: the 8 / 16 thruster matrix of cfg.NT)."""
    D = plant_b.get("D")
    if D is None:
        D = cfg.D
    if D is None:
        from .models.sys_model import allocation_matrix_16, allocation_matrix_8
        D = allocation_matrix_16() if cfg.NT == 16 else allocation_matrix_8()
    D = np.asarray(D, dtype=np.float64).reshape(6, -1)
    m = float(plant_b["mass"]) if plant_b.get("mass") is not None else float(cfg.mass)
    J = np.asarray(plant_b["J"] if plant_b.get("J") is not None else cfg.J, dtype=np.float64).reshape(3, 3)
    f = np.asarray(plant_b["force"], dtype=np.float64).reshape(3) if plant_b.get("force") is not None else np.zeros(3)
    t = np.asarray(plant_b["torque"], dtype=np.float64).reshape(3) if plant_b.get("torque") is not None else np.zeros(3)
    a = np.where(np.asarray(ub) > 0, np.asarray(u, dtype=np.float64).reshape(-1), 0.0) + np.asarray(stuck, dtype=np.float64).reshape(-1)
    gen = D @ a
    F, tau = gen[0:3], gen[3:6]

    def rhs(x):
        v, q, w = x[3:6], x[6:10], x[10:13]
        return np.concatenate([v, (_rot(q).T @ F + f) / m, 0.5 * _omega(w) @ q, np.linalg.solve(J, tau + t - np.cross(w, J @ w))])
    x = np.asarray(x, dtype=np.float64).reshape(13)
    dt = float(cfg.dt)
    k1 = rhs(x)
    k2 = rhs(x + dt / 2 * k1)
    k3 = rhs(x + dt / 2 * k2)
    k4 = rhs(x + dt * k3)
    return x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
