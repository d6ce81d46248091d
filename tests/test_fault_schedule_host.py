"""CPU: the host side of thruster faults that start mid-run (ft_mpc_amd/faults.py, include/ftmpc.h ftmpc_fault_schedule):
the reference-style actuator_failures -> schedule helper, the hull tables stacked over every pattern, and the NumPy
warm-start repairs that the fault-event kernel restates."""
import numpy as np
import pytest

from ft_mpc_amd import faults as fl
from ft_mpc_amd.controllers.tools.input_bounds import hull_tables
from ft_mpc_amd.models.sys_model import SystemModel, allocation_matrix_16
from ft_mpc_amd.util.broken_thruster import BrokenThruster

D16 = allocation_matrix_16()


def test_failures_helper_is_cumulative_and_converts_times_to_steps():
    cfg = [dict(act_id=3, intensity=0.5, start_time=1.0), dict(act_id=10, intensity=1.0, start_time=0),
           dict(act_id=11, intensity=0.25, start_time=2.04), dict(act_id=4, intensity=0.0, start_time=1.0)]
    ub, stuck, f = fl.schedule_from_failures(cfg, dt=0.1, NT=16)
    assert ub[10] == 0.0 and stuck[10] == 3.4 and (np.delete(ub, 10) == 3.4).all() and (np.delete(stuck, 10) == 0).all()
    assert f["onset"].tolist() == [10, 20]                          # 1.0 / 0.1 and round(2.04 / 0.1); same step: one event
    # the pattern after each event is what SystemModel.set_fault leaves after all failures up to it
    m = SystemModel(0.1)
    m.set_fault(BrokenThruster(10, 1.0))
    for e, fs in enumerate([[(3, 0.5), (4, 0.0)], [(11, 0.25)]]):
        for i, a in fs:
            m.set_fault(BrokenThruster(i, a))
        assert np.array_equal(f["ub"][e], m.u_ub_physical) and np.allclose(f["stuck"][e], m.faulty_force.reshape(-1))
    _, _, f0 = fl.schedule_from_failures([dict(act_id=1, intensity=1.0, start_time=0)], dt=0.1)
    assert f0["onset"].shape == (0,) and f0["ub"].shape == (0, 16)


def test_normalize_schedule_broadcasts_and_delays_detection():
    f = dict(onset=np.array([[3, -1], [2, 5]]), ub=np.full((2, 2, 16), 3.4), stuck=np.zeros((2, 2, 16)))
    on, de, ub, st = fl.normalize_schedule(f, 2, 16, detect_delay=np.array([1, 2]))
    assert on.dtype == np.int32 and de.tolist() == [[4, -1], [4, 7]] and ub.shape == (2, 2, 16)
    on, de, _, _ = fl.normalize_schedule(dict(onset=[4], ub=np.full((1, 16), 3.4), stuck=np.zeros((1, 16))), 3, 16)
    assert on.shape == (3, 1) and (de == 4).all()
    with pytest.raises(ValueError):
        fl.normalize_schedule(f, 2, 16, detect_delay=-1)


def _patterns(B, E, seed):
    rng = np.random.default_rng(seed)
    ub, stuck = np.full((B, 16), 3.4), np.zeros((B, 16))
    eu, es = np.full((B, E, 16), 3.4), np.zeros((B, E, 16))
    for b in range(B):
        dead = list(rng.choice(16, E + 1, replace=False))
        if b % 2:                                              # faulty, then worse
            ub[b, dead[0]], stuck[b, dead[0]] = 0.0, 3.4 * rng.uniform()
        for e in range(E):                                     # cumulative: event e adds one more broken thruster
            eu[b, e], es[b, e] = (eu[b, e - 1], es[b, e - 1]) if e else (ub[b], stuck[b])
            eu[b, e, dead[e + 1]], es[b, e, dead[e + 1]] = 0.0, 3.4 * rng.uniform()
    onset = np.tile(np.arange(E, dtype=np.int32) + 2, (B, 1))
    onset[0, 1:] = -1                                          # vehicle 0: one event only
    return ub, stuck, eu, es, onset


def test_stacked_hull_tables_give_each_pattern_its_own_rows():
    B, E = 6, 2
    ub, stuck, eu, es, onset = _patterns(B, E, 4)
    h = fl.fault_hull_tables(D16, ub, stuck, eu, es, onset)
    assert not h["degenerate"].any()
    assert h["ev_set"].shape == (B, E) and h["ev_b"].shape == (B, E, h["rows"])

    def same(A_rows, b_rows, alone):
        r = alone["rows"]
        assert np.allclose(A_rows[:r], alone["A"][alone["set"][0]]) and np.allclose(b_rows[:r], alone["b"][0])
        assert (A_rows[r:] == 0).all() and (b_rows[r:] == 1).all()          # padding: a zero normal, never active

    for b in range(B):
        same(h["A"][h["set"][b]], h["b"][b], hull_tables(D16, ub[b:b + 1], stuck[b:b + 1]))
        for e in range(E):
            u, s = (eu[b, e], es[b, e]) if onset[b, e] >= 0 else (ub[b], stuck[b])
            same(h["A"][h["ev_set"][b, e]], h["ev_b"][b, e], hull_tables(D16, u[None], s[None]))
    # a flat hull in any event pattern is flagged on its vehicle
    eu2 = eu.copy()
    eu2[3, 1, :11] = 0.0
    assert fl.fault_hull_tables(D16, ub, stuck, eu2, es, onset)["degenerate"].tolist() == [False, False, False, True, False, False]


def test_warm_repair_keeps_the_new_hull_with_its_margin_and_leaves_inside_points():
    rng = np.random.default_rng(7)
    ub, stuck = np.full(16, 3.4), np.zeros(16)
    ub[[10, 11]] = 0.0
    stuck[[10, 11]] = 3.4
    h = hull_tables(D16, ub[None], stuck[None])
    A, b = h["A"][h["set"][0]], h["b"][0]
    ctr = D16 @ (ub / 2 + stuck)
    s0 = b - A @ ctr
    # the healthy vehicle's hull is larger: its points fall outside the new hull, many of them
    G = np.array([D16 @ rng.uniform(0, 3.4, 16) for _ in range(40)])
    out = fl.pull_into_hull(G, D16, ub, stuck, A, b)
    assert ((b[:, None] - A @ G.T).T < 0).any(axis=1).sum() > 5
    slack = (b[:, None] - A @ out.T).T
    assert (slack >= 1e-8 * s0 * (1 - 1e-6)).all()
    # a stage already inside with the margin is not moved, bit for bit
    inside = ctr + 0.3 * (G - ctr)
    keep = ((b[:, None] - A @ inside.T).T >= 1e-8 * s0).all(axis=1)
    assert keep.any()
    assert np.array_equal(fl.pull_into_hull(inside, D16, ub, stuck, A, b)[keep], inside[keep])
    # the thruster form: clipped elementwise to [0, ub]
    U = rng.uniform(-1, 4, (3, 5, 16))
    C = fl.clip_warm(U, np.tile(ub, (3, 1)))
    assert (C >= 0).all() and (C <= ub).all() and np.array_equal(C[(U >= 0) & (U <= ub)], U[(U >= 0) & (U <= ub)])
