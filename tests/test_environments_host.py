"""CPU: the time-varying disturbance on the host (ft_mpc_amd.environments) and its way through BatchedMPC.simulate to the C entries.

1. Statistics of the restatement: over 4096 vehicles at one step the stationary draw and its successor have the standard deviation
   sigma within 5 % and the lag-one correlation phi within 0.05, per component.  The sampling error at that count is 1 / sqrt(2 n) =
   1.1 % and (1 - phi^2) / sqrt(n) <= 0.016, so both margins are beyond four standard errors; measured with the seed below: 1.7 % and
   0.030 at the worst of the six components.
2. A stationary start continued from `state` is the whole run exactly; slices draw what the whole campaign draws.
3. `request` refuses what the library refuses, naming the field.
4. Dispatch with a recording stand-in, as tests/test_simulate_dispatch_host.py: environment= reaches the three new entries with the
   struct in the last position, and the wrench form on the driver raises before any call."""
import ctypes as C
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from ft_mpc_amd import _lib
from ft_mpc_amd import environments as EV
from ft_mpc_amd.batch import BatchedMPC, MPCConfig, _simulate

ROOT = Path(__file__).resolve().parents[1]
N, NT, B, T = 4, 8, 3, 2
F_MAX = 3.4
EST = dict(every=1, p0=(0.05, 0.05, 0.02, 0.02), proc_sigma=(1e-4, 1e-3, 1e-4, 1e-3), meas_sigma=(1e-3, 1e-3, 1e-3, 1e-3))
DIST = dict(p0=(1, 1), proc_sigma=(0, 0))


# ---- 1. statistics

def test_stationary_spread_and_lag_one_correlation():
    n, dt, sigma, tau, seed, c = 4096, 0.1, (0.4, 0.03), (0.5, 0.2), 20261021, 17
    phi, innov = EV.process(sigma, tau, dt)
    assert np.allclose(phi, np.exp(-dt / np.asarray(tau))) and np.allclose(innov ** 2 + (phi * sigma) ** 2, np.asarray(sigma) ** 2)
    w, g1 = EV.wrench(c, None, dt, sigma, tau, seed, index0=100, index_total=n + 200, B=n)
    g0 = EV.stationary(n, sigma, seed, c, 100, n + 200)
    assert np.array_equal(w, g0)                  # no base, no periodic term, no kick: the wrench is the process
    worst_s = worst_r = 0.0
    for j in range(6):
        a = j // 3
        for g in (g0, g1):
            dev = abs(np.std(g[:, j], ddof=1) / sigma[a] - 1.0)
            worst_s = max(worst_s, dev)
            assert dev < 0.05, (j, dev)
            assert abs(np.mean(g[:, j])) < 4.5 * sigma[a] / np.sqrt(n)
        r = np.corrcoef(g0[:, j], g1[:, j])[0, 1]
        worst_r = max(worst_r, abs(r - phi[a]))
        assert abs(r - phi[a]) < 0.05, (j, r, phi[a])
    print(f"worst std deviation {worst_s:.4f}, worst correlation deviation {worst_r:.4f}")
    # components are independent of each other
    cc = np.corrcoef(g0.T)
    assert np.abs(cc - np.eye(6)).max() < 4.5 / np.sqrt(n)


def test_sigma_zero_switches_a_process_off():
    w, g = EV.wrench(3, None, 0.1, (0.0, 0.02), (np.nan, 0.5), 7, base=np.ones((5, 6)))
    assert np.array_equal(w[:, 0:3], np.ones((5, 3))) and np.array_equal(g[:, 0:3], np.zeros((5, 3)))
    assert np.std(w[:, 3:6]) > 0


# ---- 2. continuation and slices

def _env(Bv, rng, **kw):
    return dict(seed=99, sigma=(0.4, 0.03), tau=(1.5, 0.7), period=2.3, amp_force=0.3 * rng.normal(size=(Bv, 3)),
                amp_torque=0.02 * rng.normal(size=(Bv, 3)), phase=rng.uniform(0, 6, size=Bv), kick=rng.normal(size=(Bv, 6)),
                window=np.stack([rng.integers(0, 8, size=Bv), rng.integers(4, 16, size=Bv)], axis=1), **kw)


def test_continued_replay_is_the_whole_replay():
    Bv, dt = 9, 0.1
    env = _env(Bv, np.random.default_rng(1))
    plant = dict(force=np.full((Bv, 3), 0.2))
    whole = EV.replay(Bv, 12, dt, env, plant)
    first = EV.replay(Bv, 5, dt, env, plant)
    second = EV.replay(Bv, 7, dt, dict(env, step0=5, state=first["state"]), plant)
    assert np.array_equal(np.concatenate([first["wrench"], second["wrench"]]), whole["wrench"])
    assert np.array_equal(second["state"], whole["state"])


def test_a_slice_draws_what_the_whole_campaign_draws():
    Bv, dt = 9, 0.1
    env = _env(Bv, np.random.default_rng(2))
    whole = EV.replay(Bv, 6, dt, env)
    per_vehicle = ("amp_force", "amp_torque", "phase", "kick", "window")
    part = EV.replay(5, 6, dt, dict(env, **{k: env[k][4:] for k in per_vehicle}), index0=4, index_total=Bv)
    assert np.array_equal(part["wrench"], whole["wrench"][:, 4:]) and np.array_equal(part["state"], whole["state"][4:])


def test_kick_acts_exactly_inside_its_window():
    Bv, dt = 4, 0.1
    kick = np.arange(1.0, 25.0).reshape(Bv, 6)
    window = np.array([[3, 6], [6, 3], [10, 40], [0, 2]])
    env = dict(step0=2, kick=kick, window=window)
    w = EV.replay(Bv, 7, dt, env)["wrench"]
    for t in range(7):
        c = 2 + t
        for b in range(Bv):
            inside = window[b, 0] <= c < window[b, 1]
            assert np.array_equal(w[t, b], kick[b] if inside else np.zeros(6)), (t, b)


def test_sample_is_keyed_by_the_vehicle_number():
    a = EV.sample(96, 11, amp_force=0.3, amp_torque=0.02, kick_force=2.0, kick_torque=0.1, kick_from=(2, 9), kick_length=(0, 4))
    b = EV.sample(56, 11, index0=40, amp_force=0.3, amp_torque=0.02, kick_force=2.0, kick_torque=0.1, kick_from=(2, 9), kick_length=(0, 4))
    assert sorted(a) == ["amp_force", "amp_torque", "kick", "phase", "window"]
    for k in a:
        assert np.array_equal(a[k][40:], b[k]), k
    assert np.abs(a["amp_force"]).max() <= 0.3 and np.abs(a["kick"][:, 3:]).max() <= 0.1
    assert a["window"].dtype == np.int32 and a["window"][:, 0].min() >= 2 and a["window"][:, 0].max() <= 9
    length = a["window"][:, 1] - a["window"][:, 0]
    assert length.min() == 0 and length.max() == 4
    assert (a["phase"] >= 0).all() and (a["phase"] < 2 * np.pi).all()
    assert EV.sample(5, 1) == {}
    EV.request(a, 96, 10)          # what it draws is a valid request


# ---- 3. refusals

REFUSALS = [
    (dict(nonsense=1), {}, "unknown keys"),
    (dict(step0=-1), {}, "step0"),
    (dict(step0=3), dict(sensor=dict(step0=2)), "step0"),
    (dict(sigma=(-1.0, 0.0)), {}, "sigma"),
    (dict(sigma=(0.0, np.inf)), {}, "sigma"),
    (dict(sigma=(0.1, 0.0), tau=(0.0, 1.0)), {}, "tau"),
    (dict(sigma=(0.0, 0.1), tau=(1.0, np.nan)), {}, "tau"),
    (dict(amp_force=np.ones((B, 3)), period=0.0), {}, "period"),
    (dict(amp_torque=np.ones((B, 3)), period=np.inf), {}, "period"),
    (dict(amp_force=np.full((B, 3), np.nan)), {}, "amp_force"),
    (dict(amp_torque=np.ones((B, 2))), {}, "amp_torque"),
    (dict(phase=np.array([0.0, np.inf, 0.0])), {}, "phase"),
    (dict(kick=np.ones((B, 6))), {}, "kick"),
    (dict(kick=np.full((B, 6), np.nan), window=np.zeros((B, 2))), {}, "kick"),
    (dict(window=np.zeros((B, 3))), {}, "window"),
    (dict(state=np.full((B, 6), np.nan)), {}, "state"),
    (dict(est_err_sq=np.zeros((B, 2))), {}, "est_err_sq"),
    (dict(fields=("est_err_sq",)), {}, "est_err_sq"),
    (dict(est_err_sq=-np.ones((B, 2))), dict(disturbance=DIST), "est_err_sq"),
    (dict(fields=("nothing",)), {}, "fields"),
]


@pytest.mark.parametrize("env,call,field", REFUSALS)
def test_request_refuses(env, call, field):
    with pytest.raises(ValueError, match=field):
        EV.request(env, B, T, **call)


def test_request_fills_defaults_and_copies():
    state = np.ones((B, 6))
    r = EV.request(dict(sigma=0.2, state=state, fields=("wrench", "state")), B, T, sensor=dict(step0=0))
    assert r["sigma"].tolist() == [0.2, 0.2] and r["tau"].tolist() == [1.0, 1.0] and r["step0"] == 0 and r["seed"] == 0
    assert r["state"] is not state and np.array_equal(r["state"], state)
    assert r["amp_force"] is None and r["window"] is None
    assert EV.request(dict(est_err_sq=np.zeros((B, 2))), B, T, disturbance=DIST)["est_err_sq"].shape == (B, 2)


# ---- 4. layout and dispatch

def test_struct_layout_matches_the_header(tmp_path):
    fields = [n for n, _ in _lib.ftmpc_environment._fields_]
    body = "".join(f'printf("{f} %zu\\n", offsetof(ftmpc_environment, {f}));' for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftmpc.h"\nint main(void){printf("sizeof %zu\\n", '
                   'sizeof(ftmpc_environment));' + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.ftmpc_environment) == 128
    for f in fields:
        assert int(got[f]) == getattr(_lib.ftmpc_environment, f).offset, f


class Recorder:
    """Stands in for the loaded library: every ftmpc_* attribute is a function that records its call and returns FTMPC_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("ftmpc_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def _stand_in():
    real = _lib.load_library()
    cfg = MPCConfig(N=N, NT=NT)
    c = BatchedMPC.make_c_config(real, cfg)
    rec = Recorder()
    obj = SimpleNamespace(cfg=cfg, lib=rec, _c=c, _h=C.c_void_p(1234), D=np.array(list(c.D))[:6 * NT].reshape(6, NT))
    obj._check = lambda rc: None if rc == 0 else pytest.fail(f"rc = {rc}")
    return obj, rec, real


def _call(obj, multi, wrench, **kw):
    x0 = np.zeros((B, 13))
    x0[:, 6] = 1.0
    args = dict(uref_traj=None, noise=(0, 0, 0, 0), seed=3, return_inputs=True, sqp_iters=0, backtracks=8, tol=1e-9,
                formulation="wrench" if wrench else "thruster", hull=None, penalty=0.0, faults=None, detect_delay=0, return_states=False,
                outcomes=None, return_status=False, index0=0, index_total=None)
    args.update(kw)
    return _simulate(obj, multi, x0, np.full((B, NT), F_MAX), np.zeros((B, NT)), np.zeros((9, T + N)), T, **args)


ENV = dict(sigma=(0.1, 0.01), tau=(1.0, 1.0), fields=("wrench", "state"))


@pytest.mark.parametrize("wrench,multi,want", [(False, False, "ftmpc_simulate_environment_batch"),
                                               (True, False, "ftmpc_simulate_wrench_environment_batch"),
                                               (False, True, "ftmpc_multi_simulate_environment_batch")])
@pytest.mark.parametrize("others", [{}, dict(estimator=EST, disturbance=DIST, plant=dict(mass=np.full(B, 12.0)))])
def test_environment_reaches_its_entry_with_the_struct_last(wrench, multi, want, others):
    obj, rec, real = _stand_in()
    others = dict(others)
    if wrench and "disturbance" in others:
        others["disturbance"] = dict(others["disturbance"], wrench=True)
    env = dict(ENV, fields=ENV["fields"] + (("est_err_sq",) if "disturbance" in others else ()))
    out = _call(obj, multi, wrench, environment=env, **others)
    assert len(rec.calls) == 1
    name, got = rec.calls[0]
    assert name == want
    assert len(got) == len(getattr(real, name).argtypes)
    assert got[0] is obj._h and got[1] == B and got[2] == T
    ev = got[-1]._obj
    assert isinstance(ev, _lib.ftmpc_environment)
    assert ev.struct_size == C.sizeof(_lib.ftmpc_environment) and ev.reserved == 0 and list(ev.sigma) == [0.1, 0.01]
    assert bool(ev.wrench_hist) and bool(ev.state) and not ev.amp_force and not ev.kick and not ev.window
    assert bool(ev.est_err_sq) == ("disturbance" in others)
    assert got[-2] is None                              # no outage
    # the state asked back from a stationary start is the restatement's draw, handed over
    assert np.array_equal(out["environment"]["state"], EV.stationary(B, ENV["sigma"], 0, 0))
    assert out["environment"]["wrench"].shape == (T, B, 6)


def test_without_the_keyword_the_call_reaches_the_entry_it_reached():
    obj, rec, _ = _stand_in()
    _call(obj, False, False, estimator=EST)
    _call(obj, False, False, estimator=EST, environment=None)
    assert [n for n, _ in rec.calls] == ["ftmpc_simulate_estimator_batch"] * 2


def test_wrench_environment_on_the_driver_is_refused_before_any_call():
    obj, rec, _ = _stand_in()
    with pytest.raises(ValueError, match="MultiGPUMPC is not built"):
        _call(obj, True, True, environment=ENV)
    assert rec.calls == []


def test_a_refused_request_makes_no_call():
    obj, rec, _ = _stand_in()
    with pytest.raises(ValueError, match="est_err_sq"):
        _call(obj, False, False, environment=dict(fields=("est_err_sq",)))
    with pytest.raises(ValueError, match="step0"):
        _call(obj, False, False, environment=dict(step0=4), sensor=dict(sigma=(1e-3,) * 4, step0=3))
    assert rec.calls == []
