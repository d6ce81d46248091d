"""CPU: which C entry ft_mpc_amd.batch._simulate calls, and with what.

_simulate builds its argument list once and calls the narrowest closed-loop entry that carries every feature present, so that the Python
suite keeps exercising every ABI level of the forwarding chain in include/ftmpc.h.  Here it runs against a recording stand-in for the
library (no handle, no GPU): for each single feature and for the full set, on both forms, on the single handle and on the multi-GPU
driver, the entry's name is the one in the table below (taken from the ladder of calls this dispatch replaced), the argument count is
the length of that entry's argtypes in ft_mpc_amd._lib, and each feature struct sits at its position."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from ft_mpc_amd import _lib
from ft_mpc_amd.batch import BatchedMPC, MPCConfig, _simulate

N, NT, B, T = 4, 8, 3, 2
F_MAX = 3.4
EST = dict(every=1, p0=(0.05, 0.05, 0.02, 0.02), proc_sigma=(1e-4, 1e-3, 1e-4, 1e-3), meas_sigma=(1e-3, 1e-3, 1e-3, 1e-3))
DIAG = dict(every=1, levels=(0.0, F_MAX), resid_sigma=(1e-2, 1e-2), drift_sigma=(0, 0), threshold=18.0, max_detect=2)

FULL = dict(outcomes=dict(fields=["err_int", "cost"]), plant=dict(mass=np.full(B, 12.0)), actuator=dict(tau_on=0.02),
            sensor=dict(sigma=(1e-3,) * 4), estimator=EST, diagnosis=DIAG)
# the request of each case: the feature itself and what it cannot go without (an estimate needs the estimator)
FEATURES = {
    "plain": {},
    "sqp": dict(sqp_iters=2),
    "states": dict(return_states=True),
    "outcomes": dict(outcomes=dict(fields=["err_int"])),
    "plant": dict(plant=dict(mass=np.full(B, 12.0))),
    "mission": dict(mission=dict(tables=np.zeros((1, 9, T + N + 1)))),
    "cost": dict(outcomes=dict(fields=["cost"])),
    "actuator": dict(actuator=dict(tau_on=0.02)),
    "sensor": dict(sensor=dict(sigma=(1e-3,) * 4)),
    "estimator": dict(estimator=EST),
    "diagnosis": dict(diagnosis=DIAG),
    "disturbance": dict(estimator=EST, disturbance=dict(p0=(1, 1), proc_sigma=(0, 0))),
    "bias": dict(estimator=EST, bias_estimate=dict(p0=(0.05, 0.02), proc_sigma=(0, 0))),
    "all_with_disturbance": dict(FULL, disturbance=dict(p0=(1, 1), proc_sigma=(0, 0))),
    "all_with_bias": dict(FULL, bias_estimate=dict(p0=(0.05, 0.02), proc_sigma=(0, 0))),      # (the two estimates exclude each other)
}
# the entry each case reaches: (thruster, wrench) on the single handle; the multi-GPU driver has the entries from outcomes up, and
# takes a case below them to its outcomes entry
SINGLE = {
    "plain": ("ftmpc_simulate_batch_ex", "ftmpc_simulate_wrench_batch"),
    "sqp": ("ftmpc_simulate_batch_ex", "ftmpc_simulate_wrench_batch_ex"),
    "states": ("ftmpc_simulate_faults_batch", "ftmpc_simulate_wrench_faults_batch"),
    "outcomes": ("ftmpc_simulate_outcomes_batch", "ftmpc_simulate_wrench_outcomes_batch"),
    "plant": ("ftmpc_simulate_plant_batch", "ftmpc_simulate_wrench_plant_batch"),
    "mission": ("ftmpc_simulate_mission_batch", "ftmpc_simulate_wrench_mission_batch"),
    "cost": ("ftmpc_simulate_mission_batch", "ftmpc_simulate_wrench_mission_batch"),
    "actuator": ("ftmpc_simulate_actuator_batch", "ftmpc_simulate_wrench_actuator_batch"),
    "sensor": ("ftmpc_simulate_sensor_batch", "ftmpc_simulate_wrench_sensor_batch"),
    "estimator": ("ftmpc_simulate_estimator_batch", "ftmpc_simulate_wrench_estimator_batch"),
    "diagnosis": ("ftmpc_simulate_diagnosis_batch", "ftmpc_simulate_wrench_diagnosis_batch"),
    "disturbance": ("ftmpc_simulate_disturbance_batch", "ftmpc_simulate_wrench_disturbance_batch"),
    "bias": ("ftmpc_simulate_bias_batch", "ftmpc_simulate_wrench_bias_batch"),
    "all_with_disturbance": ("ftmpc_simulate_disturbance_batch", "ftmpc_simulate_wrench_disturbance_batch"),
    "all_with_bias": ("ftmpc_simulate_bias_batch", "ftmpc_simulate_wrench_bias_batch"),
}
BELOW_OUTCOMES = ("plain", "sqp", "states")
# position of each feature struct behind the entry's fixed arguments (17 on the thruster form, 24 on the wrench form, whose diagnosis
# is followed by the offsets and the no-hull steps)
STRUCTS = (("outcomes", _lib.ftmpc_outcomes), ("plant", _lib.ftmpc_plant_model), ("mission", _lib.ftmpc_mission),
           ("actuator", _lib.ftmpc_actuator), ("sensor", _lib.ftmpc_sensor), ("estimator", _lib.ftmpc_estimator),
           ("diagnosis", _lib.ftmpc_diagnosis), ("disturbance", _lib.ftmpc_disturbance), ("bias", _lib.ftmpc_bias_estimate))
# the wrench form's bias entry exists on the single handle only: the driver refuses the request (last test)
CASES = [(case, wrench, multi) for case in sorted(FEATURES) for wrench in (False, True) for multi in (False, True)
         if not (multi and wrench and "bias_estimate" in FEATURES[case])]


def _present(kw):
    """The feature structs a request hands to its entry (the outcomes struct goes to every entry that has the parameter)."""
    names = {"outcomes"} | {n for n, _ in STRUCTS if n in kw}
    if "bias_estimate" in kw:
        names.add("bias")
    if "mission" in kw or "cost" in (kw.get("outcomes") or {}).get("fields", ()):
        names.add("mission")
    return names


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


def _pointee(arg):
    return arg._obj if arg is not None else None      # (what C.byref refers to)


@pytest.mark.parametrize("case,wrench,multi", CASES)
def test_entry_and_arguments(case, wrench, multi):
    kw = {k: (dict(v) if isinstance(v, dict) else v) for k, v in FEATURES[case].items()}
    if wrench and "diagnosis" in kw:
        kw["diagnosis"] = dict(kw["diagnosis"], rebuild_hull=True)
    if wrench and "disturbance" in kw:
        kw["disturbance"] = dict(kw["disturbance"], wrench=True)
    obj, rec, real = _stand_in()
    x0 = np.zeros((B, 13))
    x0[:, 6] = 1.0
    ub, stuck = np.full((B, NT), F_MAX), np.zeros((B, NT))
    xref = None if "mission" in kw else np.zeros((9, T + N))
    args = dict(uref_traj=None, noise=(0, 0, 0, 0), seed=3, return_inputs=True, sqp_iters=0, backtracks=8, tol=1e-9,
                formulation="wrench" if wrench else "thruster", hull=None, penalty=0.0, faults=None, detect_delay=0, return_states=False,
                outcomes=None, return_status=False, index0=0, index_total=None)
    args.update(kw)
    _simulate(obj, multi, x0, ub, stuck, xref, T, **args)
    assert len(rec.calls) == 1
    name, got = rec.calls[0]
    want = SINGLE[case][wrench]
    if multi:
        want = (SINGLE["outcomes"][wrench] if case in BELOW_OUTCOMES else want).replace("ftmpc_simulate_", "ftmpc_multi_simulate_")
    assert name == want
    assert len(got) == len(getattr(real, name).argtypes)
    assert got[0] is obj._h and got[1] == B and got[2] == T
    if case in BELOW_OUTCOMES and not multi:
        return
    present = _present(kw)
    at = 24 if wrench else 17
    for feature, struct in STRUCTS:
        if at >= len(got):
            assert feature not in present      # the entry is the narrowest one: nothing present is left out
            continue
        if feature in present:
            assert isinstance(_pointee(got[at]), struct), (feature, at)
        else:
            assert got[at] is None, (feature, at)
        at += 1
        if wrench and feature == "diagnosis":      # out_hull_b [B][rows] and no_hull_step [B], with a diagnosis only
            assert (got[at] is None) == (got[at + 1] is None) == ("diagnosis" not in present)
            at += 2
    assert at == len(got)


def test_wrench_bias_on_the_driver_is_refused_before_any_call():
    obj, rec, _ = _stand_in()
    x0 = np.zeros((B, 13))
    x0[:, 6] = 1.0
    with pytest.raises(ValueError, match="MultiGPUMPC is not built"):
        _simulate(obj, True, x0, np.full((B, NT), F_MAX), np.zeros((B, NT)), np.zeros((9, T + N)), T, None, (0, 0, 0, 0), 3, True, 0, 8,
                  1e-9, "wrench", None, 0.0, None, 0, False, None, False, 0, None, estimator=EST,
                  bias_estimate=dict(p0=(0.05, 0.02), proc_sigma=(0, 0)))
    assert rec.calls == []
