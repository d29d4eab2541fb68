"""Inverse dynamics without a GPU: the fp64 reference (tests/inverse_ref.py) against the oracle's own forward dynamics, and the C-ABI's
argument checks (include/hb.h: hb_inverse, hb_inverse_dev)."""
import ctypes
import os

import numpy as np

from inverse_ref import forward_at, inverse_ref
from oracle_lib import GOLDEN, Oracle, MODELS_DIR as MODELS

SOL_NEWTON = 2
HB_EINVAL = -1  # include/hb.h


def _newton(o):
    o.set_opt(solver=SOL_NEWTON, iterations=100, tolerance=1e-12)


def _scale(o):
    return max(1.0, np.abs(o.qfrc_bias).max(), np.abs(o.qfrc_actuator).max(), np.abs(o.qfrc_constraint).max())


def test_reference_round_trip_on_golden_states():
    """mj_forward's qacc (Newton, converged) in, qfrc_actuator + qfrc_applied out, on the 128 golden humanoid states."""
    g = np.load(os.path.join(GOLDEN, "humanoid27_steps.npz"))
    o = Oracle()
    _newton(o)
    worst, rows = 0.0, 0
    for k in range(len(g["env"])):
        forward_at(o, g["qpos"][k], g["qvel"][k], g["ctrl"][k])
        got = inverse_ref(o, o.qacc.copy())
        worst = max(worst, np.abs(got - (o.qfrc_actuator + o.qfrc_applied)).max() / _scale(o))
        rows += o.nefc
    assert rows > 0
    assert worst < 1e-8, worst  # (measured 7e-14: converged Newton)


def _model_states(name, tmp_path, nstate=12, stride=40):
    import humanoid_mujoco_amd as hb
    p = str(tmp_path / (name + ".hbm"))
    hb.Model.load(os.path.join(MODELS, name + ".xml")).save(p)
    o = Oracle(p)
    _newton(o)
    o.reset(0 if name == "chain" else -1)
    states = []
    for t in range(nstate * stride):
        o.ctrl[:] = np.sign(np.sin(0.01 * t + 1.0 + np.arange(o.nu)))  # (full controls, switching slowly: into the limits)
        o.step()
        if t % stride == stride - 1:
            states.append((o.qpos.copy(), o.qvel.copy(), o.ctrl.copy()))
    if name == "pendulum_limit":  # (its motor does not reach the limits: angles across the range [-0.5, 0.3] and beyond)
        states = [(np.array([q]), np.array([v]), np.array([c])) for q, v, c in zip(np.linspace(-0.6, 0.4, nstate), np.linspace(1, -1, nstate), np.linspace(-1, 1, nstate))]
    return o, states


def test_reference_round_trip_on_test_models(tmp_path):
    """The same on the small models: joint limits, a fixed tendon, multi-tree contacts, a height field; continuous and discrete."""
    for name in ("pendulum_limit", "chain", "capsules", "ball_hfield"):
        o, states = _model_states(name, tmp_path)
        worst_c = worst_d = 0.0
        rows = 0
        for qpos, qvel, ctrl in states:
            forward_at(o, qpos, qvel, ctrl)
            want = o.qfrc_actuator + o.qfrc_applied
            worst_c = max(worst_c, np.abs(inverse_ref(o, o.qacc.copy()) - want).max() / _scale(o))
            rows += o.nefc
            # discrete: one step from here, (qvel' - qvel) / h, inverted at the state before the step
            h = o.opt("timestep")
            o.step()
            qacc_d = (o.qvel - qvel) / h
            forward_at(o, qpos, qvel, ctrl)
            worst_d = max(worst_d, np.abs(inverse_ref(o, qacc_d, discrete=True) - want).max() / _scale(o))
        assert rows > 0, name
        assert worst_c < 1e-8 and worst_d < 1e-8, (name, worst_c, worst_d)


def test_abi_exports_and_null_arguments():
    import humanoid_mujoco_amd as hb
    L = hb.lib()
    assert hasattr(L, "hb_inverse") and hasattr(L, "hb_inverse_dev")
    q = np.zeros(27, dtype=np.float32)
    out = np.zeros(27, dtype=np.float32)
    vp = ctypes.c_void_p
    assert L.hb_inverse(None, q.ctypes.data_as(vp), 0, out.ctypes.data_as(vp), None) == HB_EINVAL
    assert L.hb_inverse_dev(None, q.ctypes.data_as(vp), 1, out.ctypes.data_as(vp), None) == HB_EINVAL
    assert L.hb_inverse(None, None, 0, None, None) == HB_EINVAL
    assert hb.engine.HB_INV_DISCRETE == 1
