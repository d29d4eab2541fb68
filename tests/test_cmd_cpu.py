"""Velocity commands without a GPU (include/hb.h: hb_env_commands): the exports and the ctypes mirror, every refusal that needs no
device with its message, and tests/cmd_ref.py itself - the statistics of its draws and the two frames of its reward."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cmd_ref
from oracle_lib import HUMANOID_HBM, ROOT

SEED = 11  # the seed of the draw statistics below


def _cfg(hbmod, model, **kw):
    import humanoid_mujoco_amd.engine as eng
    c = eng.HbEnvCommands()
    assert hbmod.lib().hb_env_default_commands(model._h, ctypes.byref(c)) == 0
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _error(hbmod):
    return hbmod.lib().hb_error().decode()


def test_library_exports_the_entry_points(hbmod):
    L = ctypes.CDLL(hbmod.LIB_PATH)
    for name in ("hb_env_default_commands", "hb_env_commands_check", "hb_env_commands_configure", "hb_env_get_commands", "hb_env_set_commands", "hb_error"):
        assert hasattr(L, name), name


def test_ctypes_struct_matches_the_header(hbmod, humanoid_model, tmp_path):
    import humanoid_mujoco_amd.engine as eng
    cls = eng.HbEnvCommands
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hb.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(hb_env_commands));']
    lines += ['printf("%s %%zu\\n", offsetof(hb_env_commands, %s));' % (f, f) for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls) == 48
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f
    # the defaults fill every field of the mirror, and pass their own check
    c = _cfg(hbmod, humanoid_model)
    assert (c.vx_min, c.vx_max, c.vy_min, c.vy_max, c.yaw_min, c.yaw_max) == (-1.0, 1.0, -0.5, 0.5, -1.0, 1.0)
    assert c.resample_time == 5.0 and abs(c.zero_fraction - 0.1) < 1e-7 and c.w_yaw == 2.5 and (c.frame, c.observe, c.seed) == (1, 1, 0)
    assert hbmod.lib().hb_env_commands_check(humanoid_model._h, ctypes.byref(c)) == 0 and _error(hbmod) == ""


def test_refusals_without_a_device(hbmod, humanoid_model):
    L, m = hbmod.lib(), humanoid_model
    import humanoid_mujoco_amd.engine as eng
    # a NULL batch, a NULL argument
    c = _cfg(hbmod, m)
    assert L.hb_env_commands_configure(None, ctypes.byref(c)) == -1 and "NULL batch" in _error(hbmod)
    assert L.hb_env_commands_configure(None, None) == -1 and "NULL batch" in _error(hbmod)
    out = np.zeros(3, np.float32)
    assert L.hb_env_get_commands(None, out.ctypes.data_as(ctypes.c_void_p)) == -1 and "NULL" in _error(hbmod)
    assert L.hb_env_set_commands(None, out.ctypes.data_as(ctypes.c_void_p), None) == -1 and "NULL" in _error(hbmod)
    assert L.hb_env_default_commands(None, ctypes.byref(c)) == -1 and "NULL" in _error(hbmod)
    assert L.hb_env_default_commands(m._h, None) == -1 and "NULL" in _error(hbmod)
    assert L.hb_env_commands_check(m._h, None) == -1 and L.hb_env_commands_check(None, ctypes.byref(c)) == -1
    # the fields: a refused check names its reason, an accepted one clears it
    floats = [f for f, t in eng.HbEnvCommands._fields_ if t is ctypes.c_float]
    assert len(floats) == 9
    for f in floats:
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert L.hb_env_commands_check(m._h, ctypes.byref(_cfg(hbmod, m, **{f: bad}))) == -1, (f, bad)
            assert "not finite" in _error(hbmod), (f, bad)
    for lo, hi in (("vx_min", "vx_max"), ("vy_min", "vy_max"), ("yaw_min", "yaw_max")):
        assert L.hb_env_commands_check(m._h, ctypes.byref(_cfg(hbmod, m, **{lo: 0.5, hi: 0.25}))) == -1 and "min > max" in _error(hbmod)
        assert L.hb_env_commands_check(m._h, ctypes.byref(_cfg(hbmod, m, **{lo: 0.5, hi: 0.5}))) == 0 and _error(hbmod) == ""  # (an empty range is one)
    for z in (-0.01, 1.01):
        assert L.hb_env_commands_check(m._h, ctypes.byref(_cfg(hbmod, m, zero_fraction=z))) == -1 and "zero_fraction" in _error(hbmod)
    for z in (0.0, 1.0):
        assert L.hb_env_commands_check(m._h, ctypes.byref(_cfg(hbmod, m, zero_fraction=z))) == 0
    for v in (-1, 2):
        assert L.hb_env_commands_check(m._h, ctypes.byref(_cfg(hbmod, m, frame=v))) == -1 and "frame" in _error(hbmod)
        assert L.hb_env_commands_check(m._h, ctypes.byref(_cfg(hbmod, m, observe=v))) == -1 and "observe" in _error(hbmod)
    assert L.hb_env_commands_check(m._h, ctypes.byref(_cfg(hbmod, m, resample_time=-1.0, w_yaw=-3.0))) == 0  # (no draw inside an episode; any weight)
    # a model whose observation has no free root
    arm = hbmod.Model.from_xml_string('<mujoco><worldbody><body><joint type="hinge" axis="0 1 0"/><geom type="capsule" size="0.05" fromto="0 0 0 0.3 0 0"/>'
                                      '</body></worldbody></mujoco>')
    assert L.hb_env_commands_check(arm._h, ctypes.byref(_cfg(hbmod, m))) == -1 and "free root" in _error(hbmod)


def test_reference_draws():
    """4096 draws at zero_fraction 0.25: inside their ranges, the zero command 1024 +- 5 sigma times (sigma = sqrt(4096 * 0.25 * 0.75) = 27.7),
    and distinct across envs, episodes and k"""
    import types
    C = types.SimpleNamespace(seed=SEED, vx_min=-0.5, vx_max=1.5, vy_min=-0.25, vy_max=0.75, yaw_min=-2.0, yaw_max=1.0, resample_time=0.015,
                              zero_fraction=0.25, w_yaw=1.0, frame=1, observe=1)
    draws = np.stack([cmd_ref.draw(C, g, ep, k) for g in range(16) for ep in range(16) for k in range(16)])
    assert draws.shape == (4096, 3) and draws.dtype == np.float32
    lo, hi = np.float32([C.vx_min, C.vy_min, C.yaw_min]), np.float32([C.vx_max, C.vy_max, C.yaw_max])
    zero = ~draws.any(axis=1)
    assert (draws[~zero] >= lo).all() and (draws[~zero] <= hi).all()
    assert 885 <= int(zero.sum()) <= 1163, int(zero.sum())
    assert len(np.unique(draws[~zero], axis=0)) == int((~zero).sum())
    # a draw is a function of (seed, g, ep, k) alone, and the seed matters
    assert np.array_equal(cmd_ref.draw(C, 5, 3, 2), draws[(5 * 16 + 3) * 16 + 2])
    C2 = types.SimpleNamespace(**dict(vars(C), seed=SEED + 1))
    assert not np.array_equal(np.stack([cmd_ref.draw(C2, g, 0, 0) for g in range(16)]), draws[::256])
    # zero_fraction 0 never gives the zero command, 1 always
    C0, C1 = types.SimpleNamespace(**dict(vars(C), zero_fraction=0.0)), types.SimpleNamespace(**dict(vars(C), zero_fraction=1.0))
    assert all(cmd_ref.draw(C0, g, 0, 0).any() for g in range(64)) and not any(cmd_ref.draw(C1, g, 0, 0).any() for g in range(64))
    # the resample rule: float32 time against the float32 product
    assert cmd_ref.due(C, np.float32(0.015), 1) and not cmd_ref.due(C, np.float32(0.0149999), 1) and not cmd_ref.due(C0, np.float32(0.029), 2)
    assert not cmd_ref.due(types.SimpleNamespace(**dict(vars(C), resample_time=0.0)), np.float32(9.0), 1)
    sched = cmd_ref.Schedule(C, 4)
    k0 = sched.cmd.copy()
    old = sched.step(np.float32([0.005, 0.015, 0.005, 0.02]), np.array([False, False, True, True]))
    assert np.array_equal(old, k0) and np.array_equal(sched.k, [1, 2, 1, 1]) and np.array_equal(sched.ep, [0, 0, 1, 1])
    assert np.array_equal(sched.cmd[0], k0[0]) and np.array_equal(sched.cmd[1], cmd_ref.draw(C, 1, 0, 1)) and np.array_equal(sched.cmd[3], cmd_ref.draw(C, 3, 1, 0))


def _state(hbmod, seed):
    """a 27-dof humanoid state with a tilted, yawed root and every velocity non-zero"""
    m = hbmod.Model.load(HUMANOID_HBM)
    rng = np.random.default_rng(seed)
    qpos = m.array("qpos0").astype(np.float64)
    qpos[7:] += rng.uniform(-0.2, 0.2, m.nq - 7)
    q = np.array([np.cos(0.45), 0.0, 0.0, np.sin(0.45)]) + rng.uniform(-0.15, 0.15, 4)
    qpos[3:7] = q
    qvel = rng.uniform(-1.0, 1.0, m.nv)
    return m, qpos, qvel, rng


@pytest.mark.parametrize("kind", [0, 1])
def test_reference_reward_frames(hbmod, kind):
    """turning the whole state about world z leaves the heading-frame reward where it was (to fp64 rounding) and moves the world-frame
    reward of a non-zero command; the zero-weight, target-velocity configuration gives env_ref's reward back"""
    import types
    import env_ref
    m, qpos, qvel, rng = _state(hbmod, 3 + kind)
    import humanoid_mujoco_amd.engine as eng
    cfg = eng.HbEnvConfig()
    assert hbmod.lib().hb_env_default_config(m._h, ctypes.byref(cfg)) == 0
    cfg.reward_kind, cfg.w_vvel, cfg.max_time = kind, 1.5, 0.0
    tq, prev, act = rng.uniform(-30, 30, m.nv - 6), rng.uniform(-1, 1, m.nu), rng.uniform(-1, 1, m.nu)
    cmd = np.float32([0.8, -0.3, 0.6])
    C = types.SimpleNamespace(w_yaw=2.5, frame=1)
    args = (tq, prev, act, False)
    r1, te, tr = cmd_ref.reward(cfg, C, cmd, 0.5, qpos, qvel, *args)
    assert not te and r1 > 5.0
    C0 = types.SimpleNamespace(w_yaw=2.5, frame=0)
    r0 = cmd_ref.reward(cfg, C0, cmd, 0.5, qpos, qvel, *args)[0]
    for angle in (0.7, -2.1, 3.0):
        q2, v2 = cmd_ref.rotate_state_z(qpos, qvel, angle)
        assert abs(cmd_ref.yaw_rate(q2, v2) - cmd_ref.yaw_rate(qpos, qvel)) < 1e-13
        assert abs(cmd_ref.reward(cfg, C, cmd, 0.5, q2, v2, *args)[0] - r1) < 1e-12
        assert abs(cmd_ref.reward(cfg, C0, cmd, 0.5, q2, v2, *args)[0] - r0) > 1e-3
    # the two frames differ for this yawed root, and agree for a root whose x axis points along world x
    assert abs(r1 - r0) > 1e-3
    c, s = cmd_ref.heading(qpos)
    q3, v3 = cmd_ref.rotate_state_z(qpos, qvel, -np.arctan2(s, c))
    assert abs(cmd_ref.reward(cfg, C, cmd, 0.5, q3, v3, *args)[0] - cmd_ref.reward(cfg, C0, cmd, 0.5, q3, v3, *args)[0]) < 1e-12
    # a root pointing straight up has no heading: the frame falls back to the world's
    up = qpos.copy(); up[3:7] = [np.sqrt(0.5), 0.0, -np.sqrt(0.5), 0.0]
    assert cmd_ref.heading(up) == (1.0, 0.0)
    # neutral: no yaw weight, frame 0, the command = target_velocity gives env_ref's own reward
    cfg.target_velocity[0], cfg.target_velocity[1] = 0.25, -0.125
    base = (env_ref.control_input_reward if kind == 1 else env_ref.standup_reward)(cfg, 0.5, qpos, qvel, *args)
    got = cmd_ref.reward(cfg, types.SimpleNamespace(w_yaw=0.0, frame=0), np.float32([0.25, -0.125, 9.0]), 0.5, qpos, qvel, *args)
    assert abs(got[0] - base[0]) < 1e-12 and got[1:] == base[1:]
    L, width = cmd_ref.layout(48, 21, 6, True, True, True)
    assert width == 78 and L["command"] == slice(75, 78) and L["height_scan"] == slice(69, 75) and L["prev_action"] == slice(48, 69)
    assert cmd_ref.layout(48, 21, 6, False, False, True) == ({"base": slice(0, 48), "command": slice(48, 51)}, 51)
