"""What tests/test_gpu_cmd.py and tools/gpu_cmd_parity.py share: the command configuration of the GPU tests, a VecEnv with it, the fp64
reference rewards of a step from the device's own state, torques and actions (tests/cmd_ref.py, tests/env_ref.py), and the measurement
behind profiles/cmd_parity.txt.  Test infrastructure only."""
import numpy as np

import cmd_ref
import env_ref
from oracle_lib import HUMANOID_HBM, Oracle

# ranges that are not symmetric, a draw every three control steps of 5 ms, a quarter of the draws zero, the heading frame, observed
CMD = dict(seed=5, vx_min=-0.5, vx_max=1.5, vy_min=-0.25, vy_max=0.75, yaw_min=-2.0, yaw_max=1.0, resample_time=0.015, zero_fraction=0.25, w_yaw=2.5,
           frame=1, observe=1)


def model(hbmod):
    return hbmod.Model.load(HUMANOID_HBM)


def env(hbmod, gpu, n, commands=CMD, mdl=None, **kw):
    kw.setdefault("target_z", 10.0)  # (out of reach: standing, which the reset pose is, ends no episode)
    return hbmod.VecEnv(mdl if mdl is not None else model(hbmod), n, gpu, seed=7, commands=None if commands is None else dict(commands), **kw)


def actions(rng, n, nu, scale=1.0):
    return rng.uniform(-scale, scale, (n, nu)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def self_collisions(o, m, st0, act):
    """the self-collision flag of the step from st0 under act, per env: the oracle's contacts at the pre-step state (one physics step per
    env step), as tests/test_gpu_env.py takes it"""
    out = np.zeros(len(st0), dtype=bool)
    for e in range(len(st0)):
        o.reset()
        o.qpos[:] = st0[e, 1:1 + m.nq]; o.qvel[:] = st0[e, 1 + m.nq:1 + m.nq + m.nv]; o.qacc_warmstart[:] = st0[e, 1 + m.nq + m.nv:]
        o.ctrl[:] = act[e]
        o.forward()
        out[e] = any(c["geom1"] != 0 for c in o.contacts())
    return out


def reference_rewards(cfg, C, cmd, st1, torques, prev, act, selfcol):
    """(reward [n] float64, terminated [n], truncated [n]) of the states st1 a step ended in; cmd [n, 3] the commands in force during it,
    or C = None: no commands, env_ref's reward"""
    n, nv = len(st1), torques.shape[1] + 6
    nq = nv + 1  # (a free root and scalar joints)
    r, te, tr = np.zeros(n), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    base = env_ref.control_input_reward if cfg.reward_kind == 1 else env_ref.standup_reward
    for e in range(n):
        q, v = st1[e, 1:1 + nq], st1[e, 1 + nq:1 + nq + nv]
        args = (st1[e, 0], q, v, torques[e].astype(np.float64), prev[e].astype(np.float64), act[e].astype(np.float64), bool(selfcol[e]))
        r[e], te[e], tr[e] = base(cfg, *args) if C is None else cmd_ref.reward(cfg, C, cmd[e], *args)
    return r, te, tr


def measure_parity(hbmod, gpu, n=64, steps=4, log=print):
    """Both frames and both reward kinds, from a perturbed reset with a yawed and tilted root (reset_quat_perturb 0.2) that is given a
    planar velocity of up to 1 m/s a component and an angular velocity of up to 1 rad/s a component, so that frame and yaw term matter
    (controlInputReward with its vertical-velocity term on; standupReward has none): the worst absolute difference of the device's reward from cmd_ref in fp64 on the device's own states, joint torques and actions, and next to it the
    difference of the reward WITHOUT commands from env_ref on the same states (a twin batch stepped with the same actions).  Four steps: the
    draw after step 3 changes the commands in between.  Returns {(kind, frame): dict(cmd=..., plain=..., scale=..., frames_differ=...)}."""
    m = model(hbmod)
    o = Oracle()
    out = {}
    for kind in (0, 1):
        for frame in (0, 1):
            kw = dict(reward_kind=kind, reset_quat_perturb=0.2, max_time=0.0, auto_reset=0, w_vvel=1.5 if kind == 1 else 0.0)
            a, c = env(hbmod, gpu, n, dict(CMD, frame=frame), m, **kw), env(hbmod, gpu, n, None, m, **kw)
            other = type(a.commands_cfg).from_buffer_copy(a.commands_cfg)
            other.frame = 1 - frame
            sched = cmd_ref.Schedule(a.commands_cfg, n)
            a.reset(); c.reset()
            rng = np.random.default_rng(17 + 2 * kind + frame)
            st = a.batch.get_state(hbmod.STATE_INTEGRATION)
            st[:, 1 + m.nq:1 + m.nq + 2] = rng.uniform(-1.0, 1.0, (n, 2))
            st[:, 1 + m.nq + 3:1 + m.nq + 6] = rng.uniform(-1.0, 1.0, (n, 3))
            a.batch.set_state(hbmod.STATE_INTEGRATION, st); c.batch.set_state(hbmod.STATE_INTEGRATION, st)
            prev = np.zeros((n, m.nu), np.float32)
            res = dict(cmd=0.0, plain=0.0, scale=0.0, frames_differ=0.0, terminated=0)
            for t in range(steps):
                act = actions(rng, n, m.nu)
                st0 = a.batch.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
                _, ra, tea, tra, _ = a.step_arrays(act)
                _, rc, tec, trc, _ = c.step_arrays(act)
                st1 = a.batch.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
                assert np.array_equal(st1, c.batch.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64))  # (commands do not touch the physics)
                tq = a.batch.env_joint_torques()[:, 6:]
                col = self_collisions(o, m, st0, act)
                cmd = sched.step(st1[:, 0].astype(np.float32), np.zeros(n, dtype=bool))
                want, te, tr = reference_rewards(a.cfg, a.commands_cfg, cmd, st1, tq, prev, act, col)
                plain, tep, trp = reference_rewards(c.cfg, None, None, st1, tq, prev, act, col)
                assert np.array_equal(te, tea) and np.array_equal(tr, tra) and np.array_equal(tep, tec) and np.array_equal(trp, trc)
                swapped = reference_rewards(a.cfg, other, cmd, st1, tq, prev, act, col)[0]
                res["cmd"] = max(res["cmd"], float(np.abs(ra - want).max()))
                res["plain"] = max(res["plain"], float(np.abs(rc - plain).max()))
                res["scale"] = max(res["scale"], float(np.abs(want).max()))
                res["frames_differ"] = max(res["frames_differ"], float(np.abs(swapped - want)[~te].max(initial=0.0)))
                res["terminated"] += int(te.sum())
                prev = act
            assert np.array_equal(bits(a.commands()), bits(sched.cmd)) and sched.k.max() >= 2
            log("reward_kind %d frame %d: %d envs x %d steps, worst |reward - cmd_ref| %.3e, without commands worst |reward - env_ref| %.3e, largest |reward| %.2f, "
                "%d terminal rewards, the other frame would differ by up to %.3f" % (kind, frame, n, steps, res["cmd"], res["plain"], res["scale"], res["terminated"],
                                                                                    res["frames_differ"]))
            out[(kind, frame)] = res
            a.close(); c.close()
    return out
