"""What tests/test_gpu_feet.py and tools/gpu_feet_parity.py share: the feet configuration of the GPU tests, the landing scenario, the
fp64 reference reward of a step (tests/env_ref.py or tests/cmd_ref.py for the base, tests/feet_ref.py for the contact terms) on the
device's own states, joint torques, actions and contact read-out, and the measurement behind profiles/feet_parity.txt.
Test infrastructure only.

What was chosen (the issue leaves it to the tests):
  bodies      humanoid27.hbm: torso 1, head 2, shins 6 and 9, right foot 7, left foot 10, lower arms 12 and 15.  Four "feet" are the two feet
              and the two shins.  Penalised: the right foot (a collision count as soon as it stands), both lower arms, both thighs.
              Terminal: torso and head - or, in the variant "foot", the left foot, so that a touchdown is the terminating event.
  weights     contact_threshold 1 N; w_air_time 2 with a target of 0.05 s (the drop lasts 0 to 0.1 s); w_force -0.01 above force_max = a
              quarter of the model's weight, so a foot that carries half of it pays; w_stumble -1.5 at a ratio of 0.2, well below the
              floor's friction; w_collision -0.75.
  scenario    reset; every env's root lifted by 5 cm * (e % 16) / 15; every eighth env (e % 8 == 5) laid flat - pitched forward by a
              quarter turn, the root 0.3 m above the floor -, so that torso and head reach the floor inside the run and end episodes by
              contact; random actions in [-0.6, 0.6] from seed 21.  80 control steps (n_substeps 1: the flat envs' torsos reach the floor after about 55) or
              30 (n_substeps 4).
  base reward standupReward (reward_kind 0) with target_z out of reach and no time limit, so nothing but a contact ends an episode;
              self_collision_penalty 0, so the reference needs no collision detection of its own.  One case runs controlInputReward.
"""
import numpy as np

import cmd_lib
import cmd_ref
import env_ref
import feet_ref
from oracle_lib import HUMANOID_HBM

TORSO, HEAD, THIGH_R, SHIN_R, FOOT_R, THIGH_L, SHIN_L, FOOT_L, ARM_R, ARM_L = 1, 2, 5, 6, 7, 8, 9, 10, 12, 15
FEET = {1: (FOOT_R,), 2: (FOOT_R, FOOT_L), 4: (FOOT_R, FOOT_L, SHIN_R, SHIN_L)}
PENALISED = (FOOT_R, ARM_R, ARM_L, THIGH_R, THIGH_L)
TERMINAL = {"torso": (TORSO, HEAD), "foot": (FOOT_L,)}
WEIGHTS = dict(contact_threshold=1.0, w_air_time=2.0, air_time_target=0.05, w_force=-0.01, w_stumble=-1.5, stumble_ratio=0.2, w_collision=-0.75)
ZERO_WEIGHTS = dict(w_air_time=0.0, w_force=0.0, w_stumble=0.0, w_collision=0.0)
SEED = 21
# gate 2 and 3: the gate on with NO commands installed, so it reads hb_env_config.target_velocity - above air_cmd_min = 0.5 (open: 0.37 > 0.25)
# and below it (closed: 0.18 < 0.25)
TARGET_VELOCITY = {2: (0.6, 0.1), 3: (0.3, 0.3)}
bits = cmd_lib.bits


def model(hbmod):
    return hbmod.Model.load(HUMANOID_HBM)


def feet_options(hbmod, mdl, n_feet=2, gate=0, terminal="torso", observe=0, **kw):
    """the feet=dict(...) of the GPU tests: force_max a quarter of the model's weight (the default is twice the weight)"""
    import ctypes
    d = hbmod.engine.HbEnvFeet()
    assert hbmod.lib().hb_env_default_feet(mdl._h, ctypes.byref(d)) == 0
    opts = dict(WEIGHTS, bodies=FEET[n_feet], penalised=PENALISED, terminal=TERMINAL[terminal], force_max=d.force_max / 8.0, air_gate=1 if gate else 0,
                air_cmd_min=0.5, observe=int(observe))
    opts.update(kw)
    return opts


def env(hbmod, gpu, n, feet, commands=None, mdl=None, **kw):
    """a VecEnv of the scenario: feet a dict (feet_options) or None, commands cmd_lib.CMD-like or None"""
    kw.setdefault("target_z", 10.0)
    kw.setdefault("max_time", 0.0)
    kw.setdefault("auto_reset", 0)
    kw.setdefault("self_collision_penalty", 0.0)
    return hbmod.VecEnv(mdl if mdl is not None else model(hbmod), n, gpu, seed=7, commands=None if commands is None else dict(commands),
                        feet=None if feet is None else dict(feet), **kw)


def lift(hbmod, envs):
    """the scenario's start, after reset(): the same lifted (and, for every eighth env, flat) state in every env of `envs`"""
    a = envs[0]
    st = a.batch.get_state(hbmod.STATE_INTEGRATION)
    n = len(st)
    e = np.arange(n)
    st[:, 1 + 2] += (0.05 * (e % 16) / 15.0).astype(np.float32)
    flat = e % 8 == 5
    st[flat, 1 + 2] = 0.3
    st[flat, 1 + 3:1 + 7] = np.float32([np.sqrt(0.5), 0.0, np.sqrt(0.5), 0.0])  # a quarter turn about the y axis
    for v in envs:
        v.batch.set_state(hbmod.STATE_INTEGRATION, st)
    return st


def reference(cfg, C, cmd, F, rec, st1, torques, prev, act, wrench):
    """One step evaluation of every env in fp64: the base reward (env_ref, or cmd_ref with the commands cmd in force) plus the feet
    terms of F on the read-out `wrench`, through the Record rec (None: no feet).  Returns (reward, terminated, truncated, feet results)."""
    n = len(st1)
    no_col = np.zeros(n, dtype=bool)
    r, te, tr = cmd_lib.reference_rewards(cfg, C, cmd, st1, torques, prev, act, no_col)
    if rec is None:
        return r, te, tr, None
    xy = cmd[:, :2] if C is not None else np.tile(np.float32([cfg.target_velocity[0], cfg.target_velocity[1]]), (n, 1))
    res = rec.step(wrench, st1[:, 0].astype(np.float32), xy)
    for e, f in enumerate(res):
        if not te[e]:
            r[e] += f["reward"]
        if f["terminated"]:
            te[e] = True
        if te[e]:
            r[e] = cfg.terminal_reward
    return r, te, tr, res


def run_scenario(hbmod, gpu, n=64, n_substeps=1, n_feet=2, gate=0, terminal="torso", reward_kind=0, steps=None, twin=True, log=None):
    """The landing scenario with every term on.  After every step: masks, contact flags and t_last of the device against feet_ref bit for
    bit, terminated and truncated equal, and the worst |reward - reference| collected - next to the same figure of a feet-less twin
    (contact_forces=True) stepped with the same actions, whose states must stay equal bit for bit.  Returns the figures and the
    reference's own counts of what happened."""
    mdl = model(hbmod)
    steps = steps if steps is not None else (80 if n_substeps == 1 else 30)
    commands = cmd_lib.CMD if gate == 1 else None
    kw = dict(n_substeps=n_substeps, reward_kind=reward_kind)
    if gate >= 2:
        kw.update(target_velocity=TARGET_VELOCITY[gate])
    if reward_kind == 1:
        kw.update(w_vvel=1.5, upright_tol=10.0, min_z_grounded=-1.0)  # (controlInputReward's own fall test out of reach: contacts alone end episodes)
    a = env(hbmod, gpu, n, feet_options(hbmod, mdl, n_feet, gate, terminal), commands, mdl, **kw)
    c = env(hbmod, gpu, n, None, commands, mdl, contact_forces=True, **kw) if twin else None
    both = [a] + ([c] if twin else [])
    for v in both:
        v.reset()
    lift(hbmod, both)
    Fc = a.feet_cfg
    rec = feet_ref.Record(Fc, n, a.batch.get_state(hbmod.STATE_TIME).reshape(-1))
    sched = cmd_ref.Schedule(a.commands_cfg, n) if commands else None
    t_last, contact = a.batch.feet()
    assert np.array_equal(bits(t_last), bits(rec.t_last)) and np.array_equal(contact, rec.contact())
    rng = np.random.default_rng(SEED)
    prev = np.zeros((n, mdl.nu), np.float32)
    out = dict(feet=0.0, plain=0.0, scale=0.0, touchdowns=np.zeros(n_feet, dtype=int), impact=0, stumble=0, collision=0, terminated=0, gated=0, steps=steps, n=n)
    for t in range(steps):
        act = cmd_lib.actions(rng, n, mdl.nu, 0.6)
        _, ra, tea, tra, _ = a.step_arrays(act)
        st1 = a.batch.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
        wrench = a.batch.body_contact()
        tq = a.batch.env_joint_torques()[:, 6:]
        cmd = sched.step(st1[:, 0].astype(np.float32), np.zeros(n, dtype=bool)) if commands else None
        want, te, tr, res = reference(a.cfg, a.commands_cfg, cmd, Fc, rec, st1, tq, prev, act, wrench)
        t_last, contact = a.batch.feet()
        assert np.array_equal(contact, rec.contact()), ("contact flags", t)
        assert np.array_equal(bits(t_last), bits(rec.t_last)), ("t_last", t)
        assert np.array_equal(te, tea.astype(bool)) and np.array_equal(tr, tra.astype(bool)), ("terminated / truncated", t)
        out["feet"] = max(out["feet"], float(np.abs(ra - want).max()))
        out["scale"] = max(out["scale"], float(np.abs(want).max()))
        for f in res:
            paid = [td and f["gate"] for td in f["touchdown"]]
            out["touchdowns"] += np.array(paid, dtype=int)
            out["gated"] += int(any(f["touchdown"]) and not f["gate"])
            out["impact"] += int(f["force"] != 0.0)
            out["stumble"] += int(f["stumble"])
            out["collision"] += int(f["collisions"] > 0)
            out["terminated"] += int(f["terminated"])
        if twin:
            _, rc, tec, trc, _ = c.step_arrays(act)
            assert np.array_equal(bits(c.batch.get_state(hbmod.STATE_INTEGRATION)), bits(a.batch.get_state(hbmod.STATE_INTEGRATION))), ("the terms moved the physics", t)
            assert np.array_equal(bits(c.batch.body_contact()), bits(wrench))
            plain, tep, trp, _ = reference(c.cfg, c.commands_cfg, cmd, None, None, st1, c.batch.env_joint_torques()[:, 6:], prev, act, None)
            assert np.array_equal(tep, tec.astype(bool)) and np.array_equal(trp, trc.astype(bool))
            out["plain"] = max(out["plain"], float(np.abs(rc - plain).max()))
        prev = act
    if log:
        log("n_substeps %d, %d feet, gate %d, terminal %s, reward_kind %d: %d envs x %d steps, worst |reward - reference| %.3e, feet-less twin %.3e, "
            "largest |reward| %.2f; rewarded touchdowns per foot %s (%d more gated off), env-steps with an impact term %d, a stumble %d, a collision %d, "
            "terminated by contact %d" % (n_substeps, n_feet, gate, terminal, reward_kind, n, steps, out["feet"], out["plain"], out["scale"], out["touchdowns"].tolist(),
                                          out["gated"], out["impact"], out["stumble"], out["collision"], out["terminated"]))
    for v in both:
        v.close()
    return out


# (n_substeps, n_feet, gate, terminal, reward_kind): both substep counts, 1, 2 and 4 feet, the gate off, on with commands (1) and on
# with the target velocity of hb_env_config (2: open), both ways of ending an episode, both reward kinds
CASES = [(1, 2, 0, "torso", 0), (4, 2, 1, "torso", 0), (1, 1, 1, "torso", 0), (4, 1, 0, "foot", 0), (1, 4, 0, "torso", 1), (4, 4, 1, "foot", 0), (1, 2, 1, "foot", 1),
         (4, 2, 2, "torso", 0)]


def measure_parity(hbmod, gpu, log=print):
    """every case of CASES: {case: run_scenario's figures}"""
    return {case: run_scenario(hbmod, gpu, 64, *case, log=log) for case in CASES}
