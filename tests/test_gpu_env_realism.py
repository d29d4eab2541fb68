"""the sensor / actuation realism of CPUEnv on the device (hb_env_randomization) —
action noise and delay (cpu_env.py:656-674), observation noise and delay lines (:465-545), pushes (:612-654),
controlInputReward semantics (reward_functions.py:116-245) and the reset-until-collision-free protocol
(:374-416) — against the numpy restatement in tests/env_ref.py."""
import numpy as np
import pytest

import dr_ref
from env_ref import RealismRef, control_input_reward, obs_from_state
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu
STATE_XFRC = 1 << 7  # mjSTATE_XFRC_APPLIED (engine.STATE_XFRC_APPLIED)


def make_env(hbmod, m, n, gpu, **kw):
    rkw = {k: kw.pop(k) for k in list(kw) if k in ("seed", "frozen_noise", "push_enabled", "min_delay", "max_delay", "factor",
                                                    "joint_angle_noise", "joint_velocity_noise", "gyro_noise", "imu_noise", "action_noise")}
    env = hbmod.VecEnv(m, n, gpu, auto_reset=0, max_time=0.0, target_z=10.0, **kw)
    R = env.batch.env_default_randomization()
    R.push_enabled = 0
    for k, v in rkw.items():
        setattr(R, k, v)
    env.batch.env_randomize(R)
    return env, R


def test_noise_and_delay_lines_match_numpy(hbmod, humanoid_model, gpu):
    m = humanoid_model
    n, T, off = 6, 40, 0
    env, R = make_env(hbmod, m, n, gpu, seed=11, min_delay=0.0, max_delay=0.06)  # 0..12 steps of 5 ms
    refs = [RealismRef(R, off + e, m.nu, 21, 17, 0.005) for e in range(n)]
    assert len({tuple(r.delay) for r in refs}) > 1 and max(max(r.delay) for r in refs) >= 6
    obs = env.reset()
    b = env.batch
    st = b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
    for e in range(n):
        assert np.allclose(obs[e], refs[e].observe(st[e, 1:1 + m.nq], st[e, 1 + m.nq:1 + m.nq + m.nv]), atol=2e-5)
    rng = np.random.default_rng(0)
    for t in range(T):
        act = rng.uniform(-1, 1, size=(n, m.nu)).astype(np.float32)
        obs, rew, term, trunc, info = env.step_arrays(act)
        st = b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
        for e in range(n):
            ref = refs[e].observe(st[e, 1:1 + m.nq], st[e, 1 + m.nq:1 + m.nq + m.nv])
            assert np.abs(obs[e] - ref).max() < 5e-5, (t, e, np.abs(obs[e] - ref).max())


def test_action_delay_is_a_pure_shift(hbmod, humanoid_model, gpu):
    """No noise, a fixed delay of d control steps: the physics sees zeros for d steps, then action[t - d] — the same
    states, bit for bit, as a plain env fed the shifted tape."""
    m = humanoid_model
    n, T, d = 5, 30, 4
    env, R = make_env(hbmod, m, n, gpu, min_delay=d * 0.005, max_delay=d * 0.005, action_noise=0.0)
    plain = hbmod.VecEnv(m, n, gpu, auto_reset=0, max_time=0.0, target_z=10.0)
    env.reset(); plain.reset()
    rng = np.random.default_rng(1)
    tape = rng.uniform(-1, 1, size=(T, n, m.nu)).astype(np.float32)
    for t in range(T):
        env.step_arrays(tape[t])
        plain.step_arrays(tape[t - d] if t >= d else np.zeros((n, m.nu), np.float32))
        assert np.array_equal(env.batch.get_state(hbmod.STATE_INTEGRATION), plain.batch.get_state(hbmod.STATE_INTEGRATION)), t


def test_noise_statistics_and_frozen_mode(hbmod, humanoid_model, gpu):
    m = humanoid_model
    n, T = 256, 12
    zeros = np.zeros((n, m.nu), np.float32)
    env, R = make_env(hbmod, m, n, gpu, seed=5, min_delay=0.0, max_delay=0.0, factor=0.5)
    env.reset()
    errs = []
    for t in range(T):
        obs, *_ = env.step_arrays(zeros)
        true, *_ = env.batch.obs(want_reward=False)
        errs.append(obs - true)
    errs = np.array(errs)  # [T, n, 48]
    assert abs(errs[..., :21].std() / (0.5 * R.joint_angle_noise) - 1) < 0.05 and abs(errs[..., :21].mean()) < 2e-3 * R.joint_angle_noise * 10
    assert abs(errs[..., 21:42].std() / (0.5 * R.joint_velocity_noise) - 1) < 0.05
    assert abs(errs[..., 42:45].std() / (0.5 * R.gyro_noise) - 1) < 0.1
    assert 0.2 * 0.5 * R.imu_noise < errs[..., 45:48].std() < 3 * 0.5 * R.imu_noise  # quaternion noise through the rotation
    assert np.abs(errs[0] - errs[1]).max() > 1e-4  # fresh noise every step
    # frozen: the reference's unsplit key - the same draw at every step of an episode
    env2, _ = make_env(hbmod, m, 16, gpu, seed=5, min_delay=0.0, max_delay=0.0, frozen_noise=1, imu_noise=0.0)
    env2.reset()
    z16 = np.zeros((16, m.nu), np.float32)
    e1 = env2.step_arrays(z16)[0] - env2.batch.obs(want_reward=False)[0]
    e2 = env2.step_arrays(z16)[0] - env2.batch.obs(want_reward=False)[0]
    assert np.abs(e1[:, :45]).max() > 1e-3 and np.allclose(e1[:, :45], e2[:, :45], atol=2e-6)


def test_push_schedule_matches_numpy(hbmod, humanoid_model, gpu):
    m = humanoid_model
    n, T = 4, 900  # 4.5 s: at least one complete push per env
    env, R = make_env(hbmod, m, n, gpu, seed=3, push_enabled=1, min_delay=0.0, max_delay=0.0)
    env.reset()
    refs = [RealismRef(R, e, m.nu, 21, 17, 0.005) for e in range(n)]
    zeros = np.zeros((n, m.nu), np.float32)
    seen = 0
    for t in range(T):
        time = env.batch.time.copy()
        env.step_arrays(zeros)
        xf = env.batch.get_state(STATE_XFRC).reshape(n, 17, 6)
        for e in range(n):
            want = refs[e].push_update(np.float32(time[e]))
            f = np.zeros((17, 6))
            if want is not None:
                f[want[0], 0], f[want[0], 1] = want[1], want[2]
                seen += 1
                assert 5.0 - 1e-4 <= np.hypot(want[1], want[2]) <= 15.0 + 1e-4
            assert np.allclose(xf[e], f, atol=1e-4), (t, e)
    assert seen > 4 * 10  # every env was pushed for at least 10 steps (0.05 s)


def test_control_input_reward_semantics(hbmod, humanoid_model, gpu):
    m = humanoid_model
    n = 10
    env = hbmod.VecEnv(m, n, gpu, auto_reset=0, max_time=0.0575, reward_kind=1, w_vvel=5.0, w_hvel=15.0)
    cfg = env.cfg
    env.reset()
    b = env.batch
    o = Oracle()
    rng = np.random.default_rng(4)
    prev = np.zeros((n, m.nu))
    fell = False
    for t in range(14):
        act = rng.uniform(-1.5, 1.5, size=(n, m.nu)).astype(np.float32)
        st = b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
        obs, rew, term, trunc, info = env.step_arrays(act)
        st1 = b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
        for e in range(n):
            o.reset()
            o.qpos[:] = st[e, 1:1 + m.nq]; o.qvel[:] = st[e, 1 + m.nq:1 + m.nq + m.nv]; o.qacc_warmstart[:] = st[e, 1 + m.nq + m.nv:]
            o.ctrl[:] = act[e]
            o.forward()
            torques = (o.qfrc_smooth + o.qfrc_constraint)[6:]
            selfcol = any(c["geom1"] != 0 for c in o.contacts())
            r_ref, te, tr = control_input_reward(cfg, st1[e, 0], st1[e, 1:1 + m.nq], st1[e, 1 + m.nq:1 + m.nq + m.nv], torques, prev[e], act[e].astype(np.float64), selfcol)
            assert abs(rew[e] - r_ref) <= 2e-3 * max(1.0, abs(r_ref)), (t, e, rew[e], r_ref)
            assert bool(term[e]) == te and bool(trunc[e]) == tr
        assert trunc.all() == (t >= 11) and trunc.any() == (t >= 11)  # the time limit (12 steps of 5 ms) is a truncation here
        prev = act.astype(np.float64)
    # a toppled torso is terminal with the terminal reward
    q = b.get_state(hbmod.STATE_QPOS, dtype=np.float64)
    q[:, 3:7] = np.array([0.7071, 0.7071, 0.0, 0.0])  # lying on the side
    b.set_state(hbmod.STATE_QPOS, q.astype(np.float32))
    obs, rew, term, trunc, info = env.step_arrays(np.zeros((n, m.nu), np.float32))
    assert term.all() and np.allclose(rew, cfg.terminal_reward)


def test_reset_until_collision_free(hbmod, humanoid_model, gpu):
    """reset_collision_mode = 1 (the reference's any-contact test): every env takes the settle step; envs whose step
    ends in contact are re-drawn (new episode number), at most 8 times, without disturbing the others."""
    m = humanoid_model
    n = 64
    env = hbmod.VecEnv(m, n, gpu, auto_reset=0, max_time=0.0, target_z=10.0, reset_collision_mode=1)
    env.reset()
    b = env.batch
    ncon, _, _ = b.counts()
    assert np.allclose(b.time, 0.005)        # exactly one settle step each, whatever the number of draws
    # the standing humanoid's feet touch the floor unless the height perturbation lifted it: both kinds occur,
    # and an env only ever stops collision-free or at the draw limit
    assert (ncon == 0).any()
    plain = hbmod.VecEnv(m, n, gpu, auto_reset=0, max_time=0.0, target_z=10.0)
    plain.reset()
    assert not np.allclose(plain.batch.qpos, b.qpos)  # re-drawn envs do not sit at their first draw
    # mode 2: only self-collisions count - the unperturbed reset pose has none, so one draw suffices and the
    # state is the reset pose advanced by one zero-control step
    env2 = hbmod.VecEnv(m, n, gpu, randomization_factor=0.0, auto_reset=0, max_time=0.0, target_z=10.0, reset_collision_mode=2)
    env2.reset()
    plain0 = hbmod.VecEnv(m, n, gpu, randomization_factor=0.0, auto_reset=0, max_time=0.0, target_z=10.0)
    plain0.reset()
    plain0.step_arrays(np.zeros((n, m.nu), np.float32))
    assert np.array_equal(env2.batch.get_state(hbmod.STATE_INTEGRATION), plain0.batch.get_state(hbmod.STATE_INTEGRATION))


def test_randomize_argument_checks_and_off_switch(hbmod, humanoid_model, gpu):
    m = humanoid_model
    b = hbmod.Batch(m, 8, gpu)
    R = b.env_default_randomization()
    assert abs(R.joint_angle_noise - np.deg2rad(2)) < 1e-7 and R.push_enabled == 1 and R.min_delay == pytest.approx(0.01)
    R.max_delay = 1.0  # 200 steps of 5 ms: beyond the 63-slot rings
    with pytest.raises(hbmod.HbError):
        b.env_randomize(R)
    R.max_delay = 0.05
    b.env_randomize(R)
    b.env_reset()
    o1 = b.env_step(np.zeros((8, m.nu), np.float32))[0]
    b.env_randomize(None)  # off again: observations are the true ones
    b.env_reset()
    o2 = b.env_step(np.zeros((8, m.nu), np.float32))[0]
    true, *_ = b.obs(want_reward=False)
    assert np.allclose(o2, true, atol=1e-6) and not np.allclose(o1, o2)


def test_domain_randomization_draws_and_physics(hbmod, humanoid_model, gpu):
    """hb_domain_randomization: per-env masses, armature, joint limits, actuator force ranges and floor friction are
    drawn inside the reference's bounds, differ between envs and episodes, and the physics uses them — one step from
    identical states matches the fp64 oracle whose model arrays were set to the env's parameters."""
    m = humanoid_model
    n = 6
    env = hbmod.VecEnv(m, n, gpu, auto_reset=0, max_time=0.0, target_z=10.0)
    b = env.batch
    assert b.env_domain_params() is None
    D = b.env_default_domain_randomization()
    assert D.friction_min_mult == pytest.approx(0.5) and D.max_external_mass == pytest.approx(0.2) and D.kp_nominal == 0.0
    D.seed = 9
    D.stiffness_max_change = 2.0   # the reference leaves stiffness at 0; exercised here
    D.max_mass_change = 0.5        # larger than the reference's 0.05 kg so that the physics difference is far above fp32 noise
    b.env_domain_randomize(D)
    env.reset()
    P = b.env_domain_params()
    o = Oracle()
    base_mass = o.marr("body_mass").copy(); base_arm = o.marr("dof_armature").copy(); base_rng = o.marr("jnt_range").copy()
    base_frc = o.marr("actuator_forcerange").copy(); base_stiff = o.marr("jnt_stiffness").copy(); base_margin = o.marr("jnt_margin").copy()
    base_fric = o.marr("geom_friction").copy()
    L = dr_ref.layout(m, P.shape[1])
    assert P.shape[1] == L["stride"] and L["nlimcand"] == 2 * 21 + 2 * 2  # 21 limited hinges + 2 limited tendons, lower and upper each
    mass = P[:, L["mass"]:L["mass"] + 17]
    assert np.all(np.abs(mass[:, 1:] - base_mass[1:]) <= 0.5 + 0.2 + 1e-5) and np.all(mass[:, 1:] >= 1e-5) and mass[:, 1:].std(axis=0).min() > 0
    arm = P[:, L["arm"]:L["arm"] + m.nv]
    assert np.allclose(arm[:, :6], base_arm[:6]) and np.all(arm[:, 6:] >= base_arm[6:] - 1e-9) and np.all(arm[:, 6:] <= base_arm[6:] + 0.0005 + 1e-7)
    fric = P[:, L["fric"]]
    assert np.all((fric >= 0.5 - 1e-6) & (fric <= 1.0 + 1e-6)) and fric.std() > 0
    frc = P[:, L["frc"]:L["frc"] + 2 * m.nu]
    assert np.all(np.abs(frc - base_frc) <= 0.05 + 1e-6)
    gains = P[:, L["gain"]:L["gain"] + m.nu]
    assert np.allclose(gains, o.marr("actuator_gainprm"))  # kp_nominal = 0: the model's gains
    # physics: teacher-forced steps against the oracle carrying env e's parameters
    lim_joint = [j for j in range(1, 22)]  # joints 1..21 are the limited hinges, in constraint order
    rng = np.random.default_rng(8)
    for t in range(12):
        act = rng.uniform(-1, 1, size=(n, m.nu)).astype(np.float32)
        st = b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
        env.step_arrays(act)
        q1 = b.qpos
        for e in range(n):
            o.marr("body_mass")[:] = mass[e]
            o.marr("dof_armature")[:] = arm[e]
            o.marr("jnt_stiffness")[1:] = P[e, L["stiff"] + 6:L["stiff"] + m.nv]
            for k, j in enumerate(lim_joint):
                o.marr("jnt_margin")[j] = P[e, L["lmargin"] + 2 * k]
                o.marr("jnt_range")[2 * j] = P[e, L["lrange"] + 2 * k]
                o.marr("jnt_range")[2 * j + 1] = P[e, L["lrange"] + 2 * k + 1]
            o.marr("actuator_forcerange")[:] = frc[e]
            o.marr("geom_friction")[0] = base_fric[0] * fric[e]
            o.reset()
            o.qpos[:] = st[e, 1:1 + m.nq]; o.qvel[:] = st[e, 1 + m.nq:1 + m.nq + m.nv]; o.qacc_warmstart[:] = st[e, 1 + m.nq + m.nv:]
            o.ctrl[:] = act[e]
            o.step()
            assert np.abs(q1[e] - o.qpos).max() < 2e-5, (t, e, np.abs(q1[e] - o.qpos).max())
    # and the parameters matter: the unrandomised oracle does not reproduce these steps
    o.marr("body_mass")[:] = base_mass; o.marr("dof_armature")[:] = base_arm; o.marr("jnt_range")[:] = base_rng; o.marr("actuator_forcerange")[:] = base_frc
    o.marr("jnt_stiffness")[:] = base_stiff; o.marr("jnt_margin")[:] = base_margin; o.marr("geom_friction")[:] = base_fric
    o.reset()
    o.qpos[:] = st[0, 1:1 + m.nq]; o.qvel[:] = st[0, 1 + m.nq:1 + m.nq + m.nv]; o.qacc_warmstart[:] = st[0, 1 + m.nq + m.nv:]
    o.ctrl[:] = act[0]
    o.step()
    assert np.abs(q1[0] - o.qpos).max() > 2e-5
    # the draw itself against the numpy restatement of the generator (streams 16 = per-limb change, 17 = attached mass)
    from env_ref import rng_uniform
    for e in range(n):
        want = np.array([max(1e-5, base_mass[bd] + (2 * float(rng_uniform(9, e, 0, 0, 16, bd)) - 1) * 0.5) for bd in range(17)])
        want[0] = 0.0
        bd = 1 + min(15, int(np.float32(rng_uniform(9, e, 0, 0, 17, 0)) * np.float32(16)))
        want[bd] += float(rng_uniform(9, e, 0, 0, 17, 1)) * 0.2
        assert np.allclose(mass[e], want, atol=2e-6), (e, np.abs(mass[e] - want).max())


def test_domain_randomization_redraws_per_episode_and_switches_off(hbmod, humanoid_model, gpu):
    m = humanoid_model
    n = 8
    env = hbmod.VecEnv(m, n, gpu, domain_randomization=True, seed=4, max_time=0.0149, target_z=10.0)  # 3-step episodes, auto-reset
    env.reset()
    p0 = env.batch.env_domain_params().copy()
    assert np.abs(p0[0] - p0[1]).max() > 1e-4  # envs differ
    zeros = np.zeros((n, m.nu), np.float32)
    for t in range(3):
        obs, rew, term, trunc, info = env.step_arrays(zeros)
    assert term.all()
    p1 = env.batch.env_domain_params().copy()
    assert np.abs(p1 - p0).max() > 1e-4 and np.isfinite(p1).all()  # new episode, new draw
    # same seed, same envs, same episode numbers: reproducible
    env_b = hbmod.VecEnv(m, n, gpu, domain_randomization=True, seed=4, max_time=0.0149, target_z=10.0)
    env_b.reset()
    assert np.array_equal(env_b.batch.env_domain_params(), p0)
    env.set_attr("randomization_factor", 0.0)  # factor 0 removes the layer
    assert env.batch.env_domain_params() is None
    D = env.batch.env_default_domain_randomization()
    D.range_max_change = -1.0
    with pytest.raises(hbmod.HbError):
        env.batch.env_domain_randomize(D)


def test_floor_heightmap_randomization(hbmod, gpu):
    """CPUEnv._randomize_floor_heightmap (cpu_env.py:267-280) on the device: every env gets its own 8 x 8 elevation map,
    smooth noise shifted and scaled to [0, MIN + factor (MAX - MIN)], redrawn per episode; the collision kernel reads the
    env's own map (one step from identical states matches the oracle whose hfield_data was set to that env's map)."""
    from oracle_lib import HFIELD_HBM as path
    m = hbmod.Model.load(path)
    n = 6
    env = hbmod.VecEnv(m, n, gpu, auto_reset=0, max_time=0.0, target_z=10.0)
    b = env.batch
    D = b.env_default_domain_randomization()
    assert D.floor_bump_min == 0.0 and D.floor_bump_max == pytest.approx(0.1)  # MIN / MAX_FLOOR_BUMP_HEIGHT
    # only the floor varies here, so that the oracle needs nothing but the map
    D.seed = 21
    D.friction_min_mult = D.friction_max_mult = 1.0
    D.max_mass_change = D.max_external_mass = D.armature_max_change = D.margin_max_change = D.range_max_change = D.force_limit_max_change = 0.0
    D.floor_bump_max = 0.3  # taller than the reference's 0.1 m so that the terrain clearly matters
    b.env_domain_randomize(D)
    env.reset()
    P = b.env_domain_params()
    hf = P[:, -64:].reshape(n, 8, 8)
    assert np.allclose(hf.min(axis=(1, 2)), 0.0, atol=1e-7) and np.allclose(hf.max(axis=(1, 2)), 0.3, atol=1e-6)
    assert np.abs(hf[0] - hf[1]).max() > 0.05                              # envs differ
    assert np.abs(np.diff(hf, axis=2)).mean() < 0.5 * hf.std() * 2          # smooth: neighbours are closer than random nodes would be
    o = Oracle(path)
    zero = np.zeros((n, m.nu), np.float32)
    contacts = 0
    for t in range(260):
        take = t > 60 and t % 12 == 0
        if take:
            st = b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
        env.step_arrays(zero)
        if take:
            q = b.qpos.astype(np.float64)
            nc, ne, _ = b.counts()
            for e in range(n):
                o.reset()
                o.marr("hfield_data")[:] = hf[e].ravel()
                o.qpos[:] = st[e, 1:1 + m.nq]; o.qvel[:] = st[e, 1 + m.nq:1 + m.nq + m.nv]; o.qacc_warmstart[:] = st[e, 1 + m.nq + m.nv:]
                o.ctrl[:] = 0
                o.step()
                assert (o.ncon, o.nefc) == (nc[e], ne[e]), (t, e, o.ncon, nc[e])
                contacts += o.ncon
                assert (np.abs(q[e] - o.qpos) / np.maximum(1, np.abs(o.qpos))).max() <= 1e-4
    assert contacts > 30
    # same seed: the same maps (episode numbering restarts at an explicit reset); another seed: other maps; off: none
    env.reset()
    assert np.array_equal(b.env_domain_params()[:, -64:], P[:, -64:])
    D.seed = 22
    b.env_domain_randomize(D)
    env.reset()
    assert np.abs(b.env_domain_params()[:, -64:] - P[:, -64:]).max() > 0.02
    b.env_domain_randomize(None)
    assert b.env_domain_params() is None
