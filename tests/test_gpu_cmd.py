"""Per-env velocity commands on the GPU (include/hb.h: hb_env_commands): drawn, tracked and observed on the device, against
tests/cmd_ref.py.

Model: humanoid27.hbm (48 observations, 21 actuators, control step 5 ms); with observed commands a row has 51 entries.  64 envs unless a
test says otherwise; tests/cmd_lib.py's configuration: a draw every three control steps, a quarter of the draws the zero command, the
heading frame.

Bounds:
  bits     Batch.commands(), the command columns of every row and tape, the neutral configuration against a batch without one, replays of
           recorded actions: equality;
  reward   PARITY_WORST is the worst |reward - cmd_ref| that tools/gpu_cmd_parity.py measured over both frames and both reward kinds
           (profiles/cmd_parity.txt, next to what the reward without commands shows against env_ref.py on the same states); every reward
           check here asserts 8 times that.  A handful of fp32 operations and two expf on a reward of about 30: half an ulp of the sum is
           1.9e-6.
"""
import numpy as np
import pytest

import cmd_lib
import cmd_ref
from cmd_lib import CMD, actions, bits
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

NOBS, NU = 48, 21
PARITY_WORST = 3.631e-06  # profiles/cmd_parity.txt
BOUND = 8 * PARITY_WORST


def _run_schedule(env, sched, steps, rng):
    """steps env steps with random actions: after each, Batch.commands() and the command columns of the row are the reference's"""
    n, col = env.num_envs, env.obs_layout()["command"]
    for t in range(steps):
        act = actions(rng, n, NU)
        o, r, te, tr, _ = env.step_arrays(act)
        sched.step(env.batch.time.astype(np.float32), te | tr)
        assert np.array_equal(bits(env.commands()), bits(sched.cmd)), t
        assert np.array_equal(bits(o[:, col]), bits(sched.cmd)), t


@pytest.mark.parametrize("n", [64, 17])
def test_draws(hbmod, gpu, n):
    """after reset and after 12 steps with a draw every 3: the commands are the reference's bit for bit (17 envs: a part-filled block of
    the env kernel, 16 envs each)"""
    env = cmd_lib.env(hbmod, gpu, n, max_time=0.0)
    assert env.nobs == env.batch.env_nobs == NOBS + 3 and env.obs_layout() == {"base": slice(0, NOBS), "command": slice(NOBS, NOBS + 3)}
    sched = cmd_ref.Schedule(env.commands_cfg, n)
    o = env.reset()
    assert np.array_equal(bits(env.commands()), bits(sched.cmd)) and np.array_equal(bits(o[:, NOBS:]), bits(sched.cmd))
    assert np.array_equal(bits(env.batch.obs(want_reward=False)[0][:, NOBS:]), bits(sched.cmd))  # (hb_get_obs: the same columns)
    _run_schedule(env, sched, 12, np.random.default_rng(1))
    assert (sched.k >= 4).all() and (sched.ep == 0).all()  # (draw 0 and one about every three steps since)
    zero = ~sched.cmd.any(axis=1)
    print("\n  %d envs: %d zero commands after draw 4" % (n, int(zero.sum())))
    env.close()


def test_draws_after_a_reset_with_redraws(hbmod, gpu):
    """hb_env_reset with reset_collision_mode on runs masked re-draws of the envs that start in contact: every env's command is draw 0
    of the episode number it ended up with (found among the eight the reset can assign: without zero commands draws are distinct), and a
    second reset gives the same commands again"""
    n = 64
    env = cmd_lib.env(hbmod, gpu, n, dict(CMD, zero_fraction=0.0), max_time=0.0, reset_collision_mode=1)
    C = env.commands_cfg
    o = env.reset()
    got = env.commands()
    eps = np.full(n, -1)
    for e in range(n):
        fits = [ep for ep in range(9) if np.array_equal(bits(cmd_ref.draw(C, e, ep, 0)), bits(got[e]))]
        assert len(fits) == 1, (e, fits, got[e])
        eps[e] = fits[0]
    print("\n  episode numbers after the reset: %s" % np.bincount(eps).tolist())
    assert (eps == 0).any() and (eps > 0).any(), "the re-draws touched no subset of the envs"
    assert np.array_equal(bits(o[:, NOBS:]), bits(got))
    sched = cmd_ref.Schedule(C, n)
    sched.reset(eps)
    _run_schedule(env, sched, 4, np.random.default_rng(2))
    assert np.array_equal(bits(env.reset()[:, NOBS:]), bits(got))
    env.close()


def test_schedule_terminal_rows_and_rewards(hbmod, gpu):
    """episodes of five steps (controlInputReward: the time limit truncates, the reward keeps its value), a draw every three: the command
    columns of obs[t + 1], the terminal rows and the rewards.  A twin that does not reset stands in the state the first episode ends in."""
    n = 64
    kw = dict(reward_kind=1, max_time=0.0249)
    a, c = cmd_lib.env(hbmod, gpu, n, **kw), cmd_lib.env(hbmod, gpu, n, auto_reset=0, **kw)
    m, o = a.model, Oracle()
    sched = cmd_ref.Schedule(a.commands_cfg, n)
    assert np.array_equal(a.reset(), c.reset())
    rng = np.random.default_rng(3)
    prev = np.zeros((n, NU), np.float32)
    col = slice(NOBS, NOBS + 3)
    worst, ends, changed = 0.0, 0, 0
    for t in range(12):
        act = actions(rng, n, NU, 0.3)
        before = sched.cmd.copy()
        st0 = a.batch.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
        oa, ra, te, tr, _ = a.step_arrays(act)
        done = te | tr
        if t < 5:  # (until the first episode ends the twin is in the same state, and keeps it where a resets)
            oc, rc, tec, trc, _ = c.step_arrays(act)
            st1 = c.batch.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
            assert np.array_equal(done, tec | trc) and done.all() == (t == 4) and done.any() == (t == 4)
        else:
            st1 = a.batch.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
        # the schedule runs on the times of the states the step ended in (the twin's, where a was reset in place)
        old = sched.step(st1[:, 0].astype(np.float32) if t < 5 else a.batch.time.astype(np.float32), done)
        assert np.array_equal(bits(old), bits(before))
        assert np.array_equal(bits(oa[:, col]), bits(sched.cmd)), t
        assert np.array_equal(bits(a.commands()), bits(sched.cmd)), t
        if done.any():
            ends += 1
            assert (sched.k[done] == 1).all()
            tobs = a.batch.env_terminal_obs()
            assert np.array_equal(bits(tobs[done][:, col]), bits(old[done])), t   # the command in force during the last step
            changed += int((old[done] != sched.cmd[done]).any(axis=1).sum())
        if t < 5 or not done.any():
            # reward[t] against the command in force during the step, on the state the step ended in
            tq = (c if t < 5 else a).batch.env_joint_torques()[:, 6:]
            want, wte, wtr = cmd_lib.reference_rewards(a.cfg, a.commands_cfg, old, st1, tq, prev, act, cmd_lib.self_collisions(o, m, st0, act))
            assert np.array_equal(wte, te) and np.array_equal(wtr, tr) and not te.any()
            d = float(np.abs(ra - want).max())
            worst = max(worst, d)
            moved = (old != sched.cmd).any(axis=1)
            if moved.any():  # (the new command would have given another reward: the step was not rewarded against it)
                new = cmd_lib.reference_rewards(a.cfg, a.commands_cfg, sched.cmd, st1, tq, prev, act, np.zeros(n, dtype=bool))[0]
                assert np.abs(new - want)[moved].max() > 100 * BOUND
            print("\n  step %d: worst |reward - cmd_ref| %.3e (bound %.3e), %d commands replaced" % (t, d, BOUND, int(moved.sum())), end="")
            assert d <= BOUND, t
        prev = np.where(done[:, None], 0.0, act).astype(np.float32)
    assert ends == 2 and changed > n and worst <= BOUND
    a.close(); c.close()


def test_reward_parity(hbmod, gpu):
    """both frames, both reward kinds, from a perturbed reset with a yawed root: within 8 times the measured worst of cmd_ref in fp64"""
    res = cmd_lib.measure_parity(hbmod, gpu, log=lambda s: print("\n  " + s, end=""))
    for key, r in res.items():
        assert r["frames_differ"] > 0.1, key   # (the roots are yawed: the frame matters)
        assert r["cmd"] <= BOUND, (key, r)


def test_neutral_configuration_is_the_plain_path(hbmod, gpu):
    """frame 0, both ends of each range at target_velocity, no zero draws, no yaw weight, not observed - and a configuration installed and
    removed again: rewards, flags and observations of 20 steps are those of a batch that never had one, bit for bit, from the same kernels
    in the same number of launches"""
    n = 64
    tv = (0.3, -0.2)
    neutral = dict(frame=0, vx_min=tv[0], vx_max=tv[0], vy_min=tv[1], vy_max=tv[1], yaw_min=0.0, yaw_max=0.0, zero_fraction=0.0, w_yaw=0.0, observe=0, resample_time=0.015)
    envs = [cmd_lib.env(hbmod, gpu, n, cm, max_time=0.0349, realism=True, domain_randomization=True) for cm in (None, neutral, dict(CMD))]
    envs[2].batch.commands_configure(None)
    with pytest.raises(hbmod.HbError, match="no command configuration"):
        envs[2].batch.commands()
    rows = []
    for env in envs:
        env.cfg.target_velocity[0], env.cfg.target_velocity[1] = tv
        env.batch.env_configure(env.cfg)
        assert env.batch.env_nobs == NOBS
        rng = np.random.default_rng(4)
        out = [env.batch.env_reset()]
        rew, flags, launches, names = [], [], [], set()
        for t in range(20):
            l0 = env.batch.step_launches()
            o, r, te, tr = env.batch.env_step(actions(rng, n, NU))
            launches.append(env.batch.step_launches() - l0)
            names.add(env.batch.last_kernel())
            out.append(o); rew.append(r); flags.append(np.stack([te, tr]))
        rows.append((np.stack(out), np.stack(rew), np.stack(flags), launches, names))
    assert rows[0][2].any(), "no episode ended"
    for k in (1, 2):
        assert np.array_equal(bits(rows[0][0]), bits(rows[k][0])) and np.array_equal(bits(rows[0][1]), bits(rows[k][1])) and np.array_equal(rows[0][2], rows[k][2])
        assert rows[0][3] == rows[k][3] and rows[0][4] == rows[k][4] and len(rows[0][4]) == 1, (rows[0][3:], rows[k][3:])
    assert np.array_equal(bits(envs[1].commands()), bits(np.tile(np.float32([tv[0], tv[1], 0.0]), (n, 1))))
    for env in envs:
        env.close()


def test_collection_with_scan_last_action_and_commands(hbmod, gpu):
    """collect_torch(T = 8) on the height-field model with the scan, the last action and the commands in the row: the command columns of
    the obs tape are the reference's, the scan and the last action sit at their old offsets, and the recorded actions replay bit for bit
    through step_torch"""
    torch = pytest.importorskip("torch")
    import obs_ext_ref
    import ray_cases
    n, T = 20, 8
    xs, ys, hs, cutoff = [-0.4, 0.3, 30.0], [-0.2, 0.25], dict(offset=1.0, scale=2.0, clip=(-4.0, 5.0)), 4.0
    mk = lambda: cmd_lib.env(hbmod, gpu, n, mdl=hbmod.Model.load(ray_cases.HFIELD_HBM), max_time=0.02, realism=True, domain_randomization=True,
                             height_scan=dict(body=1, xs=xs, ys=ys, z0=1.0, cutoff=cutoff), obs_extend=dict(prev_action=True, height_scan=hs))
    a, c = mk(), mk()
    L = a.obs_layout()
    want_L, width = cmd_ref.layout(NOBS, NU, 6, True, True, True)
    assert L == want_L and a.nobs == a.batch.env_nobs == width == NOBS + NU + 6 + 3
    rng = np.random.default_rng(5)
    w0 = rng.normal(0.0, 0.4, (a.nobs, 16)).astype(np.float32)
    w0[:NOBS] = 0.0
    net = ([a.nobs, 16, NU], [w0, rng.normal(0.0, 0.3, (16, NU)).astype(np.float32)], [np.zeros(16, np.float32), np.zeros(NU, np.float32)])
    a.actor_set(*net, head="gaussian", log_std=np.full(NU, -1.0, np.float32))
    sched = cmd_ref.Schedule(a.commands_cfg, n)
    o0 = a.reset()
    assert np.array_equal(o0, c.reset()) and np.array_equal(bits(o0[:, L["command"]]), bits(sched.cmd))
    buf = a.collect_torch(T, terminal_obs=True)
    out = {k: v.cpu().numpy() for k, v in buf.items()}
    assert out["obs"].shape == (T + 1, n, a.nobs)
    done = out["terminated"] | out["truncated"]
    assert done.any()
    for k in range(T):
        o, r, te, tr = c.step_torch(torch.from_numpy(out["action"][k]).to(buf["obs"].device))
        o = o.cpu().numpy()
        assert np.array_equal(bits(o), bits(out["obs"][k + 1])), k
        assert np.array_equal(bits(r.cpu().numpy()), bits(out["reward"][k])), k
        assert np.array_equal(te.cpu().numpy(), out["terminated"][k]) and np.array_equal(tr.cpu().numpy(), out["truncated"][k])
        old = sched.step(c.batch.time.astype(np.float32), done[k])
        assert np.array_equal(bits(o[:, L["command"]]), bits(sched.cmd)), k
        assert np.array_equal(bits(o[:, L["height_scan"]]), bits(obs_ext_ref.scan_entries(*c.batch.rays(), cutoff, **hs))), k
        if done[k].any():
            tobs = c.batch.env_terminal_obs()
            assert np.array_equal(bits(tobs[done[k]]), bits(out["terminal_obs"][k][done[k]]))
            assert np.array_equal(bits(tobs[done[k]][:, L["command"]]), bits(old[done[k]]))
            assert not o[done[k]][:, L["prev_action"]].any()
    assert sched.ep.max() >= 1 and (sched.k.max() >= 2 or sched.ep.max() >= 2)
    a.close(); c.close()


def test_sizing_and_order_of_calls(hbmod, gpu):
    """actor, critic, normaliser and PPO learner sized by hb_env_nobs run a collection and an update; the device refusals leave the batch
    stepping"""
    pytest.importorskip("torch")
    n, T = 16, 6
    env = cmd_lib.env(hbmod, gpu, n, max_time=0.02, normalize={})
    nobs = env.batch.env_nobs
    assert nobs == NOBS + 3 and env.nobs == nobs
    rng = np.random.default_rng(6)
    W = lambda i, o: rng.normal(0.0, 0.3, (i, o)).astype(np.float32)
    z = lambda k: np.zeros(k, np.float32)
    with pytest.raises(hbmod.HbError):  # (sized by the env's row, not the model's)
        env.actor_set([NOBS, 16, NU], [W(NOBS, 16), W(16, NU)], [z(16), z(NU)], head="gaussian", log_std=z(NU))
    env.actor_set([nobs, 16, NU], [W(nobs, 16), W(16, NU)], [z(16), z(NU)], head="gaussian", log_std=np.full(NU, -1.0, np.float32))
    env.critic_set([nobs, 16, 1], [W(nobs, 16), W(16, 1)], [z(16), z(1)])
    env.learner()
    env.reset()
    buf = env.collect_torch(T, gae=dict(gamma=0.99, lam=0.95))
    assert tuple(buf["obs"].shape) == (T + 1, n, nobs) and all(bool(np.isfinite(v.cpu().numpy()).all()) for k, v in buf.items() if v.dtype.is_floating_point)
    before = env.batch.learner_params().copy()
    log = env.ppo_update(buf, n_epochs=1, batch_size=48)
    after = env.batch.learner_params()
    assert log["n_minibatches"] == 2 and np.isfinite(after).all() and np.abs(after - before).max() > 1e-6
    # changing the width with an actor installed: refused with its reason, nothing changed, the env steps on
    b = env.batch
    cmds = b.commands()
    for cfg_kw in (dict(observe=0), None):
        with pytest.raises(hbmod.HbError, match="observation width would change"):
            b.commands_configure(None, **cfg_kw) if cfg_kw else b.commands_configure(None)
        assert b.env_nobs == nobs and np.array_equal(bits(b.commands()), bits(cmds))
    b.commands_configure(None, **dict(CMD, w_yaw=1.0, vx_max=2.0, resample_time=0.05))  # (ranges, weights and schedule may always change)
    assert np.array_equal(bits(b.commands()), bits(cmds))
    assert env.step_arrays(actions(rng, n, NU))[0].shape == (n, nobs)
    env.close()
    # nothing installed; observe going on with an actor installed
    plain = cmd_lib.env(hbmod, gpu, n, None, max_time=0.0)
    for call in (plain.commands, lambda: plain.set_commands(np.zeros(3, np.float32))):
        with pytest.raises(hbmod.HbError, match="no command configuration"):
            call()
    plain.actor_set([NOBS, 16, NU], [W(NOBS, 16), W(16, NU)], [z(16), z(NU)], head="gaussian", log_std=z(NU))
    with pytest.raises(hbmod.HbError, match="observation width would change"):
        plain.batch.commands_configure(None, **CMD)
    plain.batch.commands_configure(None, **dict(CMD, observe=0))  # (the width stays: allowed)
    plain.reset()
    assert plain.step_arrays(actions(rng, n, NU))[0].shape == (n, NOBS) and plain.commands().shape == (n, 3)
    plain.close()
    # a model whose observation has no free root
    arm = hbmod.Model.from_xml_string('<mujoco><worldbody><body><joint name="j" type="hinge" axis="0 1 0"/><geom type="capsule" size="0.05" fromto="0 0 0 0.3 0 0"/>'
                                      '</body></worldbody><actuator><motor joint="j"/></actuator></mujoco>')
    ab = hbmod.Batch(arm, 4, gpu)
    ab.env_configure(ab.env_default_config())
    with pytest.raises(hbmod.HbError, match="free root"):
        ab.commands_configure(None, **CMD)
    assert ab.env_nobs == arm.nobs
    ab.env_reset()
    assert ab.env_step(np.zeros((4, arm.nu), np.float32))[0].shape == (4, arm.nobs)
    ab.close()


def test_override(hbmod, gpu):
    """set_commands on a mask: hb_get_obs, the next observation and the next reward use the given command for the masked envs, the others
    keep theirs, and the next scheduled draw is the reference's draw k: the counters did not move"""
    n = 64
    env = cmd_lib.env(hbmod, gpu, n, max_time=0.0, reward_kind=1)
    m, o = env.model, Oracle()
    sched = cmd_ref.Schedule(env.commands_cfg, n)
    env.reset()
    rng = np.random.default_rng(7)
    act0 = actions(rng, n, NU, 0.3)
    env.step_arrays(act0)
    sched.step(env.batch.time.astype(np.float32), np.zeros(n, dtype=bool))
    mask = np.arange(n) % 3 == 0
    given = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    env.set_commands(given, mask)
    sched.set(given, mask)
    assert np.array_equal(bits(sched.cmd[mask]), bits(given[mask])) and (sched.cmd[~mask] != given[~mask]).any()
    assert np.array_equal(bits(env.commands()), bits(sched.cmd))
    assert np.array_equal(bits(env.batch.obs(want_reward=False)[0][:, NOBS:]), bits(sched.cmd))
    act = actions(rng, n, NU, 0.3)
    st0 = env.batch.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
    ob, r, te, tr, _ = env.step_arrays(act)  # (step 2 of the episode: no draw is due before 3 control steps have passed)
    assert not (te | tr).any()
    st1 = env.batch.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
    old = sched.step(st1[:, 0].astype(np.float32), np.zeros(n, dtype=bool))
    assert (sched.k == 1).all() and np.array_equal(bits(old), bits(sched.cmd)) and np.array_equal(bits(ob[:, NOBS:]), bits(sched.cmd))
    assert np.array_equal(bits(ob[mask][:, NOBS:]), bits(given[mask]))
    want = cmd_lib.reference_rewards(env.cfg, env.commands_cfg, old, st1, env.batch.env_joint_torques()[:, 6:], act0, act, cmd_lib.self_collisions(o, m, st0, act))[0]
    d = float(np.abs(r - want).max())
    print("\n  worst |reward - cmd_ref| with the overridden commands %.3e (bound %.3e)" % (d, BOUND))
    assert d <= BOUND
    for _ in range(2):  # (the third or, by the rounding of the fp32 time, the fourth step: draw 1 of every env, masked or not)
        ob = env.step_arrays(actions(rng, n, NU, 0.3))[0]
        sched.step(env.batch.time.astype(np.float32), np.zeros(n, dtype=bool))
        if (sched.k == 2).all():
            break
    assert (sched.k == 2).all() and np.array_equal(bits(ob[:, NOBS:]), bits(sched.cmd)) and np.array_equal(bits(env.commands()), bits(sched.cmd))
    assert np.array_equal(bits(sched.cmd), bits(np.stack([cmd_ref.draw(env.commands_cfg, e, 0, 1) for e in range(n)])))
    # mask None: every env
    env.set_commands(np.float32([0.5, 0.0, -0.25]))
    assert np.array_equal(bits(env.commands()), bits(np.tile(np.float32([0.5, 0.0, -0.25]), (n, 1))))
    env.close()
