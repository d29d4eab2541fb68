"""The observation extension on the GPU (include/hb.h: hb_env_obs_extend, hb_env_nobs): the last action and the height scan behind the
model's observation in every row the env adapter produces, and everything downstream sized by it.

Model: humanoid27_hfield.hbm (48 observations, 21 actuators, an 8 x 8 height field of +-10 m).  Scans of 3 x 2 and 5 x 3 rays from 1 m
above the torso in its heading frame, the last column 30 m ahead - off the field, so those entries are misses -, cutoff 4 m; transform
offset 1, scale 2, clip (-4, 5): a miss gives 2 (1 - 4) = -6, which the lower clamp turns into -4.  Rows of 48 + 21 + 6 = 75 and
48 + 21 + 15 = 84 floats.  8 to 37 envs, T of 6, hidden widths of 16.

Bounds - none of them new:
  bits     the base columns against a twin without the extension, the last action against the action, the scan against the float32
           transform (tests/obs_ext_ref.py) of Batch.rays() at the same state, replays of recorded actions: equality;
  fp64     the scan against obs_ext_ref over tests/ray_ref.py's cast: tests/test_gpu_ray.py's BOUND = 1e-5 max(1, dist) times scan_scale,
           on the rays the reference calls robust;
  mean     tests/test_gpu_collect.py's MEAN_TOL = 5e-5 max(1, |ref|) against mlp_ref in fp64;
  norm     tests/test_gpu_norm.py's Tracker (norm_lib: its derived bounds, ratio <= 1);
  learners tests/test_gpu_ppo.py's check_case and tests/test_gpu_sac.py's check_step (ppo_lib, sac_lib) with their own bounds, on the
           extended tapes.
"""
import ctypes

import numpy as np
import pytest

import mlp_ref as ml
import obs_ext_ref
import ray_cases
import ray_ref
from bounds import MEAN_TOL  # tests/test_gpu_collect.py's
from bounds import RAY_BOUND as BOUND  # tests/test_gpu_ray.py's
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

NOBS, NU = 48, 21
Z0, CUTOFF = 1.0, 4.0
HS = dict(offset=1.0, scale=2.0, clip=(-4.0, 5.0))
SCANS = {"3x2": ([-0.4, 0.3, 30.0], [-0.2, 0.25]), "5x3": ([-0.6, -0.3, 0.05, 0.4, 30.0], [-0.3, 0.02, 0.3])}
T = 6


def _model(hbmod):
    return hbmod.Model.load(ray_cases.HFIELD_HBM)


def _env(hbmod, gpu, n, scan="3x2", ext=True, **kw):
    xs, ys = SCANS[scan]
    kw.setdefault("target_z", 10.0)  # (out of reach: standing, which the reset pose is, ends no episode)
    if ext is True:
        ext = dict(prev_action=True, height_scan=HS)
    return hbmod.VecEnv(_model(hbmod), n, gpu, seed=7, height_scan=dict(body=1, xs=xs, ys=ys, z0=Z0, cutoff=CUTOFF), obs_extend=ext or None, **kw)


def _scan_of_rays(batch):
    """the float32 transform of Batch.rays() at the batch's state: the bits the scan columns must have"""
    dist, gid = batch.rays()
    return obs_ext_ref.scan_entries(dist, gid, CUTOFF, **HS)


def _actions(rng, n):
    return rng.uniform(-1.0, 1.0, (n, NU)).astype(np.float32)


def _elevations(hbmod, env):
    import dr_ref
    P = env.batch.env_domain_params()
    return dr_ref.table(P, dr_ref.layout(env.model, P.shape[1]), "hfield")


def _hold_fp64(hbmod, env, scan, rows, envs):
    """the scan columns `rows` [n, n_ray] of the env's current state against the fp64 rays, on the robust rays of the envs `envs`"""
    xs, ys = SCANS[scan]
    c = ray_cases.case("terrain")
    p, v = hbmod.height_scan_rays(xs, ys, Z0)
    c.update(pnt=p, vec=v, cutoff=CUTOFF)
    states = env.batch.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
    elev = _elevations(hbmod, env) if env.domain is not None else None
    o = Oracle(ray_cases.HFIELD_HBM)
    worst, robust = 0.0, 0
    for e in envs:
        want, res = obs_ext_ref.reference_scan(o, c, states[e], HS, hfield_data=None if elev is None else elev[e])
        ok = ~ray_ref.fragile(res)
        robust += int(ok.sum())
        d = np.where(res["geomid"] >= 0, res["dist"], CUTOFF)
        worst = max(worst, float((np.abs(rows[e].astype(np.float64) - want)[ok] / np.maximum(1.0, d[ok])).max()))
    print("\n  scan %s vs fp64: worst %.3g (bound %.3g), %d robust rays" % (scan, worst, HS["scale"] * BOUND, robust))
    assert robust >= 0.9 * len(envs) * len(p)
    assert worst <= HS["scale"] * BOUND


@pytest.mark.parametrize("scan,n,realism", [("3x2", 9, False), ("5x3", 37, True)])
def test_layout_and_bits(hbmod, gpu, scan, n, realism):
    """after a reset and after each of four steps with random actions: the base columns are the twin's, the last action the action's (with
    the realism layer on: the action of the env's own delay ago - the layer runs without action noise here, so that the applied action is
    known), the scan the transform of Batch.rays(), and close to the fp64 rays"""
    envs = [_env(hbmod, gpu, n, scan, ext=x, realism=realism, domain_randomization=realism) for x in (True, False)]
    for env in envs:
        if realism:
            env.realism.action_noise = 0.0
            env.realism.min_delay, env.realism.max_delay = 0.0, 0.012  # (delays of 0 to 2 control steps of 5 ms: inside the four steps below)
            env._apply_realism()
    a, c = envs
    nray = len(SCANS[scan][0]) * len(SCANS[scan][1])
    L = a.obs_layout()
    assert a.nobs == a.batch.env_nobs == NOBS + NU + nray and a.observation_shape == (a.nobs,) and c.nobs == NOBS
    assert (L["base"], L["prev_action"], L["height_scan"]) == (slice(0, NOBS), slice(NOBS, NOBS + NU), slice(NOBS + NU, a.nobs))
    oa, oc = a.reset(), c.reset()
    assert oa.shape == (n, a.nobs) and oa.dtype == np.float32
    rng = np.random.default_rng(3)
    acts, prevs = [], []
    for k in range(5):
        if k:
            act = _actions(rng, n)
            acts.append(act)
            oa, _, ta, ua, _ = a.step_arrays(act)
            oc, _, tc, uc, _ = c.step_arrays(act)
            assert not (ta | ua | tc | uc).any()
        assert np.array_equal(oa[:, L["base"]], oc), k
        want = _scan_of_rays(a.batch)
        assert np.array_equal(oa[:, L["height_scan"]].view(np.uint32), want.view(np.uint32)), k
        assert np.array_equal(a.batch.obs(want_reward=False)[0][:, L["height_scan"]], want)  # (hb_get_obs: the same row, without noise)
        miss = np.arange(nray) % len(SCANS[scan][0]) == len(SCANS[scan][0]) - 1
        assert (oa[:, L["height_scan"]][:, miss] == np.float32(-4.0)).all() and (oa[:, L["height_scan"]][:, ~miss] > -4.0).all()
        prevs.append(oa[:, L["prev_action"]].copy())
        if k in (0, 4):
            _hold_fp64(hbmod, a, scan, oa[:, L["height_scan"]], range(0, n, max(1, n // 4)))
    assert not prevs[0].any()
    zero = np.zeros(NU, np.float32)
    for e in range(n):
        # (delay d: the action of d steps ago, zero before the ring has d items; d = 0 without the realism layer)
        fits = [d for d in range(3 if realism else 1) if all(np.array_equal(prevs[k][e], acts[k - 1 - d][e] if k - 1 - d >= 0 else zero) for k in range(1, 5))]
        assert fits, e
    for env in envs:
        env.close()


def test_episode_ends(hbmod, gpu):
    """every env times out at the same step, under reset perturbation and terrain randomisation: the terminal rows carry the action just
    applied and the scan over the OLD elevations (a twin that does not reset stands in that state), the new rows a zero action and the
    scan at the reset state over the NEW elevations"""
    n = 16
    a = _env(hbmod, gpu, n, "5x3", domain_randomization=True, max_time=0.02)
    c = _env(hbmod, gpu, n, "5x3", domain_randomization=True, max_time=0.02, auto_reset=0)
    assert a.domain.floor_bump_max > 0 and a.cfg.reset_perturb == 1.0
    L = a.obs_layout()
    assert np.array_equal(a.reset(), c.reset())
    rng = np.random.default_rng(5)
    ended = False
    for k in range(8):
        act = _actions(rng, n)
        elev_old = _elevations(hbmod, a).copy()
        oa, _, ta, ua, _ = a.step_arrays(act)
        oc, _, tc, uc, _ = c.step_arrays(act)
        assert np.array_equal(ta | ua, tc | uc)
        if not (ta | ua).any():
            assert np.array_equal(oa, oc)
            continue
        assert (ta | ua).all(), "every env times out at the same step"
        ended = True
        tobs = a.batch.env_terminal_obs()
        # the twin did not reset: its observation is the one the episodes ended in, and its rays are cast over the old elevations
        assert np.array_equal(_elevations(hbmod, c), elev_old)
        end_scan = _scan_of_rays(c.batch)
        assert np.array_equal(tobs[:, L["base"]], oc[:, L["base"]])
        assert np.array_equal(tobs[:, L["prev_action"]], act) and act.any(axis=1).all()
        assert np.array_equal(tobs[:, L["height_scan"]].view(np.uint32), end_scan.view(np.uint32))
        assert np.array_equal(tobs, oc)
        # the new episode
        assert not oa[:, L["prev_action"]].any()
        new_scan = _scan_of_rays(a.batch)
        assert np.array_equal(oa[:, L["height_scan"]].view(np.uint32), new_scan.view(np.uint32))
        elev_new = _elevations(hbmod, a)
        assert (np.abs(elev_new - elev_old).max(axis=1) > 1e-3).any(), "no env's elevations changed across the reset"
        assert (oa[:, L["height_scan"]] != tobs[:, L["height_scan"]]).any(), "no scan entry changed across the reset"
        _hold_fp64(hbmod, a, "5x3", oa[:, L["height_scan"]], range(0, n, 4))
        # and the episode goes on: the next row has the action again
        act = _actions(rng, n)
        oa = a.step_arrays(act)[0]
        assert np.array_equal(oa[:, L["prev_action"]], act)
        assert np.array_equal(oa[:, L["height_scan"]], _scan_of_rays(a.batch))
        break
    assert ended
    a.close(); c.close()


def _ext_actor(nobs, seed=4):
    """an actor nobs -> 16 -> nu whose first layer is zero on the base columns: its mean is a function of the extension alone"""
    rng = np.random.default_rng(seed)
    t = {"actor.w0": rng.normal(0.0, 0.4, (nobs, 16)).astype(np.float32), "actor.b0": rng.normal(0.0, 0.1, 16).astype(np.float32),
         "actor.w1": rng.normal(0.0, 0.3, (16, NU)).astype(np.float32), "actor.b1": rng.normal(0.0, 0.1, NU).astype(np.float32)}
    t["actor.w0"][:NOBS] = 0.0
    return t


def test_collection(hbmod, gpu):
    torch = pytest.importorskip("torch")
    n = 20
    a, c = (_env(hbmod, gpu, n, "3x2", realism=True, domain_randomization=True, max_time=0.02) for _ in range(2))
    t = _ext_actor(a.nobs)
    sizes = [a.nobs, 16, NU]
    a.actor_set(sizes, [t["actor.w0"], t["actor.w1"]], [t["actor.b0"], t["actor.b1"]], head="gaussian", log_std=np.full(NU, -1.0, np.float32))
    with pytest.raises(hbmod.HbError):  # (sized by the env's row, not the model's)
        c.actor_set([NOBS, 16, NU], [t["actor.w0"][:NOBS], t["actor.w1"]], [t["actor.b0"], t["actor.b1"]], head="gaussian", log_std=np.zeros(NU, np.float32))
    o0 = a.reset()
    assert np.array_equal(o0, c.reset())
    buf = a.collect_torch(T, terminal_obs=True)
    assert tuple(buf["obs"].shape) == (T + 1, n, a.nobs) and tuple(buf["terminal_obs"].shape) == (T, n, a.nobs)
    out = {k: v.cpu().numpy() for k, v in buf.items()}
    done = out["terminated"] | out["truncated"]
    assert done.any() and done[:-1].any() and np.isfinite(out["obs"]).all()
    L = a.obs_layout()
    # the recorded actions through step_torch on the twin: the obs tape bit for bit, and the terminal rows where an episode ended
    for k in range(T):
        o, _, te, tr = c.step_torch(torch.from_numpy(out["action"][k]).to(buf["obs"].device))
        assert np.array_equal(o.cpu().numpy(), out["obs"][k + 1]), k
        assert np.array_equal(te.cpu().numpy(), out["terminated"][k]) and np.array_equal(tr.cpu().numpy(), out["truncated"][k])
        if done[k].any():
            assert np.array_equal(c.batch.env_terminal_obs()[done[k]], out["terminal_obs"][k][done[k]])
            assert not out["obs"][k + 1][done[k]][:, L["prev_action"]].any()
    # the mean depends on the extension alone, and agrees with the fp64 MLP on the tape's rows
    rows = out["obs"][:T].reshape(T * n, a.nobs).astype(np.float64)
    ref = ml.forward(t, "actor", 2, rows)[1]
    blind = rows.copy()
    blind[:, :NOBS] = 0.0
    assert np.array_equal(ml.forward(t, "actor", 2, blind)[1], ref)
    got = out["mean"].reshape(T * n, NU)
    worst = float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
    print("\n  actor mean on the extension: worst %.3g (bound %.0e), spread of the mean over the rows %.3g" % (worst, MEAN_TOL, float(ref.std(axis=0).max())))
    assert worst < MEAN_TOL and ref.std(axis=0).max() > 1e-3
    a.close(); c.close()


def test_normaliser(hbmod, gpu, tmp_path):
    pytest.importorskip("torch")
    import norm_lib as tn
    n = 24
    a = _env(hbmod, gpu, n, "3x2", domain_randomization=True, max_time=0.02, normalize={})
    t = _ext_actor(a.nobs)
    a.actor_set([a.nobs, 16, NU], [t["actor.w0"], t["actor.w1"]], [t["actor.b0"], t["actor.b1"]], head="gaussian", log_std=np.full(NU, -1.0, np.float32))
    o0 = a.reset()
    raw0 = a.get_original_obs()
    assert o0.shape == raw0.shape == (n, a.nobs)
    tk = tn.Tracker(n, a.nobs)
    worst = dict(obs=tn.ratio(o0, tk.reset(raw0), tk.dz_obs(raw0)), rew=0.0)
    out = a.collect(T, terminal_obs=True, raw=True)
    assert out["raw_obs"].shape == (T, n, a.nobs) and (out["terminated"] | out["truncated"]).any()
    for k in range(T):
        want = tk.step(out["raw_obs"][k], out["raw_reward"][k], out["terminated"][k], out["truncated"][k])
        worst["obs"] = max(worst["obs"], tn.ratio(out["obs"][k + 1], want["obs"], tk.dz_obs(out["raw_obs"][k])))
        worst["rew"] = max(worst["rew"], tn.ratio(out["reward"][k], want["reward"], tk.dz_rew(out["raw_reward"][k])))
    rec = a.batch.norm_stats()
    stats = tk.stats_ratio(rec)
    print("\n  normaliser over %d columns: statistics / bound %.3g, obs / bound %.3g, reward / bound %.3g" % (a.nobs, stats, worst["obs"], worst["rew"]))
    assert rec.shape == (2 * a.nobs + 4,) and stats <= 1.0 and worst["obs"] <= 1.0 and worst["rew"] <= 1.0
    assert rec[a.nobs + NOBS:2 * a.nobs].min() >= 0.0 and rec[NOBS + NU:a.nobs].max() < 0.0  # (the scan's means: below the body)
    # save / load: into an env of the same width, and refused by one of another
    path = str(tmp_path / "norm.npz")
    a.save_normalization(path)
    same = _env(hbmod, gpu, 8, "3x2", normalize={})
    same.load_normalization(path)
    assert np.array_equal(same.batch.norm_stats(), rec)
    other = _env(hbmod, gpu, 8, "3x2", ext=False, normalize={})
    before = other.batch.norm_stats()
    with pytest.raises(ValueError, match="%d observations, this env has %d" % (a.nobs, NOBS)):
        other.load_normalization(path)
    assert np.array_equal(other.batch.norm_stats(), before)
    with pytest.raises(ValueError):
        other.batch.norm_set_stats(rec)
    for e in (a, same, other):
        e.close()


def test_ppo_learner(hbmod, gpu, monkeypatch):
    torch = pytest.importorskip("torch")
    import ppo_ref as pr
    import ppo_lib as tp
    n = 16
    env = _env(hbmod, gpu, n, "3x2", domain_randomization=True, max_time=0.02)
    asz, csz = [env.nobs, 16, NU], [env.nobs, 16, 1]
    monkeypatch.setitem(tp.NETS, "obs_ext", (asz, csz))  # (its helpers look the sizes up by name)
    flat = pr.random_problem(asz, csz, 4, seed=3)[0]
    t = pr.split(flat.astype(np.float32), asz, csz, NU)
    env.actor_set(asz, [t["actor.w0"], t["actor.w1"]], [t["actor.b0"], t["actor.b1"]], head="gaussian", log_std=t["log_std"])
    env.critic_set(csz, [t["critic.w0"], t["critic.w1"]], [t["critic.b0"], t["critic.b1"]])
    cfg = tp.cfg(ent_coef=0.01)
    env.learner(**cfg)
    env.reset()
    buf = env.collect_torch(T, gae=dict(gamma=0.99, lam=0.95))
    R = T * n
    rows = {"obs": buf["obs"][:T].reshape(R, env.nobs), "action": buf["action"].reshape(R, NU), "old_log_prob": buf["log_prob"].reshape(R),
            "advantage": buf["advantage"].reshape(R), "returns": buf["returns"].reshape(R)}
    rows = {k: v.cpu().numpy().copy() for k, v in rows.items()}
    assert all(np.isfinite(v).all() for v in rows.values()) and rows["obs"][:, NOBS + NU:].std() > 0
    b = env.batch
    flat64 = b.learner_params().astype(np.float64)
    assert np.array_equal(flat64, flat.astype(np.float32).astype(np.float64))
    worst = dict(stat=0.0, head=0.0, floor=0.0, k=0.0, ratio=0.0, rel=0.0)
    tp.check_case(b, "obs_ext", flat64, rows, "mb50_index", np.random.default_rng(2).permutation(R)[:50], 0, 50, cfg, worst)
    tp.check_case(b, "obs_ext", flat64, rows, "all_rows", None, 0, R, cfg, worst)
    print("\n  ppo on %d-wide rows: statistics %.3f, head gradients %.3f of their bounds; back-propagated: measured / k %.3f" % (env.nobs, worst["stat"], worst["head"], worst["rel"]))
    log = env.ppo_update(buf, n_epochs=1, batch_size=48)
    after = b.learner_params()
    assert log["n_minibatches"] == 2 and all(np.isfinite(v) for k, v in log.items() if isinstance(v, float) and k != "explained_variance")
    assert np.isfinite(after).all() and np.abs(after - flat64).max() > 1e-5
    env.close()


def test_sac_learner(hbmod, gpu, monkeypatch):
    torch = pytest.importorskip("torch")
    import sac_ref as sr
    import sac_lib as ts
    n = 16
    env = _env(hbmod, gpu, n, "3x2", domain_randomization=True, max_time=0.02)
    asz, qsz = [env.nobs, 16, 2 * NU], [env.nobs + NU, 16, 1]
    monkeypatch.setitem(ts.NETS, "obs_ext", (asz, qsz))  # (its helpers look the sizes up by name, and the width of obs in obs | action
    monkeypatch.setattr(ts, "NOBS", env.nobs)            # in the module's NOBS)
    pb = sr.random_problem(asz, qsz, 4, seed=3)
    b = env.batch
    with pytest.raises(hbmod.HbError):  # (sized by the env's row, not the model's)
        b.q_set(0, [NOBS + NU, 16, 1], [np.zeros((NOBS + NU, 16), np.float32), np.zeros((16, 1), np.float32)], [np.zeros(16, np.float32), np.zeros(1, np.float32)])
    ts.install(b, "obs_ext", pb["flat"])
    cfg = ts.cfg(lr_actor=1e-3, lr_critic=1e-3, lr_ent=1e-3, ent_coef_init=0.3)
    env.sac_learner(**cfg)
    st = b.sac_state()
    st["params"], st["targets"] = pb["flat"].astype(np.float32), pb["targets"].astype(np.float32)
    b.sac_set_state(st)
    env.reset()
    buf = env.collect_torch(T, terminal_obs=True)
    replay = hbmod.ReplayBuffer(4 * T * n, env, device=buf["obs"].device)
    assert (replay.nobs, replay.nu) == (env.nobs, NU)
    replay.add(buf)
    R = replay.size
    assert R == T * n
    rows = {k: getattr(replay, k)[:R].cpu().numpy().copy() for k in ts.TAPES}
    done = (buf["terminated"] | buf["truncated"]).cpu().numpy().reshape(R)
    tobs = buf["terminal_obs"].cpu().numpy().reshape(R, env.nobs)
    assert done.any() and np.array_equal(rows["next_obs"][done], tobs[done]) and rows["next_obs"][done][:, NOBS:NOBS + NU].any()
    rng = np.random.default_rng(6)
    pb2 = dict(rows=rows, eps_pi=rng.normal(size=(R, NU)).astype(np.float32), eps_next=rng.normal(size=(R, NU)).astype(np.float32))
    worst = ts.new_worst()
    ts.check_step(b, "obs_ext", pb2, rng.permutation(R)[:40], cfg, worst, "mb40_index")
    print("\n  " + ts.line("sac step on %d-wide rows" % env.nobs, worst))
    before = b.sac_state()["params"].copy()
    log = env.sac_update(replay, 1, batch_size=32)
    after = b.sac_state()["params"]
    assert all(np.isfinite(v) for v in log.values()) and np.isfinite(after).all() and np.abs(after - before).max() > 1e-6
    env.close()


def _pair(hbmod, gpu, n=8):
    """a batch under test and a twin that is never refused anything, set up alike; step() steps both and holds the rows to each other"""
    m = _model(hbmod)
    xs, ys = SCANS["3x2"]
    p, v = hbmod.height_scan_rays(xs, ys, Z0)
    bs = [hbmod.Batch(m, n, gpu) for _ in range(2)]
    for b in bs:
        b.env_configure(b.env_default_config())
    return bs, (p, v)


def test_refusals(hbmod, gpu):
    (b, w), (p, v) = _pair(hbmod, gpu)
    n = b.n_env
    L = hbmod.lib()
    rng = np.random.default_rng(8)
    rays = dict(frame="yaw", frame_body=1, static=True, moving=False)

    def same_step():
        act = _actions(rng, n)
        ob, ow = b.env_step(act), w.env_step(act)
        assert all(np.array_equal(x, y) for x, y in zip(ob, ow))
        return ob[0]

    def refused(**kw):
        width = b.env_nobs
        with pytest.raises(hbmod.HbError, match="code -1"):
            b.obs_extend(**kw)
        assert b.env_nobs == width
        assert same_step().shape == (n, width)

    assert np.array_equal(b.env_reset(), w.env_reset())
    refused(height_scan=HS)                                     # no rays installed
    b.ray_configure(p, v, cutoff=0.0, **rays)
    refused(height_scan=HS)                                     # a ray configuration without a cutoff
    for x in (b, w):
        x.ray_configure(p, v, cutoff=CUTOFF, **rays)
    refused(height_scan=dict(HS, clip=(1.0, -1.0)))             # lo > hi
    for bad in (dict(HS, offset=np.inf), dict(HS, scale=np.nan), dict(HS, clip=(-np.inf, 1.0)), dict(HS, clip=(0.0, np.nan))):
        refused(prev_action=True, height_scan=bad)              # a non-finite parameter
    assert L.hb_env_obs_extend(None, None) == -1 and L.hb_env_nobs(None) == -1
    # what is sized by the observation comes later: with any of it installed the call is refused, and the extension that is on stays on
    for x in (b, w):
        x.obs_extend(prev_action=True, height_scan=HS)
    width = NOBS + NU + len(p)
    assert b.env_nobs == width
    assert np.array_equal(b.env_reset(), w.env_reset())
    t = _ext_actor(width)
    z = np.zeros
    installs = [("actor", lambda: b.actor_set([width, 16, NU], [t["actor.w0"], t["actor.w1"]], [t["actor.b0"], t["actor.b1"]], head="gaussian", log_std=z(NU, np.float32))),
                ("critic", lambda: b.critic_set([width, 16, 1], [t["actor.w0"], z((16, 1), np.float32)], [t["actor.b0"], z(1, np.float32)])),
                ("q", lambda: b.q_set(1, [width + NU, 1], [z((width + NU, 1), np.float32)], [z(1, np.float32)])),
                ("normaliser", lambda: b.norm_configure(training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8)),
                ("learner", lambda: b.learner_create())]
    fresh = []
    for name, install in installs:
        if name == "learner":  # (needs the actor and the critic; on its own batch all three exist)
            installs[0][1](); installs[1][1]()
        install()
        for kw in (dict(), dict(prev_action=True), dict(prev_action=True, height_scan=HS)):
            with pytest.raises(hbmod.HbError, match="code -1"):
                b.obs_extend(**kw)
        assert b.env_nobs == width
        row = same_step()
        assert row.shape == (n, width) and np.array_equal(row[:, NOBS + NU:], obs_ext_ref.scan_entries(*b.rays(), CUTOFF, **HS))
        # (a batch of its own for the next one: nothing installed can be taken out again)
        state = b.get_state(hbmod.STATE_INTEGRATION)
        fresh.append(b)
        b = hbmod.Batch(_model(hbmod), n, gpu)
        b.env_configure(b.env_default_config())
        b.ray_configure(p, v, cutoff=CUTOFF, **rays)
        b.obs_extend(prev_action=True, height_scan=HS)
        assert np.array_equal(b.env_reset(), w.env_reset())
    # while the scan is part of the observation the number of rays stays: another count, a removal and a lost cutoff are refused
    spec = hbmod.engine.HbRaySpec(2, 1, -1, 1, CUTOFF)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.hb_ray_configure(b._h, ctypes.byref(spec), P(p), P(v), len(p) - 1) == -1
    assert L.hb_ray_configure(b._h, None, None, None, 0) == -1
    assert L.hb_ray_configure(b._h, ctypes.byref(hbmod.engine.HbRaySpec(2, 1, -1, 1, 0.0)), P(p), P(v), len(p)) == -1
    row = same_step()
    assert row.shape == (n, width) and np.array_equal(row[:, NOBS + NU:], obs_ext_ref.scan_entries(*b.rays(), CUTOFF, **HS))
    # the same number of new rays is allowed, and is what the next observation holds
    p2 = p.copy()
    p2[:, 0] += np.float32(0.17)
    b.ray_configure(p2, v, cutoff=CUTOFF, **rays)
    act = _actions(rng, n)
    row, roww = b.env_step(act)[0], w.env_step(act)[0]
    assert np.array_equal(row[:, :NOBS + NU], roww[:, :NOBS + NU]) and not np.array_equal(row[:, NOBS + NU:], roww[:, NOBS + NU:])
    assert np.array_equal(row[:, NOBS + NU:], obs_ext_ref.scan_entries(*b.rays(), CUTOFF, **HS))
    # removal: an all-off call takes the extension out again
    b.obs_extend()
    assert b.env_nobs == NOBS and b.env_reset().shape == (n, NOBS)
    b.ray_configure(None, None)
    for x in fresh + [b, w]:
        x.close()


def test_plain_path(hbmod, gpu):
    """obs_extend=None and an all-off dict: the model's row, the same bits and the same kernels as a VecEnv that was never asked"""
    n = 16
    m = _model(hbmod)
    xs, ys = SCANS["3x2"]
    hs = dict(body=1, xs=xs, ys=ys, z0=Z0, cutoff=CUTOFF)
    envs = [hbmod.VecEnv(m, n, gpu, seed=7, height_scan=hs, realism=True, domain_randomization=True, **kw)
            for kw in (dict(), dict(obs_extend=None), dict(obs_extend=dict(prev_action=False, height_scan=None)))]
    rng = np.random.default_rng(9)
    rows, names = [], []
    acts = [_actions(rng, n) for _ in range(3)]
    for env in envs:
        assert env.nobs == env.batch.env_nobs == m.nobs == NOBS and env.observation_shape == (NOBS,) and env.obs_layout() == {"base": slice(0, NOBS)}
        out = [env.reset()]
        for act in acts:
            out.append(env.step_arrays(act)[0])
        names.append(env.batch.last_kernel())
        out.append(env.batch.obs(want_reward=False)[0])
        names.append(env.batch.last_kernel())
        rows.append(np.stack(out))
        assert rows[-1].shape == (5, n, NOBS)
    assert np.array_equal(rows[0], rows[1]) and np.array_equal(rows[0], rows[2])
    assert names[0:2] == names[2:4] == names[4:6] and names[0] and names[0] == names[1], names
    for env in envs:
        env.close()
