"""The on-device normaliser (include/hb.h: hb_norm_*, hb_env_collect_norm_dev) against the fp64 reference of tests/norm_ref.py.

Bounds (nothing here is tuned; u = 2^-53, v = 2^-24):
 * statistics.  The device and the reference evaluate the same running mean / variance in fp64 and differ in the order of the sums over
   a batch's rows (the device: chunks of 64 consecutive envs, two-pass inside a chunk, merged in chunk order with the update formula; the
   reference: numpy's mean / var over all rows, one update) and in fused multiply-adds.  norm_ref.ErrorBound carries the forward bound
   of ONE such evaluation through the updates (its docstring has the recurrences: A = n + 6 nchunk + 8 roundings per chain on quantities
   of magnitude max |x|; the cancelling d = mb - mean enters with its absolute error; every term of the merged variance is
   non-negative).  Two evaluations differ by at most twice that: |mean_dev - mean_ref| <= 2 e_mean, |var_dev - var_ref| <= 2 e_var.
   The discounted returns are themselves computed (ret gamma + reward, fused on the device, once per step): after k steps they carry
   at most 2 k u max |ret|, which enters as x_err.  Counts: 1e-4 plus row counts, one addition per chunk on the device and one per
   update in the reference, each rounded once: they differ by at most (additions so far) u count.
 * outputs.  z = (x - mean) / sqrt(var + epsilon) in fp64, rounded to fp32 once, clipped in fp32 (the clip is monotone and 1-Lipschitz).
   The two z differ by at most dz = |x - mean| inv (e'_var / 2 (var + epsilon)) + e'_mean inv + 6 u |z| (e' = 2 e; the last term: the
   subtraction, the square root, the division or reciprocal, the product), so the fp32 results differ by at most one fp32 rounding of
   |z| - a spacing, 2 v |z| at most - plus dz.  Rewards: the same with mean = 0 and x exact.
 * episode returns and lengths: each env's raw rewards are added in step order in fp64 on both sides: equal bits.  The totals are sums
   over the envs in another order, each side at most n - 1 roundings inside a step and one per step onto the running total (at most 8
   steps here): 2 (n + 8) u times the sum of the magnitudes.
HB_NORM_PARITY_OUT=<file> collects the worst values (profiles/norm_parity.txt)."""
import ctypes

import numpy as np
import pytest

import actor_ref as ar
import gae_lib as tg
import gae_ref as gr
import norm_ref as nr
from norm_lib import Tracker, ratio as _ratio
from oracle_lib import HUMANOID_HBM, TEAM_PLANE_HBM  # noqa: F401  (the model of the humanoid_model fixture)
from step_lib import report

pytestmark = pytest.mark.gpu

SEED, T = 2024, 8
CFG = dict(norm_obs=True, norm_reward=True, training=True, clip_obs=1.25, clip_reward=2.0, gamma=0.99, epsilon=1e-8)
K_STEPS = 5


def _report(line):
    report(line, "HB_NORM_PARITY_OUT")


class Dev:
    """named device buffers on a batch (the library's own allocation helpers: no torch in the primitive tests)"""

    def __init__(self, b, **arrays):
        self.b, self.meta, self.ptr = b, {}, {}
        for k, a in arrays.items():
            a = np.ascontiguousarray(a)
            self.meta[k] = (a.shape, a.dtype)
            self.ptr[k] = b.dev_alloc(max(4, a.nbytes))
            b.to_dev(self.ptr[k], a)

    def put(self, k, a):
        a = np.ascontiguousarray(a, dtype=self.meta[k][1])
        assert a.shape == self.meta[k][0]
        self.b.to_dev(self.ptr[k], a)

    def get(self, k):
        return self.b.from_dev(self.ptr[k], *self.meta[k])

    def free(self):
        for p in self.ptr.values():
            self.b.dev_free(p)
        self.ptr = {}


_data = {}


def _synthetic(n, nobs):
    """K_STEPS steps of raw inputs, made once per shape and shared read-only.  Column 0 is constant, column 1 has mean 1e3 and spread 1e-2
    (cancellation), columns 2 and 3 and the rewards carry outliers beyond the clips in the last steps; step 1 ends no episode, step 2
    ends one in every chunk of 64 envs (and at the last env), the other steps end about a fifth; terminal rows of envs that did not end
    are NaN (never read)."""
    if (n, nobs) in _data:
        return _data[(n, nobs)]
    rng = np.random.default_rng(1000 * nobs + n)
    scale = rng.uniform(0.05, 20.0, nobs)
    loc = rng.uniform(-5.0, 5.0, nobs)
    obs = (loc + scale * rng.normal(size=(K_STEPS, n, nobs))).astype(np.float32)
    obs[:, :, 0] = 0.75
    obs[:, :, 1] = (1e3 + 1e-2 * rng.normal(size=(K_STEPS, n))).astype(np.float32)
    rew = rng.normal(0.3, 1.0, size=(K_STEPS, n)).astype(np.float32)
    obs[K_STEPS - 1, 0, 2] = 1e4
    obs[K_STEPS - 1, n - 1, 3] = -1e4
    rew[K_STEPS - 1, 0] = 1e4
    if n > 1:
        rew[K_STEPS - 2, n - 1] = -1e4
    done = rng.random((K_STEPS, n)) < 0.2
    done[1] = False
    done[2] = False
    done[2, 3 % n::64] = True
    done[2, n - 1] = True
    done[K_STEPS - 1, 0] = True
    trunc = done & (rng.random((K_STEPS, n)) < 0.5)
    term = done & ~trunc
    term[2, n - 1] = trunc[2, n - 1] = True  # both flags at once
    tobs = np.full((K_STEPS, n, nobs), np.nan, np.float32)
    tobs[done] = (loc + scale * rng.normal(size=(int(done.sum()), nobs))).astype(np.float32)
    d = dict(obs=obs, rew=rew, term=term.astype(np.uint8), trunc=trunc.astype(np.uint8), tobs=tobs, done=done)
    _data[(n, nobs)] = d
    return d


def _primitive(hbmod, model, gpu, n, inplace):
    m = model
    nobs = m.nobs
    d = _synthetic(n, nobs)
    b = hbmod.Batch(m, n, gpu)
    b.norm_configure(**CFG)
    tk = Tracker(n, nobs, **CFG)
    f32 = np.float32
    dev = Dev(b, obs=d["obs"][0], rew=d["rew"][0], term=d["term"][0], trunc=d["trunc"][0], tobs=d["tobs"][0], obs_o=np.full((n, nobs), 7, f32),
              rew_o=np.full(n, 7, f32), tobs_o=np.full((n, nobs), 7, f32), ep_r=np.full(n, 7, f32), ep_l=np.full(n, 7, np.int32))
    names = dict(obs="obs", rew="rew", tobs="tobs") if inplace else dict(obs="obs_o", rew="rew_o", tobs="tobs_o")
    worst = dict(stats=0.0, obs=0.0, rew=0.0, tobs=0.0, obs_abs=0.0, rew_abs=0.0)
    clipped = dict(op=False, on=False, rp=False, rn=False)
    for k in range(K_STEPS):
        for key, src in (("obs", "obs"), ("rew", "rew"), ("term", "term"), ("trunc", "trunc"), ("tobs", "tobs")):
            dev.put(key, d[src][k])
        if not inplace:
            dev.put("tobs_o", np.full((n, nobs), 7, f32))
        b.norm_step_dev(dev.ptr["obs"], dev.ptr[names["obs"]], dev.ptr["rew"], dev.ptr["term"], dev.ptr["trunc"], reward_out=dev.ptr[names["rew"]],
                        terminal_obs_in=dev.ptr["tobs"], terminal_obs_out=dev.ptr[names["tobs"]], ep_return_out=dev.ptr["ep_r"], ep_length_out=dev.ptr["ep_l"])
        want = tk.step(d["obs"][k], d["rew"][k], d["term"][k], d["trunc"][k], d["tobs"][k])
        done = d["done"][k]
        worst["stats"] = max(worst["stats"], tk.stats_ratio(b.norm_stats()))
        o, r, t = dev.get(names["obs"]), dev.get(names["rew"]), dev.get(names["tobs"])
        worst["obs"] = max(worst["obs"], _ratio(o, want["obs"], tk.dz_obs(d["obs"][k])))
        worst["rew"] = max(worst["rew"], _ratio(r, want["reward"], tk.dz_rew(d["rew"][k])))
        worst["obs_abs"] = max(worst["obs_abs"], float(np.abs(o - want["obs"]).max()))
        worst["rew_abs"] = max(worst["rew_abs"], float(np.abs(r - want["reward"]).max()))
        if done.any():
            worst["tobs"] = max(worst["tobs"], _ratio(t[done], want["terminal_obs"][done], tk.dz_obs(d["tobs"][k][done])))
        # rows of envs that did not finish are neither read nor written
        rest = t[~done]
        assert np.isnan(rest).all() if inplace else np.all(rest == 7)
        assert np.array_equal(dev.get("ep_r"), want["ep_return"]) and np.array_equal(dev.get("ep_l"), want["ep_length"])
        clipped["op"] |= bool((o == f32(CFG["clip_obs"])).any()); clipped["on"] |= bool((o == f32(-CFG["clip_obs"])).any())
        clipped["rp"] |= bool((r == f32(CFG["clip_reward"])).any()); clipped["rn"] |= bool((r == f32(-CFG["clip_reward"])).any())
        assert np.abs(o).max() <= CFG["clip_obs"] and np.abs(r).max() <= CFG["clip_reward"]
    ret, ep_ret, ep_len = b.norm_env()
    assert np.array_equal(ep_ret, tk.ref.ep_ret) and np.array_equal(ep_len, tk.ref.ep_len)
    assert np.all(np.abs(ret - tk.ref.ret) <= 2 * K_STEPS * nr.U64 * max(tk.ret_max, 1e-300))
    tot = b.norm_episode_totals()
    assert tot[0] == tk.ref.totals[0] and tot[3] == tk.ref.totals[3] and tot[0] == d["done"].sum() > 0
    assert np.all(np.abs(tot - tk.ref.totals) <= 2 * (n + 8) * nr.U64 * tk.tot_mag)
    # the test cannot pass vacuously: something clipped on each side it can, episodes ended, and the constant and cancelling columns are there
    assert clipped["op"] and clipped["rp"] and (n == 1 or (clipped["on"] and clipped["rn"]))
    assert d["done"][2, 3 % n::64].all() and not d["done"][1].any()
    _report("norm step, %d envs x %d obs, %d steps%s: statistics / bound %.3g, obs / bound %.3g (|.| %.3g), reward / bound %.3g (|.| %.3g), terminal rows / bound %.3g; "
            "%d episodes" % (n, nobs, K_STEPS, " in place" if inplace else "", worst["stats"], worst["obs"],
                             worst["obs_abs"], worst["rew"], worst["rew_abs"], worst["tobs"], int(tot[0])))
    dev.free(); b.close()
    assert worst["stats"] <= 1.0
    assert worst["obs"] <= 1.0 and worst["rew"] <= 1.0 and worst["tobs"] <= 1.0


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("n", [1, 37, 64, 65, 200])
def test_step_matches_reference(hbmod, humanoid_model, gpu, n, inplace):
    assert humanoid_model.nobs == 48
    _primitive(hbmod, humanoid_model, gpu, n, inplace)


def test_step_matches_reference_30_observations(hbmod, gpu):
    m = hbmod.Model.load(TEAM_PLANE_HBM)
    assert m.nobs == 30
    _primitive(hbmod, m, gpu, 65, False)


def _run_steps(b, d, steps, dev=None):
    """the given steps of the synthetic data through hb_norm_step_dev in place; returns the outputs of the last one"""
    own = dev is None
    if own:
        dev = Dev(b, obs=d["obs"][0], rew=d["rew"][0], term=d["term"][0], trunc=d["trunc"][0])
    for k in steps:
        for key in ("obs", "rew", "term", "trunc"):
            dev.put(key, d[key][k])
        b.norm_step_dev(dev.ptr["obs"], dev.ptr["obs"], dev.ptr["rew"], dev.ptr["term"], dev.ptr["trunc"], reward_out=dev.ptr["rew"])
    out = dev.get("obs"), dev.get("rew")
    if own:
        dev.free()
    return out


def test_training_off_freezes_the_statistics(hbmod, humanoid_model, gpu):
    n, nobs = 65, humanoid_model.nobs
    d = _synthetic(n, nobs)
    b = hbmod.Batch(humanoid_model, n, gpu)
    b.norm_configure(**CFG)
    tk = Tracker(n, nobs, **CFG)
    _run_steps(b, d, range(3))
    for k in range(3):
        tk.step(d["obs"][k], d["rew"][k], d["term"][k], d["trunc"][k])
    rec = b.norm_stats()
    tot = b.norm_episode_totals()
    b.norm_configure(**dict(CFG, training=False))
    tk.ref.training = False
    o, r = _run_steps(b, d, [3])
    want = tk.step(d["obs"][3], d["rew"][3], d["term"][3], d["trunc"][3])
    assert b.norm_stats().tobytes() == rec.tobytes()
    assert _ratio(o, want["obs"], tk.dz_obs(d["obs"][3])) <= 1.0 and _ratio(r, want["reward"], tk.dz_rew(d["rew"][3])) <= 1.0
    # and they are the frozen statistics: hb_norm_obs_dev (no update, any number of rows) gives the same bits on a part of the rows
    dev = Dev(b, x=d["obs"][3][5:42], y=np.zeros((37, nobs), np.float32))
    b.norm_obs_dev(dev.ptr["x"], dev.ptr["y"], 37)
    assert np.array_equal(dev.get("y"), o[5:42])
    dev.free()
    # the monitor still counts
    assert d["done"][3].any() and b.norm_episode_totals()[0] == tot[0] + d["done"][3].sum() == tk.ref.totals[0]
    assert np.array_equal(b.norm_env()[2], tk.ref.ep_len)
    b.close()


def test_save_load_and_merge(hbmod, humanoid_model, gpu):
    nobs = humanoid_model.nobs
    d = _synthetic(64, nobs)
    cut = lambda lo, hi: {k: np.ascontiguousarray(v[:, lo:hi]) for k, v in d.items()}
    # get_stats -> set_stats on a fresh batch, then continuing, is not interrupting
    a = hbmod.Batch(humanoid_model, 64, gpu); a.norm_configure(**CFG)
    c = hbmod.Batch(humanoid_model, 64, gpu); c.norm_configure(**CFG)
    _run_steps(a, d, range(3))
    ret, ep_ret, ep_len = a.norm_env()
    c.norm_set_stats(a.norm_stats())
    assert c.norm_stats().tobytes() == a.norm_stats().tobytes()
    # (the per-env accumulators are not part of VecNormalize.save either: continue where no episode is open - after a step that ended all)
    full = dict(d, term=d["term"].copy())
    full["term"][2] = 1
    a2 = hbmod.Batch(humanoid_model, 64, gpu); a2.norm_configure(**CFG)
    c2 = hbmod.Batch(humanoid_model, 64, gpu); c2.norm_configure(**CFG)
    _run_steps(a2, full, range(3))
    c2.norm_set_stats(a2.norm_stats())
    oa, ra = _run_steps(a2, full, [3, 4])
    oc, rc = _run_steps(c2, full, [3, 4])
    assert np.array_equal(oa, oc) and np.array_equal(ra, rc) and a2.norm_stats().tobytes() == c2.norm_stats().tobytes()
    # two ranks of 37 and 27 rows, merged on the host with the update formula, against one batch of 64 on the same rows
    r1 = hbmod.Batch(humanoid_model, 37, gpu); r1.norm_configure(**CFG)
    r2 = hbmod.Batch(humanoid_model, 27, gpu); r2.norm_configure(**CFG)
    d1, d2 = cut(0, 37), cut(37, 64)
    tk = Tracker(64, nobs, **CFG)
    e1, e2 = Tracker(37, nobs, **CFG), Tracker(27, nobs, **CFG)
    for k in range(K_STEPS):
        _run_steps(r1, d1, [k]); _run_steps(r2, d2, [k])
        tk.step(d["obs"][k], d["rew"][k], d["term"][k], d["trunc"][k])
        e1.step(d1["obs"][k], d1["rew"][k], d1["term"][k], d1["trunc"][k]); e2.step(d2["obs"][k], d2["rew"][k], d2["term"][k], d2["trunc"][k])
    merged = nr.merge_records(r1.norm_stats(), r2.norm_stats(), nobs)
    # the device's two records against the reference's two records, merged the same way on the host (the merge itself: 10 u on its
    # non-negative terms, and it passes its inputs' errors on with weights below 1, the cancelling d with the absolute errors of both means)
    want = nr.merge_records(e1.ref.record(), e2.ref.record(), nobs)
    ref1, ref2 = e1.ref.record(), e2.ref.record()
    dm = np.abs(ref2[:nobs] - ref1[:nobs])
    e_mean = 2 * (e1.eo.mean + e2.eo.mean) + 10 * nr.U64 * (np.abs(want[:nobs]) + dm)
    e_var = 2 * (e1.eo.var + e2.eo.var) + 2 * dm * 2 * (e1.eo.mean + e2.eo.mean) + 10 * nr.U64 * want[nobs:2 * nobs]
    ratio = max(_ratio(merged[:nobs], want[:nobs], e_mean), _ratio(merged[nobs:2 * nobs], want[nobs:2 * nobs], e_var))
    # ... and the merged record against the single batch's: the prior (count 1e-4) is in it twice - the bound of tests/test_norm_cpu.py
    one = tk.ref.record()
    w_n = 1e-4 / (64 * K_STEPS)
    assert abs(merged[2 * nobs] - one[2 * nobs] - 1e-4) < 1e-9
    assert np.all(np.abs(merged[:nobs] - one[:nobs]) <= 2 * w_n * np.abs(one[:nobs]) + e_mean)
    assert np.all(np.abs(merged[nobs:2 * nobs] - one[nobs:2 * nobs]) <= 2 * w_n * (1 + one[:nobs] ** 2 + one[nobs:2 * nobs]) + e_var)
    _report("norm merge of 37 + 27 rows against their reference merge: / bound %.3g" % ratio)
    assert ratio <= 1.0
    for b in (a, c, a2, c2, r1, r2):
        b.close()
    assert ret.shape == ep_ret.shape == (64,) and ep_len.dtype == np.int32


# ---- collection

MAIN = ("obs", "action", "mean", "eps", "reward", "terminated", "truncated", "terminal_obs")


def _make_env(hbmod, model, n, gpu, team=False, **kw):
    """a time limit of 12.5 control steps: no episode that starts at the reset ends inside T = 8 (_age makes some older)"""
    max_time = 12.5 * float(model.opt.timestep)
    if team:
        return hbmod.VecEnv(model, n, gpu, team=True, max_time=max_time, **kw)
    return hbmod.VecEnv(model, n, gpu, realism=True, domain_randomization=True, seed=7, max_time=max_time, target_z=10.0, **kw)


def _age(hbmod, env):
    """the clocks of the odd envs are moved on by 7 control steps: they run into the time limit at step 5 of the window, are reset in place
    and step on in their new episode; the even envs do not finish inside T = 8"""
    t = env.batch.get_state(hbmod.STATE_TIME)
    t[1::2] += np.float32(7.0 * float(env.model.opt.timestep) * env.n_substeps)
    env.batch.set_state(hbmod.STATE_TIME, t)


def _tape_shapes(n, nobs, nu, steps, log_std):
    s = {"obs": (steps + 1, n, nobs), "action": (steps, n, nu), "mean": (steps, n, nu), "eps": (steps, n, nu), "reward": (steps, n),
         "terminated": (steps, n), "truncated": (steps, n), "terminal_obs": (steps, n, nobs)}
    if log_std:
        s["log_std"] = (steps, n, nu)
    return s


def _alloc_tapes(b, shapes, aux_shapes=None):
    arrays = {k: np.full(s, 0xEE if k in ("terminated", "truncated") else np.nan, np.uint8 if k in ("terminated", "truncated") else np.float32) for k, s in shapes.items()}
    for k, s in (aux_shapes or {}).items():
        arrays[k] = np.full(s, -7, np.int32) if k == "ep_length" else np.full(s, np.nan, np.float32)
    return Dev(b, **arrays)


_collections = {}


def _collection(hbmod, gpu, kind):
    """One normalised collection with all aux tapes, the reference over its raw tapes, and the replay of its recorded actions through
    hb_env_step_dev on a twin without a normaliser; computed once per kind and shared read-only.  kind: "plain" (65 envs), "pipelined"
    (128 envs in two segments), "team" (the reference's robot on its plane floor, 30 observations, 16 envs, squashed head)."""
    if kind in _collections:
        return _collections[kind]
    team = kind == "team"
    m = hbmod.Model.load(TEAM_PLANE_HBM if team else HUMANOID_HBM)
    n = 16 if team else 128 if kind == "pipelined" else 65
    head = ar.SQUASHED if team else ar.GAUSSIAN
    nobs, nu = m.nobs, m.nu
    a = _make_env(hbmod, m, n, gpu, team, normalize={})
    c = _make_env(hbmod, m, n, gpu, team)
    if kind == "pipelined":
        for e in (a, c):
            e.batch.pipeline(2)
            assert e.batch.segments == 2
    sizes = [nobs, 32, 2 * nu if team else nu]
    ws, bs = ar.make_actor(sizes, seed=5, scale=0.3)
    ls = np.linspace(-1.5, 0.3, nu).astype(np.float32)
    a.batch.actor_set(sizes, ws, bs, head=head, log_std=None if team else ls, seed=SEED)
    o0, raw0 = a.reset(), c.reset()
    assert np.array_equal(a.get_original_obs(), raw0)
    _age(hbmod, a); _age(hbmod, c)
    tk = Tracker(n, nobs)
    want0 = tk.reset(raw0)
    r0 = _ratio(o0, want0, tk.dz_obs(raw0))
    shapes = _tape_shapes(n, nobs, nu, T, team)
    aux = {"raw_obs": (T, n, nobs), "raw_reward": (T, n), "ep_return": (T, n), "ep_length": (T, n)}
    tp = _alloc_tapes(a.batch, shapes, aux)
    tp.put("obs", np.concatenate([o0[None], np.full((T, n, nobs), np.nan, np.float32)]))
    a.batch.env_collect_norm_dev(T, a.n_substeps, **tp.ptr)
    out = {k: tp.get(k) for k in tp.ptr}
    rec, totals, env_acc = a.batch.norm_stats(), a.batch.norm_episode_totals(), a.batch.norm_env()
    tp.free()
    # the replay on the twin: raw values bit for bit, and the raw terminal observations the reference needs
    b = c.batch
    ptr = Dev(b, action=np.zeros((n, nu), np.float32), obs=np.zeros((n, nobs), np.float32), reward=np.zeros(n, np.float32), te=np.zeros(n, np.uint8), tr=np.zeros(n, np.uint8))
    rep = {"obs": [], "reward": [], "terminated": [], "truncated": [], "terminal_obs": []}
    for t in range(T):
        ptr.put("action", out["action"][t])
        b.env_step_dev(ptr.ptr["action"], ptr.ptr["obs"], ptr.ptr["reward"], ptr.ptr["te"], ptr.ptr["tr"], c.n_substeps)
        for k, src in (("obs", "obs"), ("reward", "reward"), ("terminated", "te"), ("truncated", "tr")):
            rep[k].append(ptr.get(src))
        rep["terminal_obs"].append(b.env_terminal_obs())
    rep = {k: np.stack(v) for k, v in rep.items()}
    ptr.free()
    res = dict(out=out, rep=rep, o0=o0, r0=r0, tk=tk, rec=rec, totals=totals, env_acc=env_acc, n=n, nobs=nobs, nu=nu, head=head, ws=ws, bs=bs, ls=ls,
               state_a=a.batch.get_state(hbmod.STATE_INTEGRATION), state_c=b.get_state(hbmod.STATE_INTEGRATION))
    a.close(); c.close()
    _collections[kind] = res
    return res


@pytest.mark.parametrize("kind", ["plain", "pipelined", "team"])
def test_collection_matches_reference_and_replays(hbmod, gpu, kind):
    r = _collection(hbmod, gpu, kind)
    out, rep, tk, n = r["out"], r["rep"], r["tk"], r["n"]
    done = (out["terminated"] | out["truncated"]).astype(bool)
    assert done.any(axis=0).any() and not done.any(axis=0).all(), "some env must finish inside the window and some must not"
    assert done[:-1].any(), "no env stepped on in its new episode"
    assert set(np.unique(out["terminated"])) <= {0, 1} and set(np.unique(out["truncated"])) <= {0, 1}
    # the recorded actions through hb_env_step_dev on the twin: the raw tapes and the flags bit for bit, and the same final state
    assert np.array_equal(out["raw_obs"], rep["obs"]) and np.array_equal(out["raw_reward"], rep["reward"])
    assert np.array_equal(out["terminated"], rep["terminated"]) and np.array_equal(out["truncated"], rep["truncated"])
    assert np.array_equal(r["state_a"], r["state_c"])
    assert np.array_equal(out["obs"][0], r["o0"]) and r["r0"] <= 1.0
    worst = dict(obs=r["r0"], rew=0.0, tobs=0.0, mean=0.0)
    for t in range(T):
        # the actor read the normalised row: its mean against the fp64 actor on obs[t] (tests/test_gpu_collect.py's bound)
        ref = ar.actor(out["obs"][t], r["ws"], r["bs"], r["head"], log_std=r["ls"], eps=out["eps"][t].astype(np.float64))
        worst["mean"] = max(worst["mean"], float((np.abs(out["mean"][t] - ref["mean"]) / np.maximum(1.0, np.abs(ref["mean"]))).max()))
        want = tk.step(out["raw_obs"][t], out["raw_reward"][t], out["terminated"][t], out["truncated"][t], rep["terminal_obs"][t])
        worst["obs"] = max(worst["obs"], _ratio(out["obs"][t + 1], want["obs"], tk.dz_obs(out["raw_obs"][t])))
        worst["rew"] = max(worst["rew"], _ratio(out["reward"][t], want["reward"], tk.dz_rew(out["raw_reward"][t])))
        if done[t].any():
            worst["tobs"] = max(worst["tobs"], _ratio(out["terminal_obs"][t][done[t]], want["terminal_obs"][done[t]], tk.dz_obs(rep["terminal_obs"][t][done[t]])))
        # the other rows keep what the table copy put there
        assert np.array_equal(out["terminal_obs"][t][~done[t]], rep["terminal_obs"][t][~done[t]])
        assert np.array_equal(out["ep_return"][t], want["ep_return"]) and np.array_equal(out["ep_length"][t], want["ep_length"])
    stats = tk.stats_ratio(r["rec"])
    assert r["totals"][0] == tk.ref.totals[0] == done.sum() and r["totals"][3] == tk.ref.totals[3]
    assert np.all(np.abs(r["totals"] - tk.ref.totals) <= 2 * (n + 8) * nr.U64 * tk.tot_mag)
    assert np.array_equal(r["env_acc"][1], tk.ref.ep_ret) and np.array_equal(r["env_acc"][2], tk.ref.ep_len)
    _report("norm collection %s, %d envs x %d obs, T %d, %d episodes ended: statistics / bound %.3g, obs / bound %.3g, reward / bound %.3g, terminal rows / bound %.3g, "
            "actor mean on the normalised rows %.3g (bound 5e-05)" % (kind, n, r["nobs"], T, int(done.sum()), stats, worst["obs"], worst["rew"], worst["tobs"], worst["mean"]))
    assert stats <= 1.0 and worst["obs"] <= 1.0 and worst["rew"] <= 1.0 and worst["tobs"] <= 1.0
    assert worst["mean"] < 5e-5
    assert np.isfinite(out["obs"]).all() and np.abs(out["obs"]).max() <= 10.0 and np.abs(out["reward"]).max() <= 10.0


def _collect_pair(hbmod, model, gpu, n, cfg, norm):
    """one collection of T steps on a freshly made env: the main tapes (and the statistics record with a normaliser)"""
    env = _make_env(hbmod, model, n, gpu)
    nobs, nu = model.nobs, model.nu
    sizes = [nobs, 32, nu]
    ws, bs = ar.make_actor(sizes, seed=5, scale=0.3)
    env.batch.actor_set(sizes, ws, bs, head=ar.GAUSSIAN, log_std=np.linspace(-1.5, 0.3, nu).astype(np.float32), seed=SEED)
    o0 = env.reset()
    _age(hbmod, env)
    tp = _alloc_tapes(env.batch, _tape_shapes(n, nobs, nu, T, False))
    rec = None
    if norm:
        env.batch.norm_configure(**cfg)
        dev = Dev(env.batch, o=o0)
        env.batch.norm_reset_dev(dev.ptr["o"], dev.ptr["o"])
        o0 = dev.get("o")
        dev.free()
    tp.put("obs", np.concatenate([o0[None], np.full((T, n, nobs), np.nan, np.float32)]))
    if norm:
        lib_rc = hbmod.lib().hb_env_collect_norm_dev(env.batch._h, T, env.n_substeps, ctypes.byref(hbmod.HbCollectOut(**tp.ptr)), None)  # aux = NULL
        assert lib_rc == 0
        rec = env.batch.norm_stats()
    else:
        env.batch.env_collect_dev(T, env.n_substeps, **tp.ptr)
    out = {k: tp.get(k) for k in tp.ptr}
    tp.free(); env.close()
    return out, rec


def test_off_means_unchanged(hbmod, humanoid_model, gpu):
    off = dict(nr.DEFAULTS, norm_obs=False, norm_reward=False)
    plain, _ = _collect_pair(hbmod, humanoid_model, gpu, 65, None, False)
    normed, rec = _collect_pair(hbmod, humanoid_model, gpu, 65, off, True)
    for k in MAIN:
        assert plain[k].tobytes() == normed[k].tobytes(), k
    assert rec[2 * 48] == 1e-4 and abs(rec[2 * 48 + 3] - (1e-4 + 65 * T)) < 1e-9  # (obs_rms untouched; ret_rms is updated whether or not norm_reward is set)


def test_determinism(hbmod, humanoid_model, gpu):
    a, ra = _collect_pair(hbmod, humanoid_model, gpu, 65, nr.DEFAULTS, True)
    b, rb = _collect_pair(hbmod, humanoid_model, gpu, 65, nr.DEFAULTS, True)
    for k in MAIN:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert ra.tobytes() == rb.tobytes() and abs(ra[2 * 48] - (1e-4 + 65 * (T + 1))) < 1e-9


def test_composition_with_the_ppo_buffer(hbmod, humanoid_model, gpu):
    """collect_torch(T, gae=..., raw=True) with normalize on: value[t] is the critic on the normalised tape, advantage and returns are
    tests/gae_ref.py on the normalised reward tape, within the bounds of tests/test_gpu_gae.py"""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    m, n = humanoid_model, 37
    env = hbmod.VecEnv(m, n, gpu, realism=True, domain_randomization=True, seed=7, reward_kind=1, max_time=0.02, normalize={})
    asz = [tg.NOBS, 40, 24, tg.NU]
    aw, ab = ar.make_actor(asz, seed=11, scale=0.35)
    env.actor_set(asz, aw, ab, head="gaussian", log_std=tg.log_std(), seed=SEED)
    sizes, ws, bs = tg.critic("small")
    env.critic_set(sizes, ws, bs)
    o0 = env.reset()
    tk = Tracker(n, m.nobs)
    tk.reset(env.get_original_obs())
    out = {k: v.cpu().numpy() for k, v in env.collect_torch(T, gae=dict(gamma=tg.GAMMA, lam=tg.LAM), raw=True).items()}
    assert {"ep_return", "ep_length", "raw_obs", "raw_reward", "value", "advantage", "returns", "log_prob", "terminal_obs"} <= set(out)
    assert np.array_equal(out["obs"][0], o0)
    te, tr = out["terminated"], out["truncated"]
    boot = tr & ~te
    assert boot.any()
    for t in range(T):  # the tapes are the normalised ones
        want = tk.step(out["raw_obs"][t], out["raw_reward"][t], te[t], tr[t])
        assert _ratio(out["obs"][t + 1], want["obs"], tk.dz_obs(out["raw_obs"][t])) <= 1.0
        assert _ratio(out["reward"][t], want["reward"], tk.dz_rew(out["raw_reward"][t])) <= 1.0
    tp = {k: np.ascontiguousarray(out[k].astype(np.uint8) if out[k].dtype == bool else out[k]) for k in tg.TAPES if k in out}
    v64 = gr.values(out["obs"], ws, bs)
    tv64 = np.zeros((T, n))
    tv64[boot] = gr.values(out["terminal_obs"][boot], ws, bs)
    e_v = float((np.abs(out["value"] - v64) / np.maximum(1.0, np.abs(v64))).max())
    hand = tg.run(env.batch, T, tp, tapes=tuple(tp))
    _, _, b_adv, b_ret = tg.scan_bounds(tp, hand["value"], hand["terminal_value"], tg.GAMMA, tg.LAM)
    adv64, ret64, _, _ = tg.scan_bounds(tp, v64, tv64, tg.GAMMA, tg.LAM)
    eps_v = tg.VALUE_TOL * max(1.0, float(np.abs(v64).max()), float(np.abs(tv64).max()))
    b_adv64 = (1.0 + 2.0 * tg.GAMMA) * eps_v / (1.0 - tg.GAMMA * tg.LAM) + b_adv
    e_adv, e_ret = float(np.abs(out["advantage"] - adv64).max()), float(np.abs(out["returns"] - ret64).max())
    _report("norm + gae on a collection (%d envs, T %d): value on the normalised tape %.3g (bound %.0e), advantage %.3g (%.3g), returns %.3g (%.3g)"
            % (n, T, e_v, tg.VALUE_TOL, e_adv, b_adv64, e_ret, b_adv64 + eps_v + (b_ret - b_adv)))
    assert e_v <= tg.VALUE_TOL
    assert e_adv <= b_adv64 and e_ret <= b_adv64 + eps_v + (b_ret - b_adv)
    env.close()


def test_vecenv_surface(hbmod, humanoid_model, gpu, tmp_path):
    m, n = humanoid_model, 37
    mk = lambda **kw: hbmod.VecEnv(m, n, gpu, realism=True, domain_randomization=True, seed=7, max_time=0.012, target_z=10.0, **kw)
    env, twin = mk(normalize=dict(clip_obs=5.0)), mk()
    tk = Tracker(n, m.nobs, clip_obs=5.0)
    o, raw = env.reset(), twin.reset()
    assert np.array_equal(env.get_original_obs(), raw) and _ratio(o, tk.reset(raw), tk.dz_obs(raw)) <= 1.0
    rng = np.random.default_rng(0)
    seen_episode = False
    for step in range(4):
        act = rng.uniform(-1, 1, size=(n, m.nu)).astype(np.float32)
        o, r, done, infos = env.step(act)
        ro, rr, rdone, rinfos = twin.step(act)
        # normalize=None returns the same arrays as today: the twin's are the raw values of the normalised env
        assert np.array_equal(env.get_original_obs(), ro) and np.array_equal(env.get_original_reward(), rr) and np.array_equal(done, rdone)
        rtobs = np.zeros((n, m.nobs), np.float32)
        for i in np.flatnonzero(rdone):
            rtobs[i] = rinfos[i]["terminal_observation"]
        te = np.array([bool(d and not infos[i]["TimeLimit.truncated"]) for i, d in enumerate(done)])
        want = tk.step(ro, rr, te, done & ~te, rtobs)
        assert _ratio(o, want["obs"], tk.dz_obs(ro)) <= 1.0 and _ratio(r, want["reward"], tk.dz_rew(rr)) <= 1.0
        for i in range(n):
            if done[i]:
                seen_episode = True
                assert infos[i]["episode"] == {"r": float(want["ep_return"][i]), "l": int(want["ep_length"][i])}
                assert _ratio(infos[i]["terminal_observation"], want["terminal_obs"][i], tk.dz_obs(rtobs[i])) <= 1.0
                assert "episode" not in rinfos[i]
            else:
                assert "episode" not in infos[i]
    assert seen_episode
    # training = False freezes the statistics; normalize_obs uses them; save / load carries them to another env
    env.training = False
    assert env.training is False
    rec = env.batch.norm_stats()
    o, r, done, infos = env.step(rng.uniform(-1, 1, size=(n, m.nu)).astype(np.float32))
    assert env.batch.norm_stats().tobytes() == rec.tobytes()
    assert np.array_equal(env.normalize_obs(env.get_original_obs()), o)
    env.save_normalization(str(tmp_path / "norm.npz"))
    other = mk(normalize={})
    other.load_normalization(str(tmp_path / "norm.npz"))
    assert other.batch.norm_stats().tobytes() == rec.tobytes()
    with pytest.raises(RuntimeError):
        twin.normalize_obs(o)
    for e in (env, twin, other):
        e.close()


def test_argument_checks(hbmod, humanoid_model, gpu):
    m, n = humanoid_model, 37
    L, b = hbmod.lib(), hbmod.Batch(humanoid_model, 37, gpu)
    nobs = m.nobs
    d = _synthetic(n, nobs)
    dev = Dev(b, obs=d["obs"][0], rew=d["rew"][0], term=d["term"][0], trunc=d["trunc"][0], out=np.full((n, nobs), 7, np.float32))
    io = lambda **kw: hbmod.HbNormIo(**dict(dict(obs_in=dev.ptr["obs"], obs_out=dev.ptr["out"], reward_in=dev.ptr["rew"], terminated=dev.ptr["term"], truncated=dev.ptr["trunc"]), **kw))
    stats = np.zeros(2 * nobs + 4)
    sp = stats.ctypes.data_as(ctypes.c_void_p)
    # no normaliser configured: every call is refused
    assert L.hb_norm_step_dev(b._h, ctypes.byref(io())) == -1 and L.hb_norm_reset_dev(b._h, dev.ptr["obs"], dev.ptr["out"]) == -1
    assert L.hb_norm_obs_dev(b._h, dev.ptr["obs"], dev.ptr["out"], n) == -1 and L.hb_norm_get_stats(b._h, sp) == -1 and L.hb_norm_set_stats(b._h, sp) == -1
    assert L.hb_norm_get_env(b._h, None, None, None) == -1 and L.hb_norm_episode_totals(b._h, sp) == -1
    asz = [nobs, 8, m.nu]
    aw, ab = ar.make_actor(asz, seed=1)
    b.actor_set(asz, aw, ab, head=ar.GAUSSIAN, log_std=np.zeros(m.nu, np.float32), seed=1)
    tp = _alloc_tapes(b, _tape_shapes(n, nobs, m.nu, 2, False))
    tp.put("obs", np.zeros((3, n, nobs), np.float32))
    co = hbmod.HbCollectOut(**tp.ptr)
    assert L.hb_env_collect_norm_dev(b._h, 2, 1, ctypes.byref(co), None) == -1
    # configuration
    bad = [dict(clip_obs=0.0), dict(clip_obs=-1.0), dict(clip_obs=np.inf), dict(clip_reward=0.0), dict(clip_reward=np.nan), dict(epsilon=0.0), dict(epsilon=np.inf),
           dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=np.nan)]
    mkcfg = lambda **kw: hbmod.HbNormConfig(**dict(dict(norm_obs=1, norm_reward=1, training=1, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8), **kw))
    for kw in bad:
        assert L.hb_norm_configure(b._h, ctypes.byref(mkcfg(**kw))) == -1, kw
    assert L.hb_norm_get_stats(b._h, sp) == -1  # (none of them installed anything)
    assert L.hb_norm_configure(None, ctypes.byref(mkcfg())) == -1
    b.norm_configure(**CFG)
    _run_steps(b, d, [0])
    rec = b.norm_stats()
    acc = b.norm_env()
    same = lambda: b.norm_stats().tobytes() == rec.tobytes() and all(np.array_equal(x, y) for x, y in zip(b.norm_env(), acc))
    for kw in bad:  # a refused reconfiguration changes nothing
        assert L.hb_norm_configure(b._h, ctypes.byref(mkcfg(**kw))) == -1 and same(), kw
    # NULL required pointers, half a terminal pair
    for kw in (dict(obs_in=None), dict(obs_out=None), dict(reward_in=None), dict(terminated=None), dict(truncated=None), dict(terminal_obs_in=dev.ptr["obs"]),
               dict(terminal_obs_out=dev.ptr["out"])):
        assert L.hb_norm_step_dev(b._h, ctypes.byref(io(**kw))) == -1 and same(), kw
    assert L.hb_norm_step_dev(b._h, None) == -1 and L.hb_norm_step_dev(None, ctypes.byref(io())) == -1
    assert L.hb_norm_reset_dev(b._h, None, dev.ptr["out"]) == -1 and L.hb_norm_reset_dev(b._h, dev.ptr["obs"], None) == -1
    assert L.hb_norm_obs_dev(b._h, None, dev.ptr["out"], n) == -1 and L.hb_norm_obs_dev(b._h, dev.ptr["obs"], None, n) == -1
    assert L.hb_norm_obs_dev(b._h, dev.ptr["obs"], dev.ptr["out"], 0) == -1 and same()
    assert np.all(dev.get("out") == 7)  # a refused call writes nothing
    # collection: T < 1, and what hb_env_collect_dev refuses
    assert L.hb_env_collect_norm_dev(b._h, 0, 1, ctypes.byref(co), None) == -1 and L.hb_env_collect_norm_dev(b._h, 2, 0, ctypes.byref(co), None) == -1
    assert L.hb_env_collect_norm_dev(b._h, 2, 1, None, None) == -1 and same()
    assert np.isnan(tp.get("action")).all()
    # set_stats: a non-finite statistic, a negative var or count
    assert L.hb_norm_get_stats(b._h, None) == -1 and L.hb_norm_set_stats(b._h, None) == -1 and L.hb_norm_episode_totals(b._h, None) == -1
    for idx, val in ((0, np.nan), (3, np.inf), (nobs + 2, -1e-9), (nobs + 2, np.nan), (2 * nobs, -1.0), (2 * nobs + 1, np.inf), (2 * nobs + 2, -1.0), (2 * nobs + 3, -1e-4)):
        r2 = rec.copy()
        r2[idx] = val
        assert L.hb_norm_set_stats(b._h, r2.ctypes.data_as(ctypes.c_void_p)) == -1 and same(), (idx, val)
    # cfg = NULL removes the normaliser and its statistics; a new one starts from the prior
    b.norm_configure(None)
    assert L.hb_norm_get_stats(b._h, sp) == -1
    b.norm_configure(**CFG)
    fresh = b.norm_stats()
    assert np.all(fresh[:nobs] == 0) and np.all(fresh[nobs:2 * nobs] == 1) and list(fresh[2 * nobs:]) == [1e-4, 0.0, 1.0, 1e-4] and not b.norm_episode_totals().any()
    tp.free(); dev.free(); b.close()
