"""The PPO learner on the device (include/hb.h: hb_learner_*, hb_ppo_grad_dev, hb_ppo_adam_dev) against the fp64 reference of
tests/ppo_ref.py, at the GPU's own downloaded parameters.  Batches of 16 envs, synthetic tapes of random rows (no physics).

Bounds, u = 2^-24:
 (a) derived from the arithmetic, by row and summed (ppo_lib.derived): the statistics, the top-layer bias gradients of both networks and the
     log_std gradient.  The forward error of a network follows its layers (mlp_ref.fwd_err: a K-term f32 MFMA chain and the bias, then
     the error carried in, 4 u behind tanhf).  From the error of mean and value: log-probability, ratio (expf at
     1 ulp), the loss terms, dloss/dmean, dloss/dlog_std, dloss/dvalue, each a handful of f32 roundings; a row whose ratio stands within
     its error of a clip bound may take the other branch and counts with its whole term.  Row sums: n u sum|x| for n f32 additions.
 (b) the back-propagated gradients (every W, the hidden biases), per tensor: max|g_gpu - g_64| <= k max|g_64| with k = 8 x the float32
     noise floor, the floor being max|g_32 - g_64| / max|g_64| of torch's CPU float32 autograd on the same inputs - an independent
     single-precision evaluation; 8: summation order, MFMA accumulation and tanhf / expf differ.  k is one number per network and
     minibatch: the largest floor over the tensors that are held to it (the tensors of tier (a) do not enter).
 (c) Adam: the kernel forms the step in fp64 from the fp32 gradient, moments and parameter and rounds each result once, so against the
     fp64 reference fed the same downloaded values: |m - m_ref| <= u |m_ref|, |v - v_ref| <= u |v_ref| (the rounding), and
     |p - p_ref| <= ulp(p) / 2 + 2^-36 |delta p|: some 30 fp64 roundings and pow / sqrt at a few ulp give 2^-47, which 1 / (1 - b2^t),
     1000 at t = 1, can amplify to 2^-37.
HB_PPO_PARITY_OUT=<file> collects the measured values (profiles/ppo_parity.txt)."""
import ctypes

import numpy as np
import pytest

import ppo_ref as pr
from oracle_lib import HUMANOID_HBM  # noqa: F401  (the model of the humanoid_model fixture)
from ppo_lib import NETS, NOBS, NU, TAPES, Dev, U, cfg as _cfg, check_case as _check_case  # noqa: F401
from step_lib import report

pytestmark = pytest.mark.gpu

C32 = float(np.float32(0.2))  # (what the C struct holds: the reference gets the same number)


def _report(line):
    report(line, "HB_PPO_PARITY_OUT")


_problems = {}


def _problem(net, n_rows, seed=1):
    key = (net, n_rows, seed)
    if key not in _problems:
        _problems[key] = pr.random_problem(*NETS[net], n_rows, seed=seed)
    return _problems[key]


def _learner(hbmod, m, gpu, net, flat, **cfg):
    asz, csz = NETS[net]
    t = pr.split(flat.astype(np.float32), asz, csz, NU)
    b = hbmod.Batch(m, 16, gpu)
    b.actor_set(asz, [t["actor.w%d" % l] for l in range(len(asz) - 1)], [t["actor.b%d" % l] for l in range(len(asz) - 1)], head="gaussian",
                log_std=t["log_std"], seed=3)
    b.critic_set(csz, [t["critic.w%d" % l] for l in range(len(csz) - 1)], [t["critic.b%d" % l] for l in range(len(csz) - 1)])
    b.learner_create(**cfg)
    return b


def _cases(n_rows):
    """(name, index or None, first, mb): the minibatch shapes and index forms"""
    import humanoid_mujoco_amd.engine as eng
    ch = eng.ppo_row_chunk(50)
    rng = np.random.default_rng(9)
    asc = np.sort(rng.permutation(n_rows)[:50])
    rep = rng.permutation(n_rows)[:17]
    rep[5] = rep[11]
    return [("mb1", None, 7, 1), ("mb5_desc", np.arange(n_rows - 1, n_rows - 6, -1), 0, 5), ("mb16_first", None, 3, 16), ("mb17_repeat", rep, 0, 17),
            ("mb50_asc_gaps", asc, 0, 50), ("chunk-1", rng.permutation(n_rows)[:ch - 1], 0, ch - 1), ("chunk", None, n_rows - ch, ch),
            ("chunk+1", rng.permutation(n_rows)[:ch + 1], 0, ch + 1)]


@pytest.mark.parametrize("net", sorted(NETS))
def test_gradients_and_statistics(hbmod, humanoid_model, gpu, net):
    pytest.importorskip("torch")
    flat, rows = _problem(net, 96)
    cfg = _cfg(ent_coef=0.01)
    b = _learner(hbmod, humanoid_model, gpu, net, flat, **cfg)
    assert np.array_equal(b.learner_params(), flat.astype(np.float32))  # the flat layout is what the networks were installed from
    flat = b.learner_params().astype(np.float64)
    worst = dict(stat=0.0, head=0.0, floor=0.0, k=0.0, ratio=0.0, rel=0.0)
    for name, index, first, mb in _cases(96):
        if mb == 1:  # a row that carries a policy gradient (a clipped one has none: the second single row below)
            glp = [pr.loss_and_grads(flat, *NETS[net], rows, cfg, first=r, mb=1)[2]["glp"][0] for r in range(96)]
            first = int(np.flatnonzero(np.asarray(glp) != 0.0)[0])
            clipped = np.flatnonzero(np.asarray(glp) == 0.0)
            if len(clipped):
                _check_case(b, net, flat, rows, "mb1_clipped", None, int(clipped[0]), 1, cfg, worst)
        _check_case(b, net, flat, rows, name, index, first, mb, cfg, worst)
    b.learner_configure(normalize_advantage=0)
    _check_case(b, net, flat, rows, "mb50_raw_advantage", np.random.default_rng(2).permutation(96)[:50], 0, 50, _cfg(ent_coef=0.01, normalize_advantage=0), worst)
    b.close()
    _report("ppo gradients %-9s: statistics %.3f, head gradients %.3f of their derived bounds; back-propagated tensors: float32 floor %.2e, "
            "measured %.2e, k = %.2e (worst measured / k %.3f)" % (net, worst["stat"], worst["head"], worst["floor"], worst["ratio"], worst["k"], worst["rel"]))


def test_many_chunks_beyond_4096_rows(hbmod, humanoid_model, gpu):
    """above 4096 rows the chunk grows with mb (at most 64 chunks): 4100 contiguous rows from first = 3, chunks of 80"""
    pytest.importorskip("torch")
    import humanoid_mujoco_amd.engine as eng
    net, mb = "small", 4100
    assert eng.ppo_row_chunk(mb) == 80
    flat, rows = _problem(net, mb + 5, seed=4)
    cfg = _cfg()
    b = _learner(hbmod, humanoid_model, gpu, net, flat, **cfg)
    worst = dict(stat=0.0, head=0.0, floor=0.0, k=0.0, ratio=0.0, rel=0.0)
    _check_case(b, net, flat, rows, "mb4100", None, 3, mb, cfg, worst)
    b.close()
    _report("ppo gradients small, 4100 rows: statistics %.3f, head gradients %.3f of their derived bounds; float32 floor %.2e, measured %.2e, k = %.2e"
            % (worst["stat"], worst["head"], worst["floor"], worst["ratio"], worst["k"]))


def _state64(b):
    s = b.learner_state()
    return {k: (s[k].astype(np.float64) if k != "t" else s[k]) for k in s}


def test_adam_in_isolation(hbmod, humanoid_model, gpu):
    net = "small"
    asz, csz = NETS[net]
    flat, rows = _problem(net, 96)
    cfg = _cfg(lr=1e-3)
    b = _learner(hbmod, humanoid_model, gpu, net, flat, **cfg)
    d = Dev(b, rows)
    worst = 0.0
    for step, scale in enumerate((0.5, 2.0, 0.0)):  # clipping active, inactive, switched off
        g, _ = d.grad(50, first=step)
        gn = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
        cfg = _cfg(lr=1e-3, max_grad_norm=scale * gn)
        b.learner_configure(**cfg)
        s0 = _state64(b)
        assert s0["t"] == step
        b.ppo_adam_dev(stats=d.stats)
        s1, st = _state64(b), b.from_dev(d.stats, (16,))
        p, m, v, t, gn_ref, skipped = pr.adam_step(s0["params"], s0["m"], s0["v"], s0["t"], g, cfg)
        sc = pr.clip_scale(gn_ref, cfg["max_grad_norm"])
        assert (sc < 0.6) if step == 0 else (sc == 1.0)
        assert s1["t"] == t == step + 1 and st[10] == 0.0 and abs(st[6] - gn_ref) <= 2 * U * gn_ref
        assert (np.abs(s1["m"] - m) <= U * np.abs(m) + 1e-45).all() and (np.abs(s1["v"] - v) <= U * np.abs(v) + 1e-45).all()
        bound = 0.5 * np.maximum(np.spacing(np.abs(p).astype(np.float32)), np.spacing(np.abs(s1["params"]).astype(np.float32))) + 2.0 ** -36 * np.abs(p - s0["params"])
        worst = max(worst, float((np.abs(s1["params"] - p) / bound).max()))
        assert (np.abs(s1["params"] - p) <= bound).all(), (step, worst)
        assert np.abs(p - s0["params"]).max() > 1e-4  # (the step is there)
        assert np.array_equal(b.learner_params().astype(np.float64), s1["params"])
    # a non-finite gradient: skipped is set, parameters, moments and t stay
    bad = dict(rows)
    bad["advantage"] = rows["advantage"].copy()
    bad["advantage"][7] = np.inf
    d2 = Dev(b, bad)
    s0 = b.learner_state()
    d2.grad(50)
    b.ppo_adam_dev(stats=d2.stats)
    st, s1 = b.from_dev(d2.stats, (16,)), b.learner_state()
    assert st[10] == 1.0 and not np.isfinite(st[6]) and s1["t"] == s0["t"] == 3
    assert all(np.array_equal(s0[k], s1[k]) for k in ("params", "m", "v"))
    # and the next good step counts on from there
    d.grad(50)
    b.ppo_adam_dev(stats=d.stats)
    assert b.learner_state()["t"] == 4 and b.from_dev(d.stats, (16,))[10] == 0.0
    d.free(); d2.free()
    b.close()
    _report("ppo adam small: worst |p - p_ref| / (ulp / 2 + 2^-36 |delta p|) over three steps %.3f" % worst)


def _values(b, obs):
    """the critic over [17, 16, nobs] observation rows through hb_collect_gae_dev (T = 16)"""
    T, n = 16, 16
    po, pv = b.dev_alloc(obs.nbytes), b.dev_alloc((T + 1) * n * 4)
    b.to_dev(po, obs)
    b.collect_gae_dev(T, 0.99, 0.95, False, obs=po, value=pv)
    out = b.from_dev(pv, (T + 1, n))
    b.dev_free(po); b.dev_free(pv)
    return out


def test_repeatability_purity_and_padding(hbmod, humanoid_model, gpu):
    net = "small"
    flat, rows = _problem(net, 96)
    b = _learner(hbmod, humanoid_model, gpu, net, flat, **_cfg(lr=1e-3))
    b.reset(perturb=True)
    ctrl = np.zeros((16, humanoid_model.nu), np.float32)
    b.step(ctrl)
    idx = np.random.default_rng(5).permutation(96)[:65]
    d = Dev(b, rows, idx)
    before = (b.get_state(hbmod.STATE_INTEGRATION), b.last_kernel(), b.step_launches(), b.status().copy(), b.learner_state())
    g1, s1 = d.grad(65)
    g2, s2 = d.grad(65)
    assert np.array_equal(g1, g2) and np.array_equal(s1, s2) and np.abs(g1).max() > 0
    after = (b.get_state(hbmod.STATE_INTEGRATION), b.last_kernel(), b.step_launches(), b.status().copy(), b.learner_state())
    assert np.array_equal(before[0], after[0]) and before[1:3] == after[1:3] and np.array_equal(before[3], after[3])
    assert before[4]["t"] == after[4]["t"] and all(np.array_equal(before[4][k], after[4][k]) for k in ("params", "m", "v"))
    # three steps, then the packed operands re-made from the flat record (zero padded by construction): the same bits everywhere
    a, kw = d.args(65)
    for _ in range(3):
        b.ppo_minibatch_dev(*a, **kw)
    obs = np.random.default_rng(6).normal(size=(17, 16, NOBS)).astype(np.float32)
    g3, s3, v3 = *d.grad(65), _values(b, obs)
    b.learner_set_params(b.learner_params())
    g4, s4, v4 = *d.grad(65), _values(b, obs)
    assert np.array_equal(g3, g4) and np.array_equal(s3, s4) and np.array_equal(v3, v4) and np.isfinite(v3).all()
    assert not np.array_equal(g3, g1)
    d.free()
    b.close()


def test_checkpoint_and_resume(hbmod, humanoid_model, gpu):
    net = "mixed"
    flat, rows = _problem(net, 96)
    b = _learner(hbmod, humanoid_model, gpu, net, flat, **_cfg(lr=1e-3))
    d = Dev(b, rows)
    a, kw = d.args(40, first=10)
    b.ppo_minibatch_dev(*a, **kw)
    ck = b.learner_state()
    assert ck["t"] == 1

    def two():
        for first in (0, 50):
            aa, kk = d.args(40, first=first)
            b.ppo_minibatch_dev(*aa, **kk)
        return b.learner_state()
    x = two()
    b.learner_set_state(ck)
    y = two()
    assert x["t"] == y["t"] == 3 and all(np.array_equal(x[k], y[k]) for k in ("params", "m", "v")) and not np.array_equal(x["params"], ck["params"])
    d.free()
    b.close()


def _torch_env(hbmod, m, gpu, n, net="mixed", seed=1, **cfg):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    asz, csz = NETS[net]
    flat, _ = _problem(net, 8, seed=seed)
    t = pr.split(flat.astype(np.float32), asz, csz, NU)
    env = hbmod.VecEnv(m, n, gpu, realism=True, domain_randomization=True, seed=7)
    env.actor_set(asz, [t["actor.w%d" % l] for l in range(len(asz) - 1)], [t["actor.b%d" % l] for l in range(len(asz) - 1)], head="gaussian", log_std=t["log_std"])
    env.critic_set(csz, [t["critic.w%d" % l] for l in range(len(csz) - 1)], [t["critic.b%d" % l] for l in range(len(csz) - 1)])
    env.learner(**cfg)
    env.reset()
    return env, flat.astype(np.float32)


def test_the_updated_networks_are_the_ones_that_run(hbmod, humanoid_model, gpu):
    import actor_ref as ar
    import gae_ref as gr
    net = "mixed"
    asz, csz = NETS[net]
    env, flat0 = _torch_env(hbmod, humanoid_model, gpu, 64, net, lr=1e-2)
    gae = dict(gamma=0.99, lam=0.95)
    buf = env.collect_torch(8, gae=gae)
    log = env.ppo_update(buf, n_epochs=2, batch_size=128)
    assert log["n_minibatches"] == 8 and log["n_updates"] == 2 and log["skipped"] == 0.0 and np.isfinite(list(v for v in log.values())).all()
    flat = env.batch.learner_params()
    assert env.batch.learner_state()["t"] == 8
    t = pr.split(flat.astype(np.float64), asz, csz, NU)
    assert np.abs(flat - flat0).max() > 1e-3 and np.abs(t["log_std"] - pr.split(flat0, asz, csz, NU)["log_std"]).max() > 1e-3
    out = {k: v.cpu().numpy() for k, v in env.collect_torch(8, gae=gae).items()}
    ws, bs = [t["actor.w%d" % l] for l in range(2)], [t["actor.b%d" % l] for l in range(2)]
    mean64 = ar.network(out["obs"][:8].astype(np.float64), ws, bs, ar.GAUSSIAN)
    assert (np.abs(out["mean"] - mean64) <= 5e-5 * np.maximum(1.0, np.abs(mean64))).all()
    ls32 = t["log_std"].astype(np.float32)
    noise = np.exp(ls32.astype(np.float64)) * out["eps"].astype(np.float64)
    assert (np.abs((out["action"].astype(np.float64) - out["mean"]) - noise) <= 4 * U * (np.abs(noise) + np.abs(out["mean"]) + np.abs(out["action"]))).all()
    v64 = gr.values(out["obs"], [t["critic.w%d" % l] for l in range(2)], [t["critic.b%d" % l] for l in range(2)])
    assert (np.abs(out["value"] - v64) <= 5e-5 * np.maximum(1.0, np.abs(v64))).all()
    lp = gr.log_prob(ar.GAUSSIAN, out["eps"], ls32)
    assert (np.abs(out["log_prob"] - lp) <= (NU + 3) * U * (0.5 * out["eps"].astype(np.float64) ** 2 + np.abs(ls32) + 0.5 * gr.LOG_2PI).sum(axis=-1)).all()
    env.close()


def test_grad_dev_leaves_the_draw_counter(hbmod, humanoid_model, gpu):
    """two identically seeded envs: one runs hb_ppo_grad_dev between two collections, the other does not; the second collections -
    whose draws are indexed by the batch's draw counter - are the same bits"""
    a, _ = _torch_env(hbmod, humanoid_model, gpu, 32)
    c, _ = _torch_env(hbmod, humanoid_model, gpu, 32)
    import torch
    gae = dict(gamma=0.99, lam=0.95)
    bufa = a.collect_torch(4, gae=gae)
    c.collect_torch(4, gae=gae)
    tapes = [bufa["obs"][:4], bufa["action"], bufa["log_prob"], bufa["advantage"], bufa["returns"]]
    torch.cuda.synchronize()
    a.batch.ppo_grad_dev(*[x.data_ptr() for x in tapes], 128, 100, first=5)
    assert np.abs(a.batch.learner_grads()).max() > 0
    first_eps = bufa["eps"].cpu().numpy().copy()
    ra = {k: v.cpu().numpy() for k, v in a.collect_torch(4, gae=gae).items()}
    rc = {k: v.cpu().numpy() for k, v in c.collect_torch(4, gae=gae).items()}
    assert np.abs(ra["eps"]).max() > 0 and not np.array_equal(ra["eps"], first_eps)  # (the counter moved on from the first collection)
    for k in ra:
        assert np.array_equal(ra[k], rc[k]), k
    a.close()
    c.close()


@pytest.mark.parametrize("how", ["critic_other_sizes", "learner_create_again", "critic_same_sizes"])
def test_trained_log_std_survives_the_learner(hbmod, humanoid_model, gpu, how):
    """after Adam steps the device's log_std is newer than the actor's config; whatever then replaces or destroys the learner without
    installing a new actor, the next collection samples with the TRAINED log_std: action - mean == exp(log_std) eps"""
    import actor_ref as ar
    import gae_ref as gr
    net = "mixed"
    asz, csz = NETS[net]
    env, flat0 = _torch_env(hbmod, humanoid_model, gpu, 32, net, lr=2e-2)
    gae = dict(gamma=0.99, lam=0.95)
    env.ppo_update(env.collect_torch(4, gae=gae), n_epochs=2, batch_size=64)
    trained = pr.split(env.batch.learner_params(), asz, csz, NU)["log_std"]
    first = pr.split(flat0, asz, csz, NU)
    assert np.abs(trained - first["log_std"]).max() > 1e-2
    if how == "critic_other_sizes":
        env.critic_set([NOBS, 8, 1], [np.zeros((NOBS, 8), np.float32), np.zeros((8, 1), np.float32)], [np.zeros(8, np.float32), np.zeros(1, np.float32)])
        assert hbmod.lib().hb_learner_param_count(env.batch._h) == -1  # the learner is gone
    elif how == "critic_same_sizes":
        env.critic_set(csz, [first["critic.w%d" % l] for l in range(2)], [first["critic.b%d" % l] for l in range(2)])
        assert np.array_equal(pr.split(env.batch.learner_params(), asz, csz, NU)["log_std"], trained)
    else:
        env.batch.learner_create()
        st = env.batch.learner_state()
        assert np.array_equal(pr.split(st["params"], asz, csz, NU)["log_std"], trained) and st["t"] == 0 and not st["m"].any()
    out = {k: v.cpu().numpy() for k, v in env.collect_torch(4, gae=gae).items()}
    eps, delta = out["eps"].astype(np.float64), out["action"].astype(np.float64) - out["mean"]
    noise = np.exp(trained.astype(np.float64)) * eps
    assert (np.abs(delta - noise) <= 4 * U * (np.abs(noise) + np.abs(out["mean"]) + np.abs(out["action"]))).all()
    assert np.abs(delta - np.exp(first["log_std"].astype(np.float64)) * eps).max() > 1e-3   # (the check tells the two apart)
    lp = gr.log_prob(ar.GAUSSIAN, out["eps"], trained)
    assert (np.abs(out["log_prob"] - lp) <= (NU + 3) * U * (0.5 * eps ** 2 + np.abs(trained) + 0.5 * gr.LOG_2PI).sum(axis=-1)).all()
    env.close()


def test_ppo_update_partition_seed_and_target_kl(hbmod, humanoid_model, gpu):
    env, _ = _torch_env(hbmod, humanoid_model, gpu, 64, lr=1e-3)
    plan = env.ppo_minibatches(300, 128, 2, seed=5, update=0)
    again = env.ppo_minibatches(300, 128, 2, seed=5, update=0)
    other = env.ppo_minibatches(300, 128, 2, seed=5, update=1)
    for (perm, cuts), (perm2, _), (perm3, _) in zip(plan, again, other):
        p = perm.cpu().numpy()
        assert cuts == [(0, 128), (128, 128), (256, 44)] and sorted(p.tolist()) == list(range(300)) and p.dtype == np.int32
        assert np.array_equal(p, perm2.cpu().numpy()) and not np.array_equal(p, perm3.cpu().numpy())
    assert not np.array_equal(plan[0][0].cpu().numpy(), plan[1][0].cpu().numpy())
    buf = env.collect_torch(8, gae=dict(gamma=0.99, lam=0.95))
    st0 = env.batch.learner_state()
    a = env.ppo_update(buf, n_epochs=1, batch_size=200, seed=11)
    assert a["n_minibatches"] == 3 and not a["early_stop"]
    st1 = env.batch.learner_state()
    env.batch.learner_set_state(st0)
    env._ppo_updates -= 1
    b2 = env.ppo_update(buf, n_epochs=1, batch_size=200, seed=11)
    st2 = env.batch.learner_state()
    assert all(np.array_equal(st1[k], st2[k]) for k in ("params", "m", "v")) and a["loss"] == b2["loss"]
    # a deliberately stale old_log_prob: approx_kl of the first minibatch is far above the target, and no step is taken
    stale = dict(buf)
    stale["log_prob"] = buf["log_prob"] - 0.5
    before = env.batch.learner_state()
    c = env.ppo_update(stale, n_epochs=3, batch_size=200, target_kl=0.01)
    kl_first = float(np.exp(0.5) - 1.0 - 0.5)
    assert c["early_stop"] and c["n_minibatches"] == 0 and c["approx_kl"] > 1.5 * 0.01 and abs(c["approx_kl"] - kl_first) < 0.05
    after = env.batch.learner_state()
    assert after["t"] == before["t"] and np.array_equal(after["params"], before["params"])
    dd = env.ppo_update(buf, n_epochs=1, batch_size=512, target_kl=10.0)
    assert not dd["early_stop"] and dd["n_minibatches"] == 1 and env.batch.learner_state()["t"] == before["t"] + 1
    env.close()


def test_argument_checks_and_set_mlp_with_a_learner(hbmod, humanoid_model, gpu):
    import humanoid_mujoco_amd.engine as eng
    L = hbmod.lib()
    net = "mixed"
    asz, csz = NETS[net]
    flat, rows = _problem(net, 96)
    t = pr.split(flat.astype(np.float32), asz, csz, NU)
    aw, ab = [t["actor.w%d" % l] for l in range(2)], [t["actor.b%d" % l] for l in range(2)]
    cw, cb = [t["critic.w%d" % l] for l in range(2)], [t["critic.b%d" % l] for l in range(2)]
    b = hbmod.Batch(humanoid_model, 16, gpu)
    cfg = eng.HbPpoConfig()
    L.hb_ppo_default_config(ctypes.byref(cfg))
    assert L.hb_learner_create(b._h, ctypes.byref(cfg)) == -1          # no actor, no critic
    b.actor_set(asz, aw, ab, head="gaussian", log_std=t["log_std"])
    assert L.hb_learner_create(b._h, ctypes.byref(cfg)) == -1          # no critic
    b.critic_set(csz, cw, cb)
    assert L.hb_learner_create(b._h, None) == -1
    assert L.hb_ppo_adam_dev(b._h, None) == -1 and L.hb_learner_destroy(b._h) == -1 and L.hb_learner_param_count(b._h) == -1  # no learner
    d0 = Dev(b, rows)
    assert L.hb_learner_configure(b._h, ctypes.byref(cfg)) == -1
    assert L.hb_ppo_grad_dev(b._h, ctypes.byref(eng.HbPpoRows(*[d0.ptr[k] for k in TAPES], None, 96, 0, 40)), None) == -1
    assert L.hb_ppo_minibatch_dev(b._h, ctypes.byref(eng.HbPpoRows(*[d0.ptr[k] for k in TAPES], None, 96, 0, 40)), None) == -1
    d0.free()
    for k, bad in (("clip_range", 0.0), ("clip_range", float("nan")), ("beta1", 1.0), ("beta2", -0.1), ("lr", -1e-3), ("eps", 0.0), ("vf_coef", float("inf"))):
        with pytest.raises(hbmod.HbError):
            b.learner_create(**{k: bad})
    sq = [NOBS, 64, 2 * NU]
    sw = [aw[0], np.zeros((64, 2 * NU), np.float32)]
    b.actor_set(sq, sw, [ab[0], np.zeros(2 * NU, np.float32)], head="squashed")
    with pytest.raises(hbmod.HbError, match="SAC"):
        b.learner_create()
    assert L.hb_learner_create(b._h, ctypes.byref(cfg)) == -4
    b.actor_set(asz, aw, ab, head="deterministic")
    assert L.hb_learner_create(b._h, ctypes.byref(cfg)) == -4
    b.actor_set(asz, aw, ab, head="gaussian", log_std=t["log_std"])
    b.learner_create(lr=1e-3)
    P = b.learner_param_count()
    assert P == flat.size
    with pytest.raises(hbmod.HbError):
        b.learner_configure(clip_range=-1.0)
    buf = np.zeros(P + 1, np.float32)
    tt = ctypes.c_longlong()
    assert L.hb_learner_get_params(b._h, buf.ctypes.data, P + 1) == -1 and L.hb_learner_set_params(b._h, buf.ctypes.data, P - 1) == -1
    assert L.hb_learner_get_grads(b._h, buf.ctypes.data, P + 1) == -1 and L.hb_learner_get_params(b._h, None, P) == -1
    assert L.hb_learner_get_state(b._h, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, P + 1, ctypes.byref(tt)) == -1
    assert L.hb_learner_set_state(b._h, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, P, -1) == -1
    assert np.array_equal(b.learner_params(), flat.astype(np.float32))  # the refused calls wrote nothing
    ptr, count = b.learner_grad_dev()
    assert ptr and count == P
    d = Dev(b, rows)
    g0, _ = d.grad(40)
    assert np.array_equal(b.from_dev(ptr, (P,)), g0)                   # the device gradient buffer is the flat record
    pp = [d.ptr[k] for k in TAPES]

    def rc(**kw):
        a = dict(obs=pp[0], action=pp[1], old_log_prob=pp[2], advantage=pp[3], returns=pp[4], index=None, n_rows=96, first=0, mb=40)
        a.update(kw)
        return L.hb_ppo_grad_dev(b._h, ctypes.byref(eng.HbPpoRows(**a)), None)
    assert rc() == 0
    assert rc(mb=0) == -1 and rc(n_rows=0) == -1 and rc(first=57) == -1 and rc(first=-1) == -1 and rc(first=56) == 0
    for k in TAPES:
        assert rc(**{k: None}) == -1
    assert L.hb_ppo_grad_dev(b._h, None, None) == -1 and L.hb_ppo_minibatch_dev(b._h, None, None) == -1
    assert np.array_equal(b.learner_grads(), d.grad(40, first=56)[0])  # (refusals left the gradient of the last good call)
    # hb_critic_set_mlp with the same sizes: the learner stays, the critic's parameters are the new ones, its moments start over
    a, kw = d.args(40)
    b.ppo_minibatch_dev(*a, **kw)
    s = b.learner_state()
    cut = P - sum(w.size + x.size for w, x in zip(cw, cb))
    assert s["t"] == 1 and np.abs(s["m"][cut:]).max() > 0 and np.abs(s["m"][:cut]).max() > 0
    cw2 = [w * 0.5 for w in cw]
    b.critic_set(csz, cw2, cb)
    s2 = b.learner_state()
    assert s2["t"] == 1 and not s2["m"][cut:].any() and not s2["v"][cut:].any() and np.array_equal(s2["m"][:cut], s["m"][:cut])
    assert np.array_equal(s2["params"][:cut], s["params"][:cut])       # the trained actor and log_std stay
    assert np.array_equal(pr.split(s2["params"], asz, csz, NU)["critic.w1"], cw2[1])
    # the same for the actor: its moments and log_std's start over, the critic's stay
    b.ppo_minibatch_dev(*a, **kw)
    s = b.learner_state()
    b.actor_set(asz, aw, ab, head="gaussian", log_std=t["log_std"] + 0.25)
    s2 = b.learner_state()
    assert s2["t"] == 2 and not s2["m"][:cut].any() and np.array_equal(s2["m"][cut:], s["m"][cut:]) and np.array_equal(s2["params"][cut:], s["params"][cut:])
    assert np.array_equal(pr.split(s2["params"], asz, csz, NU)["log_std"], t["log_std"] + np.float32(0.25))
    # other sizes: the learner is destroyed
    b.critic_set([NOBS, 1], [np.zeros((NOBS, 1), np.float32)], [np.zeros(1, np.float32)])
    assert L.hb_learner_param_count(b._h) == -1 and L.hb_ppo_adam_dev(b._h, None) == -1
    b.learner_create()
    b.learner_destroy()
    assert L.hb_learner_param_count(b._h) == -1
    d.free()
    b.close()
