"""The SAC learner's step check (tests/test_gpu_sac.py), which the observation extension's test (tests/test_gpu_obs_ext.py) runs on its
own wider rows: the networks by name, the config as the C struct holds it, the device copies of a minibatch, the derived bounds of tier
(a), the float32 noise floors of tier (b), and check_step, which holds one step to tiers (a), (b) and (c).  The derivations are in
tests/test_gpu_sac.py's docstring.

TEST INFRASTRUCTURE: the product package never imports this module.
"""
import numpy as np

import mlp_ref as ml
import sac_ref as sr
from ppo_lib import worst_ratio

NOBS, NU = 48, 21  # (NOBS: the width of obs in the Q networks' obs | action input; a caller with wider rows sets it for its test)
U = 2.0 ** -24
# name -> (actor sizes, Q sizes); a caller with networks of its own adds an entry (install and check_step look the sizes up by name)
NETS = {"small": ([48, 20, 33, 42], [69, 20, 33, 1]), "one_layer": ([48, 42], [69, 1]), "mixed": ([48, 64, 42], [69, 16, 1])}
TAPES = ("obs", "action", "reward", "next_obs", "done")


def cfg(**kw):
    """the config as the C struct holds it: the reference gets the same float32 numbers"""
    c = sr.config(**kw)
    ints = ("auto_ent", "target_entropy_auto", "target_update_interval", "seed")
    return {k: (int(v) if k in ints else float(np.float32(v))) for k, v in c.items()}


_problems = {}


def problem(net, n_rows, seed=1):
    """sac_ref.random_problem for the networks `net`: made once per (net, rows, seed) and shared, never changed"""
    key = (net, n_rows, seed)
    if key not in _problems:
        _problems[key] = sr.random_problem(*NETS[net], n_rows, seed=seed)
    return _problems[key]


def layers(t, tag, sizes):
    n = len(sizes) - 1
    return [t["%s.w%d" % (tag, l)] for l in range(n)], [t["%s.b%d" % (tag, l)] for l in range(n)]


def install(b, net, flat, actor=True, head="squashed"):
    asz, qsz = NETS[net]
    t = sr.split(np.asarray(flat, dtype=np.float32), asz, qsz)
    if actor:
        b.actor_set(asz, *layers(t, "actor", asz), head=head, seed=3)
    b.q_set(0, qsz, *layers(t, "q1", qsz))
    b.q_set(1, qsz, *layers(t, "q2", qsz))


class Dev:
    """device copies of the rows, the draws of a minibatch, an index and the statistics"""

    def __init__(self, b, rows, mb, eps_pi=None, eps_next=None, index=None):
        self.b, self.n_rows, self.mb = b, len(rows["reward"]), mb
        self.ptr = {}
        for k in TAPES:
            a = np.ascontiguousarray(rows[k], dtype=np.uint8 if k == "done" else np.float32)
            self.ptr[k] = b.dev_alloc(max(a.nbytes, 4))
            b.to_dev(self.ptr[k], a)
        self.eps = [b.dev_alloc(mb * NU * 4), b.dev_alloc(mb * NU * 4)]
        for p, e in zip(self.eps, (eps_pi, eps_next)):
            b.to_dev(p, np.full((mb, NU), np.nan, np.float32) if e is None else np.ascontiguousarray(e, dtype=np.float32))
        self.stats = b.dev_alloc(64)
        b.to_dev(self.stats, np.full(16, np.nan, np.float32))
        self.index = None
        if index is not None:
            self.index = b.dev_alloc(4 * len(index))
            b.to_dev(self.index, np.ascontiguousarray(index, dtype=np.int32))

    def step(self, first=0, eps_given=True):
        self.b.sac_step_dev(*[self.ptr[k] for k in TAPES], self.n_rows, self.mb, index=self.index, first=first, eps_pi=self.eps[0],
                            eps_next=self.eps[1], eps_given=eps_given, stats=self.stats)
        return self.b.from_dev(self.stats, (16,))

    def draws(self):
        return self.b.from_dev(self.eps[0], (self.mb, NU)), self.b.from_dev(self.eps[1], (self.mb, NU))

    def free(self):
        for p in list(self.ptr.values()) + self.eps + [self.stats] + ([self.index] if self.index else []):
            self.b.dev_free(p)


def derived_critic(flat, targets, asz, qsz, rows, sel, cfg, ex, stats):
    """tier (a), critic phase: bounds of its statistics, of the Q networks' top bias gradients and of dloss / dlog_ent_coef"""
    t = sr.split(flat, asz, qsz)
    La, Lq, mb = len(asz) - 1, len(qsz) - 1, len(sel)
    nsum = mb + 2
    pi, alpha = ex["pi"], ex["alpha"]
    dlp_pi = sr.lp_err(pi, ml.fwd_err(t, "actor", La, pi["acts"])[0])
    dy = sr.target(flat, targets, asz, qsz, rows, sel, ex["nx"]["eps"], cfg)[1]
    lec = abs(float(t["log_ent_coef"][0]))
    B = {"ent_coef": 2 * U * alpha, "lp_pi": dlp_pi.mean() + U * abs(stats["lp_pi"]), "y": dy.mean() + U * abs(stats["y"])}
    B["ent_coef_loss"] = lec * dlp_pi.mean() + 2 * U * abs(stats["ent_coef_loss"]) + 1e-12
    B["log_ent_coef"] = dlp_pi.mean() + U * abs(stats["lp_pi"] + sr.target_entropy(cfg, NU))
    B["critic_loss"] = U * abs(stats["critic_loss"]) + 1e-12
    for k, tag, acts in ((1, "q1", ex["acts1"]), (2, "q2", ex["acts2"])):
        q = ex["q%d" % k]
        e_q = ml.fwd_err(t, tag, Lq, acts)[0][:, 0]
        e = q - ex["y"]
        de = e_q + dy + U * np.abs(e)
        B["q%d" % k] = e_q.mean() + U * abs(stats["q%d" % k])
        B["critic_loss"] += 0.5 * (2 * np.abs(e) * de + de * de + 2 * U * e * e).mean()
        B["%s.b%d" % (tag, Lq - 1)] = (de + 3 * U * np.abs(e)).sum() / mb + nsum * U * np.abs(e).sum() / mb
    return B


def derived_actor(flat, asz, qsz, sel, ex, alpha, stats):
    """tier (a), actor phase: bounds of actor_loss and of the mean of min Q(obs, a_pi)"""
    t = sr.split(flat, asz, qsz)
    La, Lq, mb = len(asz) - 1, len(qsz) - 1, len(sel)
    pi = ex["pi"]
    e_pi = ml.fwd_err(t, "actor", La, pi["acts"])[0]
    dlp = sr.lp_err(pi, e_pi)
    e_in = np.concatenate([np.zeros((mb, NOBS)), sr.action_err(pi, e_pi)], axis=1)
    e_q = np.maximum(ml.fwd_err(t, "q1", Lq, ex["acts1"], e0=e_in)[0][:, 0], ml.fwd_err(t, "q2", Lq, ex["acts2"], e0=e_in)[0][:, 0])
    mq = np.minimum(ex["q1"], ex["q2"])
    return {"min_q_pi": e_q.mean() + U * abs(stats["min_q_pi"]),
            "actor_loss": (alpha * dlp + e_q + 3 * U * (np.abs(alpha * pi["lp"]) + np.abs(mq))).mean() + U * abs(stats["actor_loss"]) + 1e-12}


def floors(torch_loss_index, names, flat, targets, asz, qsz, rows, sel, ep, en, cfg, ref, alpha=None):
    """the float32 noise floor per tensor: torch CPU float32 autograd of one of the three losses against the fp64 gradients ref"""
    import torch
    losses = sr.torch_losses(torch, torch.float32, flat, targets, asz, qsz, rows, sel, ep, en, cfg, alpha=alpha)
    leaves = losses[3]
    grads = torch.autograd.grad(losses[torch_loss_index], [leaves[k] for k in names])
    return {k: (float(np.abs(g.numpy().astype(np.float64) - ref[k]).max() / np.abs(ref[k]).max()) if ref[k].any() else 0.0) for k, g in zip(names, grads)}


def new_worst():
    return dict(stat=0.0, head=0.0, floor=0.0, k=0.0, ratio=0.0, rel=0.0, adam=0.0, polyak=0.0)


def state64(b):
    s = b.sac_state()
    return {k: (s[k].astype(np.float64) if k != "t" else s[k]) for k in s}


def check_step(b, net, pb, sel, cfg, worst, name, contiguous=False):
    """one step from the device's own downloaded state, held to tiers (a), (b) and (c)"""
    asz, qsz = NETS[net]
    lo, hi = sr.q_range(asz, qsz)
    rows = pb["rows"]
    mb = len(sel)
    ep, en = pb["eps_pi"][sel], pb["eps_next"][sel]
    masked = {k: (np.full_like(rows[k], np.nan) if k != "done" else np.full_like(rows[k], 1)) for k in TAPES}  # rows outside the minibatch are not read
    for k in TAPES:
        masked[k][sel] = rows[k][sel]
    d = Dev(b, masked, mb, ep, en, None if contiguous else sel)
    s0 = state64(b)
    st = d.step(first=int(sel[0]) if contiguous else 0)
    d.free()
    s1, got = state64(b), b.sac_grads().astype(np.float64)
    assert np.isfinite(st).all() and np.isfinite(got).all() and s1["t"] == s0["t"] + 1, name
    # ---- the critic phase at the pre-step state
    stats_c, g_c, ex_c = sr.critic_phase(s0["params"], s0["targets"], asz, qsz, rows, sel, ep, en, cfg)
    alpha = ex_c["alpha"]
    # ---- the actor phase at the device's post-step critics
    mid = s0["params"].copy()
    mid[lo:] = s1["params"][lo:]
    stats_a, g_a, ex_a = sr.actor_phase(mid, asz, qsz, rows, sel, ep, alpha)
    stats = {**stats_c, **stats_a}
    B = derived_critic(s0["params"], s0["targets"], asz, qsz, rows, sel, cfg, ex_c, stats)
    B.update(derived_actor(mid, asz, qsz, sel, ex_a, alpha, stats))
    for i, k in enumerate(sr.STATS):
        r = abs(float(st[i]) - stats[k]) / B[k]
        worst["stat"] = max(worst["stat"], r)
        assert r <= 1.0, (net, name, k, float(st[i]), stats[k], B[k])
    assert not st[len(sr.STATS):].any()
    gg, gr = sr.split(got, asz, qsz), {**g_c, **g_a}
    cnames = [k for k in gr if k.startswith("q") and k not in B]
    anames = [k for k in gr if k.startswith("actor")]
    fl_c = floors(1, cnames, s0["params"], s0["targets"], asz, qsz, rows, sel, ep, en, cfg, gr) if cnames else {}
    fl_a = floors(2, anames, mid, s0["targets"], asz, qsz, rows, sel, ep, en, cfg, gr, alpha=alpha)
    for k in gg:
        err = np.abs(gg[k] - gr[k])
        if k in B:
            r = worst_ratio(err, B[k])
            worst["head"] = max(worst["head"], r)
            assert r <= 1.0, (net, name, k, r)
        elif not gr[k].any():
            assert not gg[k].any(), (net, name, k)
        else:
            kk = 8.0 * max((fl_a if k.startswith("actor") else fl_c).values())
            r = float(err.max() / np.abs(gr[k]).max())
            worst["floor"], worst["k"], worst["ratio"] = max(worst["floor"], kk / 8.0), max(worst["k"], kk), max(worst["ratio"], r)
            worst["rel"] = max(worst["rel"], r / kk)
            assert r <= kk, (net, name, k, r, kk)
    # ---- tier (c): Adam on the downloaded gradient, moments and parameters; Polyak on the downloaded parameters and targets
    p, m, v = sr.critic_update(s0, got, asz, qsz, cfg)
    p, m, v = sr.actor_update(p, m, v, s1["t"], got, asz, qsz, cfg)
    assert (np.abs(s1["m"] - m) <= U * np.abs(m) + 1e-45).all() and (np.abs(s1["v"] - v) <= U * np.abs(v) + 1e-45).all(), (net, name)
    bound = 0.5 * np.maximum(np.spacing(np.abs(p).astype(np.float32)), np.spacing(np.abs(s1["params"]).astype(np.float32))) + 2.0 ** -36 * np.abs(p - s0["params"])
    worst["adam"] = max(worst["adam"], float((np.abs(s1["params"] - p) / bound).max()))
    assert (np.abs(s1["params"] - p) <= bound).all(), (net, name, worst["adam"])
    if not cfg["auto_ent"]:
        assert s1["params"][-1] == s0["params"][-1] and s1["m"][-1] == s0["m"][-1] and s1["v"][-1] == s0["v"][-1]
    else:
        assert s1["params"][-1] != s0["params"][-1]
    if sr.polyak_due(s1["t"], cfg):
        tg = sr.polyak(s1["params"][lo:hi], s0["targets"], cfg["tau"])
        tb = 0.5 * np.maximum(np.spacing(np.abs(tg).astype(np.float32)), np.spacing(np.abs(s1["targets"]).astype(np.float32)))
        worst["polyak"] = max(worst["polyak"], float((np.abs(s1["targets"] - tg) / tb).max()))
        assert (np.abs(s1["targets"] - tg) <= tb).all() and not np.array_equal(s1["targets"], s0["targets"]), (net, name)
    else:
        assert np.array_equal(s1["targets"], s0["targets"]), (net, name)
    return st


def line(what, w):
    return ("%s: statistics %.3f, head gradients %.3f of their derived bounds; back-propagated tensors: float32 floor %.2e, measured %.2e, "
            "k = %.2e (worst measured / k %.3f); Adam %.3f, Polyak %.3f of their bounds" % (what, w["stat"], w["head"], w["floor"], w["ratio"], w["k"], w["rel"], w["adam"], w["polyak"]))
