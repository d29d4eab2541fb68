"""The PPO learner's gradient check (tests/test_gpu_ppo.py), which the observation extension's test (tests/test_gpu_obs_ext.py) runs on
its own wider rows: the networks by name, the config as the C struct holds it, the device copies of a minibatch, the derived bounds of
tier (a), the float32 noise floor of tier (b), and check_case, which holds one minibatch to both.  The derivations are in
tests/test_gpu_ppo.py's docstring.

TEST INFRASTRUCTURE: the product package never imports this module.
"""
import numpy as np

import mlp_ref as ml
import ppo_ref as pr

NOBS, NU = 48, 21
U = 2.0 ** -24
# name -> (actor sizes, critic sizes); a caller with networks of its own adds an entry (check_case looks the sizes up by name)
NETS = {"small": ([48, 20, 33, 21], [48, 20, 33, 1]), "one_layer": ([48, 21], [48, 1]),
        "wide": ([48, 256, 256, 256, 21], [48, 256, 256, 256, 1]), "mixed": ([48, 64, 21], [48, 16, 1])}
TAPES = ("obs", "action", "old_log_prob", "advantage", "returns")


def cfg(**kw):
    c = pr.config(**kw)
    return {k: (int(v) if k == "normalize_advantage" else float(np.float32(v))) for k, v in c.items()}


class Dev:
    """device copies of the tapes, an index and the statistics"""

    def __init__(self, b, rows, index=None):
        self.b, self.n_rows = b, len(rows["advantage"])
        self.ptr = {k: b.dev_alloc(rows[k].nbytes) for k in TAPES}
        for k in TAPES:
            b.to_dev(self.ptr[k], np.ascontiguousarray(rows[k], dtype=np.float32))
        self.stats = b.dev_alloc(64)
        b.to_dev(self.stats, np.full(16, np.nan, np.float32))
        self.index = None
        if index is not None:
            self.index = b.dev_alloc(4 * len(index))
            b.to_dev(self.index, np.ascontiguousarray(index, dtype=np.int32))

    def args(self, mb, first=0):
        return [self.ptr[k] for k in TAPES] + [self.n_rows, mb], dict(index=self.index, first=first, stats=self.stats)

    def grad(self, mb, first=0):
        a, kw = self.args(mb, first)
        self.b.ppo_grad_dev(*a, **kw)
        return self.b.learner_grads(), self.b.from_dev(self.stats, (16,))

    def free(self):
        for p in list(self.ptr.values()) + [self.stats] + ([self.index] if self.index else []):
            self.b.dev_free(p)


def derived(flat, asz, csz, rows, sel, cfg, ex, stats, chunk):
    """tier (a): bounds of the statistics and of the head gradients (dict name -> bound)"""
    t = pr.split(flat, asz, csz, NU)
    mb = len(sel)
    nchunk = (mb + chunk - 1) // chunk
    nsum = min(mb, chunk) + nchunk
    act, old, ret = (np.asarray(rows[k], dtype=np.float64)[sel] for k in ("action", "old_log_prob", "returns"))
    mu, v, lp, ratio, A, glp = (ex[k] for k in ("mu", "v", "lp", "ratio", "A", "glp"))
    c, vf = cfg["clip_range"], cfg["vf_coef"]
    ls = t["log_std"]
    s = np.exp(ls)
    dmu_e, dv_e = ml.fwd_err(t, "actor", len(asz) - 1, ex["acts_a"])[0], ml.fwd_err(t, "critic", len(csz) - 1, ex["acts_c"])[0][:, 0]
    z = (act - mu) / s
    dz = np.abs(z) * 3 * U + dmu_e / s
    M = 0.5 * z * z + np.abs(ls) + pr.HALF_LOG_2PI
    dlp = (np.abs(z) * dmu_e / s).sum(axis=1) + (NU + 8) * U * M.sum(axis=1)
    dd = dlp + U * (np.abs(lp) + np.abs(old))
    rho = np.expm1(dd) + 2 * U
    band = np.minimum(np.abs(ratio - (1 - c)), np.abs(ratio - (1 + c))) <= ratio * rho + 2 * U * (1 + c)
    smax = np.abs(A) * np.maximum(ratio, np.clip(ratio, 1 - c, 1 + c))
    e = v - ret
    de = dv_e + U * np.abs(e)
    kl_row = (ratio - 1) - (lp - old)
    B = {}
    B["policy_loss"] = (smax * (rho + 4 * U)).mean() + U * abs(stats["policy_loss"]) + 1e-12
    B["value_loss"] = (2 * np.abs(e) * de + de * de + U * e * e).mean() + U * stats["value_loss"] + 1e-12
    B["entropy_loss"] = 2 * U * abs(stats["entropy_loss"]) + 1e-12
    B["loss"] = B["policy_loss"] + abs(cfg["ent_coef"]) * B["entropy_loss"] + vf * B["value_loss"] + U * abs(stats["loss"])
    B["approx_kl"] = (ratio * rho + U * np.abs(ratio - 1) + dd + U * np.abs(kl_row)).mean() + U * abs(stats["approx_kl"]) + 1e-12
    B["clip_fraction"] = band.sum() / mb + U
    B["adv_mean"] = U * abs(stats["adv_mean"]) + 1e-9
    B["adv_std"] = U * abs(stats["adv_std"]) + 1e-9
    B["ratio_max"] = (ratio * rho).max() + U * ratio.max()
    eglp = np.where(band, np.abs(A) * ratio / mb, np.abs(glp) * (rho + 4 * U))
    dmu = glp[:, None] * z / s
    e_dmu = (np.abs(glp)[:, None] * dz + eglp[:, None] * np.abs(z)) / s + 4 * U * np.abs(dmu)
    B["actor.b%d" % (len(asz) - 2)] = e_dmu.sum(axis=0) + nsum * U * np.abs(dmu).sum(axis=0)
    gls = glp[:, None] * (z * z - 1)
    e_gls = eglp[:, None] * np.abs(z * z - 1) + np.abs(glp)[:, None] * (2 * np.abs(z) * dz + U * (z * z + 1)) + U * np.abs(gls)
    B["log_std"] = e_gls.sum(axis=0) + (nchunk + 2) * U * np.abs(gls).sum(axis=0) + U * abs(cfg["ent_coef"])
    dv = 2 * vf * e / mb
    B["critic.b%d" % (len(csz) - 2)] = (2 * vf / mb * de + 4 * U * np.abs(dv)).sum() + nsum * U * np.abs(dv).sum()
    return B


def floor(net, flat, rows, cfg, sel):
    """the float32 noise floor per tensor: torch CPU float32 autograd against the fp64 reference, relative to the tensor's largest entry"""
    import torch
    asz, csz = NETS[net]
    _, g64, _ = pr.loss_and_grads(flat, asz, csz, rows, cfg, index=sel)
    loss, leaves, _ = pr.torch_loss(torch, torch.float32, flat, asz, csz, rows, cfg, sel)
    loss.backward()
    ref = pr.split(g64, asz, csz, NU)
    # (a tensor whose gradient is zero - a single clipped row - has no floor: the device has to give zeros there)
    return {k: float(np.abs(leaf.grad.numpy().astype(np.float64) - ref[k]).max() / np.abs(ref[k]).max()) if ref[k].any() else 0.0 for k, leaf in leaves.items()}


def worst_ratio(err, bound):
    """max err / bound, where a zero bound (a gradient that is exactly zero) admits a zero error only"""
    err, bound = np.atleast_1d(err), np.broadcast_to(bound, np.shape(np.atleast_1d(err)))
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def check_case(b, net, flat, rows, name, index, first, mb, cfg, worst):
    asz, csz = NETS[net]
    import humanoid_mujoco_amd.engine as eng
    sel = np.asarray(index) if index is not None else np.arange(first, first + mb)
    masked = {k: np.full_like(rows[k], np.nan) for k in TAPES}   # rows outside the minibatch are NaN: they are not read
    for k in TAPES:
        masked[k][sel] = rows[k][sel]
    d = Dev(b, masked, index)
    got, st = d.grad(mb, first)
    d.free()
    assert np.isfinite(got).all() and np.isfinite(st).all(), name
    stats, g64, ex = pr.loss_and_grads(flat, asz, csz, rows, cfg, index=sel)
    B = derived(flat, asz, csz, rows, sel, cfg, ex, stats, eng.ppo_row_chunk(mb))
    for i, k in enumerate(pr.STATS):
        if k in ("grad_norm", "skipped"):
            assert st[i] == 0.0, (name, k)  # (hb_ppo_adam_dev's)
            continue
        r = abs(float(st[i]) - stats[k]) / B[k]
        worst["stat"] = max(worst["stat"], r)
        assert r <= 1.0, (net, name, k, float(st[i]), stats[k], B[k])
    assert not st[11:].any()
    gg, gr = pr.split(got.astype(np.float64), asz, csz, NU), pr.split(g64, asz, csz, NU)
    fl = floor(net, flat, rows, cfg, sel)
    for k in gg:
        err = np.abs(gg[k] - gr[k])
        if k in B:
            r = worst_ratio(err, B[k])
            worst["head"] = max(worst["head"], r)
            assert r <= 1.0, (net, name, k, r)
        elif not gr[k].any():
            assert not gg[k].any(), (net, name, k)
        else:
            kk = 8.0 * max(v for name_, v in fl.items() if name_ not in B)  # (the floors of the tensors held to k)
            r = float(err.max() / np.abs(gr[k]).max())
            worst["floor"], worst["k"], worst["ratio"] = max(worst["floor"], kk / 8.0), max(worst["k"], kk), max(worst["ratio"], r)
            worst["rel"] = max(worst["rel"], r / kk)
            assert r <= kk, (net, name, k, r, kk, fl)
