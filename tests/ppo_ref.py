"""fp64 numpy restatement of the PPO learner (include/hb.h: hb_ppo_grad_dev, hb_ppo_adam_dev): stable-baselines3's PPO.train for separate
actor and critic MLPs (mlp_ref.py: the chosen hidden activation, tanh by default, linear top) and a state-independent log_std - the loss
and its statistics, the analytic gradients, global-norm clipping, Adam, and the flat parameter record with its per-tensor split.
test_ppo_cpu.py holds it against torch autograd and torch.optim.Adam in float64; test_gpu_ppo.py holds the kernels against it."""
import numpy as np

import mlp_ref as ml

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
DEFAULTS = dict(clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, normalize_advantage=1, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5)
STATS = ("policy_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction", "grad_norm", "adv_mean", "adv_std", "ratio_max", "skipped")


def config(**kw):
    c = dict(DEFAULTS)
    for k in kw:
        assert k in c, k
    c.update(kw)
    return c


def flat_shapes(actor_sizes, critic_sizes, nu):
    """(name, shape) of the tensors of the flat record in order: the actor's layers W [K, N] | b [N], log_std [nu], the critic's layers"""
    return ml.net_shapes("actor", actor_sizes) + [("log_std", (nu,))] + ml.net_shapes("critic", critic_sizes)


def split(flat, actor_sizes, critic_sizes, nu):
    return ml.split(flat, flat_shapes(actor_sizes, critic_sizes, nu))


def join(tensors, actor_sizes, critic_sizes, nu):
    return ml.join(tensors, flat_shapes(actor_sizes, critic_sizes, nu))


def loss_and_grads(flat, actor_sizes, critic_sizes, rows, cfg, index=None, first=0, mb=None, act_actor="tanh", act_critic="tanh"):
    """rows: dict obs [R, nobs], action [R, nu], old_log_prob, advantage, returns [R].  Returns (stats dict, flat fp64 gradient, extras)."""
    nu = actor_sizes[-1]
    t = split(np.asarray(flat, dtype=np.float64), actor_sizes, critic_sizes, nu)
    sel = np.asarray(index, dtype=np.int64) if index is not None else np.arange(first, first + mb)
    mb = len(sel)
    obs, act = np.asarray(rows["obs"], dtype=np.float64)[sel], np.asarray(rows["action"], dtype=np.float64)[sel]
    old, adv, ret = (np.asarray(rows[k], dtype=np.float64)[sel] for k in ("old_log_prob", "advantage", "returns"))
    c = float(cfg["clip_range"])
    La, Lc = len(actor_sizes) - 1, len(critic_sizes) - 1
    acts_a, mu, _ = ml.forward(t, "actor", La, obs, act_actor)
    acts_c, v, _ = ml.forward(t, "critic", Lc, obs, act_critic)
    v = v[:, 0]
    ls = t["log_std"]
    s2 = np.exp(2.0 * ls)
    lp = (-(act - mu) ** 2 / (2.0 * s2) - ls - HALF_LOG_2PI).sum(axis=1)
    adv_mean = adv.mean()
    adv_std = adv.std(ddof=1) if mb > 1 else 0.0
    A = (adv - adv_mean) / (adv_std + 1e-8) if cfg["normalize_advantage"] and mb > 1 else adv
    d = lp - old
    ratio = np.exp(d)
    s1, s2c = A * ratio, A * np.clip(ratio, 1.0 - c, 1.0 + c)
    policy_loss = -np.minimum(s1, s2c).mean()
    value_loss = ((ret - v) ** 2).mean()
    entropy_loss = -(0.5 + HALF_LOG_2PI + ls).sum()
    stats = dict(policy_loss=policy_loss, value_loss=value_loss, entropy_loss=entropy_loss,
                 loss=policy_loss + cfg["ent_coef"] * entropy_loss + cfg["vf_coef"] * value_loss,
                 approx_kl=((ratio - 1.0) - d).mean(), clip_fraction=(np.abs(ratio - 1.0) > c).mean(),
                 adv_mean=adv_mean, adv_std=adv_std, ratio_max=ratio.max())
    inside = (ratio >= 1.0 - c) & (ratio <= 1.0 + c)
    glp = np.where(inside | (s1 < s2c), -A * ratio / mb, 0.0)
    grads = {}
    ml.backward(t, "actor", La, acts_a, glp[:, None] * (act - mu) / s2, act_actor, grads)
    grads["log_std"] = (glp[:, None] * ((act - mu) ** 2 / s2 - 1.0)).sum(axis=0) - cfg["ent_coef"]
    ml.backward(t, "critic", Lc, acts_c, (2.0 * cfg["vf_coef"] * (v - ret) / mb)[:, None], act_critic, grads)
    g = join(grads, actor_sizes, critic_sizes, nu)
    stats["grad_norm"] = float(np.sqrt((g ** 2).sum()))
    return stats, g, dict(mu=mu, v=v, lp=lp, ratio=ratio, A=A, glp=glp, acts_a=acts_a, acts_c=acts_c)


def clip_scale(grad_norm, max_grad_norm):
    return min(1.0, max_grad_norm / (grad_norm + 1e-6)) if max_grad_norm > 0 else 1.0


def adam_step(p, m, v, t, g, cfg):
    """clip_grad_norm_ then torch.optim.Adam on flat fp64 records; returns (p, m, v, t, grad_norm, skipped)"""
    p, m, v, g = (np.asarray(x, dtype=np.float64) for x in (p, m, v, g))
    gn = float(np.sqrt((g ** 2).sum()))
    if not np.isfinite(gn):
        return p.copy(), m.copy(), v.copy(), t, gn, True
    p, m, v = ml.adam(p, m, v, t + 1, g * clip_scale(gn, float(cfg["max_grad_norm"])), cfg["lr"], cfg)
    return p, m, v, t + 1, gn, False


def torch_loss(torch, dtype, flat, asz, csz, rows, cfg, sel, act_actor="tanh", act_critic="tanh"):
    """SB3's PPO.train loss written with torch ops on CPU leaves of `dtype` (one leaf per tensor of the flat record): autograd in float64
    is what the reference is held to, in float32 it is the noise floor of an independent single-precision evaluation"""
    nu = asz[-1]
    leaves = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in split(flat, asz, csz, nu).items()}
    obs, act, old, adv, ret = (torch.tensor(np.asarray(rows[k], dtype=np.float64)[sel], dtype=dtype) for k in ("obs", "action", "old_log_prob", "advantage", "returns"))
    mu = ml.torch_mlp(torch, leaves, "actor", len(asz) - 1, obs, act_actor)
    v = ml.torch_mlp(torch, leaves, "critic", len(csz) - 1, obs, act_critic)[:, 0]
    dist = torch.distributions.Normal(mu, torch.ones_like(mu) * leaves["log_std"].exp())
    lp = dist.log_prob(act).sum(dim=1)
    if cfg["normalize_advantage"] and len(sel) > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(lp - old)
    c = cfg["clip_range"]
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - c, 1 + c)).mean()
    value_loss = torch.nn.functional.mse_loss(ret, v)
    entropy_loss = -dist.entropy().sum(dim=1).mean()
    loss = policy_loss + cfg["ent_coef"] * entropy_loss + cfg["vf_coef"] * value_loss
    return loss, leaves, dict(policy_loss=policy_loss, value_loss=value_loss, entropy_loss=entropy_loss, loss=loss)


def random_problem(actor_sizes, critic_sizes, n_rows, seed, stale=0.3):
    """Random networks (flat fp64 record, entries that are float32 values) and random tapes; old_log_prob is the current log-probability
    moved by N(0, stale), so that a good share of the rows is clipped and a good share is not."""
    rng = np.random.default_rng(seed)
    nu = actor_sizes[-1]
    t = {}
    for name, sh in flat_shapes(actor_sizes, critic_sizes, nu):
        if name == "log_std":
            t[name] = rng.uniform(-0.7, 0.2, sh)
        elif len(sh) == 2:
            t[name] = rng.normal(0.0, 1.0 / np.sqrt(sh[0]), sh)
        else:
            t[name] = rng.normal(0.0, 0.1, sh)
    flat = join(t, actor_sizes, critic_sizes, nu).astype(np.float32).astype(np.float64)
    obs = rng.normal(0.0, 1.0, (n_rows, actor_sizes[0])).astype(np.float32)
    mu = ml.forward(split(flat, actor_sizes, critic_sizes, nu), "actor", len(actor_sizes) - 1, obs)[1]
    ls = split(flat, actor_sizes, critic_sizes, nu)["log_std"]
    action = (mu + np.exp(ls) * rng.normal(0.0, 1.0, mu.shape)).astype(np.float32)
    lp = (-(action - mu) ** 2 / (2.0 * np.exp(2.0 * ls)) - ls - HALF_LOG_2PI).sum(axis=1)
    rows = dict(obs=obs, action=action, old_log_prob=(lp + rng.normal(0.0, stale, n_rows)).astype(np.float32),
                advantage=rng.normal(0.3, 1.5, n_rows).astype(np.float32), returns=rng.normal(0.0, 1.0, n_rows).astype(np.float32))
    return flat, rows
