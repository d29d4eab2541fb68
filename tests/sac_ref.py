"""fp64 numpy restatement of the SAC learner (include/hb.h: hb_sac_step_dev): stable-baselines3's SAC.train for a squashed Gaussian actor
(mean | raw log_std, clamped to [-20, 2]), twin Q networks over obs | action, their Polyak targets and the entropy coefficient - the
networks of mlp_ref.py (the chosen hidden activation, tanh by default; the targets run the Q networks'), the log-probability in
hb_collect_gae_dev's form.  The three losses, the analytic gradients, Adam per group, the Polyak step, the flat records with their
per-tensor split, and the float32 bounds that follow the actor's forward bound (mlp_ref.fwd_err): of a sampled action (action_err), of
its log-probability (lp_err) and of the critic's target (target).  test_sac_cpu.py holds it against torch autograd and
torch.optim.Adam in float64; test_gpu_sac.py and test_gpu_act.py hold the kernels against it."""
import numpy as np

import mlp_ref as ml

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
LOG2 = np.log(2.0)
DEFAULTS = dict(gamma=0.99, tau=0.005, lr_actor=3e-4, lr_critic=3e-4, lr_ent=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, ent_coef_init=1.0,
                auto_ent=1, target_entropy_auto=1, target_entropy=0.0, target_update_interval=1, seed=0)
STATS = ("actor_loss", "critic_loss", "ent_coef_loss", "ent_coef", "lp_pi", "q1", "q2", "y", "min_q_pi")
U = ml.U
ACTOR_LOWER_SCALE, Q_LOWER_SCALE, Q_TOP_BIAS = 0.22, 0.35, 3.0


def config(**kw):
    c = dict(DEFAULTS)
    for k in kw:
        assert k in c, k
    c.update(kw)
    return c


def target_entropy(cfg, nu):
    return -float(nu) if cfg["target_entropy_auto"] else float(cfg["target_entropy"])


def flat_shapes(actor_sizes, q_sizes):
    """(name, shape) of the tensors of the flat record in order: the actor's layers W [K, N] | b [N], Q1's, Q2's, log_ent_coef [1]"""
    return ml.net_shapes("actor", actor_sizes) + ml.net_shapes("q1", q_sizes) + ml.net_shapes("q2", q_sizes) + [("log_ent_coef", (1,))]


def split(flat, actor_sizes, q_sizes):
    return ml.split(flat, flat_shapes(actor_sizes, q_sizes))


def join(tensors, actor_sizes, q_sizes):
    return ml.join(tensors, flat_shapes(actor_sizes, q_sizes))


def q_range(actor_sizes, q_sizes):
    """(lo, hi): the stretch of the flat record the targets' record mirrors (Q1 then Q2)"""
    lo = sum(int(np.prod(sh)) for name, sh in flat_shapes(actor_sizes, q_sizes) if name.startswith("actor"))
    hi = sum(int(np.prod(sh)) for name, sh in flat_shapes(actor_sizes, q_sizes)) - 1
    return lo, hi


def with_targets(tensors, targets, actor_sizes, q_sizes):
    """the tensor dict with q1.*, q2.* taken from a targets' record"""
    lo, hi = q_range(actor_sizes, q_sizes)
    flat = join(tensors, actor_sizes, q_sizes)
    flat[lo:hi] = np.asarray(targets, dtype=np.float64)
    return split(flat, actor_sizes, q_sizes)


def softplus(x):
    return np.logaddexp(0.0, x)


def head(tensors, n_layers, obs, eps, act_actor="tanh"):
    """the squashed Gaussian head on rows obs with draws eps: dict acts, mean, raw, ls, s, x, a, lp"""
    acts, out, _ = ml.forward(tensors, "actor", n_layers, obs, act_actor)
    nu = out.shape[1] // 2
    mean, raw = out[:, :nu], out[:, nu:]
    ls = np.clip(raw, -20.0, 2.0)
    s = np.exp(ls)
    eps = np.asarray(eps, dtype=np.float64)
    x = mean + s * eps
    a = np.tanh(x)
    lp = (-0.5 * eps ** 2 - ls - HALF_LOG_2PI).sum(axis=1) - (2.0 * (LOG2 - x - softplus(-2.0 * x))).sum(axis=1)
    return dict(acts=acts, mean=mean, raw=raw, ls=ls, s=s, x=x, a=a, lp=lp, eps=eps)


def critic_phase(flat, targets, actor_sizes, q_sizes, rows, sel, eps_pi, eps_next, cfg, act_actor="tanh", act_q="tanh"):
    """the entropy-coefficient and critic losses of minibatch rows sel (eps_*: [mb, nu], by minibatch row) at the parameters flat and the
    targets' record: (stats dict, grads dict of q1.*, q2.*, log_ent_coef, extras)"""
    t = split(np.asarray(flat, dtype=np.float64), actor_sizes, q_sizes)
    tt = with_targets(t, targets, actor_sizes, q_sizes)
    La, Lq, nu = len(actor_sizes) - 1, len(q_sizes) - 1, actor_sizes[-1] // 2
    mb = len(sel)
    obs, act, rew, nobs_, done = (np.asarray(rows[k], dtype=np.float64)[sel] for k in ("obs", "action", "reward", "next_obs", "done"))
    lec = float(t["log_ent_coef"][0])
    alpha = float(np.float32(np.exp(lec)))  # (the device rounds exp(log_ent_coef) to fp32 once and uses that everywhere)
    pi = head(t, La, obs, eps_pi, act_actor)
    nx = head(t, La, nobs_, eps_next, act_actor)
    te = target_entropy(cfg, nu)
    ent_loss = -(lec * (pi["lp"] + te)).mean()
    xq = np.concatenate([nobs_, nx["a"]], axis=1)
    acts_t1, qt1, _ = ml.forward(tt, "q1", Lq, xq, act_q)
    acts_t2, qt2, _ = ml.forward(tt, "q2", Lq, xq, act_q)
    y = rew + (1.0 - done) * float(cfg["gamma"]) * (np.minimum(qt1[:, 0], qt2[:, 0]) - alpha * nx["lp"])
    xin = np.concatenate([obs, act], axis=1)
    acts1, q1, _ = ml.forward(t, "q1", Lq, xin, act_q)
    acts2, q2, _ = ml.forward(t, "q2", Lq, xin, act_q)
    q1, q2 = q1[:, 0], q2[:, 0]
    critic_loss = 0.5 * (((q1 - y) ** 2).mean() + ((q2 - y) ** 2).mean())
    grads = {"log_ent_coef": np.array([-(pi["lp"] + te).mean()])}
    ml.backward(t, "q1", Lq, acts1, ((q1 - y) / mb)[:, None], act_q, grads)
    ml.backward(t, "q2", Lq, acts2, ((q2 - y) / mb)[:, None], act_q, grads)
    stats = dict(critic_loss=critic_loss, ent_coef_loss=ent_loss, ent_coef=alpha, lp_pi=pi["lp"].mean(), q1=q1.mean(), q2=q2.mean(), y=y.mean())
    return stats, grads, dict(pi=pi, nx=nx, y=y, q1=q1, q2=q2, qt1=qt1[:, 0], qt2=qt2[:, 0], acts1=acts1, acts2=acts2, acts_t1=acts_t1, acts_t2=acts_t2, alpha=alpha)


def actor_phase(flat, actor_sizes, q_sizes, rows, sel, eps_pi, alpha, act_actor="tanh", act_q="tanh"):
    """the actor loss at the parameters flat (whose Q1, Q2 are the UPDATED ones) with the given alpha: (stats, grads of actor.*, extras)"""
    t = split(np.asarray(flat, dtype=np.float64), actor_sizes, q_sizes)
    La, Lq, nu = len(actor_sizes) - 1, len(q_sizes) - 1, actor_sizes[-1] // 2
    mb = len(sel)
    obs = np.asarray(rows["obs"], dtype=np.float64)[sel]
    pi = head(t, La, obs, eps_pi, act_actor)
    xin = np.concatenate([obs, pi["a"]], axis=1)
    acts1, q1, _ = ml.forward(t, "q1", Lq, xin, act_q)
    acts2, q2, _ = ml.forward(t, "q2", Lq, xin, act_q)
    q1, q2 = q1[:, 0], q2[:, 0]
    mq = np.minimum(q1, q2)
    actor_loss = (alpha * pi["lp"] - mq).mean()
    w1 = np.where(q1 < q2, 1.0, np.where(q1 == q2, 0.5, 0.0))
    da1 = ml.backward(t, "q1", Lq, acts1, np.ones((mb, 1)), act_q)[:, -nu:]
    da2 = ml.backward(t, "q2", Lq, acts2, np.ones((mb, 1)), act_q)[:, -nu:]
    g = w1[:, None] * da1 + (1.0 - w1)[:, None] * da2
    a, s, eps = pi["a"], pi["s"], pi["eps"]
    gx = g * (1.0 - a * a)
    dmean = (2.0 * alpha * a - gx) / mb
    gate = (pi["raw"] >= -20.0) & (pi["raw"] <= 2.0)
    dls = np.where(gate, (alpha * (-1.0 + 2.0 * a * s * eps) - gx * s * eps) / mb, 0.0)
    grads = {}
    ml.backward(t, "actor", La, pi["acts"], np.concatenate([dmean, dls], axis=1), act_actor, grads)
    return dict(actor_loss=actor_loss, min_q_pi=mq.mean()), grads, dict(pi=pi, q1=q1, q2=q2, g=g, dmean=dmean, dls=dls, acts1=acts1, acts2=acts2, da1=da1, da2=da2)


def polyak(q, target, tau):
    return float(tau) * np.asarray(q, dtype=np.float64) + (1.0 - float(tau)) * np.asarray(target, dtype=np.float64)


def critic_update(state, grads_flat, actor_sizes, q_sizes, cfg):
    """Adam on Q1, Q2 (lr_critic) and, with auto_ent, on log_ent_coef (lr_ent): the new (params, m, v) as flat fp64 records"""
    lo, hi = q_range(actor_sizes, q_sizes)
    p, m, v = (np.asarray(state[k], dtype=np.float64).copy() for k in ("params", "m", "v"))
    t = state["t"] + 1
    p[lo:hi], m[lo:hi], v[lo:hi] = ml.adam(p[lo:hi], m[lo:hi], v[lo:hi], t, grads_flat[lo:hi], cfg["lr_critic"], cfg)
    if cfg["auto_ent"]:
        p[hi:], m[hi:], v[hi:] = ml.adam(p[hi:], m[hi:], v[hi:], t, grads_flat[hi:], cfg["lr_ent"], cfg)
    return p, m, v


def actor_update(p, m, v, t, grads_flat, actor_sizes, q_sizes, cfg):
    lo, _ = q_range(actor_sizes, q_sizes)
    p, m, v = (np.asarray(x, dtype=np.float64).copy() for x in (p, m, v))
    p[:lo], m[:lo], v[:lo] = ml.adam(p[:lo], m[:lo], v[:lo], t, grads_flat[:lo], cfg["lr_actor"], cfg)
    return p, m, v


def polyak_due(t_new, cfg):
    """the targets move on the steps whose count, the step included, is a multiple of target_update_interval"""
    return t_new % int(cfg["target_update_interval"]) == 0


def step(state, actor_sizes, q_sizes, rows, sel, eps_pi, eps_next, cfg, act_actor="tanh", act_q="tanh"):
    """one gradient step from state = dict(params, m, v, targets, t) (flat fp64 records): (new state, stats, flat gradient the step used)"""
    lo, hi = q_range(actor_sizes, q_sizes)
    st_c, g_c, ex_c = critic_phase(state["params"], state["targets"], actor_sizes, q_sizes, rows, sel, eps_pi, eps_next, cfg, act_actor, act_q)
    zeros = {name: np.zeros(sh) for name, sh in flat_shapes(actor_sizes, q_sizes)}
    gc = join({**zeros, **g_c}, actor_sizes, q_sizes)
    p, m, v = critic_update(state, gc, actor_sizes, q_sizes, cfg)
    st_a, g_a, ex_a = actor_phase(p, actor_sizes, q_sizes, rows, sel, eps_pi, ex_c["alpha"], act_actor, act_q)
    ga = join({**zeros, **g_a}, actor_sizes, q_sizes)
    t = state["t"] + 1
    p, m, v = actor_update(p, m, v, t, ga, actor_sizes, q_sizes, cfg)
    targets = np.asarray(state["targets"], dtype=np.float64)
    if polyak_due(t, cfg):
        targets = polyak(p[lo:hi], targets, cfg["tau"])
    stats = {**st_c, **st_a}
    return dict(params=p, m=m, v=v, targets=targets, t=t), stats, gc + ga


def action_err(pi, e_out):
    """the error of a = tanh(mean + exp(ls) eps) given the error e_out [mb, 2 nu] of the actor's output: expf at 2 ulp and the fma give
    the error dx of x; tanh' <= 1 - tanh(|x| - dx)^2 over that interval, and tanhf at 4 ulp"""
    nu = pi["mean"].shape[1]
    e_mean, e_ls = e_out[:, :nu], e_out[:, nu:]
    se = pi["s"] * np.abs(pi["eps"])
    dx = e_mean + se * (np.expm1(e_ls) + 3 * U) + U * np.abs(pi["x"])
    return (1.0 - np.tanh(np.maximum(np.abs(pi["x"]) - dx, 0.0)) ** 2) * dx + 4 * U


def lp_err(h, e_out):
    """the error of a row's log-probability given the error e_out of the actor's output (h: the head's dict)"""
    nu = h["mean"].shape[1]
    e_mean, e_ls = e_out[:, :nu], e_out[:, nu:]
    dx = e_mean + h["s"] * np.abs(h["eps"]) * (np.expm1(e_ls) + 3 * U) + U * np.abs(h["x"])
    M = 0.5 * h["eps"] ** 2 + np.abs(h["ls"]) + HALF_LOG_2PI + 2.0 * (LOG2 + np.abs(h["x"]) + LOG2)
    return (e_ls + 2.0 * dx).sum(axis=1) + (nu + 10) * U * M.sum(axis=1)


def target(flat, targets, actor_sizes, q_sizes, rows, sel, eps_next, cfg, act_actor="tanh", act_q="tanh"):
    """y = reward + (1 - done) gamma (min(Q1', Q2') - alpha lp') of rows sel, the targets on the Q networks' activation, and its float32
    bound by row: the target networks' forward errors with the next action's error carried in, lp_err, and the roundings of the sum"""
    t = split(np.asarray(flat, dtype=np.float64), actor_sizes, q_sizes)
    tt = with_targets(t, targets, actor_sizes, q_sizes)
    La, Lq = len(actor_sizes) - 1, len(q_sizes) - 1
    rew, nobs_, done = (np.asarray(rows[k], dtype=np.float64)[sel] for k in ("reward", "next_obs", "done"))
    alpha = float(np.float32(np.exp(float(t["log_ent_coef"][0]))))
    nx = head(t, La, nobs_, eps_next, act_actor)
    e_nx = ml.fwd_err(t, "actor", La, nx["acts"], act_actor)[0]
    xq = np.concatenate([nobs_, nx["a"]], axis=1)
    e_in = np.concatenate([np.zeros(nobs_.shape), action_err(nx, e_nx)], axis=1)
    qt, e_t = [], []
    for tag in ("q1", "q2"):
        acts, q, _ = ml.forward(tt, tag, Lq, xq, act_q)
        qt.append(q[:, 0])
        e_t.append(ml.fwd_err(tt, tag, Lq, acts, act_q, e_in)[0][:, 0])
    mq = np.minimum(qt[0], qt[1])
    y = rew + (1.0 - done) * float(cfg["gamma"]) * (mq - alpha * nx["lp"])
    dy = (1.0 - done) * float(cfg["gamma"]) * (np.maximum(e_t[0], e_t[1]) + alpha * lp_err(nx, e_nx) + 3 * U * (np.abs(mq) + np.abs(alpha * nx["lp"]))) + 2 * U * np.abs(y)
    return y, dy


def torch_losses(torch, dtype, flat, targets, actor_sizes, q_sizes, rows, sel, eps_pi, eps_next, cfg, alpha=None, act_actor="tanh", act_q="tanh"):
    """SB3's SAC.train losses written with torch ops on CPU leaves of `dtype` (one leaf per tensor of the flat record), at ONE set of
    parameters (the critic step between the critic and the actor loss is the caller's), the targets on the Q networks' activation:
    (ent_coef_loss, critic_loss, actor_loss, leaves).
    autograd in float64 is what the reference is held to; in float32 it is the noise floor of an independent evaluation."""
    nu = actor_sizes[-1] // 2
    leaves = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in split(flat, actor_sizes, q_sizes).items()}
    targ = {k: torch.tensor(v, dtype=dtype) for k, v in with_targets(split(flat, actor_sizes, q_sizes), targets, actor_sizes, q_sizes).items()}

    def q(par, tag, x):
        return ml.torch_mlp(torch, par, tag, len(q_sizes) - 1, x, act_q)

    def sample(obs, eps):
        out = ml.torch_mlp(torch, leaves, "actor", len(actor_sizes) - 1, obs, act_actor)
        mean, ls = out[:, :nu], torch.clamp(out[:, nu:], -20.0, 2.0)
        x = mean + ls.exp() * eps
        # (log 2 - x - softplus(-2 x) written as log 2 - |x| - log1p(exp(-2 |x|)): torch's softplus is x itself above its threshold of 20)
        lp = (-0.5 * eps ** 2 - ls - HALF_LOG_2PI).sum(dim=1) - (2.0 * (LOG2 - x.abs() - torch.log1p(torch.exp(-2.0 * x.abs())))).sum(dim=1)
        return torch.tanh(x), lp
    obs, act, rew, nobs_, done = (torch.tensor(np.asarray(rows[k], dtype=np.float64)[sel], dtype=dtype) for k in ("obs", "action", "reward", "next_obs", "done"))
    e_pi, e_nx = torch.tensor(np.asarray(eps_pi, dtype=np.float64), dtype=dtype), torch.tensor(np.asarray(eps_next, dtype=np.float64), dtype=dtype)
    a_pi, lp_pi = sample(obs, e_pi)
    lec = leaves["log_ent_coef"]
    # (alpha given: the value of the start of the step, where flat already holds the stepped log_ent_coef)
    alpha = torch.tensor(float(np.float32(np.exp(float(lec.detach()[0])))) if alpha is None else float(alpha), dtype=dtype)
    ent_loss = -(lec * (lp_pi.detach() + target_entropy(cfg, nu))).mean()
    with torch.no_grad():
        a_nx, lp_nx = sample(nobs_, e_nx)
        xq = torch.cat([nobs_, a_nx], dim=1)
        y = rew + (1 - done) * float(cfg["gamma"]) * (torch.min(q(targ, "q1", xq), q(targ, "q2", xq))[:, 0] - alpha * lp_nx)
    xin = torch.cat([obs, act], dim=1)
    critic_loss = 0.5 * (torch.nn.functional.mse_loss(q(leaves, "q1", xin)[:, 0], y) + torch.nn.functional.mse_loss(q(leaves, "q2", xin)[:, 0], y))
    xpi = torch.cat([obs, a_pi], dim=1)
    min_q = torch.min(q(leaves, "q1", xpi), q(leaves, "q2", xpi))[:, 0]
    actor_loss = (alpha * lp_pi - min_q).mean()
    return ent_loss, critic_loss, actor_loss, leaves


def random_problem(actor_sizes, q_sizes, n_rows, seed):
    """Random networks (flat fp64 record whose entries are float32 values), a targets' record that differs from Q1, Q2, random rows and
    both draws, [n_rows, nu] each, tied to the ROW (a minibatch of rows sel uses eps[sel]).  The bias of two log_std columns is near -26,
    of one near +4, of the others uniform in [-6, 1.5], and that half of the top layer's weights is scaled by 4: about 9 % of the raw
    log_std entries lie below -20 and 5 to 15 % above 2 (more for a one-layer actor, whose log_std sees the observations themselves).
    A row where |Q1 - Q2|(obs, a_pi) < 1e-4 max|Q| or a raw log_std lies within 1e-3 of a bound is redrawn: its gradient branch can flip
    at float32 resolution.  So that the worst-case float32 forward bound of every network (mlp_ref.fwd_err) stays below a quarter of those
    margins, the layers below the top are drawn N(0, ACTOR_LOWER_SCALE^2 / K) for the actor and N(0, Q_LOWER_SCALE^2 / K) for the Q
    networks (the top layers N(0, 1 / K)): that bound grows by about 0.8 sqrt(K) times a layer's scale per layer.  The Q networks' top
    bias is near Q_TOP_BIAS, values of a few units as a trained critic has them, which is what max|Q| and so the margin is relative to;
    Q2's is then moved so that the twins agree on average and each is the smaller one on about half of the rows.
    Returns dict(flat, targets, rows, eps_pi, eps_next, rejected)."""
    rng = np.random.default_rng(seed)
    nobs, nu = actor_sizes[0], actor_sizes[-1] // 2
    La, Lq = len(actor_sizes) - 1, len(q_sizes) - 1
    t = {}
    for name, sh in flat_shapes(actor_sizes, q_sizes):
        if name == "log_ent_coef":
            t[name] = np.array([np.log(0.3)])
        elif len(sh) == 2:
            top_layer = int(name[-1]) == (La if name.startswith("actor") else Lq) - 1
            t[name] = rng.normal(0.0, (1.0 if top_layer else ACTOR_LOWER_SCALE if name.startswith("actor") else Q_LOWER_SCALE) / np.sqrt(sh[0]), sh)
        else:
            t[name] = rng.normal(0.0, 0.1, sh)
    for tag in ("q1", "q2"):
        t["%s.b%d" % (tag, Lq - 1)] = Q_TOP_BIAS + 0.2 * t["%s.b%d" % (tag, Lq - 1)]
    top = "actor.w%d" % (La - 1), "actor.b%d" % (La - 1)
    t[top[0]][:, nu:] *= 4.0
    t[top[1]][nu:] = rng.uniform(-6.0, 1.5, nu)
    t[top[1]][nu + 1], t[top[1]][nu + 7], t[top[1]][nu + 4] = -26.0, -25.8, 4.0
    flat = join(t, actor_sizes, q_sizes).astype(np.float32).astype(np.float64)
    t = split(flat, actor_sizes, q_sizes)
    lo, hi = q_range(actor_sizes, q_sizes)

    def draw(n):
        return dict(obs=rng.normal(0.0, 1.0, (n, nobs)).astype(np.float32), next_obs=rng.normal(0.0, 1.0, (n, nobs)).astype(np.float32),
                    eps_pi=rng.normal(0.0, 1.0, (n, nu)).astype(np.float32), eps_next=rng.normal(0.0, 1.0, (n, nu)).astype(np.float32))

    def bad(d):
        pi = head(t, La, d["obs"], d["eps_pi"])
        xin = np.concatenate([d["obs"].astype(np.float64), pi["a"]], axis=1)
        q1, q2 = ml.forward(t, "q1", Lq, xin)[1][:, 0], ml.forward(t, "q2", Lq, xin)[1][:, 0]
        qmax = max(np.abs(q1).max(), np.abs(q2).max())
        near = (np.minimum(np.abs(pi["raw"] + 20.0), np.abs(pi["raw"] - 2.0)) < 1e-3).any(axis=1)
        return (np.abs(q1 - q2) < 1e-4 * qmax) | near
    d = draw(n_rows)
    # twin critics agree on average: Q2's top bias is moved so that neither network is the smaller one on nearly every row
    pi0 = head(t, La, d["obs"], d["eps_pi"])
    x0 = np.concatenate([d["obs"].astype(np.float64), pi0["a"]], axis=1)
    shift = np.float32((ml.forward(t, "q1", Lq, x0)[1] - ml.forward(t, "q2", Lq, x0)[1]).mean())
    t["q2.b%d" % (Lq - 1)] = (t["q2.b%d" % (Lq - 1)] + shift).astype(np.float32).astype(np.float64)
    flat = join(t, actor_sizes, q_sizes)
    targets = (flat[lo:hi] + rng.normal(0.0, 0.02, hi - lo)).astype(np.float32).astype(np.float64)
    rejected = 0
    for _ in range(100):
        b = np.flatnonzero(bad(d))
        # (qmax moves with the rows: the loop ends when no row of the final set fails)
        if not len(b):
            break
        rejected += len(b)
        new = draw(len(b))
        for k in d:
            d[k][b] = new[k]
    else:
        raise AssertionError("random_problem: rows keep failing the margins")
    rows = dict(obs=d["obs"], next_obs=d["next_obs"], action=np.tanh(rng.normal(0.0, 1.0, (n_rows, nu))).astype(np.float32),
                reward=rng.normal(0.0, 1.0, n_rows).astype(np.float32), done=(rng.random(n_rows) < 0.15).astype(np.uint8))
    rows["done"][:2] = (1, 0)
    return dict(flat=flat, targets=targets, rows=rows, eps_pi=d["eps_pi"], eps_next=d["eps_next"], rejected=rejected)
