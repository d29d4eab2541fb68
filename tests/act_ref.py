"""fp64 numpy restatement of an MLP with a chosen hidden activation (include/hb.h: hb_mlp_set_activation) - tanh, ReLU or ELU behind every
hidden layer, the last layer linear: the forward pass with kept activations, the backward pass that forms the derivative from the kept
OUTPUT a as the kernels do (1 - a^2; a > 0 ? 1 : 0; a > 0 ? 1 : a + 1), the derived float32 forward bound, and the margin condition of
the inputs.  Around them the two learners' losses in torch (float64: what the kernels' gradients are held to; float32: the noise floor)
and the fixed problems tests/test_gpu_act.py runs, whose conditions tests/test_act_cpu.py asserts without a device.

The forward bound is the layer recurrence of tests/test_gpu_ppo.py and sac_ref.py, e' = (K + 2) u (|a| |W| + |b|) + e |W| + c u, with the
activation's own term c: 4 ulp behind tanhf, 0 behind ReLU (a select), EXPM1_ULP behind ELU (|expm1(v)| < 1 for v <= 0, so an ulp of the
result is at most u; v > 0 is passed through).  All three have slopes of at most 1, so the error carried in is not amplified.

The margin condition: ReLU's derivative jumps at 0, so a hidden pre-activation whose fp64 value lies within the float32 forward error of 0
may land on the other side on the device and the gradient then differs by O(1).  Every hidden pre-activation z of every tested row has to
satisfy |z| >= MARGIN x the forward bound of z (the recurrence up to that layer, before the activation's term).  No row is dropped and
nothing is redrawn: with thousands of pre-activations per problem hardly any seed satisfies that by itself, so the generators move the
BIAS of a hidden unit that has a row inside the margin by the smallest multiple of the margin that frees all of its rows (clear_margins),
layer by layer - a condition on the inputs, formed from the reference alone; test_act_cpu.py asserts it for exactly the problems the GPU
tests run."""
import numpy as np

import ppo_ref as pr
import sac_ref as sr

U = 2.0 ** -24
ACTIVATIONS = ("tanh", "relu", "elu")
# expm1f on the device over every float32 in [-20, -0] against fp64: worst error 0.8905 ulp (profiles/act_parity.txt); twice that, rounded up
EXPM1_ULP = 2
ACT_ULP = {"tanh": 4, "relu": 0, "elu": EXPM1_ULP}
MARGIN = 4.0
NOBS, NU = 48, 21


def act(name, z):
    if name == "tanh":
        return np.tanh(z)
    if name == "relu":
        return np.where(z < 0.0, 0.0, z)
    assert name == "elu", name
    return np.where(z > 0.0, z, np.expm1(np.minimum(z, 0.0)))


def slope(name, a):
    """the activation's derivative from its OUTPUT a"""
    if name == "tanh":
        return 1.0 - a * a
    if name == "relu":
        return np.where(a > 0.0, 1.0, 0.0)
    assert name == "elu", name
    return np.where(a > 0.0, 1.0, a + 1.0)


def forward(tensors, tag, n_layers, x, activation):
    """acts[l]: the input of layer l (acts[0] = x); the last layer's (linear) output; zs[l]: the pre-activation of hidden layer l"""
    acts, zs, a = [], [], np.asarray(x, dtype=np.float64)
    for l in range(n_layers):
        acts.append(a)
        z = a @ np.asarray(tensors["%s.w%d" % (tag, l)], dtype=np.float64) + np.asarray(tensors["%s.b%d" % (tag, l)], dtype=np.float64)
        if l < n_layers - 1:
            zs.append(z)
            a = act(activation, z)
        else:
            a = z
    return acts, a, zs


def backward(tensors, tag, n_layers, acts, dz, activation, grads=None):
    """dz: dloss / d(the last layer's output); fills grads[tag.w*], grads[tag.b*] where grads is given; returns dloss / d(input rows)"""
    for l in range(n_layers - 1, -1, -1):
        if grads is not None:
            grads["%s.w%d" % (tag, l)] = acts[l].T @ dz
            grads["%s.b%d" % (tag, l)] = dz.sum(axis=0)
        dz = dz @ np.asarray(tensors["%s.w%d" % (tag, l)], dtype=np.float64).T
        if l > 0:
            dz = dz * slope(activation, acts[l])
    return dz


def fwd_err(tensors, tag, n_layers, acts, activation, e0=None):
    """(the bound of the last layer's output by row and column, [the bound of every hidden layer's PRE-activation])"""
    e = np.zeros_like(acts[0]) if e0 is None else e0
    pre = []
    for l in range(n_layers):
        W, bias = np.abs(tensors["%s.w%d" % (tag, l)]), np.abs(tensors["%s.b%d" % (tag, l)])
        e = (W.shape[0] + 2) * U * (np.abs(acts[l]) @ W + bias) + e @ W
        if l < n_layers - 1:
            pre.append(e)
            e = e + ACT_ULP[activation] * U
    return e, pre


def margin(tensors, tag, n_layers, x, activation, e0=None):
    """the smallest |z| / forward bound of z over the hidden pre-activations of rows x (inf for a network without hidden layers)"""
    acts, _, zs = forward(tensors, tag, n_layers, x, activation)
    _, pre = fwd_err(tensors, tag, n_layers, acts, activation, e0)
    return min([float((np.abs(z) / e).min()) for z, e in zip(zs, pre)], default=np.inf)


def clear_margins(views, tag, n_layers, activation, target=3.0 * MARGIN):
    """views: [(tensors, x, e0)] - the network `tag` on rows x (input error e0 or None), possibly at several parameter sets that share their
    hidden biases up to an offset.  Moves, in every view alike, the bias of each hidden unit that has a pre-activation within target x its
    forward bound, until none has; the bias stays a float32 value in views[0].  Returns the number of biases moved."""
    moved = 0
    for l in range(n_layers - 1):
        for _ in range(20):
            zs, es = [], []
            for t, x, e0 in views:
                acts, _, z = forward(t, tag, n_layers, x, activation)
                zs.append(z[l])
                es.append(fwd_err(t, tag, n_layers, acts, activation, e0)[1][l])
            z, e = np.concatenate(zs), np.concatenate(es)
            bad = np.flatnonzero((np.abs(z) < target * e).any(axis=0))
            if not len(bad):
                break
            for j in bad:
                step = target * e[:, j].max()
                d = next(s * k * step for k in range(1, 1000) for s in (1.0, -1.0) if (np.abs(z[:, j] + s * k * step) >= 1.5 * target * e[:, j]).all())
                b0 = views[0][0]["%s.b%d" % (tag, l)]
                delta = float(np.float32(b0[j] + d)) - b0[j]
                for t, _, _ in views:
                    t["%s.b%d" % (tag, l)][j] += delta
                moved += 1
        else:
            raise AssertionError("clear_margins: layer %d of %s keeps rows inside the margin" % (l, tag))
    return moved


def layers(t, tag, sizes):
    n = len(sizes) - 1
    return [np.asarray(t["%s.w%d" % (tag, l)], dtype=np.float32) for l in range(n)], [np.asarray(t["%s.b%d" % (tag, l)], dtype=np.float32) for l in range(n)]


# ---- the shapes of tests/test_gpu_act.py: 24 envs, minibatches of 40 rows (neither a multiple of the 16-row tile).  Hidden widths 20
# (two tiles: split K, the merge loop's hook) and 72 (five tiles, not a multiple of 16: the direct hook); one hidden layer of 256; the Q
# networks' input nobs + nu = 69 is no multiple of 4 (its pad columns are used)
N_ENV, MB, N_ROWS = 24, 40, 56
HIDDEN = {"h20_72": (20, 72), "h256": (256,)}


SEL = np.random.default_rng(77).permutation(N_ROWS)[:MB]   # the minibatch: rows SEL of the N_ROWS
# the seeds of the problems test_gpu_act.py runs, (net, activation) -> seed (SAC: the first from 1 whose problem also keeps the raw
# log_std off the clamp bounds and Q1 off Q2 at obs | a_pi, sac_conditions; test_act_cpu.py asserts all of it)
PPO_SEEDS = {(net, a): 1 for net in HIDDEN for a in ("relu", "elu")}
SAC_SEEDS = {("h20_72", "relu"): 1, ("h20_72", "elu"): 1, ("h256", "relu"): 14, ("h256", "elu"): 2}


def ppo_sizes(net):
    return [NOBS, *HIDDEN[net], NU], [NOBS, *HIDDEN[net], 1]


def sac_sizes(net):
    return [NOBS, *HIDDEN[net], 2 * NU], [NOBS + NU, *HIDDEN[net], 1]


# ---- PPO

def torch_act(torch, activation):
    return {"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU, "elu": torch.nn.ELU}[activation]()


def torch_mlp(torch, par, tag, n, x, activation):
    f = torch_act(torch, activation)
    for l in range(n):
        x = x @ par["%s.w%d" % (tag, l)] + par["%s.b%d" % (tag, l)]
        if l < n - 1:
            x = f(x)
    return x


def torch_ppo_loss(torch, dtype, flat, asz, csz, rows, cfg, sel, act_actor, act_critic):
    """ppo_ref.torch_loss with the hidden activations as torch.nn modules: (loss, leaves)"""
    nu = asz[-1]
    leaves = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in pr.split(flat, asz, csz, nu).items()}
    obs, action, old, adv, ret = (torch.tensor(np.asarray(rows[k], dtype=np.float64)[sel], dtype=dtype) for k in ("obs", "action", "old_log_prob", "advantage", "returns"))
    mu = torch_mlp(torch, leaves, "actor", len(asz) - 1, obs, act_actor)
    v = torch_mlp(torch, leaves, "critic", len(csz) - 1, obs, act_critic)[:, 0]
    dist = torch.distributions.Normal(mu, torch.ones_like(mu) * leaves["log_std"].exp())
    lp = dist.log_prob(action).sum(dim=1)
    if cfg["normalize_advantage"] and len(sel) > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(lp - old)
    c = cfg["clip_range"]
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - c, 1 + c)).mean()
    value_loss = torch.nn.functional.mse_loss(ret, v)
    entropy_loss = -dist.entropy().sum(dim=1).mean()
    return policy_loss + cfg["ent_coef"] * entropy_loss + cfg["vf_coef"] * value_loss, leaves


def torch_grads(torch, loss, leaves, names):
    g = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    return {k: (np.zeros(tuple(leaves[k].shape)) if x is None else x.detach().numpy().astype(np.float64)) for k, x in zip(names, g)}


def ppo_problem(net, act_actor, act_critic, seed):
    """ppo_ref.random_problem's networks and tapes with the actions and old log-probabilities formed by the chosen activation's actor:
    (flat fp64 record of float32 values, rows)"""
    asz, csz = ppo_sizes(net)
    flat, rows = pr.random_problem(asz, csz, N_ROWS, seed=seed)
    t = pr.split(flat, asz, csz, NU)
    obs = np.asarray(rows["obs"], dtype=np.float64)
    clear_margins([(t, obs, None)], "actor", len(asz) - 1, act_actor)
    clear_margins([(t, obs, None)], "critic", len(csz) - 1, act_critic)
    flat = pr.join(t, asz, csz, NU)
    assert np.array_equal(flat, flat.astype(np.float32))
    rng = np.random.default_rng(seed + 10000)
    _, mu, _ = forward(t, "actor", len(asz) - 1, rows["obs"], act_actor)
    ls = t["log_std"]
    action = (mu + np.exp(ls) * rng.normal(0.0, 1.0, mu.shape)).astype(np.float32)
    lp = (-(action - mu) ** 2 / (2.0 * np.exp(2.0 * ls)) - ls - pr.HALF_LOG_2PI).sum(axis=1)
    rows = dict(rows, action=action, old_log_prob=(lp + rng.normal(0.0, 0.3, N_ROWS)).astype(np.float32))
    return flat, rows


def ppo_margin(net, flat, rows, act_actor, act_critic):
    asz, csz = ppo_sizes(net)
    t = pr.split(flat, asz, csz, NU)
    obs = np.asarray(rows["obs"], dtype=np.float64)
    return min(margin(t, "actor", len(asz) - 1, obs, act_actor), margin(t, "critic", len(csz) - 1, obs, act_critic))


# ---- SAC

def sac_cfg(**kw):
    """the learner's config of the GPU test as the C struct holds it (float32 numbers)"""
    c = sr.config(**dict(dict(lr_actor=1e-3, lr_critic=1e-3, lr_ent=1e-3, ent_coef_init=0.3), **kw))
    ints = ("auto_ent", "target_entropy_auto", "target_update_interval", "seed")
    return {k: (int(v) if k in ints else float(np.float32(v))) for k, v in c.items()}


def sac_head(t, n_layers, obs, eps, activation):
    """sac_ref.head with the chosen hidden activation"""
    acts, out, zs = forward(t, "actor", n_layers, obs, activation)
    nu = out.shape[1] // 2
    mean, raw = out[:, :nu], out[:, nu:]
    ls = np.clip(raw, -20.0, 2.0)
    s = np.exp(ls)
    eps = np.asarray(eps, dtype=np.float64)
    x = mean + s * eps
    a = np.tanh(x)
    lp = (-0.5 * eps ** 2 - ls - sr.HALF_LOG_2PI).sum(axis=1) - (2.0 * (sr.LOG2 - x - sr.softplus(-2.0 * x))).sum(axis=1)
    return dict(acts=acts, mean=mean, raw=raw, ls=ls, s=s, x=x, a=a, lp=lp, eps=eps)


def torch_sac_losses(torch, dtype, flat, targets, asz, qsz, rows, sel, eps_pi, eps_next, cfg, act_actor, act_q, alpha=None):
    """sac_ref.torch_losses with the hidden activations as torch.nn modules (the targets run the Q networks' activation):
    (ent_coef_loss, critic_loss, actor_loss, leaves)"""
    nu = asz[-1] // 2
    leaves = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in sr.split(flat, asz, qsz).items()}
    targ = {k: torch.tensor(v, dtype=dtype) for k, v in sr.with_targets(sr.split(flat, asz, qsz), targets, asz, qsz).items()}

    def sample(obs, eps):
        out = torch_mlp(torch, leaves, "actor", len(asz) - 1, obs, act_actor)
        mean, ls = out[:, :nu], torch.clamp(out[:, nu:], -20.0, 2.0)
        x = mean + ls.exp() * eps
        lp = (-0.5 * eps ** 2 - ls - sr.HALF_LOG_2PI).sum(dim=1) - (2.0 * (sr.LOG2 - x.abs() - torch.log1p(torch.exp(-2.0 * x.abs())))).sum(dim=1)
        return torch.tanh(x), lp
    obs, action, rew, nobs_, done = (torch.tensor(np.asarray(rows[k], dtype=np.float64)[sel], dtype=dtype) for k in ("obs", "action", "reward", "next_obs", "done"))
    e_pi, e_nx = torch.tensor(np.asarray(eps_pi, dtype=np.float64), dtype=dtype), torch.tensor(np.asarray(eps_next, dtype=np.float64), dtype=dtype)
    Lq = len(qsz) - 1
    a_pi, lp_pi = sample(obs, e_pi)
    lec = leaves["log_ent_coef"]
    alpha = torch.tensor(float(np.float32(np.exp(float(lec.detach()[0])))) if alpha is None else float(alpha), dtype=dtype)
    ent_loss = -(lec * (lp_pi.detach() + sr.target_entropy(cfg, nu))).mean()
    with torch.no_grad():
        a_nx, lp_nx = sample(nobs_, e_nx)
        xq = torch.cat([nobs_, a_nx], dim=1)
        y = rew + (1 - done) * float(cfg["gamma"]) * (torch.min(torch_mlp(torch, targ, "q1", Lq, xq, act_q), torch_mlp(torch, targ, "q2", Lq, xq, act_q))[:, 0] - alpha * lp_nx)
    xin = torch.cat([obs, action], dim=1)
    critic_loss = 0.5 * (torch.nn.functional.mse_loss(torch_mlp(torch, leaves, "q1", Lq, xin, act_q)[:, 0], y) +
                         torch.nn.functional.mse_loss(torch_mlp(torch, leaves, "q2", Lq, xin, act_q)[:, 0], y))
    xpi = torch.cat([obs, a_pi], dim=1)
    min_q = torch.min(torch_mlp(torch, leaves, "q1", Lq, xpi, act_q), torch_mlp(torch, leaves, "q2", Lq, xpi, act_q))[:, 0]
    actor_loss = (alpha * lp_pi - min_q).mean()
    return ent_loss, critic_loss, actor_loss, leaves


def sac_mid(torch, net, flat, targets, rows, sel, eps_pi, eps_next, cfg, act_actor, act_q):
    """the parameters the actor phase runs at: the reference's critic step (torch float64 autograd, sac_ref's Adam) from zero moments"""
    asz, qsz = sac_sizes(net)
    losses = torch_sac_losses(torch, torch.float64, flat, targets, asz, qsz, rows, sel, eps_pi, eps_next, cfg, act_actor, act_q)
    g = torch_grads(torch, losses[0] + losses[1], losses[3], [k for k, _ in sr.flat_shapes(asz, qsz)])
    state = dict(params=flat, m=np.zeros_like(flat), v=np.zeros_like(flat), t=0)
    return sr.critic_update(state, sr.join(g, asz, qsz), asz, qsz, cfg)[0]


def sac_problem(torch, net, act_actor, act_q, seed):
    """Random networks in sac_ref.random_problem's scales (flat fp64 record of float32 values), a targets' record that differs from Q1, Q2,
    N_ROWS random rows and both draws; the minibatch is rows SEL with sac_cfg().  The hidden biases are moved (clear_margins) until the
    actor on obs, Q1 and Q2 on obs | action and - at the reference's critic step, sac_mid - Q1 and Q2 on obs | a_pi keep the margin on the
    minibatch's rows.  sac_conditions states everything the minibatch has to satisfy; the seed takes care of the rest."""
    asz, qsz = sac_sizes(net)
    rng = np.random.default_rng(seed)
    La, Lq = len(asz) - 1, len(qsz) - 1
    t = {}
    for name, sh in sr.flat_shapes(asz, qsz):
        if name == "log_ent_coef":
            t[name] = np.array([np.log(0.3)])
        elif len(sh) == 2:
            top = int(name[-1]) == (La if name.startswith("actor") else Lq) - 1
            t[name] = rng.normal(0.0, (1.0 if top else sr.ACTOR_LOWER_SCALE if name.startswith("actor") else sr.Q_LOWER_SCALE) / np.sqrt(sh[0]), sh)
        else:
            t[name] = rng.normal(0.0, 0.1, sh)
    t["q1.b%d" % (Lq - 1)] = sr.Q_TOP_BIAS + 0.2 * t["q1.b%d" % (Lq - 1)]
    t["q2.b%d" % (Lq - 1)] = sr.Q_TOP_BIAS + 0.2 * t["q2.b%d" % (Lq - 1)]
    t["actor.w%d" % (La - 1)][:, NU:] *= 4.0
    t["actor.b%d" % (La - 1)][NU:] = rng.uniform(-6.0, 1.5, NU)
    t["actor.b%d" % (La - 1)][NU + 1], t["actor.b%d" % (La - 1)][NU + 4] = -26.0, 4.0   # (a log_std column below the clamp, one above)
    flat = sr.join(t, asz, qsz).astype(np.float32).astype(np.float64)
    lo, hi = sr.q_range(asz, qsz)
    targets = (flat[lo:hi] + rng.normal(0.0, 0.02, hi - lo)).astype(np.float32).astype(np.float64)
    n = N_ROWS
    rows = dict(obs=rng.normal(0.0, 1.0, (n, NOBS)).astype(np.float32), next_obs=rng.normal(0.0, 1.0, (n, NOBS)).astype(np.float32),
                action=np.tanh(rng.normal(0.0, 1.0, (n, NU))).astype(np.float32), reward=rng.normal(0.0, 1.0, n).astype(np.float32),
                done=(rng.random(n) < 0.15).astype(np.uint8))
    rows["done"][:2] = (1, 0)
    pb = dict(flat=flat, targets=targets, rows=rows, eps_pi=rng.normal(0.0, 1.0, (n, NU)).astype(np.float32),
              eps_next=rng.normal(0.0, 1.0, (n, NU)).astype(np.float32))
    cfg = sac_cfg()
    ep, en = pb["eps_pi"][SEL], pb["eps_next"][SEL]
    obs, action = np.asarray(rows["obs"], dtype=np.float64)[SEL], np.asarray(rows["action"], dtype=np.float64)[SEL]
    t = sr.split(flat, asz, qsz)
    clear_margins([(t, obs, None)], "actor", La, act_actor)
    pi = sac_head(t, La, obs, ep, act_actor)
    e_in = np.concatenate([np.zeros((MB, NOBS)), sr.action_err(pi, fwd_err(t, "actor", La, pi["acts"], act_actor)[0])], axis=1)
    xin, xpi = np.concatenate([obs, action], axis=1), np.concatenate([obs, pi["a"]], axis=1)
    for _ in range(8):
        tm = sr.split(sac_mid(torch, net, sr.join(t, asz, qsz), targets, rows, SEL, ep, en, cfg, act_actor, act_q), asz, qsz)
        if not sum(clear_margins([(t, xin, None), (tm, xpi, e_in)], tag, Lq, act_q) for tag in ("q1", "q2")):
            break
    else:
        raise AssertionError("sac_problem: the critic step keeps moving rows into the margin")
    pb["flat"] = sr.join(t, asz, qsz)
    assert np.array_equal(pb["flat"], pb["flat"].astype(np.float32))
    return pb


def lp_err(h, e_out):
    """the error of a row's log-probability given the error of the actor's output (tests/test_gpu_sac.py: _lp_err)"""
    nu = h["mean"].shape[1]
    e_mean, e_ls = e_out[:, :nu], e_out[:, nu:]
    dx = e_mean + h["s"] * np.abs(h["eps"]) * (np.expm1(e_ls) + 3 * U) + U * np.abs(h["x"])
    M = 0.5 * h["eps"] ** 2 + np.abs(h["ls"]) + sr.HALF_LOG_2PI + 2.0 * (sr.LOG2 + np.abs(h["x"]) + sr.LOG2)
    return (e_ls + 2.0 * dx).sum(axis=1) + (nu + 10) * U * M.sum(axis=1)


def sac_target(net, flat, targets, rows, sel, eps_next, cfg, act_actor, act_q):
    """y = reward + (1 - done) gamma (min(Q1', Q2') - alpha lp') of rows sel with the targets on the Q networks' activation, and its
    float32 bound by row (tests/test_gpu_sac.py: _derived_critic's dy)"""
    asz, qsz = sac_sizes(net)
    t = sr.split(np.asarray(flat, dtype=np.float64), asz, qsz)
    tt = sr.with_targets(t, targets, asz, qsz)
    La, Lq = len(asz) - 1, len(qsz) - 1
    rew, nobs_, done = (np.asarray(rows[k], dtype=np.float64)[sel] for k in ("reward", "next_obs", "done"))
    alpha = float(np.float32(np.exp(float(t["log_ent_coef"][0]))))
    nx = sac_head(t, La, nobs_, eps_next, act_actor)
    e_nx = fwd_err(t, "actor", La, nx["acts"], act_actor)[0]
    xq = np.concatenate([nobs_, nx["a"]], axis=1)
    e_in = np.concatenate([np.zeros((len(sel), NOBS)), sr.action_err(nx, e_nx)], axis=1)
    qt, e_t = [], []
    for tag in ("q1", "q2"):
        acts, q, _ = forward(tt, tag, Lq, xq, act_q)
        qt.append(q[:, 0])
        e_t.append(fwd_err(tt, tag, Lq, acts, act_q, e_in)[0][:, 0])
    mq = np.minimum(qt[0], qt[1])
    y = rew + (1.0 - done) * float(cfg["gamma"]) * (mq - alpha * nx["lp"])
    dy = (1.0 - done) * float(cfg["gamma"]) * (np.maximum(e_t[0], e_t[1]) + alpha * lp_err(nx, e_nx) + 3 * U * (np.abs(mq) + np.abs(alpha * nx["lp"]))) + 2 * U * np.abs(y)
    return y, dy


def sac_conditions(net, flat, rows, sel, eps_pi, act_actor, act_q, e_flat=0.0):
    """What a SAC gradient's branches hang on, each as (distance to the branch point) / (float32 forward bound), smallest over rows sel:
    hidden pre-activations of the actor on obs and of Q1, Q2 on obs | action and on obs | a_pi; the raw log_std against the clamp bounds;
    Q1 - Q2 at obs | a_pi (which network is the smaller one).  flat: the parameters the actor phase runs at."""
    asz, qsz = sac_sizes(net)
    t = sr.split(np.asarray(flat, dtype=np.float64), asz, qsz)
    La, Lq = len(asz) - 1, len(qsz) - 1
    obs, action = np.asarray(rows["obs"], dtype=np.float64)[sel], np.asarray(rows["action"], dtype=np.float64)[sel]
    pi = sac_head(t, La, obs, eps_pi, act_actor)
    e_out, _ = fwd_err(t, "actor", La, pi["acts"], act_actor)
    out = dict(actor=margin(t, "actor", La, obs, act_actor))
    out["log_std"] = float((np.minimum(np.abs(pi["raw"] + 20.0), np.abs(pi["raw"] - 2.0)) / e_out[:, NU:]).min())
    xin = np.concatenate([obs, action], axis=1)
    xpi = np.concatenate([obs, pi["a"]], axis=1)
    e_in = np.concatenate([np.zeros((len(sel), NOBS)), sr.action_err(pi, e_out)], axis=1)
    q, e_q = [], []
    for tag in ("q1", "q2"):
        out[tag] = margin(t, tag, Lq, xin, act_q)
        out[tag + "_pi"] = margin(t, tag, Lq, xpi, act_q, e_in)
        acts, qq, _ = forward(t, tag, Lq, xpi, act_q)
        q.append(qq[:, 0])
        e_q.append(fwd_err(t, tag, Lq, acts, act_q, e_in)[0][:, 0])
    out["q1_q2"] = float((np.abs(q[0] - q[1]) / (e_q[0] + e_q[1])).min())
    return out


