"""The fixed problems tests/test_gpu_act.py runs on the MLPs' chosen hidden activation (include/hb.h: hb_mlp_set_activation; the fp64 MLP,
its derivative from the kept output and its float32 forward bound: mlp_ref.py; the two learners' losses with the activations as
arguments: ppo_ref.py, sac_ref.py), the margin condition of their inputs, and that condition's generator.  tests/test_act_cpu.py asserts
the conditions without a device.

The margin condition: ReLU's derivative jumps at 0, so a hidden pre-activation whose fp64 value lies within the float32 forward error of 0
may land on the other side on the device and the gradient then differs by O(1).  Every hidden pre-activation z of every tested row has to
satisfy |z| >= MARGIN x the forward bound of z (mlp_ref.fwd_err's recurrence up to that layer, before the activation's term).  No row is
dropped and nothing is redrawn: with thousands of pre-activations per problem hardly any seed satisfies that by itself, so the generators
move the BIAS of a hidden unit that has a row inside the margin by the smallest multiple of the margin that frees all of its rows
(clear_margins), layer by layer - a condition on the inputs, formed from the reference alone; test_act_cpu.py asserts it for exactly the
problems the GPU tests run."""
import numpy as np

import mlp_ref as ml
import ppo_ref as pr
import sac_ref as sr

MARGIN = 4.0
NOBS, NU = 48, 21


def margin(tensors, tag, n_layers, x, activation, e0=None):
    """the smallest |z| / forward bound of z over the hidden pre-activations of rows x (inf for a network without hidden layers)"""
    acts, _, zs = ml.forward(tensors, tag, n_layers, x, activation)
    _, pre = ml.fwd_err(tensors, tag, n_layers, acts, activation, e0)
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
                acts, _, z = ml.forward(t, tag, n_layers, x, activation)
                zs.append(z[l])
                es.append(ml.fwd_err(t, tag, n_layers, acts, activation, e0)[1][l])
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
    _, mu, _ = ml.forward(t, "actor", len(asz) - 1, rows["obs"], act_actor)
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


def sac_mid(torch, net, flat, targets, rows, sel, eps_pi, eps_next, cfg, act_actor, act_q):
    """the parameters the actor phase runs at: the reference's critic step (torch float64 autograd, sac_ref's Adam) from zero moments"""
    asz, qsz = sac_sizes(net)
    losses = sr.torch_losses(torch, torch.float64, flat, targets, asz, qsz, rows, sel, eps_pi, eps_next, cfg, act_actor=act_actor, act_q=act_q)
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
    pi = sr.head(t, La, obs, ep, act_actor)
    e_in = np.concatenate([np.zeros((MB, NOBS)), sr.action_err(pi, ml.fwd_err(t, "actor", La, pi["acts"], act_actor)[0])], axis=1)
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


def sac_target(net, flat, targets, rows, sel, eps_next, cfg, act_actor, act_q):
    """sac_ref.target for the networks of `net`: (y, its float32 bound by row)"""
    return sr.target(flat, targets, *sac_sizes(net), rows, sel, eps_next, cfg, act_actor, act_q)


def sac_conditions(net, flat, rows, sel, eps_pi, act_actor, act_q, e_flat=0.0):
    """What a SAC gradient's branches hang on, each as (distance to the branch point) / (float32 forward bound), smallest over rows sel:
    hidden pre-activations of the actor on obs and of Q1, Q2 on obs | action and on obs | a_pi; the raw log_std against the clamp bounds;
    Q1 - Q2 at obs | a_pi (which network is the smaller one).  flat: the parameters the actor phase runs at."""
    asz, qsz = sac_sizes(net)
    t = sr.split(np.asarray(flat, dtype=np.float64), asz, qsz)
    La, Lq = len(asz) - 1, len(qsz) - 1
    obs, action = np.asarray(rows["obs"], dtype=np.float64)[sel], np.asarray(rows["action"], dtype=np.float64)[sel]
    pi = sr.head(t, La, obs, eps_pi, act_actor)
    e_out, _ = ml.fwd_err(t, "actor", La, pi["acts"], act_actor)
    out = dict(actor=margin(t, "actor", La, obs, act_actor))
    out["log_std"] = float((np.minimum(np.abs(pi["raw"] + 20.0), np.abs(pi["raw"] - 2.0)) / e_out[:, NU:]).min())
    xin = np.concatenate([obs, action], axis=1)
    xpi = np.concatenate([obs, pi["a"]], axis=1)
    e_in = np.concatenate([np.zeros((len(sel), NOBS)), sr.action_err(pi, e_out)], axis=1)
    q, e_q = [], []
    for tag in ("q1", "q2"):
        out[tag] = margin(t, tag, Lq, xin, act_q)
        out[tag + "_pi"] = margin(t, tag, Lq, xpi, act_q, e_in)
        acts, qq, _ = ml.forward(t, tag, Lq, xpi, act_q)
        q.append(qq[:, 0])
        e_q.append(ml.fwd_err(t, tag, Lq, acts, act_q, e_in)[0][:, 0])
    out["q1_q2"] = float((np.abs(q[0] - q[1]) / (e_q[0] + e_q[1])).min())
    return out
