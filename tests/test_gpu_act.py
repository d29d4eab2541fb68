"""The hidden activation of the installed MLPs (include/hb.h: hb_mlp_set_activation) on the device, ReLU and ELU: every forward kernel
against the fp64 MLP of tests/mlp_ref.py within the derived forward bound, both learners' gradients against torch float64 autograd
on the same rows, an Adam step of each learner, the rules of the interface, and tanh set explicitly against tanh never set, bit for bit.
27-dof humanoid, 24 envs, minibatches of 40 rows; hidden widths 20 | 72 (split-K merge hook | direct hook) and 256 (act_ref.HIDDEN).

Bounds, u = 2^-24:
 - forward: mlp_ref.fwd_err, the layer recurrence e' = (K + 2) u (|a| |W| + |b|) + e |W| + c u with c = 4 (tanhf), 0 (ReLU), 2 (ELU: twice
   the measured worst error of expm1f, profiles/act_parity.txt); behind a tanh output (hb_policy_eval) one more 4 u, behind the clamp of
   log_std nothing (both have slopes of at most 1);
 - gradients, per tensor: max|g_gpu - g_64| <= k max|g_64|, k = 8 x the float32 noise floor - the largest max|g_32 - g_64| / max|g_64| over
   the tensors of the network group, g_32 and g_64 being torch's CPU float32 and float64 autograd of the same loss on the same rows (the
   bound of tests/test_gpu_ppo.py and test_gpu_sac.py; here every tensor of the record is held to it, the head tensors included);
 - the inputs keep the margin condition of act_ref (asserted by tests/test_act_cpu.py for these seeds, and here at the parameters the
   device's own critic step left for the actor phase).
HB_ACT_PARITY_OUT=<file> collects the measured ratios (profiles/act_parity.txt)."""
import os

import numpy as np
import pytest

import act_ref as ac
import mlp_ref as ml
import ppo_ref as pr
import sac_ref as sr
from oracle_lib import HUMANOID_HBM  # noqa: F401  (the model of the humanoid_model fixture)
from sac_lib import state64 as _state64

pytestmark = pytest.mark.gpu

NOBS, NU, U = ac.NOBS, ac.NU, ml.U
N, MB, SEL = ac.N_ENV, ac.MB, ac.SEL
ACTS = ("relu", "elu")
NETS = sorted(ac.HIDDEN)


def _report(line):
    print("\n  " + line)
    out = os.environ.get("HB_ACT_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _ratio(err, bound):
    err, bound = np.atleast_1d(err), np.broadcast_to(bound, np.shape(np.atleast_1d(err)))
    return float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)).max())


def _net(tag, sizes, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    t = {}
    for l in range(len(sizes) - 1):
        t["%s.w%d" % (tag, l)] = rng.normal(0.0, scale / np.sqrt(sizes[l]), (sizes[l], sizes[l + 1])).astype(np.float32)
        t["%s.b%d" % (tag, l)] = rng.normal(0.0, 0.1, sizes[l + 1]).astype(np.float32)
    return t


class Mem:
    """device copies of host arrays, released together"""

    def __init__(self, b):
        self.b, self.ptrs = b, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.b.dev_alloc(max(4, a.nbytes))
        self.b.to_dev(p, a)
        self.ptrs.append(p)
        return p

    def nan(self, shape):
        return self.up(np.full(shape, np.nan, np.float32))

    def free(self):
        for p in self.ptrs:
            self.b.dev_free(p)
        self.ptrs = []


def _env(hbmod, m, gpu, seed=7):
    env = hbmod.VecEnv(m, N, gpu, seed=seed)
    env.reset()
    return env


def _collect(b, mem, obs0, T=1, log_std=False):
    """T collected steps from obs0 through device tapes: dict of numpy tapes"""
    n = b.n_env
    shape = {"obs": (T + 1, n, NOBS), "action": (T, n, NU), "mean": (T, n, NU), "eps": (T, n, NU), "reward": (T, n)}
    if log_std:
        shape["log_std"] = (T, n, NU)
    ptr = {k: mem.nan(s) for k, s in shape.items()}
    first = np.full(shape["obs"], np.nan, np.float32)
    first[0] = obs0
    b.to_dev(ptr["obs"], first)
    b.env_collect_dev(T, 1, **ptr)
    return {k: b.from_dev(ptr[k], s) for k, s in shape.items()}, ptr


def _obs0(seed):
    return np.random.default_rng(seed).normal(0.0, 1.0, (N, NOBS)).astype(np.float32)


# ---- 1. forward

@pytest.mark.parametrize("net", NETS + ["h300_64"])
@pytest.mark.parametrize("activation", ACTS)
def test_policy_eval(hbmod, humanoid_model, gpu, activation, net):
    """hb_policy_kernel, hb_policy_lean_kernel (policy_lean=2) and for a width above 256 the layer-by-layer path; tanh at the top"""
    hidden = (300, 64) if net == "h300_64" else ac.HIDDEN[net]
    sizes = [NOBS, *hidden, NU]
    t = _net("p", sizes, 21)
    b = hbmod.Batch(humanoid_model, N, gpu)
    b.reset(perturb=True)
    b.rollout_halton(30)
    b.set_policy_mlp(*ac.layers(t, "p", sizes), activation=activation)
    assert b.mlp_activation("policy") == activation
    obs, _, _, _ = b.obs(want_reward=False)
    acts, out, _ = ml.forward(t, "p", len(sizes) - 1, obs, activation)
    bound = ml.fwd_err(t, "p", len(sizes) - 1, acts, activation)[0] + 4 * U
    worst = []
    for lean in (1, 2):
        b.tune(policy_lean=lean)
        ctrl = b.policy_eval()
        worst.append(_ratio(np.abs(ctrl - np.tanh(out)), bound))
        assert worst[-1] <= 1.0, (activation, net, lean, worst)
    b.close()
    _report("act forward policy_eval %-4s %-7s: |ctrl - ctrl_64| / bound %.3f (one launch or by layer), %.3f (policy_lean = 2)" % (activation, net, *worst))


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("activation", ACTS)
def test_collected_step_values_and_q(hbmod, humanoid_model, gpu, activation, net):
    """hb_actor_kernel (mean | log_std of one collected step), hb_value_kernel (the GAE call's values), hb_sac_forward_kernel's twin
    (hb_q_values_dev, input nobs + nu = 69: pad columns), each network with `activation`"""
    asz, qsz = ac.sac_sizes(net)
    csz = ac.ppo_sizes(net)[1]
    t = {**_net("actor", asz, 31, 0.5), **_net("critic", csz, 32), **_net("q1", qsz, 33), **_net("q2", qsz, 34)}
    env = _env(hbmod, humanoid_model, gpu)
    b, mem = env.batch, Mem(env.batch)
    b.actor_set(asz, *ac.layers(t, "actor", asz), head="squashed", seed=3, activation=activation)
    b.critic_set(csz, *ac.layers(t, "critic", csz), activation=activation)
    b.q_set(0, qsz, *ac.layers(t, "q1", qsz), activation=activation)
    b.q_set(1, qsz, *ac.layers(t, "q2", qsz), activation=activation)
    assert [b.mlp_activation(k) for k in ("actor", "critic", "q1", "q2")] == [activation] * 4
    tapes, ptr = _collect(b, mem, _obs0(41), log_std=True)
    La = len(asz) - 1
    acts, out, _ = ml.forward(t, "actor", La, tapes["obs"][0], activation)
    e = ml.fwd_err(t, "actor", La, acts, activation)[0]
    r_mean = _ratio(np.abs(tapes["mean"][0] - out[:, :NU]), e[:, :NU])
    r_ls = _ratio(np.abs(tapes["log_std"][0] - np.clip(out[:, NU:], -20.0, 2.0)), e[:, NU:])
    assert r_mean <= 1.0 and r_ls <= 1.0, (r_mean, r_ls)
    # the critic over the collection's obs tape [2][24][48] (row 1: what the env returned)
    pv = mem.nan((2, N))
    b.collect_gae_dev(1, 0.99, 0.95, True, obs=ptr["obs"], value=pv)
    rows = tapes["obs"].reshape(2 * N, NOBS)
    assert np.isfinite(rows).all()
    acts, v, _ = ml.forward(t, "critic", len(csz) - 1, rows, activation)
    r_v = _ratio(np.abs(b.from_dev(pv, (2 * N,)) - v[:, 0]), ml.fwd_err(t, "critic", len(csz) - 1, acts, activation)[0][:, 0])
    assert r_v <= 1.0, r_v
    rng = np.random.default_rng(42)
    obs, action = rng.normal(size=(MB, NOBS)).astype(np.float32), np.tanh(rng.normal(size=(MB, NU))).astype(np.float32)
    p1, p2 = mem.nan(MB), mem.nan(MB)
    b.q_values_dev(mem.up(obs), mem.up(action), MB, q1=p1, q2=p2)
    xin = np.concatenate([obs, action], axis=1)
    r_q = 0.0
    for tag, p in (("q1", p1), ("q2", p2)):
        acts, q, _ = ml.forward(t, tag, len(qsz) - 1, xin, activation)
        r_q = max(r_q, _ratio(np.abs(b.from_dev(p, (MB,)) - q[:, 0]), ml.fwd_err(t, tag, len(qsz) - 1, acts, activation)[0][:, 0]))
    assert r_q <= 1.0, r_q
    mem.free()
    env.close()
    _report("act forward %-4s %-6s: mean %.3f, log_std %.3f, critic values %.3f, q_values %.3f of the derived forward bounds" % (activation, net, r_mean, r_ls, r_v, r_q))


@pytest.mark.parametrize("hidden", [21, 72])
def test_relu_gives_exact_zeros(hbmod, humanoid_model, gpu, hidden):
    """one hidden layer and a top layer that copies the first 21 hidden units (an exact f32 product): the Gaussian head's mean IS the
    hidden activation, 0.0f wherever the fp64 pre-activation is negative, positive elsewhere; widths 21 (merge hook) and 72 (direct hook)"""
    sizes = [NOBS, hidden, NU]
    t = _net("actor", sizes, 51)
    t["actor.w1"], t["actor.b1"] = np.eye(hidden, NU, dtype=np.float32), np.zeros(NU, np.float32)
    obs0 = _obs0(52)
    t = {k: v.astype(np.float64) for k, v in t.items()}
    ac.clear_margins([(t, obs0.astype(np.float64), None)], "actor", 2, "relu")
    assert ac.margin(t, "actor", 2, obs0, "relu") >= ac.MARGIN
    env = _env(hbmod, humanoid_model, gpu)
    b, mem = env.batch, Mem(env.batch)
    b.actor_set(sizes, *ac.layers(t, "actor", sizes), head="gaussian", log_std=np.zeros(NU, np.float32), seed=3, activation="relu")
    tapes, _ = _collect(b, mem, obs0)
    z = ml.forward(t, "actor", 2, obs0, "relu")[2][0][:, :NU]
    mean = tapes["mean"][0]
    assert (z < 0).sum() > 50 and (z > 0).sum() > 50
    assert (mean[z < 0] == 0.0).all() and (mean[z > 0] > 0.0).all()
    mem.free()
    env.close()


# ---- 2. and 4. PPO: one minibatch through hb_ppo_grad_dev, then one Adam step and the collection behind it

@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("activation", ACTS)
def test_ppo_gradients_and_adam_step(hbmod, humanoid_model, gpu, activation, net):
    torch = pytest.importorskip("torch")
    asz, csz = ac.ppo_sizes(net)
    flat, rows = ac.ppo_problem(net, activation, activation, ac.PPO_SEEDS[(net, activation)])
    t = pr.split(flat.astype(np.float32), asz, csz, NU)
    cfg = {k: (int(v) if k == "normalize_advantage" else float(np.float32(v))) for k, v in pr.config(ent_coef=0.01, lr=1e-2).items()}
    env = _env(hbmod, humanoid_model, gpu)
    b, mem = env.batch, Mem(env.batch)
    b.actor_set(asz, *ac.layers(t, "actor", asz), head="gaussian", log_std=t["log_std"], seed=3, activation=activation)
    b.critic_set(csz, *ac.layers(t, "critic", csz), activation=activation)
    b.learner_create(**cfg)
    assert np.array_equal(b.learner_params(), flat.astype(np.float32))
    names = ("obs", "action", "old_log_prob", "advantage", "returns")
    masked = {k: np.full_like(rows[k], np.nan) for k in names}   # rows outside the minibatch are not read
    for k in names:
        masked[k][SEL] = rows[k][SEL]
    stats = mem.nan(16)
    b.ppo_grad_dev(*[mem.up(masked[k]) for k in names], ac.N_ROWS, MB, index=mem.up(SEL.astype(np.int32)), stats=stats)
    got = pr.split(b.learner_grads().astype(np.float64), asz, csz, NU)
    assert all(np.isfinite(g).all() for g in got.values())
    tensors = list(got)
    g64, g32 = ({k: v for k, v in ac.torch_grads(torch, *pr.torch_loss(torch, dt, flat, asz, csz, rows, cfg, SEL, activation, activation)[:2], tensors).items()}
                for dt in (torch.float64, torch.float32))
    worst = 0.0
    for group in ("actor", "critic"):   # (log_std goes with the actor)
        ks = [k for k in tensors if k.startswith(group) or (group == "actor" and k == "log_std")]
        kk = 8.0 * max(float(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max()) for k in ks)
        for k in ks:
            r = float(np.abs(got[k] - g64[k]).max() / np.abs(g64[k]).max())
            worst = max(worst, r / kk)
            assert r <= kk, (activation, net, k, r, kk)
    # one Adam step moves the parameters the next collection reads
    b.ppo_adam_dev()
    new = b.learner_params().astype(np.float64)
    assert np.abs(new - flat).max() > 1e-3
    tn = pr.split(new, asz, csz, NU)
    tapes, _ = _collect(b, mem, _obs0(61))
    acts, mu, _ = ml.forward(tn, "actor", len(asz) - 1, tapes["obs"][0], activation)
    r_mean = _ratio(np.abs(tapes["mean"][0] - mu), ml.fwd_err(tn, "actor", len(asz) - 1, acts, activation)[0])
    _, mu_old, _ = ml.forward(t, "actor", len(asz) - 1, tapes["obs"][0], activation)
    assert r_mean <= 1.0 and np.abs(mu - mu_old).max() > 1e-3, r_mean
    mem.free()
    env.close()
    _report("act ppo gradients %-4s %-6s: worst tensor measured / k %.3f; the mean behind an Adam step %.3f of its forward bound" % (activation, net, worst, r_mean))


# ---- 3. and 4. SAC: one hb_sac_step_dev with recorded draws, the collection behind it, and a second step's targets

def _sac_env(hbmod, m, gpu, net, pb, act_actor, act_q, **cfg):
    asz, qsz = ac.sac_sizes(net)
    t = sr.split(pb["flat"].astype(np.float32), asz, qsz)
    env = _env(hbmod, m, gpu)
    b = env.batch
    b.actor_set(asz, *ac.layers(t, "actor", asz), head="squashed", seed=3, activation=act_actor)
    b.q_set(0, qsz, *ac.layers(t, "q1", qsz), activation=act_q)
    b.q_set(1, qsz, *ac.layers(t, "q2", qsz), activation=act_q)
    b.sac_create(**cfg)
    st = b.sac_state()
    st["params"], st["targets"] = pb["flat"].astype(np.float32), pb["targets"].astype(np.float32)
    b.sac_set_state(st)
    return env


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("activation", ACTS)
def test_sac_step_gradients_and_targets(hbmod, humanoid_model, gpu, activation, net):
    torch = pytest.importorskip("torch")
    asz, qsz = ac.sac_sizes(net)
    lo, hi = sr.q_range(asz, qsz)
    pb = ac.sac_problem(torch, net, activation, activation, ac.SAC_SEEDS[(net, activation)])
    cfg = ac.sac_cfg()
    rows, ep, en = pb["rows"], pb["eps_pi"][SEL], pb["eps_next"][SEL]
    env = _sac_env(hbmod, humanoid_model, gpu, net, pb, activation, activation, **cfg)
    b, mem = env.batch, Mem(env.batch)
    names = ("obs", "action", "reward", "next_obs", "done")
    masked = {k: (np.full_like(rows[k], np.nan) if k != "done" else np.full_like(rows[k], 1)) for k in names}
    for k in names:
        masked[k][SEL] = rows[k][SEL]
    ptr = [mem.up(masked[k]) for k in names]
    index, pe, pn, stats = mem.up(SEL.astype(np.int32)), mem.up(ep), mem.up(en), mem.nan(16)

    def step():
        b.sac_step_dev(*ptr, ac.N_ROWS, MB, index=index, eps_pi=pe, eps_next=pn, eps_given=True, stats=stats)
        return b.from_dev(stats, (16,))
    s0 = _state64(b)
    st = step()
    s1, got = _state64(b), sr.split(b.sac_grads().astype(np.float64), asz, qsz)
    assert np.isfinite(st).all() and s1["t"] == 1 and all(np.isfinite(g).all() for g in got.values())
    mid = s0["params"].copy()
    mid[lo:] = s1["params"][lo:]
    # the inputs' conditions at what the device's own critic step left (test_act_cpu.py: at the reference's)
    cond = ac.sac_conditions(net, mid, rows, SEL, ep, activation, activation)
    assert min(cond[k] for k in ("actor", "log_std", "q1_pi", "q2_pi", "q1_q2")) >= ac.MARGIN, cond
    alpha = float(np.float32(np.exp(s0["params"][-1])))
    cnames = [k for k in got if not k.startswith("actor")]
    anames = [k for k in got if k.startswith("actor")]
    ref, floor = {}, {}
    for dt, dst in ((torch.float64, ref), (torch.float32, floor)):
        lc = sr.torch_losses(torch, dt, s0["params"], s0["targets"], asz, qsz, rows, SEL, ep, en, cfg, act_actor=activation, act_q=activation)
        dst.update(ac.torch_grads(torch, lc[0] + lc[1], lc[3], cnames))
        la = sr.torch_losses(torch, dt, mid, s0["targets"], asz, qsz, rows, SEL, ep, en, cfg, alpha=alpha, act_actor=activation, act_q=activation)
        dst.update(ac.torch_grads(torch, la[2], la[3], anames))
    worst = 0.0
    for ks in (cnames, anames):
        kk = 8.0 * max(float(np.abs(floor[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in ks)
        for k in ks:
            r = float(np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max())
            worst = max(worst, r / kk)
            assert r <= kk, (activation, net, k, r, kk)
    # the step moved every group, and the next collection runs the updated actor
    assert all(np.abs(s1["params"][a:z] - s0["params"][a:z]).max() > 1e-4 for a, z in ((0, lo), (lo, hi)))
    assert not np.array_equal(s1["targets"], s0["targets"])
    t1 = sr.split(s1["params"], asz, qsz)
    tapes, _ = _collect(b, mem, _obs0(71), log_std=True)
    acts, out, _ = ml.forward(t1, "actor", len(asz) - 1, tapes["obs"][0], activation)
    e = ml.fwd_err(t1, "actor", len(asz) - 1, acts, activation)[0]
    r_act = max(_ratio(np.abs(tapes["mean"][0] - out[:, :NU]), e[:, :NU]), _ratio(np.abs(tapes["log_std"][0] - np.clip(out[:, NU:], -20.0, 2.0)), e[:, NU:]))
    assert r_act <= 1.0, r_act
    # a second step: its y comes from the targets the Polyak step left, on the Q networks' activation.  One row, so that y is not an
    # average: the row of the minibatch where targets that ran tanh instead would stand furthest outside the bound (chosen from the
    # references alone)
    y, dy = ac.sac_target(net, s1["params"], s1["targets"], rows, SEL, en, cfg, activation, activation)
    y_tanh = ac.sac_target(net, s1["params"], s1["targets"], rows, SEL, en, cfg, activation, "tanh")[0]
    b_y = dy + U * np.abs(y)
    i = int(np.argmax(np.abs(y - y_tanh) / b_y))
    r_tanh = float(np.abs(y - y_tanh)[i] / b_y[i])
    assert r_tanh > 2.0, r_tanh
    b.sac_step_dev(*ptr, ac.N_ROWS, 1, first=int(SEL[i]), eps_pi=mem.up(ep[i:i + 1]), eps_next=mem.up(en[i:i + 1]), eps_given=True, stats=stats)
    y_dev = float(b.from_dev(stats, (16,))[sr.STATS.index("y")])
    r_y = abs(y_dev - y[i]) / b_y[i]
    assert r_y <= 1.0, (r_y, y_dev, y[i], y_tanh[i])
    mem.free()
    env.close()
    _report("act sac step %-4s %-6s: worst tensor measured / k %.3f; the actor behind the step %.3f, a second step's y %.3f of their bounds (the same row through tanh targets: %.1f)"
            % (activation, net, worst, r_act, r_y, r_tanh))


# ---- 5. the rules of the interface

def test_interface_rules(hbmod, humanoid_model, gpu):
    import humanoid_mujoco_amd.engine as eng
    net = "h20_72"
    asz, csz = ac.ppo_sizes(net)
    sasz, qsz = ac.sac_sizes(net)
    t = {**_net("actor", asz, 81), **_net("critic", csz, 82), **_net("sq", sasz, 83), **_net("q1", qsz, 84), **_net("q2", qsz, 85), **_net("p", asz, 86)}
    L = hbmod.lib()
    b = hbmod.Batch(humanoid_model, N, gpu)
    # nothing installed: every net is refused, by the getter too
    for k in range(5):
        assert L.hb_mlp_set_activation(b._h, k, eng.ACT_RELU) == -1 and L.hb_mlp_get_activation(b._h, k) == -1
    b.set_policy_mlp(*ac.layers(t, "p", asz))
    b.actor_set(asz, *ac.layers(t, "actor", asz), head="gaussian", log_std=np.zeros(NU, np.float32), seed=3)
    b.critic_set(csz, *ac.layers(t, "critic", csz))
    assert [b.mlp_activation(k) for k in ("policy", "actor", "critic")] == ["tanh"] * 3
    assert L.hb_mlp_get_activation(b._h, eng.NET_Q1) == -1 and L.hb_mlp_set_activation(b._h, eng.NET_Q2, eng.ACT_ELU) == -1
    for bad in ((5, 0), (-1, 0), (eng.NET_ACTOR, 3), (eng.NET_ACTOR, -1)):
        assert L.hb_mlp_set_activation(b._h, *bad) == -1
    assert b.mlp_activation("actor") == "tanh"                       # a refused call changes nothing
    for k, a in (("policy", "elu"), ("actor", "relu"), ("critic", "elu")):
        b.mlp_set_activation(k, a)
        assert b.mlp_activation(k) == a
    b.set_policy_mlp(*ac.layers(t, "p", asz))                         # set_mlp installs tanh again
    b.critic_set(csz, *ac.layers(t, "critic", csz))
    assert [b.mlp_activation(k) for k in ("policy", "actor", "critic")] == ["tanh", "relu", "tanh"]
    # the PPO learner: the value in force keeps it, another one on the actor or the critic destroys it
    for which, a in (("actor", "elu"), ("critic", "relu")):
        b.learner_create()
        b.mlp_set_activation(which, b.mlp_activation(which))
        b.mlp_set_activation("policy", "relu")                        # (not the learner's network)
        assert b.learner_param_count() > 0
        b.mlp_set_activation(which, a)
        with pytest.raises(hbmod.HbError):
            b.learner_param_count()
    # the SAC learner: Q1 and Q2 must agree, the actor may differ; a change on the actor, Q1 or Q2 destroys it
    b.actor_set(sasz, *ac.layers(t, "sq", sasz), head="squashed", seed=3, activation="relu")
    b.q_set(0, qsz, *ac.layers(t, "q1", qsz), activation="elu")
    b.q_set(1, qsz, *ac.layers(t, "q2", qsz))
    with pytest.raises(hbmod.HbError):
        b.sac_create()
    for which, a in (("actor", "tanh"), ("q1", "relu"), ("q2", "relu")):
        b.mlp_set_activation("q1", "elu")
        b.mlp_set_activation("q2", "elu")
        b.sac_create()
        b.mlp_set_activation(which, b.mlp_activation(which))
        b.mlp_set_activation("critic", "elu")                         # (not the learner's network)
        assert b.sac_param_count() > 0
        b.mlp_set_activation(which, a)
        with pytest.raises(hbmod.HbError):
            b.sac_param_count()
    b.close()


def test_the_draw_counter_survives_a_change(hbmod, humanoid_model, gpu):
    """two envs of one seed collect a step, one of them changes the actor's activation and back, both collect again: the same draws,
    which are not the first step's (actor_set would have set the counter back)"""
    asz = ac.ppo_sizes("h20_72")[0]
    t = _net("actor", asz, 91)
    eps = []
    for change in (False, True):
        env = _env(hbmod, humanoid_model, gpu)
        b, mem = env.batch, Mem(env.batch)
        b.actor_set(asz, *ac.layers(t, "actor", asz), head="gaussian", log_std=np.zeros(NU, np.float32), seed=3, activation="relu")
        first, _ = _collect(b, mem, _obs0(92))
        if change:
            b.mlp_set_activation("actor", "elu")
            b.mlp_set_activation("actor", "relu")
        second, _ = _collect(b, mem, _obs0(92))
        eps.append((first["eps"], second["eps"], second["mean"]))
        mem.free()
        env.close()
    assert np.array_equal(eps[0][0], eps[1][0]) and np.array_equal(eps[0][1], eps[1][1]) and np.array_equal(eps[0][2], eps[1][2])
    assert np.abs(eps[0][1]).max() > 0 and not np.array_equal(eps[0][0], eps[0][1])


# ---- 6. tanh is untouched

def test_tanh_set_explicitly_equals_tanh_never_set(hbmod, humanoid_model, gpu):
    torch = pytest.importorskip("torch")
    net = "h20_72"
    asz, csz = ac.ppo_sizes(net)
    sasz, qsz = ac.sac_sizes(net)
    flat, rows = ac.ppo_problem(net, "tanh", "tanh", 1)
    tp = pr.split(flat.astype(np.float32), asz, csz, NU)
    pb = ac.sac_problem(torch, net, "tanh", "tanh", 1)
    outs = []
    for explicit in (False, True):
        def chosen(b, *nets):
            if explicit:
                for k in nets:
                    b.mlp_set_activation(k, "tanh")
        got = {}
        env = _env(hbmod, humanoid_model, gpu)
        b, mem = env.batch, Mem(env.batch)
        b.set_policy_mlp(*ac.layers(tp, "actor", asz))
        chosen(b, "policy")
        got["policy_eval"] = b.policy_eval()
        b.actor_set(asz, *ac.layers(tp, "actor", asz), head="gaussian", log_std=tp["log_std"], seed=3)
        b.critic_set(csz, *ac.layers(tp, "critic", csz))
        chosen(b, "actor", "critic")
        tapes, ptr = _collect(b, mem, _obs0(95), T=4)
        got.update({"tape." + k: v for k, v in tapes.items()})
        pv, pa, pr_ = mem.nan((5, N)), mem.nan((4, N)), mem.nan((4, N))
        term = mem.up(np.zeros((4, N), np.uint8))
        b.collect_gae_dev(4, 0.99, 0.95, False, obs=ptr["obs"], reward=ptr["reward"], terminated=term, truncated=term, value=pv, advantage=pa, returns=pr_)
        got["value"], got["advantage"], got["returns"] = b.from_dev(pv, (5, N)), b.from_dev(pa, (4, N)), b.from_dev(pr_, (4, N))
        b.learner_create()
        names = ("obs", "action", "old_log_prob", "advantage", "returns")
        b.ppo_grad_dev(*[mem.up(rows[k]) for k in names], ac.N_ROWS, MB, index=mem.up(SEL.astype(np.int32)))
        got["ppo_grads"] = b.learner_grads()
        mem.free()
        env.close()
        env = _sac_env(hbmod, humanoid_model, gpu, net, pb, "tanh", "tanh", **ac.sac_cfg())
        b, mem = env.batch, Mem(env.batch)
        if explicit:
            chosen(b, "actor", "q1", "q2")
            assert b.sac_param_count() > 0                            # (the value in force: the learner stays)
        snames = ("obs", "action", "reward", "next_obs", "done")
        b.sac_step_dev(*[mem.up(pb["rows"][k]) for k in snames], ac.N_ROWS, MB, index=mem.up(SEL.astype(np.int32)), eps_pi=mem.up(pb["eps_pi"][SEL]),
                       eps_next=mem.up(pb["eps_next"][SEL]), eps_given=True)
        got["sac_params"] = b.sac_params()
        mem.free()
        env.close()
        outs.append(got)
    assert set(outs[0]) == set(outs[1])
    for k in outs[0]:
        assert np.isfinite(outs[0][k]).all() and np.abs(outs[0][k]).max() > 0, k
        assert np.array_equal(outs[0][k], outs[1][k]), k
