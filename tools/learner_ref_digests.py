#!/usr/bin/env python3
"""What the learners' fp64 references (tests/mlp_ref.py, ppo_ref.py, sac_ref.py, act_ref.py) compute on seeded problems, as one SHA-256
per array.  CPU only: numpy and torch, no library is loaded.  fp64 numpy on one machine is deterministic, so two checkouts whose
references state the same expressions print the same lines; a line that differs is a changed expression.
  ppo_ref: the networks small, one_layer, mixed and wide of tools/gpu_learner_bits.py on random_problem(..., 200, seed=1): loss_and_grads
           of rows 0 .. 99 (every statistic, the flat gradient, mu, v), adam_step from zero moments, and for small and mixed torch_loss in
           float64 with its autograd gradient
  sac_ref: the same names on random_problem(..., 200, seed=1): two consecutive steps on rows 0 .. 99 (state, statistics, the gradient
           used), the forward, action and log-probability bounds of the first step's pi, the target y with its bound dy, and for small
           and mixed torch_losses in float64 with their gradients
  act_ref: every problem of PPO_SEEDS and SAC_SEEDS (record, rows or targets, margins, conditions, sac_target) and the references'
           loss_and_grads / step on them with their ReLU and ELU activations
A checkout from before tests/mlp_ref.py existed gives the same quantities from where they stood then (_before_mlp_ref): that is how the
left column of profiles/learner_ref_digests.txt was made.
usage: learner_ref_digests.py [--out FILE] [--beside FILE]
  --beside FILE: print FILE's digests (another checkout's --out) next to this run's, and fail if a line differs"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import act_ref as ac  # noqa: E402
import ppo_ref as pr  # noqa: E402
import sac_ref as sr  # noqa: E402

WIDE_A, WIDE_V, WIDE_Q = [48, 256, 256, 256], [48, 256, 256, 256, 1], [69, 256, 256, 256, 1]
PPO_NETS = {"small": ([48, 20, 33, 21], [48, 20, 33, 1]), "one_layer": ([48, 21], [48, 1]), "mixed": ([48, 64, 21], [48, 16, 1]), "wide": (WIDE_A + [21], WIDE_V)}
SAC_NETS = {"small": ([48, 20, 33, 42], [69, 20, 33, 1]), "one_layer": ([48, 42], [69, 1]), "mixed": ([48, 64, 42], [69, 16, 1]), "wide": (WIDE_A + [42], WIDE_Q)}
NU = 21


def _before_mlp_ref():
    """the calls below as a checkout without tests/mlp_ref.py spells them: sac_ref's own tanh fwd_err, act_ref's lp_err and sac_target,
    and ppo_ref / sac_ref run on act_ref's forward and backward where an activation is asked for"""
    sizes_of = ac.sac_sizes
    ac.sac_sizes = lambda net: net if isinstance(net, tuple) else sizes_of(net)

    def on(mod, a, fn):
        keep = mod.forward, mod.backward
        mod.forward = lambda t, tag, n, x: ac.forward(t, tag, n, x, a)[:2]
        mod.backward = lambda t, tag, n, acts, dz, grads=None: ac.backward(t, tag, n, acts, dz, a, grads)
        try:
            return fn()
        finally:
            mod.forward, mod.backward = keep
    return dict(fwd_err=sr.fwd_err, lp_err=ac.lp_err,
                target=lambda flat, targets, asz, qsz, rows, sel, en, cfg: ac.sac_target((asz, qsz), flat, targets, rows, sel, en, cfg, "tanh", "tanh"),
                ppo_grads=lambda a, *args, **kw: on(pr, a, lambda: pr.loss_and_grads(*args, **kw)),
                sac_step=lambda a, *args: on(sr, a, lambda: sr.step(*args)))


try:
    import mlp_ref as ml  # noqa: E402
    API = dict(fwd_err=lambda *args: ml.fwd_err(*args)[0], lp_err=sr.lp_err, target=sr.target,
               ppo_grads=lambda a, *args, **kw: pr.loss_and_grads(*args, act_actor=a, act_critic=a, **kw),
               sac_step=lambda a, *args: sr.step(*args, act_actor=a, act_q=a))
except ImportError:
    API = _before_mlp_ref()

LINES = []


def put(name, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.size and not np.isnan(a).any(), name
    LINES.append("%-44s %7d f64  %s" % (name, a.size, hashlib.sha256(a.tobytes()).hexdigest()))
    print(LINES[-1], flush=True)


def put_all(prefix, d, keys=None):
    for k in (keys or sorted(d)):
        put("%s %s" % (prefix, k), d[k])


def ppo_ref_lines():
    for net, (asz, csz) in PPO_NETS.items():
        flat, rows = pr.random_problem(asz, csz, 200, seed=1)
        cfg = pr.config(ent_coef=0.01, lr=1e-3)
        stats, g, ex = pr.loss_and_grads(flat, asz, csz, rows, cfg, index=None, first=0, mb=100)
        put_all("ppo_ref %s stat" % net, stats)
        put_all("ppo_ref %s" % net, dict(grad=g, mu=ex["mu"], v=ex["v"]))
        p, m, v, t, gn, skipped = pr.adam_step(flat, np.zeros_like(flat), np.zeros_like(flat), 0, g, cfg)
        put_all("ppo_ref %s adam" % net, dict(p=p, m=m, v=v, t_gn_skipped=[t, gn, skipped]))
        if net in ("small", "mixed"):
            loss, leaves = pr.torch_loss(torch, torch.float64, flat, asz, csz, rows, cfg, np.arange(100))[:2]
            names = [k for k, _ in pr.flat_shapes(asz, csz, NU)]
            put_all("ppo_ref %s torch" % net, dict(loss=loss.detach().numpy(), grad=pr.join(ac.torch_grads(torch, loss, leaves, names), asz, csz, NU)))


def sac_ref_lines():
    sel = np.arange(100)
    for net, (asz, qsz) in SAC_NETS.items():
        pb = sr.random_problem(asz, qsz, 200, seed=1)
        cfg = sr.config(lr_actor=1e-3, lr_critic=1e-3, lr_ent=1e-3, ent_coef_init=0.3, tau=0.05)
        ep, en = pb["eps_pi"][sel], pb["eps_next"][sel]
        state = dict(params=pb["flat"], m=np.zeros_like(pb["flat"]), v=np.zeros_like(pb["flat"]), targets=pb["targets"], t=0)
        for k in (1, 2):
            state, stats, g = sr.step(state, asz, qsz, pb["rows"], sel, ep, en, cfg)
            put_all("sac_ref %s step%d" % (net, k), dict(state, grad=g, stats=[stats[s] for s in sr.STATS]))
        pi = sr.critic_phase(pb["flat"], pb["targets"], asz, qsz, pb["rows"], sel, ep, en, cfg)[2]["pi"]
        e_pi = API["fwd_err"](sr.split(pb["flat"], asz, qsz), "actor", len(asz) - 1, pi["acts"])
        put_all("sac_ref %s pi" % net, dict(fwd_err=e_pi, action_err=sr.action_err(pi, e_pi), lp_err=API["lp_err"](pi, e_pi)))
        y, dy = API["target"](pb["flat"], pb["targets"], asz, qsz, pb["rows"], sel, en, cfg)
        put_all("sac_ref %s target" % net, dict(y=y, dy=dy))
        if net in ("small", "mixed"):
            ent, crit, actor, leaves = sr.torch_losses(torch, torch.float64, pb["flat"], pb["targets"], asz, qsz, pb["rows"], sel, ep, en, cfg)
            names = [k for k, _ in sr.flat_shapes(asz, qsz)]
            put("sac_ref %s torch losses" % net, [float(x.detach()) for x in (ent, crit, actor)])
            put("sac_ref %s torch grad ent+critic" % net, sr.join(ac.torch_grads(torch, ent + crit, leaves, names), asz, qsz))
            put("sac_ref %s torch grad actor" % net, sr.join(ac.torch_grads(torch, actor, leaves, names), asz, qsz))


def act_ref_lines():
    for (net, a), seed in sorted(ac.PPO_SEEDS.items()):
        asz, csz = ac.ppo_sizes(net)
        flat, rows = ac.ppo_problem(net, a, a, seed)
        tag = "act_ref ppo %s %s" % (net, a)
        put_all(tag, dict(rows, flat=flat, margin=ac.ppo_margin(net, flat, {k: v[ac.SEL] for k, v in rows.items()}, a, a)))
        stats, g, _ = API["ppo_grads"](a, flat, asz, csz, rows, pr.config(ent_coef=0.01, lr=1e-2), index=ac.SEL)
        put_all(tag + " stat", stats)
        put(tag + " grad", g)
    for (net, a), seed in sorted(ac.SAC_SEEDS.items()):
        asz, qsz = ac.sac_sizes(net)
        pb = ac.sac_problem(torch, net, a, a, seed)
        tag = "act_ref sac %s %s" % (net, a)
        ep, en, cfg = pb["eps_pi"][ac.SEL], pb["eps_next"][ac.SEL], ac.sac_cfg()
        put_all(tag, dict(pb["rows"], flat=pb["flat"], targets=pb["targets"], eps_pi=pb["eps_pi"], eps_next=pb["eps_next"]))
        put_all(tag + " condition", ac.sac_conditions(net, pb["flat"], pb["rows"], ac.SEL, ep, a, a))
        y, dy = ac.sac_target(net, pb["flat"], pb["targets"], pb["rows"], ac.SEL, en, cfg, a, a)
        put_all(tag + " target", dict(y=y, dy=dy))
        state = dict(params=pb["flat"], m=np.zeros_like(pb["flat"]), v=np.zeros_like(pb["flat"]), targets=pb["targets"], t=0)
        state, stats, g = API["sac_step"](a, state, asz, qsz, pb["rows"], ac.SEL, ep, en, cfg)
        put_all(tag + " step", dict(state, grad=g, stats=[stats[s] for s in sr.STATS]))


ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--beside", default=None)
args = ap.parse_args()
ppo_ref_lines()
sac_ref_lines()
act_ref_lines()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
if args.beside:
    with open(args.beside) as f:
        other = f.read().splitlines()
    differ = len(other) != len(LINES)
    print("\n%-58s %-64s  %-64s" % ("array", args.beside, "this checkout"))
    for a, b in zip(other, LINES):
        differ |= a != b
        print("%-58s %s  %s  %s" % (b[:-64].rstrip(), a.split()[-1], b.split()[-1], "equal" if a == b else "DIFFERS"))
    print("%d arrays, %s" % (len(LINES), "a line DIFFERS" if differ else "every line equal"))
    sys.exit(1 if differ else 0)
