#!/usr/bin/env python3
"""What the on-device SAC learner (include/hb.h: hb_sac_step_dev; VecEnv.sac_update) costs against the same loop written in torch on the
same GPU: 1024 envs of the 27-dof model, the 48-256-256-42 squashed actor and two 69-256-256-1 Q networks, a replay buffer filled by one
collect_torch(16, terminal_obs=True) and trained on by both, 64 gradient steps at batch_size 256 (stable-baselines3's default) and at 4096.
  (dev)   env.sac_update(replay, 64, batch_size): sixteen launches per gradient step on the batch's stream, the statistics read once at
          the end; the next collection runs the trained actor as it is
  (torch) torch.nn.Linear networks with the matching activation module, autograd, three torch.optim.Adam, the Polyak step, over minibatches drawn the same way, then the
          ONE thing the torch loop owes the next collection: the actor's parameters to the host and actor_set - on a second VecEnv of
          the same size that has NO learner, which is what a torch-only user runs
Both are timed on the host clock around a device synchronisation (launch overhead is part of what is compared), alternated in one process,
three rounds after a warm-up round; printed: medians with minimum and maximum, the time per gradient step and the spread of the per-round
ratio.  Every configuration runs in a child process of its own under its own time limit, and the first one that fails ends the run.
usage: gpu_sac_bench.py [--reps N] [--activation tanh|relu|elu] [--out FILE]     (results: profiles/sac_bench.txt)"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--activation", choices=("tanh", "relu", "elu"), default="tanh", help="hidden activation of every network, both sides")
ap.add_argument("--child", type=int, default=None, metavar="BATCH")
args = ap.parse_args()
N, T, STEPS, ACTOR, QNET = 1024, 16, 64, [48, 256, 256, 42], [69, 256, 256, 1]

if args.child is None:
    lines = []
    for mb in (256, 4096):
        limit = 240
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(mb), "--reps", str(args.reps), "--activation", args.activation], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit("gpu_sac_bench: batch %d ran into its time limit of %d s - nothing more is started" % (mb, limit))
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            sys.exit("gpu_sac_bench: batch %d failed with status %d - nothing more is started" % (mb, r.returncode))
        lines += r.stdout.splitlines()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402

MB = args.child
if not torch.cuda.is_available():
    sys.exit("gpu_sac_bench: no GPU visible - nothing is measured without one")
dev = torch.device("cuda", 0)
model = hb.Model.load(os.path.join(ROOT, "humanoid_mujoco_amd", "assets", "humanoid27.hbm"))
rng = np.random.default_rng(0)
NU = model.nu


def mlp(sizes):
    ws = [rng.uniform(-1, 1, size=(a, c)).astype(np.float32) / np.sqrt(a) for a, c in zip(sizes[:-1], sizes[1:])]
    bs = [rng.uniform(-1, 1, size=c).astype(np.float32) / np.sqrt(a) for a, c in zip(sizes[:-1], sizes[1:])]
    return ws, bs


def torch_net(ws, bs):
    layers = []
    for l, (w, b) in enumerate(zip(ws, bs)):
        lin = torch.nn.Linear(w.shape[0], w.shape[1])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w.T.copy()))
            lin.bias.copy_(torch.from_numpy(b))
        layers.append(lin)
        if l + 1 < len(ws):
            layers.append({"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU, "elu": torch.nn.ELU}[args.activation]())
    return torch.nn.Sequential(*layers).to(dev)


aw, ab = mlp(ACTOR)
qw, qb = zip(mlp(QNET), mlp(QNET))
env = hb.VecEnv(model, N, 0, seed=1, reward_kind=1, max_time=0.1)
env.actor_set(ACTOR, aw, ab, head="squashed", seed=1, activation=args.activation)
for k in range(2):
    env.q_set(k, QNET, qw[k], qb[k], activation=args.activation)
env.sac_learner()
env.reset()
plain = hb.VecEnv(model, N, 0, seed=1, reward_kind=1, max_time=0.1)   # the torch learner's env: no device learner behind actor_set
plain.actor_set(ACTOR, aw, ab, head="squashed", seed=1, activation=args.activation)
replay = hb.ReplayBuffer(N * T, model.nobs, NU, dev)
replay.add(env.collect_torch(T, terminal_obs=True))

actor = torch_net(aw, ab)
qs = [torch_net(qw[k], qb[k]) for k in range(2)]
qts = [torch_net(qw[k], qb[k]) for k in range(2)]
log_ent = torch.nn.Parameter(torch.zeros(1, device=dev))
opt_a = torch.optim.Adam(actor.parameters(), lr=3e-4)
opt_q = torch.optim.Adam([p for q in qs for p in q.parameters()], lr=3e-4)
opt_e = torch.optim.Adam([log_ent], lr=3e-4)
LOG2, HALF_LOG_2PI = float(np.log(2.0)), float(0.5 * np.log(2 * np.pi))


def sample(o):
    out = actor(o)
    mean, ls = out[:, :NU], torch.clamp(out[:, NU:], -20.0, 2.0)
    eps = torch.randn_like(mean)
    x = mean + ls.exp() * eps
    lp = (-0.5 * eps ** 2 - ls - HALF_LOG_2PI).sum(1) - (2.0 * (LOG2 - x - torch.nn.functional.softplus(-2.0 * x))).sum(1)
    return torch.tanh(x), lp


def torch_update():
    """SAC.train of stable-baselines3 on the ring, and the weight round trip a torch learner owes the next collection"""
    for _ in range(STEPS):
        idx = torch.randint(0, replay.size, (MB,), device=dev)
        o, a, r, o2, d = replay.obs[idx], replay.action[idx], replay.reward[idx], replay.next_obs[idx], replay.done[idx].float()
        a_pi, lp = sample(o)
        alpha = log_ent.exp().detach()
        ent_loss = -(log_ent * (lp.detach() - NU)).mean()
        opt_e.zero_grad(set_to_none=True)
        ent_loss.backward()
        opt_e.step()
        with torch.no_grad():
            a2, lp2 = sample(o2)
            x2 = torch.cat([o2, a2], 1)
            y = r + (1 - d) * 0.99 * (torch.min(qts[0](x2), qts[1](x2)).squeeze(-1) - alpha * lp2)
        x = torch.cat([o, a], 1)
        critic_loss = 0.5 * sum(torch.nn.functional.mse_loss(q(x).squeeze(-1), y) for q in qs)
        opt_q.zero_grad(set_to_none=True)
        critic_loss.backward()
        opt_q.step()
        xp = torch.cat([o, a_pi], 1)
        actor_loss = (alpha * lp - torch.min(qs[0](xp), qs[1](xp)).squeeze(-1)).mean()
        opt_a.zero_grad(set_to_none=True)
        actor_loss.backward()
        opt_a.step()
        with torch.no_grad():
            for q, qt in zip(qs, qts):
                for p, pt in zip(q.parameters(), qt.parameters()):
                    pt.mul_(1 - 0.005).add_(p, alpha=0.005)
    with torch.no_grad():
        lin = [m for m in actor if isinstance(m, torch.nn.Linear)]
        plain.actor_set(ACTOR, [m.weight.T.cpu().numpy() for m in lin], [m.bias.cpu().numpy() for m in lin], head="squashed", seed=1, activation=args.activation)


def timed(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0)


ms = {"dev": [], "torch": []}
for rep in range(args.reps + 1):  # (the first round warms both up and is not counted)
    td = timed(lambda: env.sac_update(replay, STEPS, batch_size=MB))
    tt = timed(torch_update)
    if rep:
        ms["dev"].append(td)
        ms["torch"].append(tt)
ratio = np.array(ms["torch"]) / np.array(ms["dev"])
print(("%s, ring of %d rows, actor %s, Q networks %s, " + args.activation + " hidden layers, batch_size %d, %d gradient steps, %d rounds after a warm-up round [host clock around a device synchronisation]") % (
    env.batch.device_name(), replay.size, "-".join(map(str, ACTOR)), "-".join(map(str, QNET)), MB, STEPS, args.reps))
for k, name in (("dev", "sac_update (device learner)"), ("torch", "torch learner + actor_set")):
    print("  %-32s median %10.2f ms (min %10.2f max %10.2f), %8.1f us per gradient step" % (name, float(np.median(ms[k])), min(ms[k]), max(ms[k]),
                                                                                            1e3 * float(np.median(ms[k])) / STEPS))
print("  torch / device per round: median %.2f (min %.2f max %.2f)%s" % (float(np.median(ratio)), ratio.min(), ratio.max(),
                                                                          "" if ratio.min() > 1.0 else "  - THE DEVICE LEARNER IS NOT FASTER IN EVERY ROUND"))
env.close()
plain.close()
