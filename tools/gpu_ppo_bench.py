#!/usr/bin/env python3
"""What the on-device PPO learner (include/hb.h: hb_ppo_minibatch_dev; VecEnv.ppo_update) costs against the same loop written in torch on the
same GPU: 4096 envs of the 27-dof model, T = 32 (131 072 rows), the 48-256-256-21 Gaussian actor and a 48-256-256-1 critic, one buffer
collected with collect_torch(T, gae=...) and trained on by both.  Minibatches of 64 (stable-baselines3's default), 4096 and 32 768 rows,
one epoch and ten (at 64 rows the torch loop of ten epochs is 20 480 steps: only one epoch is measured there unless --full).
  (dev)   env.ppo_update(buf, n_epochs, batch_size): seven launches per minibatch on the batch's stream, the statistics read once at the end;
          the next collection runs the trained networks as they are
  (torch) torch.nn.Linear networks with the matching activation module, autograd, clip_grad_norm_ and torch.optim.Adam over the same rows in the same minibatch scheme
          (one randperm per epoch), then what the torch learner needs before the next collection: the parameters to the host and
          actor_set / critic_set - on a second VecEnv of the same size that has NO learner, which is what a torch-only user runs
Both are timed on the host clock around a device synchronisation (launch overhead is part of what is compared), alternated in one process
after a warm-up round; printed: medians with minimum and maximum and the spread of the per-round ratio.  Every configuration runs in a child
process of its own under its own time limit, and the first one that fails ends the run.
usage: gpu_ppo_bench.py [--reps N] [--full] [--activation tanh|relu|elu] [--out FILE]     (results: profiles/ppo_bench.txt)"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--full", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--activation", choices=("tanh", "relu", "elu"), default="tanh", help="hidden activation of actor and critic, both sides")
ap.add_argument("--child", nargs=2, type=int, default=None, metavar=("BATCH", "EPOCHS"))
args = ap.parse_args()
N, T, ACTOR, CRITIC = 4096, 32, [48, 256, 256, 21], [48, 256, 256, 1]

if args.child is None:
    configs = [(64, 1), (4096, 1), (4096, 10), (32768, 1), (32768, 10)] + ([(64, 10)] if args.full else [])
    lines = []
    for mb, ep in configs:
        limit = 900 if mb == 64 else 300
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(mb), str(ep), "--reps", str(args.reps if mb > 64 else min(args.reps, 3)), "--activation", args.activation],
                               capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit("gpu_ppo_bench: batch %d, %d epoch(s) ran into its time limit of %d s - nothing more is started" % (mb, ep, limit))
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            sys.exit("gpu_ppo_bench: batch %d, %d epoch(s) failed with status %d - nothing more is started" % (mb, ep, r.returncode))
        lines += [l for l in r.stdout.splitlines() if not (lines and l.startswith("AMD") and l in lines)]
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402

MB, EPOCHS = args.child
if not torch.cuda.is_available():
    sys.exit("gpu_ppo_bench: no GPU visible - nothing is measured without one")
dev = torch.device("cuda", 0)
model = hb.Model.load(os.path.join(ROOT, "humanoid_mujoco_amd", "assets", "humanoid27.hbm"))
rng = np.random.default_rng(0)


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
cw, cb = mlp(CRITIC)
log_std0 = np.full(ACTOR[-1], -1.0, np.float32)
env = hb.VecEnv(model, N, 0, seed=1, reward_kind=1, max_time=0.1)
env.actor_set(ACTOR, aw, ab, head="gaussian", log_std=log_std0, seed=1, activation=args.activation)
env.critic_set(CRITIC, cw, cb, activation=args.activation)
env.learner()
env.reset()
plain = hb.VecEnv(model, N, 0, seed=1, reward_kind=1, max_time=0.1)   # the torch learner's env: no device learner behind actor_set / critic_set
plain.actor_set(ACTOR, aw, ab, head="gaussian", log_std=log_std0, seed=1, activation=args.activation)
plain.critic_set(CRITIC, cw, cb, activation=args.activation)
buf = env.collect_torch(T, gae=dict(gamma=0.99, lam=0.95))
R = N * T
obs, action = buf["obs"][:T].reshape(R, -1), buf["action"].reshape(R, -1)
old_lp, adv, ret = (buf[k].reshape(R) for k in ("log_prob", "advantage", "returns"))

actor, critic = torch_net(aw, ab), torch_net(cw, cb)
log_std = torch.nn.Parameter(torch.from_numpy(log_std0).to(dev))
params = list(actor.parameters()) + [log_std] + list(critic.parameters())
opt = torch.optim.Adam(params, lr=3e-4, eps=1e-5)


def torch_update():
    """PPO.train of stable-baselines3 on the buffer, and the weight round trip a torch learner owes the next collection"""
    for _ in range(EPOCHS):
        perm = torch.randperm(R, device=dev)
        for s0 in range(0, R, MB):
            idx = perm[s0:s0 + MB]
            a = adv[idx]
            if len(idx) > 1:
                a = (a - a.mean()) / (a.std() + 1e-8)
            o = obs[idx]
            dist = torch.distributions.Normal(actor(o), log_std.exp())
            ratio = torch.exp(dist.log_prob(action[idx]).sum(-1) - old_lp[idx])
            policy_loss = -torch.min(a * ratio, a * torch.clamp(ratio, 0.8, 1.2)).mean()
            value_loss = torch.nn.functional.mse_loss(ret[idx], critic(o).squeeze(-1))
            loss = policy_loss + 0.5 * value_loss
            opt.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, 0.5)
            opt.step()
    with torch.no_grad():
        lin = [m for m in actor if isinstance(m, torch.nn.Linear)]
        plain.actor_set(ACTOR, [m.weight.T.cpu().numpy() for m in lin], [m.bias.cpu().numpy() for m in lin], head="gaussian", log_std=log_std.cpu().numpy(), seed=1,
                        activation=args.activation)
        lin = [m for m in critic if isinstance(m, torch.nn.Linear)]
        plain.critic_set(CRITIC, [m.weight.T.cpu().numpy() for m in lin], [m.bias.cpu().numpy() for m in lin], activation=args.activation)


def timed(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0)


ms = {"dev": [], "torch": []}
for rep in range(args.reps + 1):  # (the first round warms both up and is not counted)
    td = timed(lambda: env.ppo_update(buf, n_epochs=EPOCHS, batch_size=MB))
    tt = timed(torch_update)
    if rep:
        ms["dev"].append(td)
        ms["torch"].append(tt)
steps = EPOCHS * ((R + MB - 1) // MB)
ratio = np.array(ms["torch"]) / np.array(ms["dev"])
print("%s, %d rows, actor %s critic %s, minibatch %d, %d epoch(s) = %d steps, %d rounds after a warm-up round [host clock around a device synchronisation]" % (
    env.batch.device_name(), R, "-".join(map(str, ACTOR)), "-".join(map(str, CRITIC)), MB, EPOCHS, steps, args.reps))
for k, name in (("dev", "ppo_update (device learner)"), ("torch", "torch learner + actor_set / critic_set")):
    print("  %-40s median %10.2f ms (min %10.2f max %10.2f), %8.1f us per minibatch" % (name, float(np.median(ms[k])), min(ms[k]), max(ms[k]),
                                                                                           1e3 * float(np.median(ms[k])) / steps))
print("  torch / device per round: median %.2f (min %.2f max %.2f)%s" % (float(np.median(ratio)), ratio.min(), ratio.max(),
                                                                          "" if ratio.min() > 1.0 else "  - THE DEVICE LEARNER IS NOT FASTER IN EVERY ROUND"))
env.close()
plain.close()
