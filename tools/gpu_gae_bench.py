#!/usr/bin/env python3
"""What the on-device PPO buffer (include/hb.h: hb_collect_gae_dev; VecEnv.collect_torch(T, gae=...)) costs beside the collection it follows,
and what the same quantities cost in torch: 4096 envs of the 27-dof model, T = 32, the 48-256-256-21 Gaussian actor and a 48-256-256-1 critic,
reward_kind 1 with a 0.1 s time limit (every env is truncated - and bootstrapped - once or twice inside the window).  Three variants, alternated
in one process after a warm-up round, REPS windows each, every window from a fresh reset and timed with device events on the caller's stream:
  (i)   collect_torch(T, terminal_obs=True)                      the collection alone
  (ii)  collect_torch(T, gae=dict(gamma, lam))                   the collection and hb_collect_gae_dev behind it on the batch's stream
  (iii) (i), then the same quantities in torch on the same tapes: a torch.nn.Linear critic over obs, its values of terminal_obs[boot] (a masked
        gather) folded into the reward, Normal(mean, std).log_prob(action).sum(-1), and the reverse loop of T steps
Printed: the medians with minimum and maximum, the per-round differences (ii) - (i) and (iii) - (i) with their spread (maximum - minimum over
the rounds), and whether the median of (ii) - (i) lies below the median of (iii) - (i) by more than the larger of the two spreads; if not, the
tool says so.  The two computations are compared once (largest differences) so that the torch variant is known to compute the same thing.
usage: gpu_gae_bench.py [--reps N] [--out FILE]     (results: profiles/gae_bench.txt)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default=None)
ap.add_argument("--activation", choices=("tanh", "relu", "elu"), default="tanh", help="hidden activation of actor and critic, both sides")
args = ap.parse_args()
N, T, ACTOR, CRITIC = 4096, 32, [48, 256, 256, 21], [48, 256, 256, 1]
GAMMA, LAM = 0.99, 0.95
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


if not torch.cuda.is_available():
    sys.exit("gpu_gae_bench: no GPU visible - nothing is measured without one")
dev = torch.device("cuda", 0)
model = hb.Model.load(os.path.join(ROOT, "humanoid_mujoco_amd", "assets", "humanoid27.hbm"))
rng = np.random.default_rng(0)


def mlp(sizes):
    ws = [rng.uniform(-1, 1, size=(a, c)).astype(np.float32) / np.sqrt(a) for a, c in zip(sizes[:-1], sizes[1:])]
    bs = [rng.uniform(-1, 1, size=c).astype(np.float32) / np.sqrt(a) for a, c in zip(sizes[:-1], sizes[1:])]
    return ws, bs


aw, ab = mlp(ACTOR)
cw, cb = mlp(CRITIC)
log_std = np.full(ACTOR[-1], -1.0, np.float32)
layers = []
for l, (w, b) in enumerate(zip(cw, cb)):
    lin = torch.nn.Linear(w.shape[0], w.shape[1])
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(w.T.copy()))
        lin.bias.copy_(torch.from_numpy(b))
    layers.append(lin)
    if l + 1 < len(cw):
        layers.append({"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU, "elu": torch.nn.ELU}[args.activation]())
critic = torch.nn.Sequential(*layers).to(dev)
std = torch.from_numpy(np.exp(log_std)).to(dev)

env = hb.VecEnv(model, N, 0, seed=1, reward_kind=1, max_time=0.1)
env.actor_set(ACTOR, aw, ab, head="gaussian", log_std=log_std, seed=1, activation=args.activation)
env.critic_set(CRITIC, cw, cb, activation=args.activation)
say(("%s, %d envs, T = %d, actor %s (Gaussian head), critic %s, " + args.activation + " hidden layers, gamma %.2f lam %.2f, %d windows per variant after one warm-up round [%s]") % (
    env.batch.device_name(), N, T, "-".join(map(str, ACTOR)), "-".join(map(str, CRITIC)), GAMMA, LAM, args.reps, "device events"))


def torch_buffer(t):
    """the quantities of hb_collect_gae_dev in torch, as a training script would write them"""
    with torch.no_grad():
        value = critic(t["obs"]).squeeze(-1)
        te, tr = t["terminated"], t["truncated"]
        boot = tr & ~te
        reward = t["reward"].clone()
        reward[boot] += GAMMA * critic(t["terminal_obs"][boot]).squeeze(-1)
        log_prob = torch.distributions.Normal(t["mean"], std).log_prob(t["action"]).sum(-1)
        nt = 1.0 - (te | tr).float()
        adv = torch.empty_like(reward)
        last = torch.zeros_like(reward[0])
        for k in range(T - 1, -1, -1):
            delta = reward[k] + GAMMA * nt[k] * value[k + 1] - value[k]
            last = delta + GAMMA * LAM * nt[k] * last
            adv[k] = last
        return {"value": value, "log_prob": log_prob, "advantage": adv, "returns": adv + value[:-1]}


def window(variant):
    obs = torch.from_numpy(env.reset()).to(dev)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    if variant == "ii":
        out = env.collect_torch(T, obs0=obs, gae=dict(gamma=GAMMA, lam=LAM))
    else:
        out = env.collect_torch(T, obs0=obs, terminal_obs=True)
        if variant == "iii":
            out = dict(out, **torch_buffer(out))
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), out


# the two computations on the tapes of one collection
_, dev_out = window("ii")
ref = torch_buffer(dev_out)
boot = dev_out["truncated"] & ~dev_out["terminated"]
say("one window: %d of %d rows end an episode, %d bootstrapped; largest |device - torch|: %s" % (
    int((dev_out["truncated"] | dev_out["terminated"]).sum()), N * T, int(boot.sum()),
    ", ".join("%s %.2e (max |.| %.1f)" % (k, float((dev_out[k] - ref[k]).abs().max()), float(ref[k].abs().max())) for k in ("value", "log_prob", "advantage", "returns"))))

ms = {v: [] for v in ("i", "ii", "iii")}
for rep in range(args.reps + 1):  # (the first round warms every variant up and is not counted)
    for v in ms:
        t, _ = window(v)
        if rep:
            ms[v].append(t)
names = {"i": "(i)   collection alone", "ii": "(ii)  collection + hb_collect_gae_dev", "iii": "(iii) collection + torch buffer"}
med = {v: float(np.median(ms[v])) for v in ms}
for v in ms:
    say("  %-40s median %8.3f ms (min %8.3f max %8.3f), %.1f us per collected step" % (names[v], med[v], min(ms[v]), max(ms[v]), 1e3 * med[v] / T))
d2 = np.array(ms["ii"]) - np.array(ms["i"])
d3 = np.array(ms["iii"]) - np.array(ms["i"])
s2, s3 = float(d2.max() - d2.min()), float(d3.max() - d3.min())
say("  (ii) - (i)  per round: median %8.3f ms, spread (max - min) %.3f ms" % (float(np.median(d2)), s2))
say("  (iii) - (i) per round: median %8.3f ms, spread (max - min) %.3f ms" % (float(np.median(d3)), s3))
gap = float(np.median(d3) - np.median(d2))
ok = gap > max(s2, s3)
say("  the device buffer is %.3f ms per window cheaper than the torch one; larger than either spread: %s" % (gap, "yes" if ok else "NO - THE REQUIREMENT IS NOT MET"))
env.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
