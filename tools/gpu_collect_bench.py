#!/usr/bin/env python3
"""What on-device rollout collection (include/hb.h: hb_env_collect_dev; VecEnv.collect_torch) buys a training loop: 4096 envs of the 27-dof
model, 64 env steps per window, the 48-256-256-21 Gaussian actor, with the realism layer and domain randomisation off and with both on.
Env-steps per second of three loops, alternated in one process, every shape warmed up first, REPS windows per figure (median, minimum
and maximum are printed), each window timed by the host clock around work that ends in a device synchronisation:
  (a) collect      VecEnv.collect_torch(T=64): the actor kernel and the env step chained on the batch's stream by one call
  (b) torch loop   the same 64 steps driven from Python: the same MLP as a torch module on the same GPU, its Gaussian sample, step_torch
  (c) env only     step_torch fed actions made beforehand: the env loop without any policy
Expectation to check: (a) >= (b), and (a) approaches (c) less the actor kernel's own time (take that from a kernel trace of
`--legs a --reps 1` in a run of its own).  If (a) is slower than (b) the tool says so.
usage: gpu_collect_bench.py [--reps N] [--legs abc] [--out FILE]     (results: profiles/collect_bench.txt)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--legs", default="abc")
ap.add_argument("--out", default=None)
args = ap.parse_args()
N, T, SIZES = 4096, 64, [48, 256, 256, 21]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


if not torch.cuda.is_available():
    sys.exit("gpu_collect_bench: no GPU visible - nothing is measured without one")
dev = torch.device("cuda", 0)
model = hb.Model.load(os.path.join(ROOT, "humanoid_mujoco_amd", "assets", "humanoid27.hbm"))
rng = np.random.default_rng(0)
ws = [rng.uniform(-1, 1, size=(a, c)).astype(np.float32) / np.sqrt(a) for a, c in zip(SIZES[:-1], SIZES[1:])]
bs = [rng.uniform(-1, 1, size=c).astype(np.float32) / np.sqrt(a) for a, c in zip(SIZES[:-1], SIZES[1:])]
log_std = np.full(SIZES[-1], -1.0, np.float32)
layers = []
for l, (w, b) in enumerate(zip(ws, bs)):
    lin = torch.nn.Linear(w.shape[0], w.shape[1])
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(w.T.copy()))
        lin.bias.copy_(torch.from_numpy(b))
    layers.append(lin)
    if l + 1 < len(ws):
        layers.append(torch.nn.Tanh())
net = torch.nn.Sequential(*layers).to(dev)
std = torch.from_numpy(np.exp(log_std)).to(dev)
say("%s, %d envs, %d env steps per window, actor %s (Gaussian head), %d windows per figure after one warm-up round" % (
    hb.Batch(model, 1, 0).device_name(), N, T, "-".join(map(str, SIZES)), args.reps))

for on in (False, True):
    env = hb.VecEnv(model, N, 0, realism=on, domain_randomization=on, seed=1)
    env.actor_set(SIZES, ws, bs, head="gaussian", log_std=log_std, seed=1)
    tape = torch.from_numpy(rng.uniform(-1, 1, size=(T, N, SIZES[-1])).astype(np.float32)).to(dev)

    def window(leg):
        obs = torch.from_numpy(env.reset()).to(dev)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if leg == "a":
            env.collect_torch(T, obs0=obs)
        elif leg == "b":
            with torch.no_grad():
                for _ in range(T):
                    mean = net(obs)
                    obs = env.step_torch(mean + std * torch.randn_like(mean))[0]
        else:
            for t in range(T):
                env.step_torch(tape[t])
        torch.cuda.synchronize(dev)
        return N * T / (time.perf_counter() - t0)

    rate = {leg: [] for leg in args.legs}
    for rep in range(args.reps + 1):  # (the first round warms every shape up and is not counted)
        for leg in args.legs:
            r = window(leg)
            if rep:
                rate[leg].append(r)
    say("realism and domain randomisation %s [%s]:" % ("ON" if on else "off", env.batch.last_kernel()))
    names = {"a": "(a) collect_torch", "b": "(b) torch MLP + step_torch", "c": "(c) step_torch, no policy"}
    med = {leg: float(np.median(rate[leg])) for leg in args.legs}
    for leg in args.legs:
        say("  %-28s %.3e env-steps/s (min %.3e max %.3e), %.1f us per env step of the batch" % (names[leg], med[leg], min(rate[leg]), max(rate[leg]), 1e6 * N / med[leg]))
    if "a" in med and "b" in med:
        say("  (a) / (b) = %.2f%s" % (med["a"] / med["b"], "" if med["a"] >= med["b"] else "   COLLECTION IS SLOWER THAN THE PYTHON LOOP"))
    if "a" in med and "c" in med:
        say("  (a) takes %.1f us per step more than (c): the actor kernel and its place in the chain" % (1e6 * N / med["a"] - 1e6 * N / med["c"]))
    env.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
