#!/usr/bin/env python3
"""What the on-device normaliser (include/hb.h: hb_env_collect_norm_dev; VecEnv(normalize=...).collect_torch) costs beside the plain
collection, and what the same semantics cost the only other way there is: T rounds of step_torch with the actor and VecNormalize /
VecMonitor written in torch.  tools/gpu_gae_bench.py's setup: 4096 envs of the 27-dof model, T = 32, the 48-256-256-21 Gaussian actor,
reward_kind 1 with a 0.1 s time limit.  Three variants, alternated in one process after a warm-up round, REPS windows each, every window
from a fresh reset and timed with device events on the caller's stream:
  (a) collect_torch(T, terminal_obs=True) on an env without a normaliser        hb_env_collect_dev (gae_bench's variant (i))
  (b) collect_torch(T, terminal_obs=True) on an env with normalize={}           hb_env_collect_norm_dev: two more launches per step
  (c) T x [torch actor on the normalised observation, Normal sample, step_torch, running mean / variance updates in fp64, normalise and
      clip observation and reward, discounted return, episode return / length bookkeeping], the tapes written as the collection writes them
Printed: the medians with minimum and maximum, (b) - (a) per collection and per step with its spread over the rounds (maximum - minimum),
the ratio (c) / (b), and whether (b) lies below (c) by more than the larger spread; if not, the tool says so.  The torch normaliser is run
once over the raw tapes of a device collection so that it is known to compute the same thing.
usage: gpu_norm_bench.py [--reps N] [--out FILE]     (results: profiles/norm_bench.txt)"""
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
args = ap.parse_args()
N, T, ACTOR = 4096, 32, [48, 256, 256, 21]
GAMMA, EPSILON, CLIP = 0.99, 1e-8, 10.0
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


if not torch.cuda.is_available():
    sys.exit("gpu_norm_bench: no GPU visible - nothing is measured without one")
dev = torch.device("cuda", 0)
model = hb.Model.load(os.path.join(ROOT, "humanoid_mujoco_amd", "assets", "humanoid27.hbm"))
rng = np.random.default_rng(0)
aw = [rng.uniform(-1, 1, size=(a, c)).astype(np.float32) / np.sqrt(a) for a, c in zip(ACTOR[:-1], ACTOR[1:])]
ab = [rng.uniform(-1, 1, size=c).astype(np.float32) / np.sqrt(a) for a, c in zip(ACTOR[:-1], ACTOR[1:])]
log_std = np.full(ACTOR[-1], -1.0, np.float32)
layers = []
for l, (w, b) in enumerate(zip(aw, ab)):
    lin = torch.nn.Linear(w.shape[0], w.shape[1])
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(w.T.copy()))
        lin.bias.copy_(torch.from_numpy(b))
    layers.append(lin)
    if l + 1 < len(aw):
        layers.append(torch.nn.Tanh())
actor = torch.nn.Sequential(*layers).to(dev)
std = torch.from_numpy(np.exp(log_std)).to(dev)

envs = {}
for name, norm in (("plain", None), ("norm", {})):
    envs[name] = hb.VecEnv(model, N, 0, seed=1, reward_kind=1, max_time=0.1, normalize=norm)
    envs[name].actor_set(ACTOR, aw, ab, head="gaussian", log_std=log_std, seed=1)
say("%s, %d envs, T = %d, actor %s (Gaussian head), VecNormalize defaults (clip 10, gamma 0.99, epsilon 1e-8), %d windows per variant after one warm-up round [device events]" % (
    envs["plain"].batch.device_name(), N, T, "-".join(map(str, ACTOR)), args.reps))


class TorchRms:
    """stable-baselines3's RunningMeanStd on the device, in fp64, without a host synchronisation"""

    def __init__(self, shape):
        self.mean = torch.zeros(shape, dtype=torch.float64, device=dev)
        self.var = torch.ones(shape, dtype=torch.float64, device=dev)
        self.count = torch.full((), 1e-4, dtype=torch.float64, device=dev)

    def update(self, x):
        x = x.double()
        n = x.shape[0]
        mb, vb = x.mean(0), x.var(0, unbiased=False)
        d = mb - self.mean
        tot = self.count + n
        self.mean = self.mean + d * n / tot
        self.var = (self.var * self.count + vb * n + d * d * self.count * n / tot) / tot
        self.count = tot


class TorchNorm:
    def __init__(self):
        self.obs_rms, self.ret_rms = TorchRms((ACTOR[0],)), TorchRms(())
        self.ret = torch.zeros(N, dtype=torch.float64, device=dev)
        self.ep_ret = torch.zeros(N, dtype=torch.float64, device=dev)
        self.ep_len = torch.zeros(N, dtype=torch.int32, device=dev)

    def norm_obs(self, o):
        return (((o.double() - self.obs_rms.mean) / torch.sqrt(self.obs_rms.var + EPSILON)).float()).clamp(-CLIP, CLIP)

    def reset(self, o):
        self.obs_rms.update(o)
        return self.norm_obs(o)

    def step(self, o, r, done):
        self.obs_rms.update(o)
        on = self.norm_obs(o)
        self.ret = self.ret * GAMMA + r.double()
        self.ret_rms.update(self.ret)
        rn = ((r.double() / torch.sqrt(self.ret_rms.var + EPSILON)).float()).clamp(-CLIP, CLIP)
        self.ep_ret = self.ep_ret + r.double()
        self.ep_len = self.ep_len + 1
        zero = torch.zeros_like(self.ep_ret)
        er, el = torch.where(done, self.ep_ret, zero).float(), torch.where(done, self.ep_len, torch.zeros_like(self.ep_len))
        self.ep_ret, self.ep_len = torch.where(done, zero, self.ep_ret), torch.where(done, torch.zeros_like(self.ep_len), self.ep_len)
        self.ret = torch.where(done, zero, self.ret)
        return on, rn, er, el


f32 = dict(dtype=torch.float32, device=dev)
tapes_c = {"obs": torch.empty((T + 1, N, ACTOR[0]), **f32), "action": torch.empty((T, N, ACTOR[-1]), **f32), "mean": torch.empty((T, N, ACTOR[-1]), **f32),
           "reward": torch.empty((T, N), **f32), "terminated": torch.empty((T, N), dtype=torch.bool, device=dev), "truncated": torch.empty((T, N), dtype=torch.bool, device=dev),
           "ep_return": torch.empty((T, N), **f32), "ep_length": torch.empty((T, N), dtype=torch.int32, device=dev)}


def torch_loop(env, obs_raw):
    with torch.no_grad():
        nm = TorchNorm()
        t = tapes_c
        t["obs"][0] = nm.reset(obs_raw)
        for k in range(T):
            mean = actor(t["obs"][k])
            t["mean"][k] = mean
            # (a tensor of its own, released at once: step_torch marks its argument as in use on the batch's stream, and a block that
            # carries that mark must be released while the stream exists - the tapes outlive the env)
            action = mean + std * torch.randn_like(mean)
            t["action"][k] = action
            o, r, te, tr = env.step_torch(action)
            del action
            t["obs"][k + 1], t["reward"][k], t["ep_return"][k], t["ep_length"][k] = nm.step(o, r, te | tr)
            t["terminated"][k], t["truncated"][k] = te, tr
        return t


def window(variant):
    env = envs["norm" if variant == "b" else "plain"]
    obs = torch.from_numpy(env.reset()).to(dev)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = torch_loop(env, obs) if variant == "c" else env.collect_torch(T, obs0=obs, terminal_obs=True)
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), out


# the two normalisers on the raw tapes of one device collection
env = envs["norm"]
env.reset()
raw0 = torch.from_numpy(env.get_original_obs()).to(dev)
out = env.collect_torch(T, terminal_obs=True, raw=True)
with torch.no_grad():
    nm = TorchNorm()
    worst = {"obs": float((nm.reset(raw0) - out["obs"][0]).abs().max()), "reward": 0.0, "ep_return": 0.0}
    for k in range(T):
        on, rn, er, el = nm.step(out["raw_obs"][k], out["raw_reward"][k], out["terminated"][k] | out["truncated"][k])
        worst["obs"] = max(worst["obs"], float((on - out["obs"][k + 1]).abs().max()))
        worst["reward"] = max(worst["reward"], float((rn - out["reward"][k]).abs().max()))
        worst["ep_return"] = max(worst["ep_return"], float((er - out["ep_return"][k]).abs().max()))
        assert torch.equal(el, out["ep_length"][k])
say("one window: %d of %d rows end an episode; largest |device - torch| over its raw tapes: %s" % (
    int((out["truncated"] | out["terminated"]).sum()), N * T, ", ".join("%s %.2e" % kv for kv in worst.items())))

names = {"a": "(a) hb_env_collect_dev", "b": "(b) hb_env_collect_norm_dev", "c": "(c) step_torch x T + torch actor / normaliser"}
ms = {v: [] for v in names}
for rep in range(args.reps + 1):  # (the first round warms every variant up and is not counted)
    for v in ms:
        t, _ = window(v)
        if rep:
            ms[v].append(t)
med = {v: float(np.median(ms[v])) for v in ms}
for v in ms:
    say("  %-48s median %8.3f ms (min %8.3f max %8.3f), %.1f us per collected step" % (names[v], med[v], min(ms[v]), max(ms[v]), 1e3 * med[v] / T))
dba = np.array(ms["b"]) - np.array(ms["a"])
dcb = np.array(ms["c"]) - np.array(ms["b"])
sba, scb = float(dba.max() - dba.min()), float(dcb.max() - dcb.min())
say("  (b) - (a) per round: median %8.3f ms per collection, %.2f us per step, spread (max - min) %.3f ms" % (float(np.median(dba)), 1e3 * float(np.median(dba)) / T, sba))
say("  (c) - (b) per round: median %8.3f ms, spread (max - min) %.3f ms; (c) / (b) = %.2f" % (float(np.median(dcb)), scb, med["c"] / med["b"]))
ok = float(np.median(dcb)) > max(sba, scb)
say("  the device normaliser's collection is faster than the torch loop by more than either spread: %s" % ("yes" if ok else "NO - THE CLAIM IS NOT SUPPORTED"))
for e in envs.values():
    e.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
