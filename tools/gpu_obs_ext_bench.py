#!/usr/bin/env python3
"""What the observation extension (include/hb.h: hb_env_obs_extend; VecEnv(obs_extend=...)) costs and saves a perceptive training loop:
4096 envs of humanoid27_hfield.hbm with terrain randomisation, 32 env steps per window, a 17 x 11 height scan under the torso, the
Gaussian actor 48-256-256-21 widened to 256-256-256-21 by the extension (48 + 21 last-action + 187 scan entries).
Microseconds per collected step of the batch for three loops, alternated in one process, every shape warmed up first, REPS windows per
figure (median, minimum and maximum), each window timed by the host clock around work that ends in a device synchronisation:
  (p) plain        collect_torch without the extension: the path that must not have moved (run this leg on the parent commit too)
  (e) extended     collect_torch with obs_extend=dict(prev_action=True, height_scan=...)
  (t) torch loop   the same observation built from Python: step_torch + height_scan_torch + torch.cat, the same MLP as a torch module
The share of the added time that is the second, masked pass comes from a kernel trace of `--legs e --reps 1` under
rocprofv3 --kernel-trace --stats, in a run of its own: --trace FILE reads its kernel_trace csv (no GPU needed) and splits the kinematics
and ray dispatches into those ahead of the env kernel and those behind it.
usage: gpu_obs_ext_bench.py [--reps N] [--legs pet] [--out FILE] | --trace KERNEL_TRACE_CSV [--out FILE]     (results: profiles/obs_ext_bench.txt)"""
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
ap.add_argument("--legs", default="pet")
ap.add_argument("--trace", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
N, T, NU, HIDDEN = 4096, 32, 21, [256, 256]
XS, YS, Z0, CUTOFF = np.linspace(-0.8, 0.8, 17), np.linspace(-0.5, 0.5, 11), 1.0, 4.0
SCAN = dict(offset=Z0, scale=1.0, clip=(-1.0, 1.0))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def trace_summary(path):
    """GPU time per collected step of the extension's launches, from rocprofv3's kernel trace of the extended leg"""
    import csv
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(path))), key=lambda r: r[0])
    tot, cnt, last, steps, all_ns = {}, {}, "", 0, 0
    for t0, t1, name in rows:
        all_ns += t1 - t0
        if "hb_ray" in name or "hb_kin" in name:
            key = ("second pass " if "hb_env_kernel" in last else "first pass  ") + ("rays" if "hb_ray" in name else "poses")
            tot[key] = tot.get(key, 0) + t1 - t0
            cnt[key] = cnt.get(key, 0) + 1
        elif "hb_env_kernel" in name or "hb_step" in name or "hb_actor" in name or "hb_reset" in name:
            last = name
            steps += "hb_actor" in name
    say("kernel trace of the extended leg: %d collected steps, %.1f us of GPU time per step in all kernels" % (steps, 1e-3 * all_ns / max(1, steps)))
    for key in sorted(tot):
        say("  %-20s %6d dispatches, %7.1f us per collected step" % (key, cnt[key], 1e-3 * tot[key] / max(1, steps)))
    second = sum(v for k, v in tot.items() if k.startswith("second"))
    if tot:
        say("  the second, masked pass is %.0f %% of the GPU time of the extension's own launches (%.1f of %.1f us per step)"
            % (100.0 * second / sum(tot.values()), 1e-3 * second / max(1, steps), 1e-3 * sum(tot.values()) / max(1, steps)))


if args.trace:
    trace_summary(args.trace)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)
if not torch.cuda.is_available():
    sys.exit("gpu_obs_ext_bench: no GPU visible - nothing is measured without one")
dev = torch.device("cuda", 0)
model = hb.Model.load(os.path.join(ROOT, "humanoid_mujoco_amd", "assets", "humanoid27_hfield.hbm"))
extended = hasattr(hb.Batch, "obs_extend")  # (the parent commit runs leg p alone)
legs = [leg for leg in args.legs if leg == "p" or extended]


def make(leg):
    kw = dict(domain_randomization=True, seed=1)
    if leg in "et":
        kw["height_scan"] = dict(body=1, xs=XS, ys=YS, z0=Z0, cutoff=CUTOFF)
    if leg == "e":
        kw["obs_extend"] = dict(prev_action=True, height_scan=SCAN)
    env = hb.VecEnv(model, N, 0, **kw)
    nobs = model.nobs + NU + len(XS) * len(YS) if leg in "et" else model.nobs
    sizes = [nobs, *HIDDEN, NU]
    rng = np.random.default_rng(0)
    ws = [rng.uniform(-1, 1, size=(a, c)).astype(np.float32) / np.sqrt(a) for a, c in zip(sizes[:-1], sizes[1:])]
    bs = [rng.uniform(-1, 1, size=c).astype(np.float32) / np.sqrt(a) for a, c in zip(sizes[:-1], sizes[1:])]
    log_std = np.full(NU, -1.0, np.float32)
    net = None
    if leg == "t":
        mods = []
        for l, (w, b) in enumerate(zip(ws, bs)):
            lin = torch.nn.Linear(w.shape[0], w.shape[1])
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(w.T.copy()))
                lin.bias.copy_(torch.from_numpy(b))
            mods.append(lin)
            if l + 1 < len(ws):
                mods.append(torch.nn.Tanh())
        net = torch.nn.Sequential(*mods).to(dev)
    else:
        assert getattr(env, "nobs", model.nobs) == nobs
        env.actor_set(sizes, ws, bs, head="gaussian", log_std=log_std, seed=1)
    return env, net, torch.from_numpy(np.exp(log_std)).to(dev)


def scan_columns(env):
    d = env.height_scan_torch().reshape(N, -1)
    return torch.clamp(SCAN["scale"] * (SCAN["offset"] - d), *SCAN["clip"])


def window(leg, env, net, std):
    obs = torch.from_numpy(env.reset()).to(dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    if leg != "t":
        env.collect_torch(T, obs0=obs)
    else:
        with torch.no_grad():
            act = torch.zeros((N, NU), device=dev)
            for _ in range(T):
                row = torch.cat([obs, act, scan_columns(env)], dim=1)
                mean = net(row)
                act = mean + std * torch.randn_like(mean)
                obs = env.step_torch(act)[0]
    torch.cuda.synchronize(dev)
    return 1e6 * (time.perf_counter() - t0) / T


say("%s, %d envs of humanoid27_hfield.hbm, terrain randomisation on, %d env steps per window, scan %d x %d, hidden %s, %d windows per figure after one warm-up round"
    % (hb.Batch(model, 1, 0).device_name(), N, T, len(XS), len(YS), "-".join(map(str, HIDDEN)), args.reps))
setup = {leg: make(leg) for leg in legs}
us = {leg: [] for leg in legs}
for rep in range(args.reps + 1):  # (the first round warms every shape up and is not counted)
    for leg in legs:
        r = window(leg, *setup[leg])
        if rep:
            us[leg].append(r)
names = {"p": "(p) collect_torch, plain", "e": "(e) collect_torch, extended", "t": "(t) step_torch + height_scan_torch + cat"}
med = {leg: float(np.median(us[leg])) for leg in legs}
for leg in legs:
    say("  %-44s %8.1f us per collected step (min %.1f max %.1f) [%d observations, %s]"
        % (names[leg], med[leg], min(us[leg]), max(us[leg]), setup[leg][0].observation_shape[0] if leg != "t" else model.nobs + NU + len(XS) * len(YS),
           setup[leg][0].batch.last_kernel()))
if "p" in med and "e" in med:
    say("  the extension adds %.1f us per step (%.1f %%)" % (med["e"] - med["p"], 100.0 * (med["e"] - med["p"]) / med["p"]))
if "e" in med and "t" in med:
    say("  (t) / (e) = %.2f%s" % (med["t"] / med["e"], "" if med["t"] >= med["e"] else "   THE DEVICE PATH IS SLOWER THAN THE PYTHON LOOP"))
for env, _, _ in setup.values():
    env.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
