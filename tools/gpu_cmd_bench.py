#!/usr/bin/env python3
"""What per-env velocity commands (include/hb.h: hb_env_commands; VecEnv(commands=...)) cost a perceptive training loop, and whether the
path without them moved: the configuration of profiles/obs_ext_bench.txt - 4096 envs of humanoid27_hfield.hbm with terrain
randomisation, a height scan and the last action in the observation, the Gaussian actor with hidden layers 256-256 - and 32 env steps
per collect_torch window.  The scan is 16 x 11, not that file's 17 x 11: with the three command entries its row of 256 would be 259 wide,
above the 256 the actor kernel takes.  Microseconds per collected step for three cases:
  (off)     no command configuration
  (on)      commands installed and observed (the row grows by 3)
  (parent)  the no-commands path of another build of the package, given with --parent DIR: a checkout of the parent commit, built
Every figure comes from a process of its own, started here one at a time under its own time limit, that builds the env, runs one warm-up
window and times ONE window by the host clock around work that ends in a device synchronisation.  The cases alternate over --rounds
rounds; a child that fails or runs out of time ends the run (nothing is tried again).
usage: gpu_cmd_bench.py [--rounds 5] [--parent DIR] [--out FILE]        (results: profiles/cmd_bench.txt)"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, NU, HIDDEN = 4096, 32, 21, [256, 256]
CHILD_LIMIT = 180  # seconds: the env, two windows of 32 steps and the interpreter's start take a few


def child(case, root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import humanoid_mujoco_amd as hb
    if not torch.cuda.is_available():
        sys.exit("gpu_cmd_bench: no GPU visible - nothing is measured without one")
    dev = torch.device("cuda", 0)
    model = hb.Model.load(os.path.join(root, "humanoid_mujoco_amd", "assets", "humanoid27_hfield.hbm"))
    xs, ys = np.linspace(-0.8, 0.8, 16), np.linspace(-0.5, 0.5, 11)
    kw = dict(domain_randomization=True, seed=1, height_scan=dict(body=1, xs=xs, ys=ys, z0=1.0, cutoff=4.0),
              obs_extend=dict(prev_action=True, height_scan=dict(offset=1.0, scale=1.0, clip=(-1.0, 1.0))))
    if case == "on":
        kw["commands"] = dict(resample_time=0.05)  # (a draw every ten control steps: three inside every window)
    env = hb.VecEnv(model, N, 0, **kw)
    sizes = [env.nobs, *HIDDEN, NU]
    rng = np.random.default_rng(0)
    ws = [rng.uniform(-1, 1, size=(a, c)).astype(np.float32) / np.sqrt(a) for a, c in zip(sizes[:-1], sizes[1:])]
    bs = [rng.uniform(-1, 1, size=c).astype(np.float32) / np.sqrt(a) for a, c in zip(sizes[:-1], sizes[1:])]
    env.actor_set(sizes, ws, bs, head="gaussian", log_std=np.full(NU, -1.0, np.float32), seed=1)
    us = 0.0
    for timed in (False, True):
        obs = torch.from_numpy(env.reset()).to(dev)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        env.collect_torch(T, obs0=obs)
        torch.cuda.synchronize(dev)
        us = 1e6 * (time.perf_counter() - t0) / T
    print("RESULT %.3f %d %s %s" % (us, env.nobs, env.batch.last_kernel(), env.batch.device_name().replace(" ", "_")), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmd_bench.txt"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.root)
    import numpy as np
    cases = [("off", ROOT), ("on", ROOT)] + ([("parent", os.path.abspath(args.parent))] if args.parent else [])
    us, info, rounds = {c: [] for c, _ in cases}, {}, []
    for rnd in range(args.rounds):
        for case, root in cases:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--root", root], capture_output=True, text=True, timeout=CHILD_LIMIT)
            res = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or len(res) != 1:
                sys.exit("gpu_cmd_bench: case %s of round %d ended with code %d\n%s\n%s" % (case, rnd, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            f = res[0].split()
            us[case].append(float(f[1]))
            info[case] = (int(f[2]), f[3], f[4].replace("_", " "))
            print("round %d %-6s %8.1f us per collected step" % (rnd, case, us[case][-1]), flush=True)
        rounds.append("  round %d:" % rnd + "".join("  %s %.1f" % (case, us[case][-1]) for case, _ in cases))
    names = {"off": "(off)    no command configuration", "on": "(on)     commands installed and observed", "parent": "(parent) the parent commit's build, no commands"}
    lines = ["%s, %d envs of humanoid27_hfield.hbm, terrain randomisation on, scan 16 x 11 and the last action in the row, hidden %s, collect_torch(T = %d);"
             % (info["off"][2], N, "-".join(map(str, HIDDEN)), T),
             "%d rounds, the cases alternating, one process and one timed window (after one warm-up window) per figure" % args.rounds]
    med = {}
    for case, _ in cases:
        med[case] = float(np.median(us[case]))
        lines.append("  %-50s %8.1f us per collected step (min %.1f max %.1f) [%d observations, %s]"
                     % (names[case], med[case], min(us[case]), max(us[case]), info[case][0], info[case][1]))
    lines.append("  commands add %.1f us per step (%.2f %%); spread of (off) %.1f us, of (on) %.1f us"
                 % (med["on"] - med["off"], 100.0 * (med["on"] - med["off"]) / med["off"], max(us["off"]) - min(us["off"]), max(us["on"]) - min(us["on"])))
    if "parent" in med:
        spread = max(max(us[c]) - min(us[c]) for c in ("off", "parent"))
        moved = abs(med["off"] - med["parent"]) > spread
        above = sum(a > b for a, b in zip(us["off"], us["parent"]))
        lines.append("  the no-commands path against the parent: %+.1f us per step (%+.2f %%), spread %.1f us: %s; (off) above (parent) in %d of %d rounds"
                     % (med["off"] - med["parent"], 100.0 * (med["off"] - med["parent"]) / med["parent"], spread,
                        "MOVED beyond the spread" if moved else "inside the spread", above, args.rounds))
    lines += rounds
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
