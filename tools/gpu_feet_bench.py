#!/usr/bin/env python3
"""What the foot-contact terms (include/hb.h: hb_env_feet; VecEnv(feet=...)) cost a perceptive training loop, and whether the paths without
them moved: the configuration of profiles/cmd_bench.txt - 4096 envs of humanoid27_hfield.hbm with terrain randomisation, a 16 x 11 height
scan, the last action and observed velocity commands in the row, the Gaussian actor with hidden layers 256-256 - and 32 env steps per
collect_torch window.  Microseconds per collected step for:
  (feet)            every term on, both feet, five penalised and two terminal bodies, the flags observed (the row grows by 2)
  (readout)         contact_forces=True and no feet: the price of the read-out alone, which forces the full step kernel
  (neither)         neither
  (parent-feet)     (feet),
  (parent-readout)  (readout) and
  (parent-neither)  (neither) in another build of the package, given with --parent DIR: a checkout of the parent commit, built
Every figure comes from a process of its own, started here one at a time under its own time limit, that builds the env, runs one warm-up
window and times ONE window by the host clock around work that ends in a device synchronisation.  The cases alternate over --rounds
rounds; a child that fails or runs out of time ends the run (nothing is tried again).
usage: gpu_feet_bench.py [--rounds 5] [--parent DIR] [--out FILE]        (results: profiles/feet_bench.txt)"""
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
        sys.exit("gpu_feet_bench: no GPU visible - nothing is measured without one")
    dev = torch.device("cuda", 0)
    model = hb.Model.load(os.path.join(root, "humanoid_mujoco_amd", "assets", "humanoid27_hfield.hbm"))
    xs, ys = np.linspace(-0.8, 0.8, 16), np.linspace(-0.5, 0.5, 11)
    kw = dict(domain_randomization=True, seed=1, height_scan=dict(body=1, xs=xs, ys=ys, z0=1.0, cutoff=4.0),
              obs_extend=dict(prev_action=True, height_scan=dict(offset=1.0, scale=1.0, clip=(-1.0, 1.0))), commands=dict(resample_time=0.05))
    if case.endswith("feet"):
        kw["feet"] = dict(bodies=("foot_right", "foot_left"), penalised=("shin_right", "shin_left", "lower_arm_right", "lower_arm_left", "pelvis"),
                          terminal=("torso", "head"), observe=1)
    elif case.endswith("readout"):
        kw["contact_forces"] = True
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


NAMES = {"feet": "(feet)           every term on, flags observed", "readout": "(readout)        contact_forces=True, no feet", "neither": "(neither)        no read-out, no feet",
         "parent-feet": "(parent-feet)    the parent commit's build", "parent-readout": "(parent-readout) the parent commit's build", "parent-neither": "(parent-neither) the parent commit's build"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feet_bench.txt"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.root)
    import numpy as np
    cases = [("feet", ROOT), ("readout", ROOT), ("neither", ROOT)]
    if args.parent:
        cases += [("parent-" + case, os.path.abspath(args.parent)) for case in ("feet", "readout", "neither")]
    us, info, rounds = {c: [] for c, _ in cases}, {}, []
    for rnd in range(args.rounds):
        for case, root in cases:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--root", root], capture_output=True, text=True, timeout=CHILD_LIMIT)
            res = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or len(res) != 1:
                sys.exit("gpu_feet_bench: case %s of round %d ended with code %d\n%s\n%s" % (case, rnd, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            f = res[0].split()
            us[case].append(float(f[1]))
            info[case] = (int(f[2]), f[3], f[4].replace("_", " "))
            print("round %d %-15s %8.1f us per collected step" % (rnd, case, us[case][-1]), flush=True)
        rounds.append("  round %d:" % rnd + "".join("  %s %.1f" % (case, us[case][-1]) for case, _ in cases))
    lines = ["%s, %d envs of humanoid27_hfield.hbm, terrain randomisation on, scan 16 x 11, the last action and observed commands in the row, hidden %s, collect_torch(T = %d);"
             % (info["feet"][2], N, "-".join(map(str, HIDDEN)), T),
             "%d rounds, the cases alternating, one process and one timed window (after one warm-up window) per figure" % args.rounds]
    med, spread = {}, {}
    for case, _ in cases:
        med[case], spread[case] = float(np.median(us[case])), max(us[case]) - min(us[case])
        lines.append("  %-50s %8.1f us per collected step (min %.1f max %.1f) [%d observations, %s]"
                     % (NAMES[case], med[case], min(us[case]), max(us[case]), info[case][0], info[case][1]))
    lines.append("  the feet terms add %+.1f us per step (%+.2f %%) on top of the read-out; spread of (feet) %.1f us, of (readout) %.1f us"
                 % (med["feet"] - med["readout"], 100.0 * (med["feet"] - med["readout"]) / med["readout"], spread["feet"], spread["readout"]))
    lines.append("  the read-out itself (it forces the full step kernel; profiles/contact_readout_bench.txt): %+.1f us per step (%+.2f %%) over (neither); the whole bill of the feet: %+.1f us (%+.2f %%)"
                 % (med["readout"] - med["neither"], 100.0 * (med["readout"] - med["neither"]) / med["neither"], med["feet"] - med["neither"],
                    100.0 * (med["feet"] - med["neither"]) / med["neither"]))
    for case in ("feet", "readout", "neither"):
        p = "parent-" + case
        if p in med:
            s = max(spread[case], spread[p])
            above = sum(a > b for a, b in zip(us[case], us[p]))
            lines.append("  (%s) against the parent: %+.1f us per step (%+.2f %%), spread %.1f us: %s; above the parent in %d of %d rounds"
                         % (case, med[case] - med[p], 100.0 * (med[case] - med[p]) / med[p], s, "MOVED beyond the spread" if abs(med[case] - med[p]) > s else "inside the spread",
                            above, args.rounds))
    lines += rounds
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
