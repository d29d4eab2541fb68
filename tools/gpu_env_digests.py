#!/usr/bin/env python3
"""What the env adapter computes with every env feature on, as one SHA-256 per array: two checkouts whose env kernels compute the same
bits print the same lines.
  configuration: 64 envs of humanoid27_hfield.hbm; the realism layer; domain randomisation with terrain; the last action and an 8 x 5 height
           scan in the row; observed velocity commands redrawn every 15 ms; every foot-contact term, two feet, five penalised and two
           terminal bodies, the flags observed; auto-reset with max_time = 60 ms, so that every env ends several episodes inside the run
           (by the time limit or by a terminal contact); terminal observations; 40 control steps of seeded random actions
  arrays:  over all steps - observations (the reset's first), rewards, terminated and truncated flags, the terminal-observation table
           after every step; at the end - the states, the episode numbers (an env's count of ended episodes: with auto-reset the device's
           counter, which the library does not hand out, advances with each; the commands and the domain parameters are drawn from it),
           the commands, the feet records (t_last and the contact bits) and the domain parameters
The run is one child process under its own time limit, started once; --root DIR runs the package of another checkout (built) instead.
usage: gpu_env_digests.py [--root DIR] [--out FILE] [--beside FILE [FILE]]
  --beside A [B]: print the digests of earlier runs (their --out) next to this run's.  With two files, A and B are two runs of one tree:
           an array that differs between THEM is listed as not comparable.  Fails if a comparable line differs from this run's."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS, NU = 64, 40, 21
CHILD_LIMIT = 240  # seconds: the interpreter's start, the env and 40 steps of 64 envs take a few


def child(root):
    sys.path.insert(0, root)
    import numpy as np
    import humanoid_mujoco_amd as hb
    model = hb.Model.load(os.path.join(root, "humanoid_mujoco_amd", "assets", "humanoid27_hfield.hbm"))
    xs, ys = np.linspace(-0.7, 0.7, 8), np.linspace(-0.4, 0.4, 5)
    env = hb.VecEnv(model, N, 0, seed=3, realism=True, domain_randomization=True, auto_reset=1, max_time=0.06, target_z=10.0,
                    height_scan=dict(body=1, xs=xs, ys=ys, z0=1.0, cutoff=4.0),
                    obs_extend=dict(prev_action=True, height_scan=dict(offset=1.0, scale=1.0, clip=(-1.0, 1.0))),
                    commands=dict(resample_time=0.015),
                    feet=dict(bodies=("foot_right", "foot_left"), penalised=("shin_right", "shin_left", "lower_arm_right", "lower_arm_left", "pelvis"),
                              terminal=("torso", "head"), observe=1))
    rng = np.random.default_rng(5)
    obs, rew, term, trunc, tobs = [env.reset()], [], [], [], []
    for _ in range(STEPS):
        o, r, te, tr, _ = env.step_arrays(rng.uniform(-1.0, 1.0, (N, NU)).astype(np.float32))
        obs.append(o); rew.append(r); term.append(te); trunc.append(tr)
        tobs.append(env.batch.env_terminal_obs())
    done = np.array(term, dtype=bool) | np.array(trunc, dtype=bool)
    t_last, contact = env.batch.feet()
    arrays = [("observations", np.array(obs, np.float32)), ("rewards", np.array(rew, np.float32)), ("terminated", np.array(term, np.uint8)),
              ("truncated", np.array(trunc, np.uint8)), ("terminal observations", np.array(tobs, np.float32)),
              ("final states", env.batch.get_state(hb.STATE_INTEGRATION)), ("episode numbers", done.sum(axis=0).astype(np.int32)),
              ("commands", env.commands()), ("feet t_last", t_last), ("feet contact", contact), ("domain parameters", env.batch.env_domain_params())]
    assert done.sum(axis=0).min() >= 2, "episodes were to end inside the run"
    for name, a in arrays:
        a = np.ascontiguousarray(a)
        assert a.size and not (a.dtype.kind == "f" and np.isnan(a).any()), name
        print("DIGEST %-24s %8d %-7s %s" % (name, a.size, a.dtype, hashlib.sha256(a.tobytes()).hexdigest()), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out", default=None)
    ap.add_argument("--beside", nargs="+", default=[])
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    if args.child:
        return child(root)
    if len(args.beside) > 2:
        sys.exit("gpu_env_digests: --beside takes one or two files")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root], capture_output=True, text=True, timeout=CHILD_LIMIT)
    lines = [l[len("DIGEST "):] for l in r.stdout.splitlines() if l.startswith("DIGEST ")]
    if r.returncode != 0 or not lines:
        sys.exit("gpu_env_digests: the run ended with code %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.beside:
        others = [open(p).read().splitlines() for p in args.beside]
        differ = any(len(o) != len(lines) for o in others)
        print("\n%-42s %s  %-64s" % ("array", "  ".join("%-64s" % p for p in args.beside), "this run (--root %s)" % args.root))
        for i, b in enumerate(lines):
            col = [o[i] for o in others if i < len(o)]
            comparable = len(set(col)) == 1
            verdict = "not comparable" if not comparable else "equal" if col[0] == b else "DIFFERS"
            differ |= verdict == "DIFFERS"
            print("%-42s %s  %s  %s" % (b[:-64].rstrip(), "  ".join(c.split()[-1] for c in col), b.split()[-1], verdict))
        print("%d arrays, %s" % (len(lines), "a line DIFFERS" if differ else "every comparable line equal"))
        sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
