"""The reward with velocity commands against tests/cmd_ref.py in fp64, on the GPU: writes profiles/cmd_parity.txt (or --out).

    python tools/gpu_cmd_parity.py [--out PATH] [--gpu 0]

Both frames and both reward kinds, 64 envs of the 27-dof humanoid from a perturbed reset with a yawed root, four steps; cmd_ref is fed the
device's own states, joint torques and actions.  Next to every figure: what the reward WITHOUT commands shows against tests/env_ref.py on
the same states.  tests/test_gpu_cmd.py asserts eight times the worst figure written here (its PARITY_WORST)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmd_parity.txt"))
    ap.add_argument("--gpu", type=int, default=0)
    args = ap.parse_args()
    import humanoid_mujoco_amd as hb
    import cmd_lib
    lines = ["velocity commands: the env kernel's reward against tests/cmd_ref.py (fp64) on the device's own states, joint torques and actions",
             "humanoid27.hbm, 64 envs, reset_perturb 1, reset_quat_perturb 0.2 (yawed, tilted roots), root velocities of up to 1 m/s and 1 rad/s a component,",
             "4 steps of random actions in [-1, 1]; reward_kind 1 with w_vvel 1.5;",
             "commands: " + ", ".join("%s=%g" % kv for kv in cmd_lib.CMD.items() if kv[0] != "frame"), ""]
    res = cmd_lib.measure_parity(hb, args.gpu, log=lines.append)
    worst = max(r["cmd"] for r in res.values())
    plain = max(r["plain"] for r in res.values())
    lines += ["", "worst over the four cases: with commands %.3e, without commands (env_ref.py, same states) %.3e" % (worst, plain),
              "tests/test_gpu_cmd.py: PARITY_WORST = %.3e, asserted bound 8 x = %.3e" % (worst, 8 * worst)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
