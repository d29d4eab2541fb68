"""The reward with foot-contact terms against tests/feet_ref.py in fp64, on the GPU: writes profiles/feet_parity.txt (or --out).

    python tools/gpu_feet_parity.py [--out PATH] [--gpu 0]

The landing scenario of tests/feet_lib.py in every case of feet_lib.CASES: 64 envs of the 27-dof humanoid, lifted by 0 to 5 cm (every
eighth laid flat), random actions; the reference - tests/env_ref.py or tests/cmd_ref.py for the base, tests/feet_ref.py for the contact
terms - is fed the device's own states, joint torques, actions and contact read-out.  Next to every figure: what a feet-less twin batch
stepped with the same actions shows against its reference on the same states.  tests/test_gpu_feet.py asserts four times the worst
figure written here, rounded up to one digit."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def round_up_one_digit(x):
    if x <= 0:
        return 0.0
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feet_parity.txt"))
    ap.add_argument("--gpu", type=int, default=0)
    args = ap.parse_args()
    import humanoid_mujoco_amd as hb
    import feet_lib
    lines = ["foot-contact terms: the env kernel's reward against tests/env_ref.py / tests/cmd_ref.py + tests/feet_ref.py (fp64) on the device's own states,",
             "joint torques, actions and contact read-out; humanoid27.hbm, 64 envs lifted by 0 to 5 cm, every eighth laid flat, random actions in [-0.6, 0.6];",
             "feet: " + ", ".join("%s=%g" % kv for kv in feet_lib.WEIGHTS.items()) + ", force_max = a quarter of the model's weight, air_cmd_min 0.5 where the gate is on", ""]
    res = feet_lib.measure_parity(hb, args.gpu, log=lines.append)
    worst = max(r["feet"] for r in res.values())
    plain = max(r["plain"] for r in res.values())
    scale = min(r["scale"] for r in res.values())
    bound = round_up_one_digit(4 * worst)
    lines += ["", "worst over the %d cases: with feet %.3e, the feet-less twin (same actions, same states) %.3e" % (len(res), worst, plain),
              "tests/test_gpu_feet.py: PARITY_WORST = %.3e, asserted bound 4 x, rounded up to one digit = %.0e; the smallest largest |reward| of a case is %.2f, 1e-4 of it %.1e"
              % (worst, bound, scale, 1e-4 * scale)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
