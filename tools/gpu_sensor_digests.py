#!/usr/bin/env python3
"""What the step kernels' sensor read-out and the task rollouts compute, as one SHA-256 per array: two checkouts whose kernels write the
same bits into the same places print the same lines.
  spec:    every part of a sensor row with uneven counts - 3 framepos (one with an offset), a tree, 2 axes (x and z), 1 framelinvel,
           2 subtreelinvel, 2 touch, 1 contact force, 2 accelerometer / gyro (one with an offset), 1 frame acceleration
  arrays:  64 envs, seeded controls throughout.
           hb_rollout_sensors rows of T = 8 steps and the states they end in, for humanoid27 under PGS, under Newton and with the RK4
           integrator, the team robot (a staged step: one launch chain per step) and a chain with joint friction loss (tests/fric_models.py
           over kernel_models.chain_xml; no kernel with the body-acceleration read-out: the spec without its last two parts);
           on humanoid27 under PGS also hb_sensors of the same spec, hb_transition_fd_sensors' A, B, C, D for one point (one-sided: 1 + 2 nv + nu
           = 76 envs, so a batch of 128), and the Stand and Walk task rollouts at H = 6 - totals, per-step costs and final states, from
           host controls and from a spline tape
The run is one child process under its own time limit, started once; --root DIR runs the package of another checkout (built) instead.
usage: gpu_sensor_digests.py [--root DIR] [--out FILE] [--beside FILE]
  --beside FILE: print the digests of an earlier run (its --out) next to this run's.  Fails if a line differs."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, H = 64, 8, 6
CHILD_LIMIT = 300  # seconds: the interpreter's start, eight small batches and a few steps each take a few
OFF = (0.05, 0.02, -0.03)


def full_spec(hb, feet, acc=True):
    a, b = feet
    return hb.Batch.sensor_spec(framepos_bodies=(1, a, b), offsets=[None, OFF, None], subtree_body=1, axes=((2, 0), (b, 2)), linvel_bodies=(a,),
                                subtreelinvel_bodies=(3, b), touch_bodies=(a, b), contactforce_bodies=(b,),
                                imu=((1, (0.0, 0.0, 0.0)), (a, OFF)) if acc else (), frameacc_bodies=(b,) if acc else ())


def child(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import numpy as np
    import humanoid_mujoco_amd as hb
    from fric_models import fric_chain_xml
    assets = os.path.join(root, "humanoid_mujoco_amd", "assets")
    out = []

    def humanoid(**opt):
        m = hb.Model.load(os.path.join(assets, "humanoid27.hbm"))
        if opt:
            m.set_opt(**opt)
        return m

    def fallen(m, n=N, keyframe=-1, settle=150):
        b = hb.Batch(m, n, 0)
        b.reset(keyframe=keyframe, perturb=True)
        if settle:
            b.rollout_halton(settle)  # (from the fallen state: contacts under the feet and the limbs)
        return b

    rng = np.random.default_rng(17)
    cases = [("humanoid27 PGS", humanoid(), (7, 10), True, -1, 150), ("humanoid27 Newton", humanoid(solver=2, iterations=100), (7, 10), True, -1, 150),
             ("humanoid27 RK4", humanoid(integrator=hb.INT_RK4), (7, 10), True, -1, 150),
             ("team robot", hb.Model.load(os.path.join(assets, "team_robot.hbm")), (14, 5), True, 0, 20),
             ("friction chain", hb.Model.from_xml_string(fric_chain_xml("fric28_cd3_pgs")), (4, 9), False, -1, 60)]
    for name, m, feet, acc, keyframe, settle in cases:
        b = fallen(m, keyframe=keyframe, settle=settle)
        spec = full_spec(hb, feet, acc)
        rows, _ = b.rollout_sensors(rng.uniform(-0.5, 0.5, (T, N, m.nu)).astype(np.float32), spec)
        assert rows.shape[2] == (53 if acc else 35) and not b.status().any(), name
        out += [(name + ": sensor rows", rows), (name + ": final states", b.get_state(hb.STATE_INTEGRATION)), (name + ": kernel " + b.last_kernel(), np.zeros(1, np.uint8))]
        if name == "humanoid27 PGS":
            out.append((name + ": hb_sensors", b.sensors(spec, rng.uniform(-0.5, 0.5, (N, m.nu)).astype(np.float32))))
            x = np.concatenate([b.qpos[:1], b.qvel[:1]], axis=1).astype(np.float64)
        b.close()
    m = cases[0][1]
    spec = full_spec(hb, (7, 10))
    b = hb.Batch(m, 128, 0)
    for k, a in zip("ABCD", b.transition_fd(x, rng.uniform(-0.5, 0.5, (1, m.nu)), centered=False, sensor_spec=spec)):
        out.append(("transition_fd " + k, a))
    b.close()
    ctrl = rng.uniform(-0.5, 0.5, (H - 1, N, m.nu)).astype(np.float32)
    knots, times = rng.uniform(-0.5, 0.5, (N, 3, m.nu)).astype(np.float32), np.array([0.0, 0.04, 0.08], np.float32)
    for task in ("stand", "walk"):
        for source in ("host controls", "spline tape"):
            b = fallen(m)
            run, spec_of = getattr(b, "rollout_task_" + task), getattr(b, "task_%s_default" % task)
            if source == "spline tape":
                b.ctrl_tape_splines(knots, times, 2, 0.0, H - 1)
            total, costs = run(ctrl if source == "host controls" else ("tape", H - 1), spec_of(), want_costs=True)
            label = "%s task, %s: " % (task, source)
            out += [(label + "totals", total), (label + "costs", costs), (label + "final states", b.get_state(hb.STATE_INTEGRATION))]
            b.close()
    for name, a in out:
        a = np.ascontiguousarray(a)
        assert a.size and not (a.dtype.kind == "f" and np.isnan(a).any()), name
        print("DIGEST %-52s %8d %-7s %s" % (name, a.size, a.dtype, hashlib.sha256(a.tobytes()).hexdigest()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out", default=None)
    ap.add_argument("--beside", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    if args.child:
        return child(root)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root], capture_output=True, text=True, timeout=CHILD_LIMIT)
    lines = [l[len("DIGEST "):] for l in r.stdout.splitlines() if l.startswith("DIGEST ")]
    if r.returncode != 0 or not lines:
        sys.exit("gpu_sensor_digests: the run ended with code %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.beside:
        other = open(args.beside).read().splitlines()
        differ = len(other) != len(lines)
        print("\n%-78s %-64s  %-64s" % ("array", args.beside, "this run (--root %s)" % args.root))
        for a, b in zip(other, lines):
            same = a == b
            differ |= not same
            print("%-78s %s  %s  %s" % (b[:-64].rstrip(), a.split()[-1], b.split()[-1], "equal" if same else "DIFFERS"))
        print("%d arrays, %s" % (len(lines), "a line DIFFERS" if differ else "every line equal"))
        sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
