#!/usr/bin/env python3
"""What a terrain height scan costs (include/hb.h: hb_rays_dev) beside one step of the same batch: 4096 envs x a 17 x 11 grid of downward
rays in the torso's heading frame, geoms of the world body only (VecEnv's height scan), on humanoid27_hfield.hbm and team_robot.hbm, after
100 untimed steps of the Halton workload from the perturbed reset.  Alternated in one process and timed with device events (hb_timer_*),
every shape warmed up first, K calls per window and REPS windows per figure (the median, minimum and maximum are printed):
  scan (yaw)    microseconds per hb_rays_dev call, calls enqueued back to back: the kinematics read-out's launch for the torso pose, then
                the ray kernel
  scan (world)  the same rays as world-frame rays: the ray kernel alone (no pose is needed)
  body poses    hb_kinematics_dev for the body poses alone: what the yaw frame adds
  step          microseconds per hb_step_dev call, enqueued back to back.  The step kernels' translation units are not touched by the ray
                read-out (profiles/ray_kernel_resources.txt: every kernel's resources as before), so this is the parent commit's step.
Where a scan costs more than a step the tool says which of its two launches the time goes to.
Results: profiles/ray_bench.txt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402

K, REPS, PRE, N = 100, 5, 100, 4096
xs, ys = np.linspace(-1.6, 1.6, 17), np.linspace(-1.0, 1.0, 11)
pnt, vec = hb.height_scan_rays(xs, ys, 1.0)
for asset in ("humanoid27_hfield.hbm", "team_robot.hbm"):
    m = hb.Model.load(os.path.join(ROOT, "humanoid_mujoco_amd", "assets", asset))
    b = hb.Batch(m, N, 0)
    b.reset(perturb=True)
    b.rollout_halton(PRE)
    b.sync()
    ctrl = b.dev_alloc(N * m.nu * 4)
    b.halton_ctrl_dev(1, PRE, 0, ctrl)
    dist, gid, pose = b.dev_alloc(N * len(pnt) * 4), b.dev_alloc(N * len(pnt) * 4), b.dev_alloc(N * m.nbody * 10 * 4)
    start = b.get_state(hb.STATE_INTEGRATION)

    def window(leg):
        b.set_state(hb.STATE_INTEGRATION, start)
        if leg.startswith("scan"):
            b.ray_configure(pnt, vec, frame="yaw" if "yaw" in leg else "world", frame_body=1, static=True, moving=False, cutoff=4.0)
        b.timer_start()
        for _ in range(K):
            if leg == "step":
                b.step_dev(ctrl)
            elif leg == "body poses":
                b.kinematics_dev(pose, None, None)
            else:
                b.rays_dev(dist, gid)
        return b.timer_stop() * 1e3 / K

    legs = ("scan (yaw)", "scan (world)", "body poses", "step")
    us, kernels = {leg: [] for leg in legs}, {}
    for rep in range(REPS + 1):  # (the first round of windows warms every shape up and is not counted)
        for leg in legs:
            t = window(leg)
            kernels[leg] = b.last_kernel()
            if rep:
                us[leg].append(t)
    hits = float((b.from_dev(gid, (N, len(pnt)), np.int32) >= 0).mean())
    print("%s, %d envs x %d rays (%d x %d), %d eligible static geoms: %d calls per window, %d windows" % (asset, N, len(pnt), len(xs), len(ys),
          int((m.array("geom_bodyid") == 0).sum()), K, REPS))
    med = {leg: float(np.median(us[leg])) for leg in legs}
    for leg in legs:
        print("  %-13s %9.2f us per call (min %.2f max %.2f) [%s]" % (leg, med[leg], min(us[leg]), max(us[leg]), kernels[leg]), flush=True)
    print("  scan / step = %.3f; %.0f %% of the world-frame rays hit" % (med["scan (yaw)"] / med["step"], 100 * hits))
    if med["scan (yaw)"] > med["step"]:
        print("  A SCAN COSTS MORE THAN A STEP: the ray kernel takes %.2f us of it, the pose launch in front of it %.2f us" % (med["scan (world)"], med["scan (yaw)"] - med["scan (world)"]), flush=True)
    for p in (ctrl, dist, gid, pose):
        b.dev_free(p)
    b.close()
