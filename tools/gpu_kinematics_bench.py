#!/usr/bin/env python3
"""What the whole-body kinematics read-out costs (include/hb.h: hb_kinematics_dev, all three outputs) beside the passes that compute
the same poses on the way: 4096 and 32768 envs of the 27-dof humanoid and of the reference's robot, after 100 untimed steps of the
Halton workload from the perturbed reset.  Alternated in one process and timed with device events (hb_timer_*), every shape warmed up
first, K calls per window and REPS windows per figure (the median, minimum and maximum are printed):
  kin_pack 1 / 0   microseconds per hb_kinematics_dev call, calls enqueued back to back; the bytes one call moves (qpos and qvel in,
                   the three arrays out) and that figure over the call's time
  forward          microseconds per hb_forward call (a synchronous call: the host's turn-around between calls is inside the window)
  step             microseconds per hb_step_dev call, enqueued back to back (they fold into launches of several steps)
The read-out does a strict subset of a forward pass' work and must take less time than it: where it does not, the tool says so in
capitals and exits with status 1 after the last shape.
Results: profiles/kinematics_bench.txt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402

K, REPS, PRE = 200, 5, 100
slower = []
for asset in ("humanoid27.hbm", "team_robot.hbm"):
    m = hb.Model.load(os.path.join(ROOT, "humanoid_mujoco_amd", "assets", asset))
    for n in (4096, 32768):
        b = hb.Batch(m, n, 0)
        b.reset(perturb=True)
        b.rollout_halton(PRE)
        b.sync()
        ctrl = b.dev_alloc(n * m.nu * 4)
        b.halton_ctrl_dev(1, PRE, 0, ctrl)
        out = [b.dev_alloc(n * w * 4) for w in (m.nbody * 10, m.nbody * 6, m.ngeom * 7)]
        nbytes = 4 * n * (m.nq + m.nv + m.nbody * 16 + m.ngeom * 7)
        start = b.get_state(hb.STATE_INTEGRATION)

        def window(leg):
            b.set_state(hb.STATE_INTEGRATION, start)
            b.timer_start()
            for _ in range(K):
                if leg == "forward":
                    b.forward()
                elif leg == "step":
                    b.step_dev(ctrl)
                else:
                    b.kinematics_dev(*out)
            return b.timer_stop() * 1e3 / K

        legs = ("kin_pack 1", "kin_pack 0", "forward", "step")
        us = {leg: [] for leg in legs}
        kernels = {}
        for rep in range(REPS + 1):  # (the first round of windows warms every shape up and is not counted)
            for leg in legs:
                if leg.startswith("kin_pack"):
                    b.tune(kin_pack=int(leg[-1]))
                t = window(leg)
                kernels[leg] = b.last_kernel()
                if rep:
                    us[leg].append(t)
        print("%s, %d envs (nbody %d, ngeom %d): %d calls per window, %d windows" % (asset, n, m.nbody, m.ngeom, K, REPS))
        for leg in legs:
            med = float(np.median(us[leg]))
            extra = "   %.2f MB per call, %.0f GB/s" % (nbytes / 1e6, nbytes / med / 1e3) if leg.startswith("kin_pack") else ""
            print("  %-11s %9.2f us per call (min %.2f max %.2f) [%s]%s" % (leg, med, min(us[leg]), max(us[leg]), kernels[leg], extra), flush=True)
        kin = min(float(np.median(us["kin_pack 1"])), float(np.median(us["kin_pack 0"])))
        print("  read-out / forward = %.3f, read-out / step = %.3f; packing %s" % (kin / float(np.median(us["forward"])), kin / float(np.median(us["step"])),
              "faster" if np.median(us["kin_pack 1"]) < np.median(us["kin_pack 0"]) else "NOT faster"), flush=True)
        if max(float(np.median(us["kin_pack 1"])), float(np.median(us["kin_pack 0"]))) >= float(np.median(us["forward"])):  # (either form)
            slower.append("%s, %d envs" % (asset, n))
            print("  FAILED: THE READ-OUT IS NOT FASTER THAN hb_forward ON THIS BATCH", flush=True)
        b.tune(kin_pack=1)
        for p in out + [ctrl]:
            b.dev_free(p)
        b.close()
if slower:
    sys.exit("the read-out is not faster than hb_forward for: " + "; ".join(slower))
