#!/usr/bin/env python3
"""What the dynamics read-out costs (include/hb.h: hb_dynamics_dev): 4096 and 32768 envs of the 27-dof humanoid, after 100 untimed steps
of the Halton workload from the perturbed reset.  Timed with device events (hb_timer_*), every shape warmed up first, K calls enqueued
back to back per window and REPS windows per figure (the median, minimum and maximum are printed):
  all            M, qfrc_bias, qfrc_passive and sixteen Jacobians
  M only         the mass matrix alone
  16 jac only    sixteen Jacobians alone
with the bytes a call writes and that figure over the call's time as a fraction of the HBM bandwidth (HBM_GBS: 8000 GB/s, MI355X), and
  step           microseconds per hb_step_dev call of the same batch in the same run, enqueued back to back (they fold into launches of several steps)
Results: profiles/dynamics_bench.txt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402
import dyn_ref  # noqa: E402

K, REPS, PRE = 100, 5, 100
HBM_GBS = 8000.0
m = hb.Model.load(os.path.join(ROOT, "humanoid_mujoco_amd", "assets", "humanoid27.hbm"))
spec = m.jac_spec(**dyn_ref.default_points(hb, m))
nv = m.nv
for n in (4096, 32768):
    b = hb.Batch(m, n, 0)
    b.reset(perturb=True)
    b.rollout_halton(PRE)
    b.sync()
    ctrl = b.dev_alloc(n * m.nu * 4)
    b.halton_ctrl_dev(1, PRE, 0, ctrl)
    dM, db, dp, dj = (b.dev_alloc(n * w * 4) for w in (nv * nv, nv, nv, spec.n * 6 * nv))
    start = b.get_state(hb.STATE_INTEGRATION)
    legs = {"all": ((dM, db, dp, spec, dj), nv * nv + 2 * nv + spec.n * 6 * nv), "M only": ((dM, None, None, None, None), nv * nv),
            "16 jac only": ((None, None, None, spec, dj), spec.n * 6 * nv), "step": (None, 0)}

    def window(leg):
        b.set_state(hb.STATE_INTEGRATION, start)
        b.timer_start()
        for _ in range(K):
            if leg == "step":
                b.step_dev(ctrl)
            else:
                b.dynamics_dev(*legs[leg][0])
        return b.timer_stop() * 1e3 / K

    us = {leg: [] for leg in legs}
    kernels = {}
    for rep in range(REPS + 1):  # (the first round of windows warms every shape up and is not counted)
        for leg in legs:
            t = window(leg)
            kernels[leg] = b.last_kernel()
            if rep:
                us[leg].append(t)
    print("humanoid27.hbm, %d envs (nv %d, %d Jacobian points): %d calls per window, %d windows" % (n, nv, spec.n, K, REPS))
    step = float(np.median(us["step"]))
    for leg in legs:
        med = float(np.median(us[leg]))
        nbytes = 4 * n * legs[leg][1]
        extra = "   %.2f MB written per call, %.0f GB/s = %.1f %% of %.0f GB/s; %.2f x a step" % (nbytes / 1e6, nbytes / med / 1e3, 100 * nbytes / med / 1e3 / HBM_GBS, HBM_GBS, med / step) if nbytes else ""
        print("  %-12s %9.2f us per call (min %.2f max %.2f) [%s]%s" % (leg, med, min(us[leg]), max(us[leg]), kernels[leg], extra), flush=True)
    for p in (dM, db, dp, dj, ctrl):
        b.dev_free(p)
    b.close()
