#!/usr/bin/env python3
"""Per-step time of the RK4 kernels against the Euler full kernel of the same solver (include/hb.h: HB_INT_RK4) on the benchmark
humanoid, 4096 envs, PGS/50 and Newton/100, on bench.py's window: every env pre-rolled 600 untimed Euler steps of the Halton workload
from the perturbed reset, then 20 warm-up and 200 timed hb_step_dev calls from that same state for both integrators, pipelined as
bench.py steps.  The Euler batch is tuned to its full kernel (lean = 0, duo = 0): the RK4 kernels are full kernels.  An RK4 step is
four forward passes minus Euler's damped solve, so a ratio near 4 is expected; it is reported, not asserted.
Results: profiles/rk4_bench.txt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402

HBM = os.path.join(ROOT, "humanoid_mujoco_amd", "assets", "humanoid27.hbm")
N, PRE, W, K = 4096, 600, 20, 200

for label, solver, iterations in (("PGS/50", 0, 50), ("Newton/100", 2, 100)):
    start, res = None, {}
    for integrator in (hb.INT_EULER, hb.INT_RK4):
        m = hb.Model.load(HBM)
        m.set_opt(solver=solver, iterations=iterations, integrator=integrator)
        b = hb.Batch(m, N, 0)
        b.tune(lean=0, duo=0)
        if start is None:  # the window's start: the Euler pre-roll, for both
            b.reset(perturb=True)
            b.rollout_halton(PRE)
            b.sync()
            start = b.get_state(hb.STATE_INTEGRATION)
        ctrl = b.dev_alloc((W + K) * N * m.nu * 4)
        b.halton_ctrl_dev(W + K, PRE, 0, ctrl)
        stride = N * m.nu * 4
        b.pipeline(True)
        us = []
        for rep in range(3):
            b.set_state(hb.STATE_INTEGRATION, start)
            for t in range(W):
                b.step_dev(ctrl + t * stride)
            b.sync()
            b.timer_start()
            for t in range(W, W + K):
                b.step_dev(ctrl + t * stride)
            us.append(b.timer_stop() * 1e3 / K)
            b.sync()
        nc, ne, ni = b.counts()
        res[integrator] = (float(np.median(us)), min(us), max(us), b.last_kernel(), nc.mean(), ne.mean(), ni.mean(), int((b.status() != 0).sum()))
        b.dev_free(ctrl)
        b.close()
    for integrator, name in ((hb.INT_EULER, "Euler"), (hb.INT_RK4, "RK4")):
        r = res[integrator]
        print("%-10s %-5s %8.1f us per step (median of 3 windows of %d steps; min %.1f max %.1f) [%s]; last step: mean ncon %.2f nefc %.2f "
              "solver iterations %.2f%s; envs with a status bit %d" % (label, name, r[0], K, r[1], r[2], r[3], r[4], r[5], r[6],
                                                                        " (last stage)" if integrator else "", r[7]), flush=True)
    print("%-10s RK4 / Euler = %.2f" % (label, res[hb.INT_RK4][0] / res[hb.INT_EULER][0]), flush=True)
