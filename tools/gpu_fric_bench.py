#!/usr/bin/env python3
"""Per-step time of the friction-loss kernels (hb_step.hip: the FRIC rows of HB_KERNELS) against the full kernels of the same chain without the
joints' frictionloss, 4096 envs, PGS/50 condim 3 and Newton/100 condim 1 on the nv = 28 capsule chain of tests/kernel_models.py with
the friction attributes of tests/test_gpu_fric.py.  Both batches start from ONE state - the plain chain pre-rolled 300 untimed steps
of the Halton workload from the perturbed reset, onto the floor - and run 20 warm-up and 200 timed hb_step_dev calls under the same
controls, pipelined as bench.py steps.  The plain batch is tuned to its full kernel (lean = 0, duo = 0): the friction kernels are full
kernels.  The PGS sweep has the same instruction count per row, so the difference should be what the friction rows cost as rows and no
more: the rows per env are printed beside the times.  Reported, not asserted.  Results: profiles/fric_bench.txt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402
from kernel_models import chain_xml  # noqa: E402
from test_gpu_fric import add_friction  # noqa: E402

N, PRE, W, K = 4096, 300, 20, 200

for label, condim, solver in (("PGS/50 condim 3", 3, "PGS"), ("Newton/100 condim 1", 1, "Newton")):
    xml = chain_xml(28, condim=condim, solver=solver)
    start, res = None, {}
    for kind, model_xml in (("plain", xml), ("friction", add_friction(xml))):
        m = hb.Model.from_xml_string(model_xml)
        b = hb.Batch(m, N, 0)
        b.tune(lean=0, duo=0)
        if start is None:  # the window's start: the plain chain's pre-roll, for both
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
        nf = int((m.array("dof_frictionloss") > 0).sum())
        res[kind] = (float(np.median(us)), min(us), max(us), b.last_kernel(), nc.mean(), ne.mean(), ni.mean(), int((b.status() != 0).sum()), nf)
        b.dev_free(ctrl)
        b.close()
    for kind in ("plain", "friction"):
        r = res[kind]
        print("%-20s %-8s %8.1f us per step (median of 3 windows of %d steps; min %.1f max %.1f) [%s]; last step: mean ncon %.2f, rows per env %.2f "
              "(%d of them friction rows), solver iterations %.2f; envs with a status bit %d" % (label, kind, r[0], K, r[1], r[2], r[3], r[4], r[5], r[8], r[6], r[7]), flush=True)
    print("%-20s friction / plain = %.3f in time, %.3f in rows" % (label, res["friction"][0] / res["plain"][0], res["friction"][5] / max(res["plain"][5], 1e-9)), flush=True)
