#!/usr/bin/env python3
"""Per-step time of the equality kernels (hb_step.hip: the FRIC 2 rows of HB_KERNELS, hb_eq_*) against the kernels the SAME model takes
with <flag equality="disable"/>, 4096 envs, PGS/50 condim 3 and Newton/100 condim 1 on the nv = 28 chain of tests/eq_models.py (nine
equality rows - three joint couplings, two connects - on top of test_gpu_fric.py's eleven friction rows; disabled, it runs the
friction-loss kernels).  Both batches start from ONE state - the disabled model pre-rolled 300 untimed steps of the Halton workload
from the perturbed reset, onto the floor - and run 20 warm-up and 200 timed hb_step_dev calls under the same controls, pipelined as
bench.py steps.  Both are full kernels.  There is no target: a reported cost, measured against the disabled-flag run of the same
build.  Results: profiles/eq_bench.txt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402
from eq_models import eq_chain_xml  # noqa: E402

N, PRE, W, K = 4096, 300, 20, 200

for label, name in (("PGS/50 condim 3", "eq28_cd3_pgs"), ("Newton/100 condim 1", "eq28_cd1_newton")):
    start, res = None, {}
    for kind, model_xml in (("disabled", eq_chain_xml(name, flag="disable")), ("equality", eq_chain_xml(name))):
        m = hb.Model.from_xml_string(model_xml)
        b = hb.Batch(m, N, 0)
        if start is None:  # the window's start: the disabled model's pre-roll, for both
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
        res[kind] = (float(np.median(us)), min(us), max(us), b.last_kernel(), nc.mean(), ne.mean(), ni.mean(), int((b.status() != 0).sum()), m.equality_rows())
        b.dev_free(ctrl)
        b.close()
    for kind in ("disabled", "equality"):
        r = res[kind]
        print("%-20s %-8s %8.1f us per step (median of 3 windows of %d steps; min %.1f max %.1f) [%s]; last step: mean ncon %.2f, rows per env %.2f "
              "(%d of them equality rows), solver iterations %.2f; envs with a status bit %d" % (label, kind, r[0], K, r[1], r[2], r[3], r[4], r[5], r[8], r[6], r[7]), flush=True)
    print("%-20s equality / disabled = %.3f in time, %.3f in rows" % (label, res["equality"][0] / res["disabled"][0], res["equality"][5] / max(res["disabled"][5], 1e-9)), flush=True)
