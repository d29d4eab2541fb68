#!/usr/bin/env python3
"""What the body-acceleration read-out (include/hb.h: hb_body_acc_readout) costs on the benchmark humanoid: per-step time of the FULL
PGS/50 step kernel (lean = 0, duo = 0) at 4096 envs with the read-out off and on - on, the launch runs that kernel's twin with the read-out - on
bench.py's window - every env pre-rolled 600 untimed steps of the Halton workload from the perturbed reset, then 20 warm-up and 200 timed
hb_step_dev calls, pipelined as bench.py steps - repeated REPS times from the same state; median, minimum and maximum are printed, the
spread of the repeats being the yardstick for any difference.
With HB_TREE naming a built checkout of another commit (the parent's, which has no such read-out) that tree's package and library are
measured instead, and only the `off` leg runs: the same kernel before the epilogue was added.
Results: profiles/body_acc_bench.txt."""
import os
import sys

ROOT = os.environ.get("HB_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402

HBM = os.path.join(ROOT, "humanoid_mujoco_amd", "assets", "humanoid27.hbm")
N, PRE, W, K, REPS = 4096, 600, 20, 200, 7
has_readout = hasattr(hb.Batch, "body_acc_readout")
print("tree: %s (%s the read-out)" % ("another commit's" if os.environ.get("HB_TREE") else "this one", "with" if has_readout else "without"), flush=True)
m = hb.Model.load(HBM)
start = None
for on in ((False, True) if has_readout else (False,)):
    b = hb.Batch(m, N, 0)
    b.tune(lean=0, duo=0)
    if start is None:
        b.reset(perturb=True)
        b.rollout_halton(PRE)
        b.sync()
        start = b.get_state(hb.STATE_INTEGRATION)
    if on:
        b.body_acc_readout(True)
    ctrl = b.dev_alloc((W + K) * N * m.nu * 4)
    b.halton_ctrl_dev(W + K, PRE, 0, ctrl)
    stride = N * m.nu * 4
    b.pipeline(True)
    us = []
    for rep in range(REPS):
        b.set_state(hb.STATE_INTEGRATION, start)
        for t in range(W):
            b.step_dev(ctrl + t * stride)
        b.sync()
        b.timer_start()
        for t in range(W, W + K):
            b.step_dev(ctrl + t * stride)
        us.append(b.timer_stop() * 1e3 / K)
        b.sync()
    print("read-out %-3s %8.2f us per step (median of %d windows of %d steps; min %.2f max %.2f) [%s]; envs with a status bit %d"
          % ("on" if on else "off", float(np.median(us)), REPS, K, min(us), max(us), b.last_kernel(), int((b.status() != 0).sum())), flush=True)
    b.dev_free(ctrl)
    b.close()
