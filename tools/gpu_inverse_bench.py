#!/usr/bin/env python3
"""Inverse dynamics against the forward pass (include/hb.h: hb_inverse_dev, hb_forward) at 4096 envs, for the 27-dof humanoid (classic
variant, PGS model) and the team robot (general variant: narrowphase launches + the 256-row kernel), and the reference's
set_mujoco_state height sweep (200 envs: keyframe, set_state, one hb_inverse) end to end.  Results: profiles/inverse_bench.txt.

hb_forward synchronises every call (and zeroes the controls first); hb_inverse_dev is timed both back to back and with a
synchronisation after every call, the like-for-like figure."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402

ASSETS = os.path.join(ROOT, "humanoid_mujoco_amd", "assets")
N, K = 4096, 50

for name, key, pre in (("humanoid27.hbm", -1, 150), ("team_robot.hbm", 0, 100)):
    m = hb.Model.load(os.path.join(ASSETS, name))
    b = hb.Batch(m, N, 0)
    b.reset(keyframe=key, perturb=key < 0)
    b.rollout_halton(pre)  # (into contact: the rows the inverse has to form)
    b.sync()
    b.forward()
    fwd_kernel = b.last_kernel()
    qd, od = b.dev_alloc(N * m.nv * 4), b.dev_alloc(N * m.nv * 4)
    b.to_dev(qd, np.random.default_rng(0).normal(size=(N, m.nv)).astype(np.float32))
    b.inverse_dev(qd, od)
    b.sync()
    inv_kernel = b.last_kernel()
    t = {}
    for rep in range(2):  # (the first round warms up)
        b.timer_start()
        for _ in range(K):
            b.forward()
        t["forward"] = b.timer_stop() * 1e3 / K
        b.timer_start()
        for _ in range(K):
            b.inverse_dev(qd, od)
        t["inverse"] = b.timer_stop() * 1e3 / K
        b.timer_start()
        for _ in range(K):
            b.inverse_dev(qd, od)
            b.sync()
        t["inverse_sync"] = b.timer_stop() * 1e3 / K
    nc, ne, _ = b.counts()
    print("%-15s %d envs (mean ncon %.1f, nefc %.1f): hb_forward %7.1f us per call [%s]; hb_inverse_dev %7.1f us back to back, %7.1f us "
          "synchronised per call [%s]" % (name, N, nc.mean(), ne.mean(), t["forward"], fwd_kernel, t["inverse"], t["inverse_sync"], inv_kernel),
          flush=True)
    b.dev_free(qd); b.dev_free(od)
    b.close()

# set_mujoco_state (controllers/mpc_utils.py:36-56): 200 root heights of a keyframe, qacc = 0, the vertical force picks the height
m = hb.Model.load(os.path.join(ASSETS, "humanoid27.hbm"))
n = 200
offsets = np.linspace(-0.001, 0.001, n)
b = hb.Batch(m, n, 0)
zero = np.zeros((n, m.nv), np.float32)
times = []
for rep in range(21):
    t0 = time.perf_counter()
    b.reset(keyframe=0)
    st = b.get_state(hb.STATE_INTEGRATION, dtype=np.float64)
    st[:, 3] += offsets
    st[:, 1 + m.nq:] = 0.0
    b.set_state(hb.STATE_INTEGRATION, st)
    best = offsets[np.argmin(np.abs(b.inverse(zero)[:, 2]))]
    times.append(time.perf_counter() - t0)
inv_t = []
for rep in range(21):
    t0 = time.perf_counter()
    b.inverse(zero)
    inv_t.append(time.perf_counter() - t0)
print("height sweep, %d envs [%s]: best offset %.3e; end to end (reset, get_state, set_state, hb_inverse) median %.1f us, the hb_inverse "
      "call alone median %.1f us" % (n, b.last_kernel(), best, 1e6 * np.median(times[1:]), 1e6 * np.median(inv_t[1:])))
b.close()
