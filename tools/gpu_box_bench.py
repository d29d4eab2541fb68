#!/usr/bin/env python3
"""Box geoms measured, on one MI355X:
  (1) the stairs model of tests/box_cases.py (four box steps, a box-footed biped, a brick: 8 boxes, 16 dofs) against its MESH TWIN (every
      box as the mesh of its eight corners) on the same build: microseconds per hb_step_dev call of 4096 envs, calls enqueued back to
      back, PGS and Newton, after 100 untimed steps under small random motor commands.  The box model runs the closed-form support point
      and four-corner plane - box contacts, the twin the hull climb and plane - hull; nobody had measured which is faster.
  (2) a 17 x 11 height scan in the torso's heading frame over a flight of eight box steps and the floor (static geoms only), beside
      profiles/ray_bench.txt's figure for a height field.
Alternated in one process, timed with device events (hb_timer_*), K calls per window, REPS windows per figure after one warm-up round.
Results: profiles/box_bench.txt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import box_cases  # noqa: E402
import humanoid_mujoco_amd as hb  # noqa: E402

K, REPS, PRE, N = 100, 5, 100, 4096


def stepper(xml):
    m = hb.Model.from_xml_string(xml)
    b = hb.Batch(m, N, 0)
    b.reset(perturb=True)
    ctrl_h = (0.3 * np.random.default_rng(0).uniform(-1, 1, (N, m.nu))).astype(np.float32)
    ctrl = b.dev_alloc(ctrl_h.nbytes)
    b.to_dev(ctrl, ctrl_h)
    for _ in range(PRE):
        b.step_dev(ctrl)
    b.sync()
    start = b.get_state(hb.STATE_INTEGRATION)

    def window():
        b.set_state(hb.STATE_INTEGRATION, start)
        b.timer_start()
        for _ in range(K):
            b.step_dev(ctrl)
        return b.timer_stop() * 1e3 / K
    return m, b, window


for solver in ("PGS", "Newton"):
    legs = {"box": stepper(box_cases.stairs_xml(False, solver)), "mesh twin": stepper(box_cases.stairs_xml(True, solver))}
    us = {k: [] for k in legs}
    for rep in range(REPS + 1):
        for k, (m, b, window) in legs.items():
            t = window()
            if rep:
                us[k].append(t)
    print("stairs model, %s, %d envs: %d calls per window, %d windows" % (solver, N, K, REPS))
    for k, (m, b, window) in legs.items():
        nc = b.counts()[0]
        print("  %-10s %8.2f us per step (min %.2f max %.2f) [%s]  mean contacts %.2f, envs with warnings %d"
              % (k, np.median(us[k]), min(us[k]), max(us[k]), b.last_kernel(), float(nc.mean()), int((b.status() != 0).sum())))
    print("  box / mesh twin = %.3f" % (np.median(us["box"]) / np.median(us["mesh twin"])))
    for _, b, _ in legs.values():
        b.close()

m = hb.Model.from_xml_string(box_cases.stairs_xml(nsteps=8))
b = hb.Batch(m, N, 0)
b.reset(perturb=True)
xs, ys = np.linspace(-1.6, 1.6, 17) + 1.5, np.linspace(-1.0, 1.0, 11)
pnt, vec = hb.height_scan_rays(xs, ys, 1.0)
dist, gid = b.dev_alloc(N * len(pnt) * 4), b.dev_alloc(N * len(pnt) * 4)
us = {"scan (yaw)": [], "scan (world)": []}
for rep in range(REPS + 1):
    for leg in us:
        b.ray_configure(pnt, vec, frame="yaw" if "yaw" in leg else "world", frame_body=m.name2id("body", "torso"), static=True, moving=False, cutoff=4.0)
        b.timer_start()
        for _ in range(K):
            b.rays_dev(dist, gid)
        t = b.timer_stop() * 1e3 / K
        if rep:
            us[leg].append(t)
print("height scan over eight box steps and the floor, %d envs x %d rays (17 x 11), 9 eligible static geoms" % (N, len(pnt)))
for leg, v in us.items():
    print("  %-14s %6.2f us per call (min %.2f max %.2f) [%s]" % (leg, np.median(v), min(v), max(v), b.last_kernel()))
print("  (profiles/ray_bench.txt: 15.9 us (yaw) / 7.8 us (world) for the same grid over one height field)")
b.close()
