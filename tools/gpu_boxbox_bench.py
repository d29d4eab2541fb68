#!/usr/bin/env python3
"""The box - box manifold measured, on one MI355X, on the stairs model of tests/box_cases.py at 4096 envs:
  (i)   mode OFF on this build against the PARENT commit (--parent DIR: a checkout of it with its library built): the off path of a box
        model must cost nothing.  Each window is a child process that imports the package of one tree, pre-rolls 100 steps and times K
        calls after one warm-up window; the two trees alternate, REPS windows each; the parent's own spread is the margin.
  (ii)  mode on against mode off on this build, alternated in one process, with the biped on the floor (the model as it is) and on the
        first step (both feet on a box): microseconds per hb_step_dev call, contacts and rows per env.
  (iii) the pose launch's own time with the mode on and off: `--pose MODE` steps the biped on the step 300 times (staged, PGS) and prints
        nothing; run it under `rocprofv3 --kernel-trace --stats`, once per mode, and read hb_pose_box_kernel's row.
Timed with device events (hb_timer_*), K calls per window.  Results: profiles/boxbox_bench.txt."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import box_cases  # noqa: E402

K, REPS, PRE, N = 100, 5, 100, 4096


def stairs(on_step, solver="PGS"):
    xml = box_cases.stairs_xml(False, solver)
    if on_step:
        assert xml.count('<body name="torso" pos="0 0 0.601">') == 1
        xml = xml.replace('<body name="torso" pos="0 0 0.601">', '<body name="torso" pos="0.42 0 %g">' % (0.601 + box_cases.STEP_RISE))
    return xml


def stepper(hb, xml, mode):
    m = hb.Model.from_xml_string(xml)
    if mode is not None:
        assert m.box_manifold(mode) == mode
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


def child(root, solver):
    """one window of the mode-off stairs model with the package of the tree `root` (the parent's has no setter: the model is left as it is)"""
    sys.path.insert(0, root)
    import humanoid_mujoco_amd as hb
    assert os.path.dirname(os.path.dirname(os.path.abspath(hb.__file__))) == os.path.abspath(root), hb.__file__
    m, b, window = stepper(hb, stairs(False, solver), None)
    window()
    print("%.4f %s" % (window(), b.last_kernel()))
    b.close()


def against_parent(parent):
    libs = {"parent": os.path.abspath(parent), "this build, mode off": ROOT}
    for solver in ("PGS", "Newton"):
        us, kernel = {k: [] for k in libs}, {}
        for rep in range(REPS + 1):
            for k, path in libs.items():
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, solver], stdout=subprocess.PIPE, text=True, timeout=300, check=True).stdout.split()
                kernel[k] = out[1]
                if rep:
                    us[k].append(float(out[0]))
        print("(i) stairs model, %s, %d envs, mode off: %d calls per window, %d windows per tree, one process per window, alternated" % (solver, N, K, REPS))
        for k in libs:
            print("  %-22s %8.2f us per step (min %.2f max %.2f) [%s]" % (k, np.median(us[k]), min(us[k]), max(us[k]), kernel[k]))
        spread = max(us["parent"]) - min(us["parent"])
        print("  this build - parent = %+.2f us (medians); the parent's own spread %.2f us" % (np.median(us["this build, mode off"]) - np.median(us["parent"]), spread))


def on_against_off():
    import humanoid_mujoco_amd as hb
    for where in ("floor", "step"):
        for solver in ("PGS", "Newton"):
            legs = {"mode off": stepper(hb, stairs(where == "step", solver), 0), "mode on": stepper(hb, stairs(where == "step", solver), 1)}
            us = {k: [] for k in legs}
            for rep in range(REPS + 1):
                for k, (m, b, window) in legs.items():
                    t = window()
                    if rep:
                        us[k].append(t)
            print("(ii) biped on the %s, %s, %d envs: %d calls per window, %d windows, alternated in one process" % (where, solver, N, K, REPS))
            for k, (m, b, window) in legs.items():
                nc, ne, _ = b.counts()
                print("  %-9s %8.2f us per step (min %.2f max %.2f) [%s]  contacts per env %.2f, rows per env %.2f, envs with warnings %d"
                      % (k, np.median(us[k]), min(us[k]), max(us[k]), b.last_kernel(), float(nc.mean()), float(ne.mean()), int((b.status() != 0).sum())))
            print("  on - off = %+.2f us%s" % (np.median(us["mode on"]) - np.median(us["mode off"]),
                                             "   (iii) no box - box pair in range here: the flag's own cost in the pose launch and the work lists" if where == "floor" else ""))
            for _, b, _ in legs.values():
                b.close()


def pose(mode):
    import humanoid_mujoco_amd as hb
    m, b, window = stepper(hb, stairs(True), mode)
    for _ in range(3):
        window()
    b.close()


if __name__ == "__main__":
    if "--pose" in sys.argv:
        pose(int(sys.argv[sys.argv.index("--pose") + 1]))
    elif "--child" in sys.argv:
        child(*sys.argv[sys.argv.index("--child") + 1:][:2])
    else:
        if "--parent" in sys.argv:
            against_parent(sys.argv[sys.argv.index("--parent") + 1])
        on_against_off()
