#!/usr/bin/env python3
"""Parity of the whole-body kinematics read-out (include/hb.h: hb_kinematics) with the fp64 oracle, on the cases of
tests/test_gpu_kinematics.py (tests/kin_ref.py: CASES, 30 states each along an oracle rollout): per model the worst pose error (xpos,
xquat up to sign and its norm, xipos, geom_xpos, the geoms' orientation as matrices against geom_xmat) and the worst velocity error
(omega | v at xipos), each relative to max(1, max |reference|) of the state, and the kernel that ran.  The test's two bounds are 3 x the
maxima printed here.
Results: profiles/kinematics_parity.txt."""
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402
import kin_ref  # noqa: E402

tmp = pathlib.Path(tempfile.mkdtemp())
worst = [0.0, 0.0]
print("%-16s %5s %5s %-16s %6s %12s %12s" % ("model", "nbody", "ngeom", "kernel", "states", "pose", "velocity"))
for name in kin_ref.CASES:
    m, o, kernel, states = kin_ref.parity_case(hb, name, tmp)
    ref = kin_ref.references(o, states)
    b = hb.Batch(m, len(states), 0)
    b.set_state(hb.STATE_INTEGRATION, np.asarray(states))
    dev = b.kinematics(geoms=True)
    ran = b.last_kernel()
    b.close()
    err = np.array([kin_ref.errors(ref, dev, k) for k in range(len(states))])
    worst = [max(worst[0], err[:, 0].max()), max(worst[1], err[:, 1].max())]
    print("%-16s %5d %5d %-16s %6d %12.3e %12.3e%s" % (name, m.nbody, m.ngeom, ran, len(states), err[:, 0].max(), err[:, 1].max(), "" if ran == kernel else "   EXPECTED " + kernel), flush=True)
print("maximum: pose %.3e, velocity %.3e; 3 x: %.3e, %.3e (the bounds may not exceed 1.8e-6)" % (worst[0], worst[1], 3 * worst[0], 3 * worst[1]))
