#!/usr/bin/env python3
"""Parity of the dynamics read-out (include/hb.h: hb_dynamics) with the fp64 oracle, on the cases of tests/test_gpu_dynamics.py
(tests/kin_ref.py: CASES, 30 states each along an oracle rollout; sixteen Jacobian points per model, tests/dyn_ref.py: default_points):
per model and quantity (M, qfrc_bias, qfrc_passive, the Jacobians) the worst error relative to max(1, max |reference|) of the quantity in
the state, and the kernel that ran.  The test's bounds are 3 x the maxima printed here, rounded down.
Results: profiles/dynamics_parity.txt."""
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402
import dyn_ref  # noqa: E402
import kin_ref  # noqa: E402

QUANT = ("M", "bias", "passive", "jac")
tmp = pathlib.Path(tempfile.mkdtemp())
worst = dict.fromkeys(QUANT, 0.0)
print("%-16s %5s %3s %-16s %6s %12s %12s %12s %12s" % ("model", "nbody", "nv", "kernel", "states", "M", "qfrc_bias", "qfrc_passive", "jac"))
for name in kin_ref.CASES:
    m, o, kernel, states = dyn_ref.parity_case(hb, name, tmp)
    spec = m.jac_spec(**dyn_ref.default_points(hb, m))
    ref = dyn_ref.references(o, states, dyn_ref.spec_points(spec))
    b = hb.Batch(m, len(states), 0)
    b.set_state(hb.STATE_INTEGRATION, np.asarray(states))
    dev = b.dynamics(jac=spec)
    ran = b.last_kernel()
    b.close()
    err = {q: max(dyn_ref.errors(ref, dev, k)[q] for k in range(len(states))) for q in QUANT}
    for q in QUANT:
        worst[q] = max(worst[q], err[q])
    print("%-16s %5d %3d %-16s %6d %12.3e %12.3e %12.3e %12.3e%s" % (name, m.nbody, m.nv, ran, len(states), err["M"], err["bias"], err["passive"], err["jac"],
                                                                   "" if ran == kernel else "   EXPECTED " + kernel), flush=True)
print("maximum: " + ", ".join("%s %.3e" % (q, worst[q]) for q in QUANT))
print("3 x:     " + ", ".join("%s %.3e" % (q, 3 * worst[q]) for q in QUANT) + "   (a maximum above 4e-4, the forward pass's qacc bound, is a defect, not a bound)")
