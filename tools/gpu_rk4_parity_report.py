#!/usr/bin/env python3
"""One-step parity of the RK4 kernels (fp32) against the fp64 reference tests/rk4_ref.py: median and maximum per quantity, for the 128
golden states under PGS/50 and Newton/100 and for the capsule chains of tests/test_gpu_rk4.py (the other kernels and sizes).  The one-step
bounds of tests/test_gpu_rk4.py are set from this report (at most 3 x the maximum).  Results: profiles/rk4_parity_report.txt."""
import os
import sys
import tempfile
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402
import rk4_ref  # noqa: E402
import test_gpu_rk4 as T  # noqa: E402

worst = {}
print("%-20s %-24s %-6s %10s %10s" % ("model", "kernel", "what", "median", "max"))


def report(name, m, o, st, ct):
    b = hb.Batch(m, len(st), 0)
    err, info = rk4_ref.device_one_step_errors(hb, b, o, st, ct)
    b.close()
    nc, ne = info["dev_counts"]
    mism = sum((nc[k], ne[k]) != rc[3][:2] for k, rc in enumerate(info["ref_counts"]))
    differ = sum(rc[3][:2] != rc[0][:2] for rc in info["ref_counts"])
    for k, v in err.items():
        print("%-20s %-24s %-6s %10.2e %10.2e" % (name, info["kernel"], k, np.median(v), v.max()))
        worst[k] = max(worst.get(k, 0.0), v.max())
    print("%-20s %d states; (ncon, nefc) differ from the reference's last stage in %d; the reference's last stage differs from its first in %d; "
          "status bits set in %d" % (name, len(st), mism, differ, int((info["status"] != 0).sum())))


with tempfile.TemporaryDirectory() as tmp:
    for name, solver, iterations in (("humanoid27_pgs", 0, 50), ("humanoid27_newton", 2, 100)):
        m, o = T._humanoid(hb, solver, iterations)
        report(name, m, o, *T._golden_states())
    for name in T.CHAINS:
        m, o, st, ct = T._rk4_chain(hb, name, Path(tmp))
        report(name, m, o, st, ct)
print("maximum over all models: " + "  ".join("%s %.2e" % kv for kv in worst.items()))
