#!/usr/bin/env python3
"""Contact-force read-out on the GPU against its fp64 reference (tests/contact_ref.py), per model, kernel and quantity: the maxima the
bounds of tests/test_gpu_contact_force.py are set from (at most 3 x the maximum measured here).
  decode_*: the device's read-out against the reference decode of the device's OWN efc_force and contacts (an fp32 sum of <= ~100 terms)
  parity_*: against the decode of the oracle's efc_force at the same state (carries the solver's fp32 error: rows held to 4e-4)
  _f: per-contact forces, _w: per-body wrenches; all relative to max(1, max |efc_force|) of the state.
usage: gpu_contact_force_report.py [out.txt]   (default: profiles/contact_force_parity_report.txt)"""
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import humanoid_mujoco_amd as hb  # noqa: E402
import contact_ref  # noqa: E402
import rk4_ref  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "contact_force_parity_report.txt")
lines = ["%-24s %-34s %4s %4s | %9s %9s %9s %9s" % ("model", "kernel", "n", "diff", "decode_f", "decode_w", "parity_f", "parity_w")]
worst = {}


def report(name, kernel, n, differ, err):
    vals = [float(err[k].max()) if k in err and len(err[k]) else float("nan") for k in ("decode_f", "decode_w", "parity_f", "parity_w")]
    for k, v in zip(("decode_f", "decode_w", "parity_f", "parity_w"), vals):
        if v == v:
            worst[k] = max(worst.get(k, 0.0), v)
    lines.append("%-24s %-34s %4d %4d | %9.2e %9.2e %9.2e %9.2e" % ((name, kernel, n, differ) + tuple(vals)))
    print(lines[-1], flush=True)


with tempfile.TemporaryDirectory() as tmp:
    for name in contact_ref.CASES:
        m, o, st, ct, tune = contact_ref.make_case(hb, name, Path(tmp))
        dev = contact_ref.device_readout(hb, m, st, ct, tune=tune)
        err, differ = contact_ref.compare(o, st, ct, dev)
        report(name, dev["kernel"], len(st), differ, err)
        if name in ("chain12_cd4", "chain12_cd6", "team_robot"):  # without the diagnostics the staged step runs its one-group fast pass first
            dev = contact_ref.device_readout(hb, m, st, ct, diag=False)
            err, differ = contact_ref.compare(o, st, ct, dev)
            report(name + " (fast pass)", dev["kernel"], len(st), differ, err)
    # RK4: the getters hold the last stage
    for name in ("humanoid27_pgs", "humanoid27_newton"):
        m, o, st, ct, _ = contact_ref.make_case(hb, name, Path(tmp))
        m.set_opt(integrator=hb.INT_RK4)
        dev = contact_ref.device_readout(hb, m, st, ct)
        rows, differ = [], 0
        for k in range(len(st)):
            rk4_ref.rk4_step(o, st[k], ct[k])  # leaves the oracle at the last stage
            r = contact_ref.compare_state(o, dev, k)
            if r is None:
                differ += 1
            else:
                rows.append(r)
        report(name + " rk4", dev["kernel"], len(st), differ, {key: np.array([r[key] for r in rows]) for key in rows[0]})
lines.append("worst: " + "  ".join("%s %.2e" % kv for kv in sorted(worst.items())))
print(lines[-1])
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
