#!/usr/bin/env python3
"""Body-acceleration read-out on the GPU against its fp64 reference (tests/acc_ref.py), per model and kernel: the maxima the bounds of
tests/test_gpu_body_acc.py are set from (at most 3 x the maximum measured here).
  decode: the device's read-out against the reference fed with the device's OWN qacc on the oracle's kinematics (what is left is the
          fp32 kinematics and the fp32 sum over the body's dofs); every state, none left out
  parity: against the reference on the oracle's qacc at the same state (carries the solver's fp32 error); states whose (ncon, nefc)
          differ from the oracle's are left out and counted
both relative to max(1, max |read-out|) of the state.  The last stage of an RK4 step is reported apart: its state is the device's own.
usage: gpu_body_acc_report.py [out.txt]   (default: profiles/body_acc_parity_report.txt)"""
import os
import sys
import tempfile
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import humanoid_mujoco_amd as hb  # noqa: E402
import acc_ref  # noqa: E402
import contact_ref  # noqa: E402
import rk4_ref  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "body_acc_parity_report.txt")
lines = ["%-34s %-30s %4s %8s | %9s %9s" % ("model", "kernel", "n", "left out", "decode", "parity")]
worst = {}


def report(name, dev, n, dec, par, left):
    vals = (float(dec.max()) if dec is not None else float("nan"), float(par.max()) if len(par) else float("nan"))
    for k, v in zip(("decode", "parity"), vals):
        if v == v:
            worst[k] = max(worst.get(k, 0.0), v)
    lines.append("%-34s %-30s %4d %8d | %9.2e %9.2e" % ((name, dev["kernel"], n, left) + vals))
    print(lines[-1], flush=True)


with tempfile.TemporaryDirectory() as tmp:
    for name in contact_ref.CASES:
        m, o, st, ct, tune = contact_ref.make_case(hb, name, Path(tmp))
        dev = acc_ref.device_readout(hb, m, st, ct, tune=tune)
        report(name, dev, len(st), *acc_ref.compare(o, st, ct, dev))
        if name in ("chain12_cd4", "chain12_cd6", "team_robot"):  # without the diagnostics the staged step runs its one-group fast pass first
            dev = acc_ref.device_readout(hb, m, st, ct, diag=False)
            report(name + " (fast pass)", dev, len(st), *acc_ref.compare(o, st, ct, dev))
    # The RK4 kernels.  A forward pass (hb_forward) is one pass of the kernel at the given state: the same two tiers as above.  After a
    # step the getter holds the LAST stage, whose state the device has reached through three fp32 stages of its own: against the
    # reference's own last stage the decode column then also carries that difference of the two stage states - a tier of its own.
    for name in ("humanoid27_pgs", "humanoid27_newton"):
        m, o, st, ct, _ = contact_ref.make_case(hb, name, Path(tmp))
        m.set_opt(integrator=hb.INT_RK4)
        dev = acc_ref.device_readout(hb, m, st, ct, forward=True)
        report(name + " rk4 forward", dev, len(st), *acc_ref.compare(o, st, ct, dev))
    lines.append("worst of the rows above: " + "  ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    print(lines[-1])
    worst.clear()
    for name in ("humanoid27_pgs", "humanoid27_newton"):
        m, o, st, ct, _ = contact_ref.make_case(hb, name, Path(tmp))
        m.set_opt(integrator=hb.INT_RK4)
        dev = acc_ref.device_readout(hb, m, st, ct)
        report(name + " rk4 last stage", dev, len(st), *acc_ref.compare(o, st, ct, dev, at_state=lambda oo, k: rk4_ref.rk4_step(oo, st[k], ct[k])))
lines.append("worst of the last stages: " + "  ".join("%s %.2e" % kv for kv in sorted(worst.items())))
print(lines[-1])
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
