"""The harness of the step-kernel tests: what a launch left behind (result, everything, snapshot) and the comparisons bit for bit (same,
same_dict); one diagnostic step (diag_step) and its comparison with the fp64 oracle under the golden bounds (vs_oracle,
state_vs_oracle); the chain specs and the expected-kernel tables that a CPU test holds to hb_step.hip; and report, which prints a
measured line and collects it for profiles/.

TEST INFRASTRUCTURE: the product package never imports this module.  It sits above oracle_lib, kernel_models and bounds and imports
no test file.
"""
import os
import re

import numpy as np

from bounds import BOUNDS
from kernel_models import kernel_table
from oracle_lib import CSRC, load_state, prove_rounding_fence

T = 5  # steps of the multi-step launches

# ---- the generated chains of the kernel matrix: name -> (nv, free base, floor, condim, solver), the arguments of kernel_models.chain_xml
CHAINS = {}
for _nv in (20, 21, 28, 29, 31, 32):
    CHAINS["chain%d_cd3_pgs" % _nv] = (_nv, True, "plane", 3, "PGS")
    CHAINS["chain%d_cd1_newton" % _nv] = (_nv, True, "plane", 1, "Newton")
for _nv in (28, 32):
    CHAINS["chain%d_cd1_pgs" % _nv] = (_nv, True, "plane", 1, "PGS")
    CHAINS["chain%d_cd3_newton" % _nv] = (_nv, True, "plane", 3, "Newton")
CHAINS["chain28_fixed_cd3_pgs"] = (28, False, "plane", 3, "PGS")
CHAINS["chain28_fixed_cd1_newton"] = (28, False, "plane", 1, "Newton")
for _nv in (20, 21, 28):
    CHAINS["chain%d_cd6_newton" % _nv] = (_nv, True, "plane", 6, "Newton")
for _nv in (21, 28):
    CHAINS["chain%d_cd4_pgs" % _nv] = (_nv, True, "plane", 4, "PGS")
    CHAINS["chain%d_cd6_pgs" % _nv] = (_nv, True, "plane", 6, "PGS")
    CHAINS["chain%d_hfield_pgs" % _nv] = (_nv, True, "hfield", 3, "PGS")

# ---- kernels outside the step-kernel matrix, by the model that must run them (Batch.last_kernel): the GPU tests run them, and a CPU
# test holds each table to hb_step.hip's (tests/test_rk4_cpu.py, tests/test_acc_ref_cpu.py)
RK4_KERNELS = {"humanoid27_pgs": "hb_rk4_kernel", "humanoid27_newton": "hb_rk4_newton28_kernel",
               "chain28_cd3_pgs": "hb_rk4_kernel", "chain32_cd3_pgs": "hb_rk4_32_kernel",
               "chain28_cd1_newton": "hb_rk4_newton28_kernel", "chain32_cd1_newton": "hb_rk4_newton32_kernel"}
# (a launch that carries the body-acceleration read-out runs the full kernel's twin with the read-out: hb_acc_* for hb_step_*,
# hb_acc_rk4_* for hb_rk4_*)
ACC_KERNELS = {"humanoid27_pgs": ("hb_acc_kernel",), "humanoid27_newton": ("hb_acc_newton28_kernel",), "humanoid27_pgs_unsized": ("hb_acc_kernel",),
               "chain12_cd4": ("hb_acc_gen_big_kernel", "hb_acc_gen_fast1_kernel"), "chain12_cd6": ("hb_acc_gen_big_kernel", "hb_acc_gen_fast1_kernel"),
               "chain12_hfield": ("hb_acc_gen_kernel", "hb_acc_gen_fast_kernel"), "team_robot": ("hb_acc_newton_big20_kernel", "hb_acc_newton_gen20_kernel")}
ACC_RK4_KERNELS = {"humanoid27_pgs": "hb_acc_rk4_kernel", "humanoid27_newton": "hb_acc_rk4_newton28_kernel"}


def kernel_names_in_source():
    names = {n for n, _ in kernel_table() if re.fullmatch(r"hb_step\w*_kernel", n)}  # rows of hb_step.hip's kernel table
    for f in ("hb_step.hip", "hb_step_duo.hip"):
        src = open(os.path.join(CSRC, f)).read()
        names |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(hb_step\w*_kernel)\s*\(", src))  # defined by hand (the duo kernels)
    return names


# ---------------------------------------------------------------------------------------------------------------- what a launch left
def result(hbmod, b):
    """(state, counts, status) of a batch"""
    return b.get_state(hbmod.STATE_INTEGRATION), b.counts(), b.status()


def same(x, y, label):
    """two results bit for bit"""
    assert np.array_equal(x[0], y[0]), (label, "state", np.abs(x[0] - y[0]).max())
    for u, w in zip(x[1], y[1]):
        assert np.array_equal(u, w), (label, "counts")
    assert np.array_equal(x[2], y[2]), (label, "status")


def everything(hbmod, b):
    """result, flat: (state, ncon, nefc, niter, status) - for the tests that compare element by element or index into it"""
    state, counts, status = result(hbmod, b)
    return (state,) + tuple(counts) + (status,)


def same_dict(a, b, label):
    """two dicts of arrays (a read-out's outputs): the same keys, shapes and bits"""
    assert a.keys() == b.keys(), label
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (label, k)


def snapshot(hbmod, b, extra=()):
    """what a read-out must leave untouched: state, status, counts, the step launches counted, and whatever else the caller lists"""
    return [b.get_state(hbmod.STATE_INTEGRATION), b.status()] + list(b.counts()) + [np.array(b.step_launches())] + list(extra)


def report(lines, env_var, lead="\n  "):
    """prints a measured line (or a list of lines) behind `lead` and appends it to the file that the environment variable names, if it
    is set: the files under profiles/ are collected this way"""
    text = lines if isinstance(lines, str) else "\n".join(lines)
    print(lead + text)
    out = os.environ.get(env_var)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


# ---------------------------------------------------------------------------------------------------------------- one diagnostic step
def diag_step(hb, m, st, ct, gpu, readout=False):
    """one step of a fresh batch from the states with the diagnostic outputs on (readout: and the contact-force read-out): everything
    it left, as float64 where it is compared with a reference, and its result"""
    b = hb.Batch(m, len(st), gpu)
    b.diag_enable(True)
    if readout:
        b.contact_readout(True)
    b.set_state(hb.STATE_INTEGRATION, st)
    b.step(ct)
    nc, ne, ni = b.counts()
    out = dict(qpos=b.qpos.astype(np.float64), qvel=b.qvel.astype(np.float64), qacc=b.qacc().astype(np.float64), force=b.efc_force().astype(np.float64),
               con=b.contacts().astype(np.float64), ncon=nc, nefc=ne, niter=ni, status=b.status(), kernel=b.last_kernel(), result=result(hb, b))
    if readout:
        out["cf"], out["bc"] = b.contact_force().astype(np.float64), b.body_contact().astype(np.float64)
    b.close()
    return out


def _contacts_ok(o, con, nc, ne):
    """the oracle's contacts (after forward) against one env's device records: None if counts, geoms or dims differ, else the worst
    (dist, pos, frame) deviations"""
    if (o.ncon, o.nefc) != (nc, ne):
        return None
    w = np.zeros(3)
    for i, c in enumerate(o.contacts()):
        if (int(con[i, 14]), int(con[i, 15])) != (c["geom1"], c["geom2"]):
            return None
        w = np.maximum(w, (abs(con[i, 0] - c["dist"]), np.abs(con[i, 1:4] - c["pos"]).max(), np.abs(con[i, 4:13] - c["frame"].reshape(-1)).max()))
    return w


def vs_oracle(hbmod, b, o, st, ct, fences_ok, label, before=None):
    """one diag step of batch b from the states against the oracle from the same states; returns the worst deviations.  before(k), if
    given, is called ahead of env k's oracle step (tests/test_gpu_domain_params.py: it writes env k's model parameters into the oracle)"""
    b.diag_enable(True)
    b.set_state(hbmod.STATE_INTEGRATION, st)
    b.step(ct)
    q, v, a = b.qpos.astype(np.float64), b.qvel.astype(np.float64), b.qacc().astype(np.float64)
    f, con = b.efc_force().astype(np.float64), b.contacts().astype(np.float64)
    nc, ne, ni = b.counts()
    b.diag_enable(False)
    assert not b.status().any(), (label, b.status())
    worst = dict(qpos=0.0, qvel=0.0, qacc=0.0, force=0.0, dist=0.0, pos=0.0, frame=0.0)
    fences = 0
    pgs = o.opt("solver") != 2
    for k in range(len(st)):
        if before is not None:
            before(k)
        load_state(o, st[k], ct[k].astype(np.float64))
        o.forward()
        w = _contacts_ok(o, con[k], nc[k], ne[k])
        on_fence = w is None and fences_ok
        if on_fence:
            got = {}

            def accept(oo):
                oo.forward()
                got["w"] = _contacts_ok(oo, con[k], nc[k], ne[k])
                return got["w"] is not None
            assert prove_rounding_fence(o, st[k], ct[k].astype(np.float64), accept, seed=k) is not None, (label, k, "contacts differ, no fence proof")
            w = got["w"]
            fences += 1
        assert w is not None, (label, k, "counts / contacts differ", (nc[k], ne[k]), (o.ncon, o.nefc))
        if pgs and ne[k]:
            assert ni[k] == o.dint("solver_niter"), (label, k, ni[k], o.dint("solver_niter"))
        worst["dist"], worst["pos"], worst["frame"] = max(worst["dist"], w[0]), max(worst["pos"], w[1]), max(worst["frame"], w[2])
        worst["qacc"] = max(worst["qacc"], np.abs(a[k] - o.qacc).max() / max(1.0, np.abs(o.qacc).max()))
        if o.nefc:
            fo = o.efc_force[:o.nefc]
            worst["force"] = max(worst["force"], np.abs(f[k, :o.nefc] - fo).max() / max(1.0, np.abs(fo).max()))
        o.step()
        if not on_fence:  # (the neighbouring state differs from the device's in qpos by construction)
            worst["qpos"] = max(worst["qpos"], (np.abs(q[k] - o.qpos) / np.maximum(1.0, np.abs(o.qpos))).max())
        worst["qvel"] = max(worst["qvel"], np.abs(v[k] - o.qvel).max() / max(1.0, np.abs(o.qvel).max()))
    print("  %-48s worst %s, %d states on a proved rounding fence" % (label, " ".join("%s %.2e" % kv for kv in worst.items()), fences))
    assert fences <= max(1, 0.05 * len(st)), (label, fences)
    for key, x in worst.items():
        assert x <= BOUNDS[key], (label, key, x, BOUNDS[key])
    return worst


def state_vs_oracle(hbmod, b, o, st, ct, fences_ok, label, before=None):
    """the state a one-step launch of batch b left (no diagnostic outputs) against the oracle's step from the same states: counts and
    PGS sweep counts identical, qpos and qvel within the golden bounds"""
    q, v = b.qpos.astype(np.float64), b.qvel.astype(np.float64)
    nc, ne, ni = b.counts()
    assert not b.status().any(), (label, b.status())
    worst = dict(qpos=0.0, qvel=0.0)
    fences = 0
    pgs = o.opt("solver") != 2
    for k in range(len(st)):
        if before is not None:
            before(k)
        load_state(o, st[k], ct[k].astype(np.float64))
        o.forward()
        on_fence = (o.ncon, o.nefc) != (nc[k], ne[k])
        if on_fence:
            assert fences_ok, (label, k, "counts differ", (nc[k], ne[k]), (o.ncon, o.nefc))

            def accept(oo):
                oo.forward()
                return (oo.ncon, oo.nefc) == (nc[k], ne[k])
            assert prove_rounding_fence(o, st[k], ct[k].astype(np.float64), accept, seed=k) is not None, (label, k, "counts differ, no fence proof")
            fences += 1
        if pgs and ne[k]:
            assert ni[k] == o.dint("solver_niter"), (label, k, ni[k], o.dint("solver_niter"))
        o.step()
        if not on_fence:
            worst["qpos"] = max(worst["qpos"], (np.abs(q[k] - o.qpos) / np.maximum(1.0, np.abs(o.qpos))).max())
        worst["qvel"] = max(worst["qvel"], np.abs(v[k] - o.qvel).max() / max(1.0, np.abs(o.qvel).max()))
    print("  %-48s worst %s, %d states on a proved rounding fence" % (label, " ".join("%s %.2e" % kv for kv in worst.items()), fences))
    assert fences <= max(1, 0.05 * len(st)), (label, fences)
    for key, x in worst.items():
        assert x <= BOUNDS[key], (label, key, x, BOUNDS[key])
    return worst
