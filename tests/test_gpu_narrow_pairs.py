"""The primitive colliders (plane_sphere, sphere_sphere, capsule_capsule of hb_kcommon.hpp) held to the fp64 oracle PAIR BY PAIR, through
every copy of their dispatch: hb_step.hip (the classic PGS and Newton kernels) and hb_collide.hpp's eval_work_item (the fused general
kernels, the staged narrowphase of hb_narrow.hip with narrow_prim 1 and 0).  One env is one case of tests/pair_cases.py, one launch
evaluates the whole table, one step; every row asserts the kernel it ran.  (The duo kernel is specialised to the humanoid and cannot run
this scene; it shares the helpers and is held bit for bit to the one-env kernel by tests/test_gpu_duo*.py.)

Rows with contact records (diagnostics on), per case against the oracle from the same fp32-rounded state:
  - the count is identical: an EXACT case (bitwise equal operands: parallel capsules with one quaternion bit pattern, coincident centres,
    a centre on an axis) must match the unperturbed oracle; an ill-conditioned case (tests/test_pair_cases_cpu.py: its perturbed oracle
    evaluations disagree on the count) may match the count of any of them; ncon and nefc;
  - geom ids and dim identical; the frame orthonormal to 1e-5, its first row the normal;
  - dist, pos and normal within BASE + K * envelope.  BASE is the project's measured contact bounds (bounds.CONVEX_TOL: dist 5e-7, pos
    3e-6, normal 3e-5).  The envelope is the oracle's own spread under one fp32 rounding of qpos (32 draws of 2^-24 max(1, |qpos|) N(0, 1)).
    K = 4, from the roundings between qpos and a geom's world axis (hb_kinematics.hpp geom_world_pose / quat_zaxis, hb_kcommon.hpp
    qnormalize): a body's position is copied and the geoms sit at the body's origin, so only the quaternion rounds.  Each component is
    rounded once by the normalisation's multiply (the common scale error of n2 and rsqrt changes |axis|, not its direction: 1e-6 of a
    0.2 m half-length, inside BASE), the product with the geom's identity quaternion is exact, and quat_zaxis adds at most four roundings
    of O(1) terms to a component, each worth half a rounding of a quaternion component (the axis is quadratic in it): three input
    roundings per body, all aligned in the worst case, six for a pair.  The envelope is the largest of 32 Gaussian draws over both
    bodies' components: in one direction it reaches 1.5 sigma sqrt(2) = 2.1 roundings or more.  6 / 2.1 = 2.8, rounded up to 4.
    An exact case has no envelope: BASE alone.
The worst measured / bound per pair type is printed, and appended to the file HB_PAIR_PARITY_OUT names (profiles/narrow_pairs_parity.txt
holds the MI355X figures).  A ratio above 1 is a failure.

Rows without contact records (the lean launch of the classic families; the staged step, narrow_prim 1 and 0): counts() under the same
rule, the state after the step within bounds.BOUNDS of the oracle's step, the two narrow_prim settings bit for bit.
"""
import collections

import numpy as np
import pytest

from bounds import BOUNDS, CONVEX_TOL as TOL
from kernel_models import kernel_table
from oracle_lib import load_state
from pair_cases import held_to, launch, reference, state_of
from step_lib import report

pytestmark = pytest.mark.gpu

K = 4.0
BASE = np.array([TOL["dist"], TOL["pos"], TOL["nrm"]])


def _big_newton_kernel(nv):
    """the big-kernel Newton row of hb_step.hip's table whose dense order holds nv dofs"""
    rows = [(int(c["NDENSE"]), n) for n, c in kernel_table() if c["SOLVER"] == "2" and c["NG"] == "kBigGroups" and int(c["NDENSE"]) >= nv
            and all(c[k] == "0" for k in ("DEFER", "LEAN", "SIZED", "INV", "INTEG", "ACC", "FRIC"))]
    return min(rows)[1]


#       id                  scene         knobs            diagnostics  kernel
ROWS = [("pgs",             "pgs",        {},              True,  "hb_step_kernel"),
        ("newton",          "newton",     {},              True,  "hb_step_newton28_kernel"),
        ("hfield",          "hfield",     {},              True,  "hb_step_gen_fast_kernel"),
        ("hfield-fused",    "hfield",     {"staged": 0},   True,  "hb_step_gen_kernel"),
        ("newton_cd6",      "newton_cd6", {},              True,  None),  # (the table's big Newton kernel for 24 dofs)
        ("pgs-lean",        "pgs",        {},              False, "hb_step_lean_kernel"),
        ("newton-lean",     "newton",     {},              False, "hb_step_newton28_lean_kernel"),
        ("hfield-staged",   "hfield",     "narrow_prim",   False, "hb_step_gen_fast_lean_kernel"),
        ("newton_cd6-staged", "newton_cd6", "narrow_prim", False, "hb_step_newton_gen28_kernel")]


def _report(label, worst):
    lines = ["%-18s %-4s worst measured / bound: dist %.3f pos %.3f normal %.3f   (%d contacts)" % ((label, k) + tuple(w[:3]) + (int(w[3]),)) for k, w in sorted(worst.items())]
    report(lines, "HB_PAIR_PARITY_OUT", lead="\n")


def _check_contacts(ref, got, label):
    nc, ne, _ = got["counts"]
    worst = collections.defaultdict(lambda: np.zeros(4))
    bad = []
    for i, c in enumerate(ref["cases"]):
        held = held_to(ref, i, int(nc[i]), int(ne[i]), bad, "oracle")
        if held is None:
            continue
        ev, env = held
        key = "-".join("f" if n == "floor" else n for n in c["pair"])
        for k, want in enumerate(ev["con"]):
            d = got["con"][i, k]
            assert (int(d[14]), int(d[15]), int(d[13])) == (want["geom1"], want["geom2"], want["dim"]), (label, c["name"], k, d[13:16])
            frame = d[4:13].reshape(3, 3)
            if np.abs(frame @ frame.T - np.eye(3)).max() > 1e-5:
                bad.append((c["name"], k, "frame not orthonormal", frame.round(4).tolist()))
            err = np.array([abs(d[0] - want["dist"]), np.abs(d[1:4] - want["pos"]).max(), np.abs(frame[0] - want["frame"][0]).max()])
            ratio = err / (BASE + K * env[k])
            worst[key] = np.append(np.maximum(worst[key][:3], ratio), worst[key][3] + 1)
            if ratio.max() > 1:
                bad.append((c["name"], k, ["%.2e" % x for x in err], ["%.2e" % x for x in BASE + K * env[k]]))
    _report(label, worst)
    print("".join("\n  %s: %s" % (label, x) for x in bad))
    assert not bad, (label, len(bad), bad[:3])


def _check_state(ref, got, label):
    """counts under the rule of the contact rows; qpos and qvel against the oracle's step from the state the counts are held to"""
    o = ref["oracle"]
    nc, ne, _ = got["counts"]
    wq = wv = 0.0
    bad = []
    for i, c in enumerate(ref["cases"]):
        held = held_to(ref, i, int(nc[i]), int(ne[i]), bad, "oracle")
        if held is None:
            continue
        load_state(o, state_of(o, held[0]["qpos"]), np.zeros(o.nu))
        o.step()
        dq = (np.abs(got["qpos"][i] - o.qpos) / np.maximum(1.0, np.abs(o.qpos))).max()
        dv = np.abs(got["qvel"][i] - o.qvel).max() / max(1.0, np.abs(o.qvel).max())
        if dq > BOUNDS["qpos"] or dv > BOUNDS["qvel"]:
            bad.append((c["name"], "qpos %.2e qvel %.2e" % (dq, dv)))
        wq, wv = max(wq, dq), max(wv, dv)
    print("\n%-18s state after the step: worst qpos %.2e (bound %.0e) qvel %.2e (bound %.0e)" % (label, wq, BOUNDS["qpos"], wv, BOUNDS["qvel"]))
    print("".join("\n  %s: %s" % (label, x) for x in bad))
    assert not bad, (label, len(bad), bad[:3])


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_narrow_pairs(hbmod, gpu, tmp_path_factory, row):
    label, scene, knobs, diag, kernel = row
    ref = reference(hbmod, scene, tmp_path_factory.mktemp("pairs"))
    kernel = kernel or _big_newton_kernel(ref["model"].nv)
    if knobs == "narrow_prim":
        got = [launch(hbmod, gpu, ref, {"narrow_prim": prim}, False) for prim in (1, 0)]
        for g in got:
            assert g["kernel"] == kernel, (label, g["kernel"], kernel)
        assert np.array_equal(got[0]["state"], got[1]["state"]) and np.array_equal(got[0]["status"], got[1]["status"]), label
        assert all(np.array_equal(a, b) for a, b in zip(got[0]["counts"], got[1]["counts"])), label
        got = got[0]
    else:
        got = launch(hbmod, gpu, ref, knobs, diag)
        assert got["kernel"] == kernel, (label, got["kernel"], kernel)
    assert not got["status"].any(), (label, got["status"])
    assert got["counts"][0].max() == 2 and (got["counts"][0] == 0).sum() >= 10
    if diag:
        _check_contacts(ref, got, label)
    else:
        _check_state(ref, got, label)
