"""Box geoms on the device, PAIR BY PAIR, through every copy of the general collision dispatch (hb_collide.hpp: eval_work_item): the fused
general kernels, the staged step's pose kernel (the analytic pairs plane - box and sphere - box) and its narrowphase kernels (the portal
search of capsule - box, box - box, box - mesh and height field - box; narrow_prim 1: the kernels without the hull climb, which a box
model without meshes takes).  A box model runs the kernels that carry the box colliders: hb_pose_box_kernel, hb_narrow*_box_kernel, and
where the step kernel collides itself the hb_box_* rows of hb_step.hip.  One env is one case of tests/box_cases.py, one launch evaluates the table, one step; every row asserts the
kernel it ran.

Rows with contact records (diagnostics on), per case against the reference from the same fp32-rounded state - box_ref for the analytic
pairs, the fp64 oracle on the MESH TWIN for the portal-search pairs (tests/box_cases.py: reference):
  - the count is identical, under the EXACT / ill-conditioned rule of tests/test_gpu_narrow_pairs.py; ncon and nefc;
  - geom ids and dim identical; the frame orthonormal to 1e-5, its first row the normal;
  - dist, pos and normal within BASE + K * envelope, BASE = bounds.CONVEX_TOL (dist 5e-7, pos 3e-6, normal 3e-5), the bounds that file
    holds hull pairs to.  K = 6, from the roundings between qpos and a box CORNER, counted as tests/test_gpu_narrow_pairs.py counts them for
    a capsule's axis, in units of one rounding of a quaternion component (which moves a corner at |h| from the centre by 2 |h| 2^-24): the
    normalisation rounds each component once (1); hb_kcommon.hpp q2mat forms an entry of the rotation from at most four rounded products
    and sums of O(1) terms, each worth half a unit (2); the corner R h is three products and two sums, each rounded relative to |h| and
    so worth half a unit (2.5): 5.5 per box, 11 for a pair of boxes when all align.  The envelope, the largest of 32 Gaussian draws over
    both bodies' components, reaches 2.1 units in one direction: 11 / 2.1 = 5.2, rounded up to 6.  (The centre's own rounding, one at
    1 - 2 m, is 1.2e-7 m: inside BASE.)  An exact case has no envelope: BASE alone.
  - the axis-aligned EXACT box - box cases: a box and its hull may pick different support corners on a flat face, so these are held to
    what is well defined: the normal and the depth (from the sizes alone) and a position inside the overlap region - over both faces,
    between the two surfaces.  NOT asserted: a position midway between the two surfaces.  The portal search does not give one, in the
    fp64 oracle either: W - P, surfaces at z = 4.142188 and 4.150000 (midway 4.146094), the oracle's contact on the twin at 4.142531, the
    device's at 4.142531.  The device agrees with the oracle on these cases in full (measured: dist 2e-7, pos 1e-7, normal 9e-7), so
    the position is held to the oracle's as well, with BASE.
Worst measured / bound per pair kind is printed and appended to the file HB_BOX_PARITY_OUT names (profiles/box_parity.txt).

The rows without contact records (the staged step; narrow_prim 1 and 0 bit for bit equal): counts() under the same rule, and for the
twin-agreement cases of plane - box and every portal-search case qpos / qvel after the step within bounds.BOUNDS of the
oracle's step on the twin.  Under Newton that is every twin-agreement case; under PGS, cut at 50 sweeps and therefore sensitive to the
ORDER of the contacts, those the twin's plane - hull collider lists in the box's corner order.
"""
import collections

import numpy as np
import pytest

import box_cases
from bounds import BOUNDS, CONVEX_TOL as TOL
from box_cases import ANALYTIC, reference, twin_agreement
from pair_cases import held_to, launch
from step_lib import report

pytestmark = pytest.mark.gpu

K = 6.0
BASE = np.array([TOL["dist"], TOL["pos"], TOL["nrm"]])

#       id              scene         knobs           diagnostics  kernel
ROWS = [("fused",       "pgs",        {"staged": 0},  True,  "hb_box_gen_kernel"),
        ("staged",      "pgs",        {},             True,  "hb_step_gen_fast_kernel"),
        ("mesh",        "mesh",       {},             True,  "hb_step_gen_fast_kernel"),
        ("newton_cd6",  "newton_cd6", {},             True,  "hb_box_newton_big28_kernel"),
        ("staged-prim", "pgs",        "narrow_prim",  False, "hb_step_gen_fast_lean_kernel"),
        ("mesh-lean",   "mesh",       {},             False, "hb_step_gen_fast_lean_kernel"),
        ("newton-prim", "newton_cd6", "narrow_prim",  False, "hb_step_newton_gen28_kernel"),
        # condim 6 under PGS (variant 3: the kPgsNefcMax-row family, a layout over 64 KB of LDS), and its body-acceleration twin
        ("pgs_cd6",     "pgs_cd6",    {},             True,  "hb_box_gen_big_kernel"),
        ("pgs_cd6-acc", "pgs_cd6",    {"body_acc": 1}, True, "hb_box_acc_gen_big_kernel"),
        ("pgs_cd6-prim", "pgs_cd6",   "narrow_prim",  False, "hb_step_gen_fast1_kernel"),
        # the other body order: the capsule / the hull AHEAD of the boxes
        ("xfirst",      "xfirst",     {},             True,  "hb_step_gen_fast_kernel"),
        ("xfirst_mesh", "xfirst_mesh", {},            True,  "hb_step_gen_fast_kernel"),
        ("xfirst-prim", "xfirst",     "narrow_prim",  False, "hb_step_gen_fast_lean_kernel"),
        ("xfirst_mesh-lean", "xfirst_mesh", {},       False, "hb_step_gen_fast_lean_kernel")]


def _report(label, worst):
    lines = ["%-12s %-12s worst measured / bound: dist %.3f pos %.3f normal %.3f   (%d contacts)" % ((label, k) + tuple(w[:3]) + (int(w[3]),)) for k, w in sorted(worst.items())]
    report(lines, "HB_BOX_PARITY_OUT", lead="\n")


def _check_exact_box_box(ref, c, d, want, bad):
    """an axis-aligned box on a box, identity quaternions: normal +z, depth 1/128 from the sizes alone, a position inside the overlap
    region (over both faces, between the two surfaces) - and, beyond what is well defined, the oracle's own position on the twin"""
    info = ref["info"]
    g1, g2 = c["geoms"]
    pos = {}
    for g in (g1, g2):
        b = int(info["geom_bodyid"][g])
        pos[g] = info["geom_pos"][3 * g:3 * g + 3] if b == 0 else c["qpos"][7 * (b - 1):7 * (b - 1) + 3]
    h1, h2 = info["geom_size"][3 * g1:3 * g1 + 3], info["geom_size"][3 * g2:3 * g2 + 3]
    top, bottom = pos[g1][2] + h1[2], pos[g2][2] - h2[2]
    frame = d[4:13].reshape(3, 3)
    err = np.array([abs(d[0] - (bottom - top)), np.abs(d[1:4] - want["pos"]).max(), np.abs(frame[0] - [0, 0, 1]).max()])
    lo = np.append(np.maximum(pos[g1][:2] - h1[:2], pos[g2][:2] - h2[:2]), bottom) - TOL["pos"]
    hi = np.append(np.minimum(pos[g1][:2] + h1[:2], pos[g2][:2] + h2[:2]), top) + TOL["pos"]
    if (err > BASE).any() or (d[1:4] < lo).any() or (d[1:4] > hi).any():
        bad.append((c["name"], "exact box - box", ["%.2e" % x for x in err], d[1:4].tolist(), lo.tolist(), hi.tolist()))
    return err / BASE


def _check_contacts(ref, got, label):
    nc, ne, _ = got["counts"]
    worst = collections.defaultdict(lambda: np.zeros(4))
    bad = []
    for i, c in enumerate(ref["cases"]):
        held = held_to(ref, i, int(nc[i]), int(ne[i]), bad, "reference")
        if held is None:
            continue
        ev, env = held
        for k, want in enumerate(ev["con"]):
            d = got["con"][i, k]
            assert (int(d[14]), int(d[15]), int(d[13])) == (want["geom1"], want["geom2"], want["dim"]), (label, c["name"], k, d[13:16])
            frame = d[4:13].reshape(3, 3)
            if np.abs(frame @ frame.T - np.eye(3)).max() > 1e-5:
                bad.append((c["name"], k, "frame not orthonormal", frame.round(4).tolist()))
            if c["exact"] and c["kind"] == "box-box":
                ratio = _check_exact_box_box(ref, c, d, want, bad)
            else:
                err = np.array([abs(d[0] - want["dist"]), np.abs(d[1:4] - want["pos"]).max(), np.abs(frame[0] - want["frame"][0]).max()])
                ratio = err / (BASE + K * env[k])
                if ratio.max() > 1:
                    bad.append((c["name"], k, ["%.2e" % x for x in err], ["%.2e" % x for x in BASE + K * env[k]]))
            worst[c["kind"]] = np.append(np.maximum(worst[c["kind"]][:3], ratio), worst[c["kind"]][3] + 1)
    _report(label, worst)
    print("".join("\n  %s: %s" % (label, x) for x in bad))
    assert not bad, (label, len(bad), bad[:3])


def _check_state(ref, got, label):
    o = ref["oracle"]
    nc, ne, _ = got["counts"]
    # PGS is cut at 50 sweeps and what it then has depends on the order of the rows (the oracle's own step moves by 2.9e-3 in qvel when
    # its two contacts of "plane-Q edge 2 down" are swapped; its Newton step by 9e-17): under PGS only the cases whose contacts the
    # twin's plane - hull collider lists in the box's corner order are comparable, under Newton every twin-agreement case is
    newton = ref["model"].opt.solver == 2
    agree = {i for i, ordered in twin_agreement(ref).items() if ordered or newton}
    wq = wv = 0.0
    n = n_agree = 0
    bad = []
    for i, c in enumerate(ref["cases"]):
        held = held_to(ref, i, int(nc[i]), int(ne[i]), bad, "reference")
        if held is None or (c["kind"] in ANALYTIC and i not in agree):
            continue
        n_agree += c["kind"] in ANALYTIC
        o.load(held[0]["qpos"])
        o.step()
        if (o.ncon, o.nefc) != (int(nc[i]), int(ne[i])):
            bad.append((c["name"], "counts", (int(nc[i]), int(ne[i])), "oracle on the twin", (o.ncon, o.nefc)))
            continue
        dq = (np.abs(got["qpos"][i] - o.qpos) / np.maximum(1.0, np.abs(o.qpos))).max()
        dv = np.abs(got["qvel"][i] - o.qvel).max() / max(1.0, np.abs(o.qvel).max())
        if dq > BOUNDS["qpos"] or dv > BOUNDS["qvel"]:
            bad.append((c["name"], "qpos %.2e qvel %.2e" % (dq, dv)))
        wq, wv, n = max(wq, dq), max(wv, dv), n + 1
    line = "%-12s state after the step, %d cases against the oracle on the twin: worst qpos %.2e (bound %.0e) qvel %.2e (bound %.0e)" % (label, n, wq, BOUNDS["qpos"], wv, BOUNDS["qvel"])
    report(line, "HB_BOX_PARITY_OUT", lead="\n")
    print("".join("\n  %s: %s" % (label, x) for x in bad))
    assert n_agree >= 20 and n - n_agree >= 70 and not bad, (label, n_agree, n, len(bad), bad[:3])


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_box_pairs(hbmod, gpu, tmp_path_factory, row):
    label, scene, knobs, diag, kernel = row
    ref = reference(hbmod, scene, tmp_path_factory.mktemp("boxes"))
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
    assert got["counts"][0].max() == 4 and (got["counts"][0] == 0).sum() >= 10
    if diag:
        _check_contacts(ref, got, label)
    else:
        _check_state(ref, got, label)


@pytest.mark.parametrize("scene", ["pgs", "mesh"])
def test_two_envs_per_wave_narrowphase(hbmod, gpu, tmp_path_factory, scene):
    """A launch that covers a whole batch of 512 envs or more runs the narrowphase two envs per wave (hb_narrow2_prim_box_kernel without
    meshes, hb_narrow2_box_kernel with): the case table three times over in one unpipelined launch, every copy bit for bit the table's own
    own launch (one env per wave), which the rows above hold to the reference"""
    ref = reference(hbmod, scene, tmp_path_factory.mktemp("boxes"))
    one, three = launch(hbmod, gpu, ref, {}, False), launch(hbmod, gpu, ref, {}, False, tiles=3)
    n = len(ref["cases"])
    assert 3 * n >= 512 and not three["status"].any() and three["kernel"] == one["kernel"]
    for t in range(3):
        assert np.array_equal(three["state"][t * n:(t + 1) * n], one["state"]), (scene, t)
        assert all(np.array_equal(a[t * n:(t + 1) * n], b) for a, b in zip(three["counts"], one["counts"])), (scene, t)


def test_body_acceleration_kernel_of_a_newton_box_model(hbmod, gpu):
    """the stairs model under Newton with the body-acceleration read-out: the box table's own twin of the full kernel"""
    m = hbmod.Model.from_xml_string(box_cases.stairs_xml(solver="Newton"))
    b = hbmod.Batch(m, 16, gpu)
    b.diag_enable(True)
    b.body_acc_readout(True)
    b.step(np.zeros((16, m.nu), dtype=np.float32))
    assert b.last_kernel() == "hb_box_acc_newton_big20_kernel" and not b.status().any()
    acc = b.body_acc()
    b.close()
    assert np.isfinite(acc).all() and np.abs(acc).max() > 0


# ---- standing: the stairs model of tests/box_cases.py (tests/models/box_stairs.xml), 16 envs, 400 steps ------------------------------
def _brick_on_the_oracle(hbmod, solver, directory, steps):
    """the brick of the stairs model's MESH TWIN in the fp64 oracle: (largest |sum of its normal contact forces - m g| over the steps,
    its height after every step)"""
    from oracle_lib import Oracle
    p = str(directory / ("stairs_twin_%s.hbm" % solver))
    hbmod.Model.from_xml_string(box_cases.stairs_xml(True, solver)).save(p)
    o = Oracle(p)
    brick = list(o.info["geom_name"]).index("brick")
    weight = box_cases.BRICK_MASS * 9.81
    o.reset()
    err, z = [], []
    for _ in range(steps):
        o.step()
        f = sum(o.efc_force[c["efc_address"]:c["efc_address"] + 4].sum() for c in o.contacts() if brick in (c["geom1"], c["geom2"]))
        err.append(abs(f - weight))
        z.append(o.qpos[o.nq - 5])
    return max(err), max(err[-100:]), np.array(z)


@pytest.mark.parametrize("solver", ["PGS", "Newton"])
def test_standing_on_the_stairs_model(hbmod, gpu, tmp_path, solver):
    steps, n = 400, 16
    m = hbmod.Model.from_xml_string(box_cases.stairs_xml(solver=solver))
    brick = m.name2id("geom", "brick")
    weight = box_cases.BRICK_MASS * 9.81
    bound_o, rest_o, z_o = _brick_on_the_oracle(hbmod, solver, tmp_path, steps)
    b = hbmod.Batch(m, n, gpu)
    b.diag_enable(True)
    b.contact_readout(True)
    ctrl = np.zeros((n, m.nu), dtype=np.float32)
    worst, rest, z = 0.0, 0.0, []
    for t in range(steps):
        b.step(ctrl)
        nc = b.counts()[0]
        con, frc = b.contacts(), b.contact_force()
        mine = ((con[:, :, 14] == brick) | (con[:, :, 15] == brick)) & (np.arange(con.shape[1])[None, :] < nc[:, None])
        assert (mine.sum(axis=1) == 4).all(), (t, mine.sum(axis=1))
        err = float(np.abs((frc[:, :, 0] * mine).sum(axis=1) - weight).max())
        worst, rest = max(worst, err), max(rest, err) if t >= steps - 100 else 0.0
        z.append(b.qpos[:, m.nq - 5].astype(np.float64))
    # (diagnostics on: PGS steps staged through its fast pass, which appends the pose kernel's box contacts; Newton in the full kernel)
    assert b.last_kernel() == {"PGS": "hb_step_gen_fast_kernel", "Newton": "hb_box_newton_big20_kernel"}[solver], b.last_kernel()
    assert not b.status().any() and np.isfinite(b.get_state(hbmod.STATE_INTEGRATION)).all()
    b.close()
    z = np.array(z)
    drift, drift_o = np.abs(z - z[0]).max(), np.abs(z_o - z_o[0]).max()
    line = ("standing %-6s the brick's normal forces - m g (%.3f N): oracle on the twin %.3e, device %.3e (bound 2 x the oracle's); "
            "height drift over %d steps: oracle %.3e, device %.3e" % (solver, weight, bound_o, worst, steps, drift_o, drift))
    report(line, "HB_BOX_PARITY_OUT", lead="\n")
    line = "standing %-6s the same over the last 100 steps (at rest): oracle %.3e, device %.3e (bound 2 x the oracle's + %.0e x m g)" % (solver, rest_o, rest, TOL["force"])
    report(line, "HB_BOX_PARITY_OUT", lead="")
    assert worst <= 2 * bound_o
    # The bound above is set by the landing transient of a brick released 1 mm up.  At rest: twice the oracle's own residual, plus the
    # project's bound on a constraint force in fp32, bounds.CONVEX_TOL["force"] = 3e-4 of its scale (here the weight)
    assert rest <= 2 * rest_o + TOL["force"] * weight
    assert (np.abs(z - z[0]).max(axis=1) <= drift_o + TOL["pos"] * steps).all()
