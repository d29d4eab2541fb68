"""The box - box manifold on the device (Model.box_manifold; hb_mpr.hpp: box_box), PAIR BY PAIR through the kernels that carry it - the staged
step's hb_pose_boxm_kernel and the hb_boxm_* step kernels, the family a box model takes with the mode on - and in the scenes it was built for.  One env is one case of
tests/boxbox_cases.py, one launch evaluates the table, one step; every row asserts the kernel it ran.

Per case against boxbox_ref at the same fp32-rounded state, under the EXACT / ill-conditioned rule of pair_cases.held_to:
  - ncon and nefc identical; geom ids and dim identical; every frame orthonormal to 1e-5, its first row the normal;
  - the contact ORDER identical: contact k is held to the reference's contact k;
  - dist, pos and normal within BASE + K * envelope, BASE = bounds.CONVEX_TOL (dist 5e-7, pos 3e-6, normal 3e-5) and K = 6, the count
    tests/test_gpu_box.py derives for a pair of boxes: the device computes in fp64 from its fp32 pose, so its error is the pose's
    rounding, which the envelope measures, lifted candidates included.  An EXACT case has no envelope: BASE alone.
Worst measured / bound per kind is printed and appended to the file HB_BOXBOX_PARITY_OUT names (profiles/boxbox_parity.txt).
The scene's own boxes cannot give eight contacts (tests/boxbox_cases.py); the "-octagon" rows run the octagon scene's table, whose cases
have eight and seven, through the same check: the fourth work item of a pair is reached there only.

One implementation everywhere: fused against staged, narrow_prim 1 against 0 and the table tiled three times over (two envs per wave in
the narrowphase launch) are bit for bit the table's own launch.  Mode off is today: at most one contact per case, bit for bit a model on
which the setter was never called.  A brick lying on a larger box is a brick lying on a plane at that height (the existing plane - box
collider is the reference): one Newton step within bounds.BOUNDS, and at rest under PGS/50.  The biped of the stairs model stands on the
first step on eight foot contacts.
"""
import collections

import numpy as np
import pytest

import box_cases
import boxbox_cases
from bounds import BOUNDS, CONVEX_TOL as TOL
from pair_cases import held_to, launch
from step_lib import report

pytestmark = pytest.mark.gpu

K = 6.0
BASE = np.array([TOL["dist"], TOL["pos"], TOL["nrm"]])
OUT = "HB_BOXBOX_PARITY_OUT"

#       id                scene         octagon  knobs           kernel
ROWS = [("fused",         "pgs",        False,   {"staged": 0},  "hb_boxm_gen_kernel"),
        ("staged",        "pgs",        False,   {},             "hb_step_gen_fast_kernel"),
        ("newton_cd6",    "newton_cd6", False,   {},             "hb_boxm_newton_big28_kernel"),
        ("pgs_cd6",       "pgs_cd6",    False,   {},             "hb_boxm_gen_big_kernel"),
        ("fused-octagon", "pgs",        True,    {"staged": 0},  "hb_boxm_gen_kernel"),
        ("staged-octagon", "pgs",       True,    {},             "hb_step_gen_fast_kernel"),
        ("newton_cd6-octagon", "newton_cd6", True, {},           "hb_boxm_newton_big28_kernel")]


def _check_contacts(ref, got, label):
    nc, ne, _ = got["counts"]
    worst = collections.defaultdict(lambda: np.zeros(4))
    bad = []
    for i, c in enumerate(ref["cases"]):
        held = held_to(ref, i, int(nc[i]), int(ne[i]), bad, "boxbox_ref")
        if held is None:
            continue
        ev, env = held
        for k, want in enumerate(ev["con"]):
            d = got["con"][i, k]
            assert (int(d[14]), int(d[15]), int(d[13])) == (want["geom1"], want["geom2"], want["dim"]), (label, c["name"], k, d[13:16])
            frame = d[4:13].reshape(3, 3)
            if np.abs(frame @ frame.T - np.eye(3)).max() > 1e-5:
                bad.append((c["name"], k, "frame not orthonormal", frame.round(4).tolist()))
            err = np.array([abs(d[0] - want["dist"]), np.abs(d[1:4] - want["pos"]).max(), np.abs(frame[0] - want["frame"][0]).max()])
            bound = BASE + (0.0 if c["exact"] else K) * env[k]
            ratio = err / bound
            print("  %s | %s | contact %d: dist %.2e / %.2e pos %.2e / %.2e normal %.2e / %.2e" % (label, c["name"], k, err[0], bound[0], err[1], bound[1], err[2], bound[2]))
            if ratio.max() > 1:
                bad.append((c["name"], k, ["%.2e" % x for x in err], ["%.2e" % x for x in bound]))
            kind = "exact" if c["exact"] else c["kind"]
            worst[kind] = np.append(np.maximum(worst[kind][:3], ratio), worst[kind][3] + 1)
    lines = ["%-18s %-6s worst measured / bound: dist %.3f pos %.3f normal %.3f   (%d contacts)" % ((label, k) + tuple(w[:3]) + (int(w[3]),)) for k, w in sorted(worst.items())]
    report(lines, OUT, lead="\n")
    print("".join("\n  %s: %s" % (label, x) for x in bad))
    assert not bad, (label, len(bad), bad[:3])


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_boxbox_pairs(hbmod, gpu, tmp_path_factory, row):
    label, scene, octagon, knobs, kernel = row
    ref = boxbox_cases.reference(hbmod, scene, tmp_path_factory.mktemp("boxbox"), octagon)
    got = launch(hbmod, gpu, ref, knobs, True)
    assert got["kernel"] == kernel, (label, got["kernel"], kernel)
    assert not got["status"].any(), (label, got["status"])
    # (what a build whose kernels ignore the mode cannot give: more than one contact for a pair)
    assert got["counts"][0].max() == (8 if octagon else 7) and (got["counts"][0] == 0).sum() >= 2
    _check_contacts(ref, got, label)


def _same(a, b, what):
    assert np.array_equal(a["state"], b["state"]) and np.array_equal(a["status"], b["status"]), what
    assert all(np.array_equal(x, y) for x, y in zip(a["counts"], b["counts"])), what


@pytest.mark.parametrize("octagon", [False, True], ids=["table", "octagon"])
def test_one_implementation_everywhere(hbmod, gpu, tmp_path_factory, octagon):
    ref = boxbox_cases.reference(hbmod, "pgs", tmp_path_factory.mktemp("boxbox"), octagon)
    staged = launch(hbmod, gpu, ref, {}, False)
    assert staged["kernel"] == "hb_step_gen_fast_lean_kernel" and not staged["status"].any() and staged["counts"][0].max() >= 7
    fused = launch(hbmod, gpu, ref, {"staged": 0}, False)
    assert fused["kernel"] == "hb_boxm_gen_kernel"
    _same(fused, staged, "fused against staged")
    _same(launch(hbmod, gpu, ref, {"narrow_prim": 0}, False), launch(hbmod, gpu, ref, {"narrow_prim": 1}, False), "narrow_prim 0 against 1")
    if octagon:
        return
    # the table tiled over 512 envs or more in one unpipelined launch: the two-envs-per-wave narrowphase, every copy the table's own launch
    tiles = -(-512 // len(ref["cases"]))
    many = launch(hbmod, gpu, ref, {}, False, tiles=tiles)
    n = len(ref["cases"])
    assert tiles * n >= 512 and not many["status"].any() and many["kernel"] == staged["kernel"]
    for t in range(tiles):
        assert np.array_equal(many["state"][t * n:(t + 1) * n], staged["state"]), t
        assert all(np.array_equal(a[t * n:(t + 1) * n], b) for a, b in zip(many["counts"], staged["counts"])), t


def test_mode_off_is_today(hbmod, gpu, tmp_path_factory):
    ref = boxbox_cases.reference(hbmod, "pgs", tmp_path_factory.mktemp("boxbox"))
    never = hbmod.Model.from_xml_string(box_cases.scene_xml("pgs"))
    off = hbmod.Model.from_xml_string(box_cases.scene_xml("pgs"))
    assert off.box_manifold(1) == 1 and off.box_manifold(0) == 0
    for knobs in ({}, {"staged": 0}):
        a = launch(hbmod, gpu, dict(ref, model=never), knobs, False)
        b = launch(hbmod, gpu, dict(ref, model=off), knobs, False)
        assert a["kernel"] == b["kernel"] and a["counts"][0].max() <= 1 and (a["counts"][0] == 1).sum() >= 60
        _same(a, b, knobs)


# ---- a brick on a box is a brick on a plane ------------------------------------------------------------------------------------------
SLAB_TOP = 0.2


def _brick_xml(on, solver):
    """the stairs model's brick face-down 1 mm over a static box whose top face is larger in both extents ("box"), or over a plane at that height"""
    support = ('<geom name="slab" type="box" size="0.4 0.3 0.1" pos="0 0 %g"/>' % (SLAB_TOP - 0.1)) if on == "box" else '<geom name="floor" type="plane" size="0 0 1" pos="0 0 %g"/>' % SLAB_TOP
    opt = 'iterations="100" tolerance="1e-8" solver="Newton"' if solver == "Newton" else 'iterations="50" tolerance="0" solver="PGS"'
    return ('<mujoco model="brick"><option timestep="0.002" %s/><default><geom condim="3" friction="1" margin="0.002"/></default><worldbody>%s'
            '<body name="brick" pos="0 0 %g"><freejoint name="brick"/><inertial pos="0 0 0" mass="%g" diaginertia="0.006 0.012 0.014"/>'
            '<geom name="brick" type="box" size="%g %g %g"/></body></worldbody></mujoco>'
            % ((opt, support, SLAB_TOP + box_cases.BRICK_HALF[2] + 0.001, box_cases.BRICK_MASS) + box_cases.BRICK_HALF))


def _brick_states(m, n):
    """n states of the brick: up to 5 cm aside, any yaw, tilted by up to 3 mrad, 0.5 .. 1.5 mm over the support (all four corners in the margin)"""
    rng = np.random.default_rng(3)
    st = np.zeros((n, 1 + m.nq + 2 * m.nv))
    for e in range(n):
        yaw, tilt = rng.uniform(0, 2 * np.pi), rng.uniform(-0.003, 0.003, 2)
        q = boxbox_cases._qmul([np.cos(0.5 * tilt[0]), np.sin(0.5 * tilt[0]), 0, 0], boxbox_cases._qmul([np.cos(0.5 * tilt[1]), 0, np.sin(0.5 * tilt[1]), 0], [np.cos(0.5 * yaw), 0, 0, np.sin(0.5 * yaw)]))
        st[e, 1:8] = np.concatenate([[rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), SLAB_TOP + box_cases.BRICK_HALF[2] + rng.uniform(0.0005, 0.0015)], q / np.linalg.norm(q)])
    return st.astype(np.float32).astype(np.float64)


def _run(hbmod, gpu, on, solver, mode, steps, window=None):
    m = hbmod.Model.from_xml_string(_brick_xml(on, solver))
    if mode:
        assert m.box_manifold(1) == 1
    n = 16
    b = hbmod.Batch(m, n, gpu)
    b.set_state(hbmod.STATE_INTEGRATION, _brick_states(m, n))
    ctrl = np.zeros((n, m.nu), dtype=np.float32)
    peak, first = 0.0, None
    for t in range(steps):
        b.step(ctrl)
        if t == 0:
            first = b.counts()[0].copy()
        if window and window[0] <= t + 1 <= window[1]:
            peak = max(peak, float(np.abs(b.qvel).max()))
    out = dict(qpos=b.qpos.astype(np.float64), qvel=b.qvel.astype(np.float64), status=b.status(), counts=b.counts(), first=first, peak=peak, kernel=b.last_kernel())
    b.close()
    return out


def test_lying_on_a_box_equals_lying_on_a_plane(hbmod, gpu):
    box, plane = _run(hbmod, gpu, "box", "Newton", 1, 1), _run(hbmod, gpu, "plane", "Newton", 0, 1)
    assert not box["status"].any() and not plane["status"].any()
    assert (box["first"] == 4).all() and (plane["first"] == 4).all()
    dq = (np.abs(box["qpos"] - plane["qpos"]) / np.maximum(1.0, np.abs(plane["qpos"]))).max()
    dv = np.abs(box["qvel"] - plane["qvel"]).max() / max(1.0, np.abs(plane["qvel"]).max())
    report("brick on a box against brick on a plane, one Newton step, 16 envs [%s / %s]: qpos %.2e (bound %.0e) qvel %.2e (bound %.0e)"
           % (box["kernel"], plane["kernel"], dq, BOUNDS["qpos"], dv, BOUNDS["qvel"]), OUT, lead="\n")
    assert dq <= BOUNDS["qpos"] and dv <= BOUNDS["qvel"]


def test_at_rest_on_a_box_as_on_a_plane(hbmod, gpu):
    window = (250, 500)
    box, plane, off = (_run(hbmod, gpu, on, "PGS", mode, 500, window) for on, mode in (("box", 1), ("plane", 0), ("box", 0)))
    report("brick at rest under PGS/50, largest |qvel| over steps 250..500 of 16 envs: on a box, manifold %.3e; on a plane %.3e (bound: twice the plane's + %.0e); "
           "on a box, mode off (one contact, reported only) %.3e" % (box["peak"], plane["peak"], BOUNDS["qvel"], off["peak"]), OUT, lead="\n")
    assert not box["status"].any() and not plane["status"].any()
    assert (box["counts"][0] == 4).all() and (plane["counts"][0] == 4).all()
    assert box["peak"] <= 2 * plane["peak"] + BOUNDS["qvel"]


def test_biped_stands_on_a_step(hbmod, gpu):
    """the stairs model's biped moved onto the first step (top at 0.1 m, 0.3 .. 0.6 m): both box feet flat on the step's top face"""
    xml = box_cases.stairs_xml()
    assert xml.count('<body name="torso" pos="0 0 0.601">') == 1
    m = hbmod.Model.from_xml_string(xml.replace('<body name="torso" pos="0 0 0.601">', '<body name="torso" pos="0.42 0 %g">' % (0.601 + box_cases.STEP_RISE)))
    assert m.box_manifold(1) == 1
    feet, step0 = {m.name2id("geom", "lfoot"), m.name2id("geom", "rfoot")}, m.name2id("geom", "step0")
    n, steps = 16, 300
    b = hbmod.Batch(m, n, gpu)
    b.diag_enable(True)
    ctrl = np.zeros((n, m.nu), dtype=np.float32)
    z0 = b.qpos[:, 2].astype(np.float64).copy()
    drift = 0.0
    for t in range(steps):
        b.step(ctrl)
        drift = max(drift, float(np.abs(b.qpos[:, 2] - z0).max()))
    nc = b.counts()[0]
    con = b.contacts()
    live = np.arange(con.shape[1])[None, :] < nc[:, None]
    on_step = live & (con[:, :, 14] == step0) & np.isin(con[:, :, 15], list(feet))
    status = b.status()
    b.close()
    report("biped on the first step, mode on, %d steps: foot contacts per env %s, torso height within %.2e m of its start (bound 1e-2)" % (steps, sorted(set(on_step.sum(axis=1).tolist())), drift), OUT, lead="\n")
    assert not status.any() and (on_step.sum(axis=1) == 8).all(), (status, on_step.sum(axis=1))
    assert drift <= 0.01
