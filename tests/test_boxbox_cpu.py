"""(CPU) The box - box manifold before any device sees it: the fp64 reference tests/boxbox_ref.py held to what follows from its definition,
the case table of tests/boxbox_cases.py proven on the reference alone, and the mode flag through the model file, the C-ABI and the tables.

  - against box_ref.plane_box: a box lying on a face of a box larger in both in-plane extents gives plane_box's contacts on the plane
    through that face, same order, to 1e-12, in both role assignments (the larger box geom 2: the normal negated, the positions unchanged);
  - the axis-aligned dyadic cases (the three of box_cases, the partial overlaps of boxbox_cases) against their closed forms: the overlap
    rectangle's corners, normal +-z, dist = bottom - top, z midway, to 1e-15 relative;
  - the corner-on-face and edge-on-face poses of box_cases.build_cases: the smallest dist is the gap, the normal the face's.  Those poses are
    rounded to fp32 when the table is built, so the gap they are held to, at 1e-12, is the one an independent fp64 enumeration of the second
    box's corners gives at the rounded state (the nominal gap of the construction within one fp32 rounding of the pose, 2e-6).  The count
    of corner contacts (a) is the number of corners in range over the face's interior by the same enumeration, and the total 1 (corner) and
    2 (edge) wherever no further corner is in range and nothing is clipped; the generic rotation of box_cases' "corner" poses on +z happens
    to lay the box nearly flat (four corners within 3 mm) and some poses reach over the rim: there the definition gives more contacts,
    asserted as at least 1 and 2;
  - against the oracle on the MESH TWIN on the corner-on-face cases: the normal and the smallest dist agree with the portal search's single
    contact within bounds.CONVEX_TOL plus the case's envelope (positions on flat faces are not compared: tests/test_gpu_box.py's header);
  - invariants on 3000 seeded configurations: every pos inside both boxes grown by |dist| / 2 + margin / 2 + 1e-12, counts <= 8, a 45 degree
    face overlap gives 8, swapping A and B negates the normal and keeps the set of (dist, pos) to 1e-12 in the face case;
  - the table: what it must cover, every decision margin of a non-exact case at least 1e-5 from zero, at most 5 % (here: none)
    ill-conditioned under pair_cases.evaluations, at least 120 cases; the OCTAGON scene's table (boxbox_cases: the scene's own boxes
    cannot give eight) has its eight-contact cases with either box the reference;
  - plumbing: setter and query, the .hbm record (kept when on, absent when off: the file byte for byte, a value of 2 a load error),
    hb_sizes unchanged, the device tables of a model without box - box pairs identical with the mode on.
"""
import collections
import os

import numpy as np
import pytest

import box_cases
import box_ref
import boxbox_cases
import boxbox_ref
import pair_ref
from bounds import CONVEX_TOL as TOL
from humanoid_mujoco_amd import engine
from oracle_lib import MODELS_DIR, parse_hbm
from pair_cases import _qaxis, _qrand, envelope
from tables_lib import fields, run as _tables

MARGIN = box_cases.MARGIN


def _rot(q):
    return pair_ref.quat2mat(np.asarray(q, dtype=np.float64) / np.linalg.norm(q))


# ---- lying on a larger box is lying on a plane -------------------------------------------------------------------------------------
@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("larger_first", [True, False])
def test_lying_on_a_larger_box_is_plane_box(face, larger_first):
    rng = np.random.default_rng(100 + face)
    big, small = np.array([0.5, 0.4, 0.3]), np.array(box_cases.BRICK_HALF)
    for trial in range(20):
        Rb = _rot(_qrand(rng))
        pb = rng.standard_normal(3)
        nl = np.zeros(3)
        nl[face // 2] = 1.0 if face % 2 else -1.0
        n = Rb @ nl
        # the brick: a face down on the big box's face, turned about the normal, tilted by up to 0.02 rad, its lowest corner -4 .. +8 mm off
        down = int(rng.integers(3))
        t1, t2 = np.eye(3)[(face // 2 + 1) % 3], np.eye(3)[(face // 2 + 2) % 3]
        yaw = rng.uniform(0, 2 * np.pi)
        L = np.zeros((3, 3))
        L[:, down] = -nl
        L[:, (down + 1) % 3] = np.cos(yaw) * t1 + np.sin(yaw) * t2
        L[:, (down + 2) % 3] = np.cross(L[:, down], L[:, (down + 1) % 3])
        tv = Rb @ (rng.uniform(-0.02, 0.02) * t1 + rng.uniform(-0.02, 0.02) * t2)
        Rs = _rot(_qaxis(tv, np.linalg.norm(tv))) @ Rb @ L if np.linalg.norm(tv) > 0 else Rb @ L
        low = min((Rs @ c) @ n for c in box_ref.corners(small))
        ps = pb + Rb @ (nl * big + rng.uniform(-0.3, 0.3, 3) * big * (nl == 0)) + n * (rng.uniform(-0.004, 0.008) - low)
        want = box_ref.plane_box(MARGIN, pb + n * big[face // 2], n, ps, Rs, small)
        labels = []
        got = boxbox_ref.box_box(MARGIN, pb, Rb, big, ps, Rs, small, labels) if larger_first else boxbox_ref.box_box(MARGIN, ps, Rs, small, pb, Rb, big, labels)
        assert ("box-box:face %s%d%s" % ("A" if larger_first else "B", face // 2, "+" if face % 2 else "-")) in labels, labels
        assert len(got) == len(want) >= 2, (trial, len(got), len(want))
        for g, w in zip(got, want):
            assert abs(g["dist"] - w["dist"]) <= 1e-12 and np.abs(g["pos"] - w["pos"]).max() <= 1e-12
            assert np.abs(g["normal"] - (n if larger_first else -n)).max() <= 1e-12


# ---- the axis-aligned dyadic cases against their closed forms --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref(hbmod, tmp_path_factory):
    return boxbox_cases.reference(hbmod, "pgs", tmp_path_factory.mktemp("boxbox"))


def _pose(info, c, g):
    b = int(info["geom_bodyid"][g])
    return info["geom_pos"][3 * g:3 * g + 3] if b == 0 else c["qpos"][7 * (b - 1):7 * (b - 1) + 3]


def test_axis_aligned_cases_have_their_closed_forms(ref):
    info = ref["info"]
    exact = [(i, c) for i, c in enumerate(ref["cases"]) if c["exact"]]
    assert len(exact) == 7 and sum(c["source"] == "partial" for _, c in exact) == 4
    for i, c in exact:
        g1, g2 = c["geoms"]
        p1, p2 = _pose(info, c, g1), _pose(info, c, g2)
        h1, h2 = info["geom_size"][3 * g1:3 * g1 + 3], info["geom_size"][3 * g2:3 * g2 + 3]
        top, bottom = p1[2] + h1[2], p2[2] - h2[2]
        lo, hi = np.maximum(p1[:2] - h1[:2], p2[:2] - h2[:2]), np.minimum(p1[:2] + h1[:2], p2[:2] + h2[:2])
        corners = {(x, y) for x in (lo[0], hi[0]) for y in (lo[1], hi[1])}
        con = ref["evals"][i][0]["con"]
        assert len(con) == 4, c["name"]
        scale = max(1.0, np.abs(p1).max())
        for k in con:
            assert abs(k["dist"] - (bottom - top)) <= 1e-15 * scale and np.array_equal(k["frame"][0], [0.0, 0.0, 1.0])
            assert abs(k["pos"][2] - 0.5 * (top + bottom)) <= 1e-15 * scale
            near = min(corners, key=lambda q: abs(q[0] - k["pos"][0]) + abs(q[1] - k["pos"][1]))
            assert max(abs(near[0] - k["pos"][0]), abs(near[1] - k["pos"][1])) <= 1e-15 * scale
            corners.discard(near)
        assert not corners
        if c["source"] == "partial":  # one corner of each rectangle inside the other, two crossings
            tests = []
            src = [k["src"] for k in boxbox_ref.box_box(MARGIN, p1, np.eye(3), h1, p2, np.eye(3), h2, None, tests)]
            assert sorted(src) == ["a", "b", "c", "c"], (c["name"], src)


# ---- a corner and an edge over a face: the poses of the box table --------------------------------------------------------------------
def _box_table_cases(info):
    return [c for c in box_cases.build_cases(info, "pgs") if c["kind"] == "box-box" and not c["exact"]]


def _face_of(name):
    return box_ref.FACES.index(name.split("on face ")[1].split(",")[0])


def test_corner_and_edge_over_a_face(ref):
    info = ref["info"]
    size = info["geom_size"].reshape(-1, 3)
    gid = {n: list(info["geom_name"]).index(n) for n in "WPQ"}
    seen = collections.Counter()
    exact_gap = 0
    for c in _box_table_cases(info):
        a, o = c["name"].split()[0].split("-")
        cfg, tag = c["name"].split()[1], c["name"].split(", ")[1]
        nominal = dict(boxbox_cases.DEPTHS)[tag]
        gpos, gmat = pair_ref.geom_poses(info, c["qpos"])
        face = _face_of(c["name"])
        nl = np.zeros(3)
        nl[face // 2] = 1.0 if face % 2 else -1.0
        n = gmat[gid[a]] @ nl
        # the second box's corners over the face, in fp64 at the rounded state: heights, and which stand over the face's interior
        pts = gpos[gid[o]] + box_ref.corners(size[gid[o]]) @ gmat[gid[o]].T
        height = (pts - gpos[gid[a]]) @ n - size[gid[a]][face // 2]
        gap = height.min()
        assert abs(gap - nominal) <= 2e-6, (c["name"], gap)
        in_range = int((height <= MARGIN).sum())
        labels = []
        con = boxbox_cases.evaluate_pair(info, c["qpos"], c["geoms"], labels)
        if tag == "outside":
            assert not con, c["name"]
            continue
        want_n = n if c["geoms"][0] == gid[a] else -n
        # the smallest dist is the gap where the lowest corner stands over the face's interior; where it hangs over the rim (an "edge" pose
        # whose two corners are level to 1e-10, the lower one outside) it is the height of a clipped point between that corner and the
        # lowest one inside
        local = (pts - gpos[gid[a]]) @ gmat[gid[a]]
        over = np.all((np.abs(local) <= size[gid[a]]) | (nl != 0), axis=1)
        least = min(k["dist"] for k in con)
        assert gap - 1e-12 <= least <= height[over].min() + 1e-12, (c["name"], gap, least)
        exact_gap += bool(over[np.argmin(height)])
        assert all(np.abs(k["frame"][0] - want_n).max() <= 1e-12 for k in con), c["name"]
        base = 1 if cfg == "corner" else 2
        assert in_range >= base
        # (a) is exactly the corners in range over the face's interior; with no further corner in range, none over the rim and no clipped
        # point in range, they are all there is
        g1, g2 = c["geoms"]
        src = [k["src"] for k in boxbox_ref.box_box(MARGIN, gpos[g1], gmat[g1], size[g1], gpos[g2], gmat[g2], size[g2])]
        assert src.count("a") == int((over & (height <= MARGIN)).sum()) >= 1 and len(src) == len(con), (c["name"], src)
        plain = in_range == base and src.count("a") == len(src)
        assert len(con) == base if plain else len(con) >= base, (c["name"], len(con))
        seen[(cfg, plain)] += 1
    assert seen[("corner", True)] >= 8 and seen[("edge", True)] >= 4 and exact_gap >= 20, (seen, exact_gap)


def test_manifold_against_the_portal_search_on_the_mesh_twin(hbmod, tmp_path_factory):
    """the corner-on-face cases of the box table: the manifold's normal and smallest dist against the oracle's single contact on the twin"""
    bref = box_cases.reference(hbmod, "pgs", tmp_path_factory.mktemp("boxes"))
    n = 0
    worst = np.zeros(2)
    for i, c in enumerate(bref["cases"]):
        if c["kind"] != "box-box" or c["exact"] or " corner " not in c["name"]:
            continue
        got = envelope(bref, i, 1)
        con = boxbox_cases.evaluate_pair(bref["info"], c["qpos"], c["geoms"])
        if got is None:
            assert not con and bref["evals"][i][0]["ncon"] == 0, c["name"]
            continue
        ev, env = got
        k = min(con, key=lambda x: x["dist"])
        err = np.array([abs(k["dist"] - ev["con"][0]["dist"]), np.abs(k["frame"][0] - ev["con"][0]["frame"][0]).max()])
        bound = np.array([TOL["dist"] + env[0][0], TOL["nrm"] + env[0][2]])
        worst = np.maximum(worst, err / bound)
        assert (err <= bound).all(), (c["name"], err, bound)
        n += 1
    print("\n  manifold against the portal search, %d corner-on-face cases: worst error / bound dist %.3f normal %.3f" % (n, worst[0], worst[1]))
    assert n >= 12


# ---- invariants -------------------------------------------------------------------------------------------------------------------------
def test_invariants_on_random_configurations():
    rng = np.random.default_rng(11)
    counts = collections.Counter()
    for k in range(3000):
        hA, hB = rng.uniform(0.03, 0.3, 3), rng.uniform(0.03, 0.3, 3)
        mA = _rot(_qrand(rng))
        if k % 2:
            mB = _rot(_qrand(rng))
        else:  # face-aligned: turned about A's z, axes permuted, tilted a little
            mB = mA @ _rot(_qaxis([0, 0, 1], rng.uniform(0, 2 * np.pi))) @ np.eye(3)[:, rng.permutation(3)] @ _rot(_qaxis(rng.standard_normal(3), 0.02))
            if np.linalg.det(mB) < 0:
                mB[:, 0] = -mB[:, 0]
        pA = rng.standard_normal(3)
        pB = pA + mA @ (rng.uniform(-1, 1, 3) * (hA + 0.8 * hB))
        labels = []
        con = boxbox_ref.box_box(MARGIN, pA, mA, hA, pB, mB, hB, labels)
        counts[len(con)] += 1
        assert len(con) <= 8 and "box-box:capped" not in labels
        for c in con:
            grow = abs(c["dist"]) / 2 + MARGIN / 2 + 1e-12
            assert (np.abs(mA.T @ (c["pos"] - pA)) <= hA + grow).all() and (np.abs(mB.T @ (c["pos"] - pB)) <= hB + grow).all(), (k, labels)
        swapped = boxbox_ref.box_box(MARGIN, pB, mB, hB, pA, mA, hA)
        assert len(swapped) == len(con), (k, labels)
        if con and any(lab.startswith("box-box:face") for lab in labels):
            left = list(swapped)
            for c in con:
                m = next((s for s in left if abs(s["dist"] - c["dist"]) <= 1e-12 and np.abs(s["pos"] - c["pos"]).max() <= 1e-12), None)
                assert m is not None and np.abs(m["normal"] + c["normal"]).max() <= 1e-12, (k, labels)
                left.remove(m)
    assert set(counts) == set(range(9)), counts
    c = np.sqrt(0.5)
    eight = boxbox_ref.box_box(MARGIN, np.zeros(3), np.eye(3), [0.1, 0.1, 0.1], [0, 0, 0.195], np.array([[c, -c, 0], [c, c, 0], [0, 0, 1.0]]), [0.1, 0.1, 0.1])
    assert len(eight) == 8 and all(k["src"] == "c" and abs(k["dist"] + 0.005) <= 1e-15 for k in eight)


# ---- the case table ---------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_what_it_must_and_is_conditioned(hbmod, ref, tmp_path_factory):
    cases, info = ref["cases"], ref["info"]
    assert len(cases) >= 120 and len({c["name"] for c in cases}) == len(cases)
    face = [c for c in cases if c["kind"] == "face"]
    assert {4, 5, 6, 7} <= {c["count"] for c in face}
    assert {1, 2, 3} <= {c["sides"] for c in face if c["source"] == "drawn"}
    assert {c["ref"] for c in face} == {"A", "B"} and {c["face"] for c in face} == {"-x", "+x", "-y", "+y", "-z", "+z"}
    edges = [c for c in cases if c["kind"] == "edge"]
    assert len({c["axes"] for c in edges}) >= 4 and all(c["count"] == 1 for c in edges)
    for kind in ("face", "edge"):  # penetrating and in the margin; outside: separated
        d = [ref["evals"][i][0]["con"][0]["dist"] for i, c in enumerate(cases) if c["kind"] == kind and not c["exact"]]
        assert min(d) < 0 < max(d) <= MARGIN
    assert sum(c["kind"] == "separated" for c in cases) >= 10 and sum(c["exact"] for c in cases) == 7
    for c in cases:
        if not c["exact"]:
            least, _ = boxbox_cases.conditioning(info, c)
            assert least >= boxbox_cases.GUARD, (c["name"], least)
    nonexact = np.array([not c["exact"] for c in cases])
    assert ref["ill"][nonexact].mean() <= 0.05, ref["ill"].sum()
    assert all(len(ev) == (1 if c["exact"] else 33) for ev, c in zip(ref["evals"], cases))
    # the octagon scene: eight contacts with either box the reference, and nothing ill-conditioned
    octo = boxbox_cases.reference(hbmod, "pgs", tmp_path_factory.mktemp("boxbox_oct"), octagon=True)
    assert {(c["count"], c["ref"]) for c in octo["cases"]} >= {(8, "A"), (8, "B")} and not octo["ill"].any()
    for c in octo["cases"]:
        assert boxbox_cases.conditioning(octo["info"], c)[0] >= boxbox_cases.GUARD


# ---- the mode flag ------------------------------------------------------------------------------------------------------------------------
def test_setter_query_and_the_model_file(hbmod, tmp_path):
    m = hbmod.Model.from_xml_string(box_cases.scene_xml("pgs"))
    sizes = [(n, getattr(m, n)) for n, _ in engine.HbSizes._fields_]
    before, after, on = tmp_path / "before.hbm", tmp_path / "after.hbm", tmp_path / "on.hbm"
    m.save(before)
    assert m.box_manifold() == 0 and m.box_manifold(1) == 1 and m.box_manifold() == 1 and m.box_manifold(-1) == 1
    m._read_sizes()
    assert sizes == [(n, getattr(m, n)) for n, _ in engine.HbSizes._fields_]
    m.save(on)
    assert m.box_manifold(0) == 0 and m.box_manifold() == 0
    m.save(after)
    assert before.read_bytes() == after.read_bytes() and b"box_manifold" not in before.read_bytes()
    assert on.read_bytes().count(b"i box_manifold 1\n") == 1 and on.read_bytes().replace(b"i box_manifold 1\n", b"") == before.read_bytes()
    assert hbmod.Model.load(on).box_manifold() == 1 and hbmod.Model.load(before).box_manifold() == 0
    for bad in (2, -2, 7):
        with pytest.raises(hbmod.HbError, match="mode must be 1 .on., 0 .off. or -1 .query."):
            m.box_manifold(bad)
        assert m.box_manifold() == 0
    edited = tmp_path / "edited.hbm"
    edited.write_bytes(on.read_bytes().replace(b"i box_manifold 1\n", b"i box_manifold 2\n"))
    with pytest.raises(hbmod.HbError, match="box_manifold must be 0 or 1"):
        hbmod.Model.load(edited)


def test_shipped_models_keep_their_bytes(hbmod, tmp_path):
    from oracle_lib import HUMANOID_HBM
    m = hbmod.Model.load(HUMANOID_HBM)
    assert m.box_manifold() == 0
    m.save(tmp_path / "h.hbm")
    assert (tmp_path / "h.hbm").read_bytes() == open(HUMANOID_HBM, "rb").read()


def _table_lines(path):
    rc, out = _tables(path)
    assert rc == 0, out
    return out


def test_device_tables(hbmod, tmp_path):
    """a model without a box - box candidate pair accepts the mode and builds the tables it built before (DevModel::box_manifold stays 0);
    with such a pair only the flag differs"""
    stairs = hbmod.Model.load(os.path.join(MODELS_DIR, "box_stairs.xml"))
    plane_only = hbmod.Model.from_xml_string('<mujoco><worldbody><geom type="plane" size="0 0 1"/><body pos="0 0 1"><freejoint/><geom type="box" size="0.1 0.2 0.3"/></body>'
                                             '<body pos="1 0 1"><freejoint/><geom type="capsule" size="0.1 0.2"/></body></worldbody></mujoco>')
    for name, m, has_pair in (("plane_only", plane_only, False), ("stairs", stairs, True)):
        off, on = tmp_path / (name + "_off.hbm"), tmp_path / (name + "_on.hbm")
        m.save(off)
        assert m.box_manifold(1) == 1
        m.save(on)
        a, b = _table_lines(off), _table_lines(on)
        assert fields(a)["box_manifold"] == 0 and fields(b)["box_manifold"] == (1 if has_pair else 0)
        assert a.replace("box_manifold 0", "box_manifold %d" % has_pair) == b, name
