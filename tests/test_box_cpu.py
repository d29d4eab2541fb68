"""(CPU) Box geoms before any device sees them: the compiler and the model file, the fp64 reference tests/box_ref.py held to independent
restatements, and the case table of tests/box_cases.py proven on the references alone.

  - compiler: a box model compiles; mass and inertia equal the closed form to 1e-12; rbound = |size|, geom_half = size (build/hb_tables);
    the .hbm round-trips; the shipped assets (no boxes) load and save to the bytes they have; bad sizes are refused with their location; a
    cylinder pair is still refused; the variant is general; a 30-dof box model gets the existing message;
  - box_ref.plane_box against a direct enumeration, the four-contact cap and the corner order; box_ref.sphere_box against a brute-force
    closest point over a sampled surface (tolerance derived from the pitch) and under the 48 signed axis permutations; box_ref.ray_box
    against the twelve triangles of the box through ray_ref's triangle routine, along a face, through an edge and from inside;
  - twin agreement: the oracle on the MESH TWIN is the reference of the portal-search pairs; the plane - box cases where plane_box and the
    oracle's plane - hull collider give the same contacts to 1e-9 are listed (at least 20); every branch label is taken at least twice;
  - conditioning: every case's envelope under one fp32 rounding of qpos (as tests/test_pair_cases_cpu.py), at most 5 % ill-conditioned.

box_cases.reference() is what tests/test_gpu_box.py holds the device to.
"""
import collections
import itertools
import os

import numpy as np
import pytest

import box_cases
import box_ref
import pair_ref
import ray_ref
from box_cases import ANALYTIC, analytic, reference, twin_agreement
from oracle_lib import ASSETS, GOLDEN, MODELS_DIR, parse_hbm
from pair_cases import GUARD, envelope
from tables_lib import GENERAL_28, STAGED, fields, run as _tables


def _xml(body, option="", tail=""):
    return '<mujoco model="t"><option timestep="0.004" %s/><worldbody><geom name="floor" type="plane" size="0 0 1"/>%s</worldbody>%s</mujoco>' % (option, body, tail)


BOX_BODY = '<body name="b" pos="0 0 1"><freejoint/><geom name="g" type="box" size="0.1 0.2 0.3" %s/></body>'


# ---- compiler and model file -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attr,mass", [('density="700"', 700 * 8 * 0.1 * 0.2 * 0.3), ('mass="2.5"', 2.5)])
def test_box_compiles_with_the_solid_box_inertia(hbmod, attr, mass):
    m = hbmod.Model.from_xml_string(_xml(BOX_BODY % attr))
    assert np.asarray(m.array("geom_type")).astype(int).tolist() == [0, 6]
    assert np.array_equal(np.asarray(m.array("geom_size")).reshape(-1, 3)[1], [0.1, 0.2, 0.3])
    assert abs(m.array("body_mass")[1] - mass) <= 1e-12 * mass
    want = mass / 3 * np.array([0.2 ** 2 + 0.3 ** 2, 0.1 ** 2 + 0.3 ** 2, 0.1 ** 2 + 0.2 ** 2])
    assert np.abs(np.asarray(m.array("body_inertia")).reshape(-1, 3)[1] - want).max() <= 1e-12
    assert abs(m.array("geom_rbound")[1] - np.sqrt(0.01 + 0.04 + 0.09)) <= 1e-15


def test_box_from_a_defaults_class(hbmod):
    xml = ('<mujoco><default><default class="brick"><geom type="box" size="0.3 0.2 0.1" mass="1"/></default></default><worldbody>'
           '<body pos="0 0 1"><freejoint/><geom class="brick"/></body><body pos="1 0 1" childclass="brick"><freejoint/><geom size="0.1 0.1 0.2"/></body></worldbody></mujoco>')
    m = hbmod.Model.from_xml_string(xml)
    assert np.asarray(m.array("geom_type")).astype(int).tolist() == [6, 6]
    assert np.array_equal(np.asarray(m.array("geom_size")).reshape(-1, 3), [[0.3, 0.2, 0.1], [0.1, 0.1, 0.2]])


def test_hbm_round_trip_of_a_box_model(hbmod, tmp_path):
    m = hbmod.Model.from_xml_string(box_cases.scene_xml("pgs"))
    a, b = str(tmp_path / "a.hbm"), str(tmp_path / "b.hbm")
    m.save(a)
    hbmod.Model.load(a).save(b)
    assert open(a, "rb").read() == open(b, "rb").read()
    info = parse_hbm(a)
    assert sorted(set(info["geom_type"].tolist())) == [0, 1, 2, 3, 6]


@pytest.mark.parametrize("name", ["humanoid27.hbm", "humanoid27_hfield.hbm", "team_robot.hbm", "team_robot_plane.hbm"])
def test_models_without_boxes_keep_their_bytes(hbmod, tmp_path, name):
    """the shipped assets were written by earlier builds: loading and saving one must give the same bytes"""
    out = str(tmp_path / name)
    hbmod.Model.load(os.path.join(ASSETS, name)).save(out)
    assert open(out, "rb").read() == open(os.path.join(ASSETS, name), "rb").read()


def test_a_model_without_boxes_compiles_to_the_parents_bytes(hbmod, tmp_path):
    """tests/golden/pairs_hfield.hbm is the "hfield" pair scene of tests/pair_cases.py as the build before box geoms compiled it"""
    import pair_cases
    out = str(tmp_path / "pairs.hbm")
    hbmod.Model.from_xml_string(pair_cases.scene_xml("hfield")).save(out)
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "pairs_hfield.hbm"), "rb").read()


@pytest.mark.parametrize("size", ["0.1 0.2", "0.1", "0.1 0.2 0", "0.1 -0.2 0.3", ""])
def test_bad_size_is_refused_with_its_location(hbmod, size):
    body = '<body name="b" pos="0 0 1"><freejoint/><geom name="brick" type="box" %s mass="1"/></body>' % ('size="%s"' % size if size else "")
    with pytest.raises(hbmod.HbError, match="box needs three positive half extents in size in .*brick"):
        hbmod.Model.from_xml_string(_xml(body))


def test_an_ellipsoid_is_still_not_a_geom_type(hbmod):
    body = '<body pos="0 0 1"><freejoint/><geom name="e" type="ellipsoid" size="0.1 0.2 0.3" mass="1"/></body>'
    with pytest.raises(hbmod.HbError, match="geom type 'ellipsoid' is not supported .*box"):
        hbmod.Model.from_xml_string(_xml(body))


def test_cylinder_pair_is_still_refused(hbmod):
    body = '<body pos="0 0 1"><freejoint/><geom name="c" type="cylinder" size="0.1 0.2" mass="1"/></body>'
    with pytest.raises(hbmod.HbError, match="cylinder / ellipsoid colliders are not implemented") as e:
        hbmod.Model.from_xml_string(_xml(body))
    assert "box" not in str(e.value)


def test_variant_is_general_and_geom_half_is_the_box(hbmod, tmp_path):
    for k, (option, variant) in enumerate((('solver="PGS"', 1), ('solver="Newton"', 2))):
        p = tmp_path / ("m%d.xml" % k)
        p.write_text(_xml(BOX_BODY % 'mass="1"', option))
        dump = tmp_path / "t.bin"
        rc, out = _tables(p, "--dump", dump)
        assert rc == 0, out
        f = fields(out)
        assert f["variant"] == variant
        raw = open(dump, "rb").read()
        array, off, count, _ = f["table"]["geom_half"]
        assert (array, count) == ("float", 6)
        # (the dump: "HBTABLE1", the DevModel, the int array, the float array - each behind its u64 length)
        pos = 8
        n = int(np.frombuffer(raw, "<u8", 1, pos)[0]); pos += 8 + n
        n = int(np.frombuffer(raw, "<u8", 1, pos)[0]); pos += 8 + 4 * n
        n = int(np.frombuffer(raw, "<u8", 1, pos)[0]); pos += 8
        fv = np.frombuffer(raw, "<f4", n, pos)
        assert np.array_equal(fv[off + 3:off + 6], np.array([0.1, 0.2, 0.3], dtype=np.float32))


def test_30_dof_box_model_gets_the_existing_message(tmp_path):
    bodies = "".join('<body pos="%d 0 1"><freejoint/><geom type="box" size="0.1 0.2 0.3" mass="1"/></body>' % k for k in range(5))
    p = tmp_path / "m.xml"
    p.write_text(_xml(bodies))
    assert _tables(p) == (1, "refused: " + GENERAL_28 + "\n")


@pytest.mark.parametrize("what,options,message", [
    ("friction loss", (), 'friction loss: %sremove the joints\' frictionloss or set <flag frictionloss="disable"/>'),
    ("equality", (), 'equality constraints: %sremove the <equality> section or set <flag equality="disable"/>'),
    ("RK4", ("--integrator", 1), "RK4: %suse the Euler integrator")])
def test_variant_rules_refuse_a_box_model(tmp_path, what, options, message):
    """The existing refusals of a model that steps in stages, word for word (tests/test_device_tables_cpu.py pins the strings).  They name
    what made a model general before boxes - "mesh hulls, height fields or condim 4 / 6" - and not the box that this model has: DESIGN.md
    3.6a and INTEGRATION.md say that a colliding box belongs in that list."""
    hinges = "".join('<body pos="%d 0 1"><joint name="j%d" type="hinge" axis="0 1 0" %s/><geom type="box" size="0.1 0.2 0.3" mass="1"/></body>'
                     % (k, k, 'frictionloss="0.1"' if what == "friction loss" else "") for k in range(2))
    tail = '<equality><joint joint1="j0" joint2="j1"/></equality>' if what == "equality" else ""
    p = tmp_path / "m.xml"
    p.write_text(_xml(hinges, tail=tail))
    assert _tables(p, *options) == (1, "refused: " + message % STAGED + "\n")


def test_the_stairs_model_file_is_the_generators(hbmod):
    """tests/models/box_stairs.xml is box_cases.stairs_xml() written out: four box steps, a box-footed biped, a brick - 16 dofs"""
    text = open(os.path.join(MODELS_DIR, "box_stairs.xml")).read()
    assert text == box_cases.stairs_xml()
    m = hbmod.Model.load(os.path.join(MODELS_DIR, "box_stairs.xml"))
    assert (m.nv, m.nu) == (16, 4) and (np.asarray(m.array("geom_type")) == 6).sum() == 8 and m.nv <= 28


# ---- box_ref against independent restatements ----------------------------------------------------------------------------------------
def _rot(rng):
    return pair_ref.quat2mat(box_cases._qrand(rng))


def test_plane_box_against_a_direct_enumeration():
    rng = np.random.default_rng(1)
    h = np.array([0.1, 0.06, 0.04])
    seen = collections.Counter()
    for k in range(300):
        R = _rot(rng) if k % 3 else np.eye(3)[:, rng.permutation(3)] * rng.choice([-1.0, 1.0], 3)  # (every third: a face flat on the plane)
        n = _rot(rng)[:, 2]
        ppos, bpos = rng.standard_normal(3), rng.standard_normal(3)
        bpos += n * (rng.uniform(-0.05, 0.15) - (bpos - ppos) @ n)
        margin = 0.01
        got = box_ref.plane_box(margin, ppos, n, bpos, R, h)
        # separately: world corners by x, then y, then z sign (x fastest), signed heights, the first four that qualify
        want = []
        for sz, sy, sx in itertools.product((-1, 1), repeat=3):
            w = bpos + R[:, 0] * sx * h[0] + R[:, 1] * sy * h[1] + R[:, 2] * sz * h[2]
            height = (w - ppos) @ n
            if (w - bpos) @ n <= 0 and height <= margin and len(want) < 4:
                want.append((height, w - 0.5 * height * n))
        assert len(got) == len(want) <= 4
        for a, (d, p) in zip(got, want):
            assert abs(a["dist"] - d) <= 1e-14 and np.abs(a["pos"] - p).max() <= 1e-14 and np.array_equal(a["normal"], n)
        assert [a["corner"] for a in got] == sorted(a["corner"] for a in got)
        seen[len(got)] += 1
    assert all(seen[c] >= 2 for c in range(5)), seen
    # the cap: a box wholly under the plane has eight qualifying corners (ldist <= 0 for four of them only: 4), a flat one in the margin four
    labels = []
    assert len(box_ref.plane_box(0.01, np.zeros(3), np.array([0, 0, 1.0]), np.array([0, 0, 0.041]), np.eye(3), h, labels)) == 4 and "plane-box:4" in labels


def test_sphere_box_against_brute_force_and_its_symmetries():
    rng = np.random.default_rng(2)
    h = np.array([0.1, 0.06, 0.04])
    # surface samples at pitch p on every face: the nearest sample to the true closest point is within p sqrt(2) / 2 of it in the face,
    # so the sampled distance exceeds the true one by at most that (and is never smaller): TOL = p sqrt(2) / 2 on dist, and the position,
    # midway between surfaces along a normal that turns by at most TOL / d, moves by no more than TOL (1 + r / d) / 2
    pitch = 0.002
    tol = pitch * np.sqrt(2) / 2
    pts = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        ub, uc = np.arange(-h[b], h[b] + 1e-12, pitch), np.arange(-h[c], h[c] + 1e-12, pitch)
        ub, uc = np.append(ub, h[b]), np.append(uc, h[c])
        gb, gc = np.meshgrid(ub, uc)
        for s in (-1, 1):
            f = np.zeros((gb.size, 3))
            f[:, a], f[:, b], f[:, c] = s * h[a], gb.ravel(), gc.ravel()
            pts.append(f)
    pts = np.concatenate(pts)
    r = 0.07
    for k in range(200):
        inside = k % 4 == 0
        c = h * rng.uniform(-0.95, 0.95, 3) if inside else h * rng.uniform(-1, 1, 3) + rng.choice([-1, 1], 3) * rng.uniform(0, 0.1, 3) * (rng.uniform(size=3) < 0.6)
        got = box_ref.sphere_box(10.0, c, r, np.zeros(3), np.eye(3), h)
        d = np.linalg.norm(pts - c, axis=1)
        i = int(np.argmin(d))
        is_in = bool((np.abs(c) <= h).all())
        want = (-d[i] if is_in else d[i]) - r
        assert -1e-12 <= (got["dist"] - want) * (-1 if not is_in else 1) <= tol, (c, got["dist"], want)
        if not is_in and d[i] > 10 * tol:
            n = (pts[i] - c) / d[i]
            assert np.abs(got["normal"] - n).max() <= 2 * tol / d[i]
            assert np.abs(got["pos"] - (c + n * (r + want / 2))).max() <= tol * (1 + r / d[i])
    # the 48 signed axis permutations of box and centre give the permuted contact
    for k in range(20):
        c = h * rng.uniform(-1.5, 1.5, 3) if k % 2 else h * rng.uniform(-0.9, 0.9, 3)
        base = box_ref.sphere_box(1.0, c, r, np.zeros(3), np.eye(3), h)
        for perm in itertools.permutations(range(3)):
            for sg in itertools.product((-1.0, 1.0), repeat=3):
                Pm = np.zeros((3, 3))
                for i in range(3):
                    Pm[i, perm[i]] = sg[i]
                got = box_ref.sphere_box(1.0, Pm @ c, r, np.zeros(3), np.eye(3), np.abs(Pm @ h))
                assert abs(got["dist"] - base["dist"]) <= 1e-15 and np.abs(got["pos"] - Pm @ base["pos"]).max() <= 1e-15 and np.abs(got["normal"] - Pm @ base["normal"]).max() <= 1e-15
    # the same through a rotated, displaced box
    R, p = _rot(rng), rng.standard_normal(3)
    c = np.array([0.13, -0.02, 0.05])
    a, b = box_ref.sphere_box(1.0, c, r, np.zeros(3), np.eye(3), h), box_ref.sphere_box(1.0, p + R @ c, r, p, R, h)
    assert abs(a["dist"] - b["dist"]) <= 1e-14 and np.abs(p + R @ a["pos"] - b["pos"]).max() <= 1e-14 and np.abs(R @ a["normal"] - b["normal"]).max() <= 1e-14
    # the tie between faces: the first of -x, +x, -y, +y, -z, +z
    lab = []
    got = box_ref.sphere_box(1.0, np.zeros(3), r, np.zeros(3), np.eye(3), h, lab)
    assert "sphere-box:face-z" in lab and np.array_equal(got["normal"], [0, 0, 1.0]) and abs(got["dist"] + 0.04 + r) <= 1e-15


def _box_triangles(h):
    c = box_ref.corners(h)
    quads = [(0, 2, 6, 4), (1, 3, 7, 5), (0, 1, 5, 4), (2, 3, 7, 6), (0, 1, 3, 2), (4, 5, 7, 6)]
    return np.array([[c[q[0]], c[q[i]], c[q[i + 1]]] for q in quads for i in (1, 2)])


def test_ray_box_against_its_twelve_triangles():
    rng = np.random.default_rng(3)
    h = np.array([0.1, 0.06, 0.04])
    tris = _box_triangles(h)
    assert len(tris) == 12
    rays = []
    for k in range(300):
        o = rng.standard_normal(3) * 0.3 if k % 3 else h * rng.uniform(-0.9, 0.9, 3)  # (every third from inside)
        t = h * rng.uniform(-1.2, 1.2, 3)
        rays.append((o, (t - o) / np.linalg.norm(t - o)))
    rays.append((np.array([-1.0, 0.03, h[2]]), np.array([1.0, 0, 0])))            # along the +z face
    rays.append((np.array([-1.0, h[1], h[2]]), np.array([1.0, 0, 0])))            # along an edge
    rays.append((np.array([-1.0, 0.02, h[2] + 1.0]), np.array([1.0, 0, -1.0]) / np.sqrt(2)))  # through the edge x = -hx, z = hz
    rays.append((np.zeros(3), np.array([0, 0, 1.0])))                             # from the centre
    labels = []
    for o, d in rays:
        got, _ = box_ref.ray_box(o, d, h, labels)
        cands = ray_ref._geom_candidates(ray_ref.HFIELD, None, o, d, tris)
        want = min(x for x, _ in cands) if cands else None
        assert (got is None) == (want is None), (o, d, got, want)
        if got is not None:
            assert abs(got - want) <= 1e-12, (o, d, got, want)
    hist = collections.Counter(labels)
    assert all(hist["ray-box:" + k] >= 2 for k in ("miss", "inside", "outside")), hist
    assert abs(box_ref.ray_box(*rays[-1], h)[0] - h[2]) <= 1e-15 and abs(box_ref.ray_box(*rays[-4], h)[0] - 0.9) <= 1e-15


def test_support_and_lowest_point():
    rng = np.random.default_rng(4)
    h = np.array([0.1, 0.06, 0.04])
    c = box_ref.corners(h)
    tie = c @ np.array([0.41421356237309503, 0.7320508075688772, 1.0])  # (hb_mpr.hpp: hull_tie)
    for k in range(200):
        ld = rng.standard_normal(3)
        if k % 2:
            ld[rng.integers(3)] = 0.0
        if k % 8 == 1:
            ld[rng.integers(3)] = -0.0
        v = c @ ld
        best = np.flatnonzero(v == v.max())
        want = c[best[np.argmax(tie[best])]]  # the hull's rule: the largest value, ties to the corner ahead along the tie direction
        assert np.array_equal(box_ref.support(h, ld), want), ld
        R = _rot(rng)
        assert abs(box_ref.lowest_point(h, R) - (c @ R.T)[:, 2].min()) <= 1e-15


# ---- the case table on the references alone (box_cases.reference) ------------------------------------------------------------------
@pytest.fixture(scope="module", params=("pgs", "mesh", "xfirst", "xfirst_mesh"))
def ref(request, hbmod, tmp_path_factory):
    return reference(hbmod, request.param, tmp_path_factory.mktemp("boxes"))


def test_pair_kinds_come_in_both_body_orders(hbmod, tmp_path_factory):
    """sphere - box in one scene (S between P and Q); capsule - box and box - mesh across the scenes with X behind and ahead of the boxes;
    box - box with the contacted face on the lower and on the higher geom id"""
    d = tmp_path_factory.mktemp("boxes")
    seen = collections.defaultdict(set)
    for v in ("pgs", "mesh", "xfirst", "xfirst_mesh"):
        r = reference(hbmod, v, d)
        body = r["info"]["geom_bodyid"]
        for c in r["cases"]:
            if c["kind"] in ("sphere-box", "capsule-box", "box-mesh") and 0 not in (body[c["geoms"][0]], body[c["geoms"][1]]):
                seen[c["kind"]].add(bool(body[c["geoms"][0]] < body[c["geoms"][1]]))
            if c["kind"] == "box-box" and not c["exact"]:
                seen["box-box face owner"].add(c["name"].split()[0] in ("W-P", "W-Q", "P-Q"))
    assert all(seen[k] == {True, False} for k in ("sphere-box", "capsule-box", "box-mesh", "box-box face owner")), dict(seen)


def test_twins_have_the_same_bodies(ref):
    a, b, tw = ref["info"], ref["twin_info"], ref["oracle"]
    names = list(a["body_name"])
    for k in ("body_mass", "body_inertia", "body_ipos", "body_iquat"):
        w = 1 if k == "body_mass" else len(a[k]) // len(names)
        for tb, n in enumerate(b["body_name"]):
            assert np.array_equal(b[k][w * tb:w * tb + w], a[k][w * names.index(n):w * names.index(n) + w]), (k, n)
    # the same candidate pairs, each in the same order of its two geoms (the order the portal search takes them in)
    mine = set(zip(a["pair_geom1"].tolist(), a["pair_geom2"].tolist()))
    theirs = {(tw.geom[g1], tw.geom[g2]) for g1, g2 in zip(b["pair_geom1"].tolist(), b["pair_geom2"].tolist())}
    assert mine == theirs and tw.same_order == (ref["model"].id2name("body", 1) != "X" or b["nmesh"] == 3)
    assert (ref["model"].nq, ref["model"].nv) == (28, 24)


def test_case_table_and_twin_agreement(ref):
    cases = ref["cases"]
    kinds = collections.Counter(c["kind"] for c in cases)
    print("\n%d cases: %s" % (len(cases), dict(kinds)))
    assert 150 <= len(cases) <= 200
    want = {"plane-box", "sphere-box", "box-box", "hfield-box", "box-mesh" if ref["twin_info"]["nmesh"] == 4 else "capsule-box"}
    assert sum(twin_agreement(ref).values()) >= 20  # (those the twin lists in the box's corner order: what a PGS step can be compared on)
    assert set(kinds) == want, kinds
    agree = twin_agreement(ref)
    print("plane - box cases whose contacts the oracle's plane - hull collider gives too: %d of %d" % (len(agree), kinds["plane-box"]))
    for i in agree:
        print("  " + cases[i]["name"])
    assert len(agree) >= 20
    # one pair in range, the pair under test; portal-search contacts off the activation boundary
    counts = collections.Counter()
    for c, ev in zip(cases, ref["evals"]):
        for x in ev[0]["con"]:
            assert (x["geom1"], x["geom2"]) == c["geoms"], c["name"]
            if c["kind"] not in ANALYTIC:
                assert x["dist"] < box_cases.MARGIN - GUARD, (c["name"], x["dist"])
        assert (ev[0]["ncon"] > 0) == ("outside" not in c["name"]), (c["name"], ev[0]["ncon"])
        counts[(c["kind"], ev[0]["ncon"])] += 1
    print(sorted(counts.items()))


def test_every_branch_is_taken_at_least_twice_and_off_its_boundary(ref):
    hist = collections.Counter()
    worst = np.inf
    for c in ref["cases"]:
        if c["kind"] not in ANALYTIC:
            continue
        labels, tests = [], []
        analytic(ref["info"], c["qpos"], c["geoms"], labels, tests)
        hist.update(set(labels))
        for t in tests:
            if t[0] == "corner":  # a corner that is low enough to count is clear of the margin and of ldist = 0
                if t[3] <= GUARD and not c["exact"]:
                    assert abs(t[1] - t[2]) > GUARD, (c["name"], t)
                    worst = min(worst, abs(t[1] - t[2]))
                if t[1] <= t[2] + GUARD:
                    assert abs(t[3]) > GUARD, (c["name"], t)
            else:
                assert abs(t[1] - t[2]) > GUARD, (c["name"], t)
                worst = min(worst, abs(t[1] - t[2]))
    print("\nbranch histogram:", sorted(hist.items()), "\nclosest activation test %.3e m off its threshold" % worst)
    need = ["plane-box:%d" % k for k in (0, 1, 2, 4)] + ["sphere-box:inside", "sphere-box:outside"] + ["sphere-box:clamped%d" % k for k in (1, 2, 3)]
    need += ["sphere-box:face" + f for f in box_ref.FACES]
    assert all(hist[k] >= 2 for k in need), {k: hist[k] for k in need}
    assert min(hist.values()) >= 2, hist


def test_conditioning_envelopes(ref):
    cases, ill = ref["cases"], ref["ill"]
    exact = np.array([c["exact"] for c in cases])
    assert exact.sum() >= 6 and not ill[exact].any()
    share = ill.mean()
    print("\nill-conditioned cases: %d of %d = %.1f %%" % (ill.sum(), len(cases), 100 * share))
    for i in np.flatnonzero(ill):
        print("  %-60s counts %s" % (cases[i]["name"], sorted({e["ncon"] for e in ref["evals"][i]})))
    assert share <= 0.05
    by = collections.defaultdict(lambda: np.zeros(3))
    for i, c in enumerate(cases):
        e = envelope(ref, i, ref["evals"][i][0]["ncon"])[1]
        if len(e):
            by[c["kind"]] = np.maximum(by[c["kind"]], e.max(axis=0))
    for k, e in sorted(by.items()):
        print("  largest envelope %-12s dist %.2e pos %.2e normal %.2e" % (k, e[0], e[1], e[2]))
