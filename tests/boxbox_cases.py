"""The box - box MANIFOLD case table and its reference (tests/test_boxbox_cpu.py, tests/test_gpu_boxbox.py): the scene of tests/box_cases.py
(scene_xml: the static box W and the free boxes P and Q; the other bodies parked as there), only the box - box poses are new.

TEST INFRASTRUCTURE.  build_cases(info, variant): a case is a name, the two geoms under test, a full qpos rounded to fp32, whether it is
EXACT, and what boxbox_ref.box_box does with it (labels, count).  The table holds
  - the box - box cases of box_cases.build_cases themselves (a corner or an edge of one box over a face of the other, three depths; the
    axis-aligned EXACT cases), so that the manifold and the portal search are held on the same states;
  - face on face: the second box's face `oface` turned by a yaw about the normal of face `face` of the first, tilted by 0.005 - 0.03 rad (no
    two corners level, and the larger face the reference), at a lateral offset, its lowest corner at the chosen gap - drawn from a seeded
    generator and KEPT only if it adds to what the table must cover: 4, 5, 6, 7 and 8 contacts, the incident box hanging over one, two and
    three sides, the reference box geom 1 and geom 2, each of the six faces the reference face;
  - edge - edge: two generic orientations, the second box moved along a generic direction until the largest separation is the gap, kept
    if the routine takes the edge case; per kept case the same pose moved along the contact normal into the margin and out of it;
  - EXACT partial overlaps: axis-aligned, dyadic offsets, one corner of each rectangle inside the other and two crossings.
Conditioning is held BY CONSTRUCTION: a drawn pose is kept only if every decision margin boxbox_ref records at the fp32-rounded state is at
least GUARD = 1e-5 from zero and its NPERT perturbed evaluations agree on the count; tests/test_boxbox_cpu.py asserts both on the
finished table.  One env per case.

reference(hbmod, variant, directory): the scene compiled with the mode ON (its own Model object) and boxbox_ref on every case with the
conditioning envelope of pair_cases.evaluations.
"""
import numpy as np

import box_cases
import boxbox_ref
import pair_ref
from box_cases import HALF, MARGIN, ROWS_PER_CONTACT, W_POS, bodies_of, scene_xml
from oracle_lib import parse_hbm
from pair_cases import _f32, _qaxis, _qmul, _qrand, evaluations

GUARD = 1e-5
DEPTHS = (("penetrating", -0.008), ("in the margin", 0.5 * MARGIN), ("outside", 1.6 * MARGIN))
FACES = ("-x", "+x", "-y", "+y", "-z", "+z")
# The scene's boxes cannot meet in an octagon: eight contacts need every corner of each face outside the other face AND every edge of one
# crossed twice, which for rectangles a x b and c x d asks a + b > sqrt(2) max(c, d) and c + d > sqrt(2) max(a, b) or nearly so, and no two
# faces of W, P and Q come close (54 000 drawn yaws and offsets over every face pair: none above seven).  The OCTAGON scene is the same
# text with Q's half extents replaced, P's +-z face (0.10 x 0.06) against Q's (0.11 x 0.07): eight contacts around a yaw of 45 degrees.
OCT_Q = (0.11, 0.07, 0.045)


def scene(variant, octagon=False):
    x = scene_xml(variant)
    if octagon:
        old = 'size="%g %g %g"' % HALF["Q"]
        assert x.count(old) == 1
        x = x.replace(old, 'size="%g %g %g"' % OCT_Q)
    return x


def mat2quat(R):
    """the unit quaternion (w, x, y, z) of a rotation matrix"""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return q / np.linalg.norm(q)


def evaluate_pair(info, qpos, geoms, labels=None, tests=None):
    """boxbox_ref.box_box on the pair under test at qpos, as Oracle.contacts() would list it"""
    gpos, gmat = pair_ref.geom_poses(info, qpos)
    g1, g2 = geoms
    size = info["geom_size"].reshape(-1, 3)
    margin = max(info["geom_margin"][g1], info["geom_margin"][g2])
    dim = int(max(info["geom_condim"][g1], info["geom_condim"][g2]))
    con = boxbox_ref.box_box(margin, gpos[g1], gmat[g1], size[g1], gpos[g2], gmat[g2], size[g2], labels, tests)
    return [dict(dist=c["dist"], pos=c["pos"], frame=c["normal"][None, :], dim=dim, geom1=int(g1), geom2=int(g2)) for c in con]


def _evaluate(info, case, qpos):
    con = evaluate_pair(info, qpos, case["geoms"])
    return dict(qpos=qpos, ncon=len(con), nefc=len(con) * ROWS_PER_CONTACT[con[0]["dim"]] if con else 0, con=con)


def conditioning(info, case):
    """(smallest |decision margin| of the case at its own state, labels)"""
    labels, tests = [], []
    evaluate_pair(info, case["qpos"], case["geoms"], labels, tests)
    return min(abs(v) for _, v in tests), labels


def describe(labels):
    """what a label list says: dict(kind 'separated' / 'edge' / 'face', count, ref 'A' / 'B', face '+z', sides: R's edges crossed, axes)"""
    d = dict(kind="separated", count=0, ref=None, face=None, sides=0, axes=None)
    for lab in labels:
        t = lab.split(":")[1]
        if t.startswith("edge"):
            d.update(kind="edge", axes=t.split()[1])
        elif t.startswith("face"):
            d.update(kind="face", ref=t.split()[1][0], face=t.split()[1][-1] + "xyz"[int(t.split()[1][1])])
        elif t.isdigit():
            d["count"] = int(t)
    return d


def build_cases(info, variant, octagon=False):
    half = dict(HALF, Q=OCT_Q) if octagon else HALF
    bodies = bodies_of(variant)
    names = list(info["geom_name"])
    gid = {n: names.index(n) for n in ("floor", "W") + bodies}
    body = {n: int(info["geom_bodyid"][gid[n]]) for n in bodies}
    qadr = {n: int(info["jnt_qposadr"][info["body_jntadr"][body[n]]]) for n in bodies}
    nq = 7 * len(bodies)
    p0 = info["geom_pos"][3 * gid["floor"]:3 * gid["floor"] + 3].copy()
    pm = pair_ref.quat2mat(info["geom_quat"][4 * gid["floor"]:4 * gid["floor"] + 4])
    e1, e2, nrm = pm[:, 0], pm[:, 1], pm[:, 2]
    rng = np.random.default_rng(20260101)
    qG = _qrand(rng)
    centre = p0 + nrm * 1.5 + 0.45 * e1 - 0.35 * e2
    cases = []

    def make(name, pair, poses, exact=False, source="drawn"):
        q = np.zeros(nq)
        for k, n in enumerate(bodies):
            pos, quat = poses[n] if n in poses else (p0 + nrm * (7.0 + 6.0 * k) + 0.3 * k * e1, _qaxis([1, 2, 3], 0.4 + k))
            q[qadr[n]:qadr[n] + 3] = pos
            q[qadr[n] + 3:qadr[n] + 7] = np.asarray(quat) / np.linalg.norm(quat)
        pair = tuple(sorted(pair, key=lambda n: gid[n]))  # as build_pairs lists two boxes: by geom id
        return dict(name=name, kind="box-box", pair=pair, geoms=tuple(gid[n] for n in pair), qpos=_f32(q), exact=exact, source=source)

    def finish(c):
        """the case with what the reference does with it, or None if it is not conditioned"""
        if not c["exact"]:
            least, labels = conditioning(info, c)
            if least < GUARD:
                return None
            counts = {len(evaluate_pair(info, c["qpos"] + 2.0 ** -24 * np.maximum(1.0, np.abs(c["qpos"])) * prng.standard_normal(nq), c["geoms"])) for _ in range(8)}
            if len(counts) > 1:
                return None
        else:
            labels = []
            evaluate_pair(info, c["qpos"], c["geoms"], labels)
        c.update(labels=tuple(labels), **describe(labels))
        return c

    prng = np.random.default_rng(5)
    # ---- the box - box cases of the box table itself
    for c in box_cases.build_cases(info, variant) if not octagon else ():
        if c["kind"] == "box-box":
            c = finish(dict(c, source="box_cases"))
            if c is not None:
                cases.append(c)

    def base_pose(a):
        return (W_POS, np.array([1.0, 0, 0, 0])) if a == "W" else (centre, _qmul(qG, _qaxis([1, 2, 3], 0.3)))

    def face_on_face(a, o, face, oface, yaw, lateral, tilt, gap):
        pa, qa = base_pose(a)
        Ra = pair_ref.quat2mat(qa)
        ha, ho = np.array(half[a]), np.array(half[o])
        fa, jo = face // 2, oface // 2
        nl = np.zeros(3)
        nl[fa] = 1.0 if face % 2 else -1.0
        t1, t2 = np.eye(3)[(fa + 1) % 3], np.eye(3)[(fa + 2) % 3]
        L = np.zeros((3, 3))  # o's axes in a's frame
        L[:, jo] = -nl * (1.0 if oface % 2 else -1.0)
        L[:, (jo + 1) % 3] = np.cos(yaw) * t1 + np.sin(yaw) * t2
        L[:, (jo + 2) % 3] = np.cross(L[:, jo], L[:, (jo + 1) % 3])
        tv = Ra @ (tilt[0] * t1 + tilt[1] * t2)
        Ro = pair_ref.quat2mat(_qaxis(tv, np.linalg.norm(tv))) @ Ra @ L
        nw = Ra @ nl
        low = min((Ro @ c) @ nw for c in _corners(ho))
        po = pa + Ra @ (nl * ha + lateral * ha * (nl == 0)) + nw * (gap - low)
        poses = {o: (po, mat2quat(Ro))}
        if a != "W":
            poses[a] = (pa, qa)
        return poses

    # ---- face on face, drawn and kept by what they add
    want = {}
    for n in (4, 5, 6, 7):  # (eight: the octagon scene)
        for r in "AB":
            want[("count", n, r)] = 5
    for f in FACES:
        for r in "AB":
            want[("face", f[0] + f[1], r)] = 2
    for k in (1, 2, 3):
        want[("sides", k)] = 5
    want[("outside",)] = 8
    owners = (("W", "P"), ("W", "Q"), ("P", "Q"), ("Q", "P"))
    if octagon:
        want = {("count", 8, "A"): 4, ("count", 8, "B"): 4, ("count", 7, "A"): 1, ("count", 7, "B"): 1, ("outside",): 2}
    for trial in range(4000):
        if not any(want.values()):
            break
        a, o = owners[rng.integers(4)] if not octagon else owners[2 + rng.integers(2)]
        face, oface = (int(rng.integers(6)), int(rng.integers(6))) if not octagon else (4 + int(rng.integers(2)), 4 + int(rng.integers(2)))
        yaw = rng.uniform(0, 2 * np.pi) if rng.random() < 0.6 else 0.5 * np.pi * rng.integers(4) + rng.uniform(-0.25, 0.25)
        lateral = rng.uniform(-1.1, 1.1, 3)
        if octagon:
            yaw, lateral = 0.25 * np.pi + 0.5 * np.pi * rng.integers(4) + rng.uniform(-0.2, 0.2), rng.uniform(-0.15, 0.15, 3)
        ang = rng.uniform(0, 2 * np.pi)
        tilt = rng.uniform(0.005, 0.03) * np.array([np.cos(ang), np.sin(ang)])
        tag, gap = DEPTHS[int(rng.integers(3))] if want[("outside",)] else DEPTHS[int(rng.integers(2))]
        c = make("%s-%s face %s on face %s, yaw %.2f, lateral (%.2f, %.2f), %s" % (o, a, FACES[oface], FACES[face], yaw, *lateral[(np.arange(3) != face // 2)], tag),
                 (a, o), face_on_face(a, o, face, oface, yaw, lateral, tilt, gap))
        quick = []
        evaluate_pair(info, c["qpos"], c["geoms"], quick)
        quick = describe(quick)
        if not ((quick["kind"] == "separated" and tag == "outside" and want[("outside",)]) or
                (quick["kind"] == "face" and (want.get(("count", quick["count"], quick["ref"]), 0) or want.get(("face", quick["face"], quick["ref"]), 0) or any(want.get(("sides", k), 0) for k in (1, 2, 3))))):
            continue
        c = finish(c)
        if c is None:
            continue
        if c["kind"] == "separated":
            keys = [("outside",)] if tag == "outside" else []
        elif c["kind"] == "face":
            c["sides"] = _count_sides(info, c)
            keys = [("count", c["count"], c["ref"]), ("face", c["face"], c["ref"])] + ([("sides", c["sides"])] if c["sides"] in (1, 2, 3) else [])
        else:
            keys = []
        keys = [k for k in keys if want.get(k, 0) > 0]
        if not keys:
            continue
        for k in keys:
            want[k] -= 1
        cases.append(c)
    # ---- edge - edge: generic orientations, moved along a generic direction until the largest separation is the gap
    per_axes = {}
    for trial in range(600 if not octagon else 0):
        if sum(per_axes.values()) >= 10 and len(per_axes) >= 5:
            break
        a, o = owners[rng.integers(4)]
        pa, qa = base_pose(a)
        qo = _qmul(qG, _qrand(rng))
        d = rng.standard_normal(3)
        d /= np.linalg.norm(d)

        def sep(r):
            return _max_sep(pa, pair_ref.quat2mat(qa), half[a], pa + d * r, pair_ref.quat2mat(qo), half[o])
        lo, hi = 0.0, 1.0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if sep(mid) < DEPTHS[0][1] else (lo, mid)
        poses = {o: (pa + d * hi, qo)}
        if a != "W":
            poses[a] = (pa, qa)
        c = finish(make("%s-%s edge on edge %d, %s" % (a, o, trial, DEPTHS[0][0]), (a, o), poses))
        if c is None or c["kind"] != "edge" or per_axes.get(c["axes"], 0) >= 2:
            continue
        # the same pose moved along the contact normal (from geom 1 to geom 2) into the margin and out of it
        con = evaluate_pair(info, c["qpos"], c["geoms"])[0]
        sign = 1.0 if gid[o] > gid[a] else -1.0
        more = []
        for tag, gap in DEPTHS[1:]:
            pz = {o: (pa + d * hi + sign * con["frame"][0] * (gap - con["dist"]), qo)}
            if a != "W":
                pz[a] = (pa, qa)
            m = finish(make("%s-%s edge on edge %d, %s" % (a, o, trial, tag), (a, o), pz))
            if m is not None and ((m["kind"] == "edge" and m["axes"] == c["axes"]) if tag != "outside" else m["kind"] == "separated"):
                more.append(m)
        if len(more) == 2:
            per_axes[c["axes"]] = per_axes.get(c["axes"], 0) + 1
            cases += [c] + more
    # ---- EXACT partial overlaps: identity quaternions, dyadic offsets; one corner of each rectangle inside the other, two crossings
    for k, (a, o, off) in enumerate((("W", "P", (0.25, 0.1875)), ("W", "Q", (-0.28125, 0.125)), ("P", "Q", (0.125, -0.09375)), ("P", "Q", (-0.09375, 0.15625))) if not octagon else ()):
        pa = W_POS if a == "W" else np.round(centre * 64) / 64
        ha, ho = np.array(half[a]), np.array(half[o])
        poses = {o: (pa + np.array([off[0], off[1], ha[2] + ho[2] - 0.0078125]), [1.0, 0, 0, 0])}
        if a != "W":
            poses[a] = (pa, [1.0, 0, 0, 0])
        cases.append(finish(make("%s-%s axis-aligned, partial overlap %d" % (a, o, k), (a, o), poses, exact=True, source="partial")))
    return cases


def _corners(h):
    return np.array([[h[0] if i & 1 else -h[0], h[1] if i & 2 else -h[1], h[2] if i & 4 else -h[2]] for i in range(8)])


def _max_sep(pA, mA, hA, pB, mB, hB):
    """the largest separation over the fifteen axes"""
    hA, hB = np.asarray(hA, dtype=np.float64), np.asarray(hB, dtype=np.float64)
    t = pB - pA
    axes = [mA[:, k] for k in range(3)] + [mB[:, k] for k in range(3)]
    for i in range(3):
        for j in range(3):
            c = np.cross(mA[:, i], mB[:, j])
            if c @ c >= boxbox_ref.EDGE_SKIP:
                axes.append(c / np.linalg.norm(c))
    return max(abs(t @ L) - np.abs(L @ mA) @ hA - np.abs(L @ mB) @ hB for L in axes)


def _count_sides(info, case):
    """how many sides of the reference rectangle the incident face hangs over: R's edges that carry a crossing, read off the (c) candidates"""
    tests = []
    evaluate_pair(info, case["qpos"], case["geoms"], None, tests)
    cr = [v for w, v in tests if w == "crossing"]
    tags = [w for w, v in tests if w.startswith("crossing")]
    assert len(cr) == 4 * 16 and len(tags) == 64, "a parallel pair in a drawn case"  # (drawn poses are tilted and turned: no pair is parallel)
    sides = set()
    for k in range(16):
        tq, _, tr, _ = cr[4 * k:4 * k + 4]
        if 0 < tq < 1 and 0 < tr < 1:
            sides.add(k % 4)
    return len(sides)


# ---------------------------------------------------------------------------------------------------------------- the reference
_cache, _tables = {}, {}


def reference(hbmod, variant, directory, octagon=False):
    """dict(model (the mode ON), path, info, cases, evals, ill) of a scene variant, computed once; what pair_cases.launch and held_to take.
    The table does not depend on the solver or condim: variants with the same geoms, bodies and qpos layout share one table."""
    if (variant, octagon) in _cache:
        return _cache[(variant, octagon)]
    m = hbmod.Model.from_xml_string(scene(variant, octagon))
    assert m.box_manifold(1) == 1
    p = str(directory / ("boxbox_%s%s.hbm" % (variant, "_oct" if octagon else "")))
    m.save(p)
    info = parse_hbm(p)
    layout = (octagon, tuple(info["geom_name"]), tuple(info["geom_bodyid"]), tuple(info["jnt_qposadr"]), tuple(info["geom_margin"]))
    if layout not in _tables:
        cases = build_cases(info, variant, octagon)
        _tables[layout] = (cases, evaluations(cases, lambda c, qpos: _evaluate(info, c, qpos)))
    cases, (evals, ill) = _tables[layout]
    dim = int(info["geom_condim"].max())  # (the evaluations' dim and nefc are the variant's own)
    evals = [[dict(e, nefc=e["ncon"] * ROWS_PER_CONTACT[dim], con=[dict(c, dim=dim) for c in e["con"]]) for e in ev] for ev in evals]
    ref = dict(model=m, path=p, info=info, cases=cases, evals=evals, ill=ill)
    _cache[(variant, octagon)] = ref
    return ref
