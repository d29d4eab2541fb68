"""fp64 reference, in numpy, of what a box geom adds ("Box geoms"): the analytic colliders plane - box and sphere - box, the
ray - box intersection and the box's support function, each with the BRANCH LABELS it took, as tests/pair_ref.py has them.

TEST INFRASTRUCTURE: the product package never imports this module.  The oracle cannot load a box; it loads the box's MESH TWIN (the
same MJCF with every box replaced by a mesh of its eight corners, tests/box_cases.py), and tests/test_box_cpu.py holds this module to it
where the two are defined alike.

    plane_box    corners i = 0..7, corner i = (i & 1 ? +hx : -hx, i & 2 ? +hy : -hy, i & 4 ? +hz : -hz); ldist = n . (corner - centre),
                 dist = n . (centre - plane_pos) + ldist; a corner with ldist > 0 or dist > margin is skipped; contact at
                 corner - n dist / 2 with the plane's normal; four at most, in corner order
    sphere_box   the centre clamped into the box in the box's frame.  Outside: normal from the centre to the clamped point (sphere ->
                 box), dist = d - r, position midway between the surfaces.  Inside: the face of least size[k] - |c[k]|, faces in the
                 order -x, +x, -y, +y, -z, +z and the first of the least kept; the normal is that face's inward one, dist = -least - r
    ray_box      the six faces; the nearest non-negative crossing that lies inside the other two extents (from inside: the exit face)
    support      (+-hx, +-hy, +-hz) by the signs of the local direction; a zero component takes +
"""
import numpy as np

MINVAL = 1e-15
GEOM_PLANE, GEOM_HFIELD, GEOM_SPHERE, GEOM_CAPSULE, GEOM_BOX, GEOM_MESH = 0, 1, 2, 3, 6, 7
FACES = ("-x", "+x", "-y", "+y", "-z", "+z")


def corners(half):
    """[8, 3] corners of the box in its own frame, in plane_box's order"""
    h = np.asarray(half, dtype=np.float64)
    return np.array([[h[0] if i & 1 else -h[0], h[1] if i & 2 else -h[1], h[2] if i & 4 else -h[2]] for i in range(8)])


def plane_box(margin, ppos, normal, bpos, bmat, half, labels=None, tests=None):
    """contacts (dicts of dist, pos, normal, corner) of a plane (ppos, unit normal) and a box at bpos with orientation bmat [3, 3]"""
    ppos, normal, bpos, bmat = (np.asarray(x, dtype=np.float64) for x in (ppos, normal, bpos, bmat))
    cdist = (bpos - ppos) @ normal
    out = []
    for i, c in enumerate(corners(half)):
        off = bmat @ c
        ldist = normal @ off
        dist = cdist + ldist
        if tests is not None:
            tests.append(("corner", dist, margin, ldist))
        if ldist > 0 or dist > margin:
            continue
        if len(out) == 4:
            if labels is not None:
                labels.append("plane-box:capped")
            break
        out.append(dict(dist=dist, pos=bpos + off - normal * (dist / 2), normal=normal.copy(), corner=i))
    if labels is not None:
        labels.append("plane-box:%d" % len(out))
    return out


def sphere_box(margin, spos, radius, bpos, bmat, half, labels=None, tests=None):
    """the contact (dict of dist, pos, normal) of a sphere (geom 1) and a box (geom 2), or None"""
    spos, bpos, bmat, h = (np.asarray(x, dtype=np.float64) for x in (spos, bpos, bmat, half))
    c = bmat.T @ (spos - bpos)
    cl = np.clip(c, -h, h)
    d = np.linalg.norm(cl - c)
    if tests is not None:
        tests.append(("sphere-box", d - radius, margin))
    if d - radius > margin:
        return None
    if d < MINVAL:
        gaps = [h[0] + c[0], h[0] - c[0], h[1] + c[1], h[1] - c[1], h[2] + c[2], h[2] - c[2]]
        k = int(np.argmin(gaps))  # (the first of the least)
        least = gaps[k]
        nl = np.zeros(3)
        nl[k // 2] = -1.0 if k % 2 else 1.0
        dist = -least - radius
        pl = c + nl * (radius - least) / 2
        if labels is not None:
            labels += ["sphere-box:inside", "sphere-box:face" + FACES[k]]
    else:
        nl = (cl - c) / d
        dist = d - radius
        pl = c + nl * (radius + dist / 2)
        if labels is not None:
            labels += ["sphere-box:outside", "sphere-box:clamped%d" % int((cl != c).sum())]  # 1 a face, 2 an edge, 3 a corner
    return dict(dist=dist, pos=bpos + bmat @ pl, normal=bmat @ nl)


def ray_box(o, d, half, labels=None):
    """(distance or None, candidates [(t, |cos|)]) of the ray o + t d (box frame, d unit) and the box's surface"""
    o, d, h = (np.asarray(x, dtype=np.float64) for x in (o, d, half))
    cands = []
    for a in range(3):
        if d[a] == 0:
            continue
        b, c = (a + 1) % 3, (a + 2) % 3
        for s in (-1.0, 1.0):
            t = (s * h[a] - o[a]) / d[a]
            p = o + t * d
            if t >= 0 and abs(p[b]) <= h[b] and abs(p[c]) <= h[c]:
                cands.append((t, abs(d[a])))
    cands.sort()
    if labels is not None:
        inside = bool((np.abs(o) < h).all())
        labels.append("ray-box:" + ("miss" if not cands else "inside" if inside else "outside"))
    return (cands[0][0] if cands else None), cands


def support(half, ld):
    """the box's support point along the local direction ld: a zero component takes the + side"""
    h, ld = np.asarray(half, dtype=np.float64), np.asarray(ld, dtype=np.float64)
    return np.where(ld >= 0, h, -h)


def lowest_point(half, bmat):
    """z of the box's lowest point relative to its centre, in the frame bmat maps into"""
    ld = -np.asarray(bmat, dtype=np.float64)[2]
    return -(np.abs(ld) @ np.asarray(half, dtype=np.float64))
