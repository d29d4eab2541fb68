"""fp64 reference, in numpy, of the clipped box - box manifold ("The box - box manifold"; hb_mpr.hpp: box_box), with the
BRANCH LABELS it took and its DECISION MARGINS, as tests/box_ref.py has them.

TEST INFRASTRUCTURE: the product package never imports this module.  The routine is this engine's own definition (not mjc_BoxBox):

    box_box(A, B, margin)   A geom 1, B geom 2, the normal from A to B; t = pB - pA
      1  fifteen axes: s(L) = |t.L| - sum |L.A_i| hA_i - sum |L.B_i| hB_i; faces A0 A1 A2 B0 B1 B2, edges A_i x B_j (i major, normalised,
         skipped where |A_i x B_j|^2 < 1e-10); any s > margin: no contact; s_face, s_edge the largest, the first of equals
      2  the edge case iff an edge axis exists and s_edge > s_face + 0.05 |s_face| + 1e-4 min(half extents): L towards B, the supporting
         edges by the box's support rule (a zero takes +), the closest points of the two lines each clamped to its edge; one contact,
         dist = s_edge, pos the midpoint, normal L
      3  the face case: n_r the face axis signed towards the other centre; the incident face the other box's largest |n_r.axis| (first
         kept); in the reference face's frame (origin the face centre, axes the box's other two in cyclic order, R = [-h1, h1] x [-h2, h2])
         with Q the incident face's corners projected along n_r, in the cyclic order (-,-), (+,-), (+,+), (-,+) over the incident box's
         other two axes in cyclic order:
           (a) the incident corners inside R (inclusive), ascending corner index of plane_box's numbering
           (b) the corners of R strictly inside Q, in the order (-,-), (+,-), (+,+), (-,+), lifted onto the incident plane along n_r
           (c) per edge of Q (cyclic) and edge of R (the order of (b)) their crossing, both parameters strictly in (0, 1), parallel pairs
               (|d_perp| < 1e-12) skipped, lifted likewise
         dist the height over the reference face along n_r; dist > margin dropped; the first eight; pos = point - n_r dist / 2; the normal
         n_r if the reference box is A, else -n_r

tests receives (what, value) pairs: `value` is the signed quantity a decision compares with zero.
"""
import numpy as np

EDGE_SKIP = 1e-10
PARALLEL = 1e-12
BIAS_REL, BIAS_ABS = 0.05, 1e-4
AXES = ("A0", "A1", "A2", "B0", "B1", "B2")


def _sep(L, t, A, hA, B, hB):
    return abs(t @ L) - np.abs(L @ A) @ hA - np.abs(L @ B) @ hB


def box_box(margin, pA, mA, hA, pB, mB, hB, labels=None, tests=None):
    """contacts (dicts of dist, pos, normal) of box A (centre pA, orientation mA [3, 3], half extents hA) and box B, 0 to 8, in order"""
    pA, mA, hA, pB, mB, hB = (np.asarray(x, dtype=np.float64) for x in (pA, mA, hA, pB, mB, hB))
    lab = labels.append if labels is not None else (lambda x: None)
    rec = (lambda what, v: tests.append((what, float(v)))) if tests is not None else (lambda what, v: None)
    t = pB - pA
    # ---- 1: the fifteen axes
    sf, kf = -np.inf, -1
    sface = []
    for k in range(6):
        L = mA[:, k] if k < 3 else mB[:, k - 3]
        s = _sep(L, t, mA, hA, mB, hB)
        sface.append(s)
        rec("axis " + AXES[k], s - margin)
        if s > sf:
            sf, kf = s, k
    se, ke, Le = -np.inf, None, None
    for i in range(3):
        for j in range(3):
            c = np.cross(mA[:, i], mB[:, j])
            l2 = c @ c
            if l2 < EDGE_SKIP:
                continue
            L = c / np.sqrt(l2)
            s = _sep(L, t, mA, hA, mB, hB)
            rec("axis A%dxB%d" % (i, j), s - margin)
            if s > se:
                se, ke, Le = s, (i, j), L
    if max(sf, se) > margin:
        lab("box-box:separated")
        return []
    # ---- 2: the edge case
    if ke is not None:
        bias = se - (sf + BIAS_REL * abs(sf) + BIAS_ABS * min(hA.min(), hB.min()))
        rec("edge over face", bias)
    if ke is not None and bias > 0:
        i, j = ke
        L = Le if t @ Le >= 0 else -Le
        cA, cB = pA.copy(), pB.copy()
        for a in range(3):
            if a != i:
                cA += (1.0 if L @ mA[:, a] >= 0 else -1.0) * hA[a] * mA[:, a]
            if a != j:
                cB += (1.0 if -(L @ mB[:, a]) >= 0 else -1.0) * hB[a] * mB[:, a]
        u, v, w = mA[:, i], mB[:, j], cA - cB
        b, d, e = u @ v, u @ w, v @ w
        den = 1.0 - b * b
        xa, xb = (b * e - d) / den, (e - b * d) / den
        rec("edge clamp A", hA[i] - abs(xa))
        rec("edge clamp B", hB[j] - abs(xb))
        xa, xb = np.clip(xa, -hA[i], hA[i]), np.clip(xb, -hB[j], hB[j])
        rec("dist", se - margin)
        lab("box-box:edge A%dxB%d" % (i, j))
        lab("box-box:1")
        return [dict(dist=se, pos=0.5 * ((cA + xa * u) + (cB + xb * v)), normal=L)]
    # ---- 3: the face case
    others = sorted(sface[:kf] + sface[kf + 1:])
    rec("face choice", sf - others[-1])
    ref_is_a = kf < 3
    a = kf % 3
    pr, mr, hr, pi, mi, hi = (pA, mA, hA, pB, mB, hB) if ref_is_a else (pB, mB, hB, pA, mA, hA)
    nr = mr[:, a] * (1.0 if (pi - pr) @ mr[:, a] >= 0 else -1.0)
    u1, u2, h1, h2 = mr[:, (a + 1) % 3], mr[:, (a + 2) % 3], hr[(a + 1) % 3], hr[(a + 2) % 3]
    cr = pr + nr * hr[a]
    dots = np.abs(nr @ mi)
    j = int(np.argmax(dots))  # (the first of the largest)
    rec("incident choice", dots[j] - np.sort(dots)[-2])
    sj = -1.0 if nr @ mi[:, j] >= 0 else 1.0
    ni = sj * mi[:, j]
    j1, j2 = (j + 1) % 3, (j + 2) % 3
    ci = pi + ni * hi[j]
    cyc = [(-1, -1), (1, -1), (1, 1), (-1, 1)]
    C = [ci + s1 * hi[j1] * mi[:, j1] + s2 * hi[j2] * mi[:, j2] for s1, s2 in cyc]
    Q = [np.array([(c - cr) @ u1, (c - cr) @ u2]) for c in C]
    lab("box-box:face %s%s" % (AXES[kf], "+" if nr @ mr[:, a] > 0 else "-"))
    lab("box-box:incident %d%s" % (j, "+" if sj > 0 else "-"))
    cand = []
    # (a) ascending corner index: bit j1 is below bit j2 unless j == 1 (axes 2, 0)
    for k in ((0, 1, 3, 2) if j != 1 else (0, 3, 1, 2)):
        rec("corner in R, x", h1 - abs(Q[k][0]))
        rec("corner in R, y", h2 - abs(Q[k][1]))
        if abs(Q[k][0]) <= h1 and abs(Q[k][1]) <= h2:
            cand.append(("a", C[k], (C[k] - cr) @ nr))
    nn = nr @ ni

    def lift(x, y):
        p0 = cr + x * u1 + y * u2
        lam = ((ci - p0) @ ni) / nn
        return p0 + lam * nr, lam

    Rc = [(-h1, -h2), (h1, -h2), (h1, h2), (-h1, h2)]
    e1, e2 = Q[1] - Q[0], Q[3] - Q[0]
    det = e1[0] * e2[1] - e1[1] * e2[0]
    for x, y in Rc:  # (b)
        dx, dy = x - Q[0][0], y - Q[0][1]
        al, be = (dx * e2[1] - dy * e2[0]) / det, (e1[0] * dy - e1[1] * dx) / det
        for v in (al, 1 - al, be, 1 - be):
            rec("R corner in Q", v)
        if 0 < al < 1 and 0 < be < 1:
            cand.append(("b",) + lift(x, y))
    for e in range(4):  # (c)
        q0, d = Q[e], Q[(e + 1) % 4] - Q[e]
        for f in range(4):
            horiz = f % 2 == 0  # R's edges 0 and 2 run along x (at y = -h2, +h2), 1 and 3 along y (at x = +h1, -h1)
            dp = d[1] if horiz else d[0]
            if abs(dp) < PARALLEL:
                continue
            line = (-h2, h1, h2, -h1)[f]
            tq = (line - (q0[1] if horiz else q0[0])) / dp
            along = (q0[0] + tq * d[0]) if horiz else (q0[1] + tq * d[1])
            # R's edge f runs from Rc[f] to Rc[f + 1]
            tr = ((along + h1) / (2 * h1), (along + h2) / (2 * h2), (h1 - along) / (2 * h1), (h2 - along) / (2 * h2))[f]
            for v in (tq, 1 - tq, tr, 1 - tr):
                rec("crossing", v)
            if 0 < tq < 1 and 0 < tr < 1:
                cand.append(("c",) + (lift(along, line) if horiz else lift(line, along)))
    out = []
    for what, p, dist in cand:
        rec("dist", dist - margin)
        if dist > margin:
            continue
        if len(out) == 8:
            lab("box-box:capped")
            break
        out.append(dict(dist=dist, pos=p - nr * (dist / 2), normal=nr if ref_is_a else -nr, src=what))
    lab("box-box:%d" % len(out))
    return out
