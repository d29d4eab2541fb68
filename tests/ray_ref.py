"""fp64 reference of the ray read-out (include/hb.h: hb_ray_configure, hb_rays): mj_rayGeom's surfaces over the oracle's geom_xpos /
geom_xmat (as kin_ref.py reads them) and the .hbm records, and for every ray what makes its result FRAGILE.

TEST INFRASTRUCTURE: the product package never imports this module.

    plane        z = 0 of the geom frame, either side, inside size[0..1] where those are > 0
    sphere       the smallest non-negative root
    capsule      the cylinder wall between the caps and the outer halves of the end spheres, smallest non-negative root
    height field the elevation surface by BRUTE FORCE over every triangle (Moeller-Trumbore, both faces) - no grid walk, so nothing is
                 shared with the device's DDA (a ray through an edge, within 1e-12 of the triangle's size, hits both neighbours); cell
                 (r, c) is cut along (r, c) - (r + 1, c + 1), the strip order of convex_hfield in oracle/mjstep_oracle.c (dr = {1, 0}: triangles (r+1,c) (r,c) (r+1,c+1) and (r,c) (r+1,c+1) (r,c+1)); no walls, no base
    mesh, cylinder, box, ellipsoid: no surface; cast() raises when one is eligible, unless it collides with nothing (a visual marker)

Per ray, beside dist / geomid (-1 / -1 for a miss):
    second, second_geom   the second-nearest candidate (a candidate: every valid root of every eligible geom, every triangle hit), inf / -1
    cosine                |cos| of the angle between the ray and the surface normal at the hit (nan for a miss)
    clearance             for a miss: the smallest distance between the ray (cut at the cutoff) and any eligible surface - for a height
                          field, any triangle, which for a miss is the distance to its edges or from the ray's ends to its face (inf
                          when nothing is eligible; nan for a hit)
A hit within FRAGILE_DIST of the cutoff has the cutoff as a candidate (second) or, beyond it, as its clearance.
"""
import numpy as np

PLANE, HFIELD, SPHERE, CAPSULE = 0, 1, 2, 3
STATIC, MOVING = 1, 2
FRAME_WORLD, FRAME_BODY, FRAME_YAW = 0, 1, 2
FRAGILE_DIST, FRAGILE_COS = 1e-4, 0.05
FAR = 1e3  # length a ray without cutoff is given for the clearances (metres)


def eligible_geoms(info, flags=STATIC | MOVING, bodyexclude=-1):
    """the geoms a spec sees, ascending; raises ValueError naming the first eligible geom without a surface"""
    out = []
    for g in range(int(info["ngeom"])):
        body, t = int(info["geom_bodyid"][g]), int(info["geom_type"][g])
        if body == bodyexclude or not (flags & (STATIC if body == 0 else MOVING)):
            continue
        if t not in (PLANE, HFIELD, SPHERE, CAPSULE):
            if info["geom_contype"][g] == 0 and info["geom_conaffinity"][g] == 0:
                continue
            raise ValueError("geom %d has no ray surface (type %d)" % (g, t))
        out.append(g)
    return out


def quat_to_mat(q):
    q = np.asarray(q, dtype=np.float64)
    q = q / np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def world_rays(frame, xpos, xquat, pnt, vec):
    """(pnt, unit vec) in world coordinates of rays given in `frame` of a body at xpos / xquat (include/hb.h: HB_RAY_FRAME_*)"""
    pnt, vec = np.asarray(pnt, dtype=np.float64).reshape(-1, 3), np.asarray(vec, dtype=np.float64).reshape(-1, 3)
    vec = vec / np.linalg.norm(vec, axis=1, keepdims=True)
    if frame == FRAME_WORLD:
        return pnt.copy(), vec
    R = quat_to_mat(xquat)
    if frame == FRAME_YAW:
        hx = R[:2, 0]
        n = np.linalg.norm(hx)
        x = np.array([hx[0] / n, hx[1] / n, 0.0]) if n >= 1e-6 else np.array([1.0, 0.0, 0.0])
        z = np.array([0.0, 0.0, 1.0])
        R = np.stack([x, np.cross(z, x), z], axis=1)
    return np.asarray(xpos, dtype=np.float64) + pnt @ R.T, vec @ R.T


def hfield_triangles(info, hid, data=None):
    """[ntri, 3, 3] vertices of the field's surface triangles in its own frame, cell (r, c) first its (r+1,c) (r,c) (r+1,c+1) half, then
    (r,c) (r+1,c+1) (r,c+1).  data: the elevations (the whole hfield_data block; default the model's)"""
    nrow, ncol, adr = int(info["hfield_nrow"][hid]), int(info["hfield_ncol"][hid]), int(info["hfield_adr"][hid])
    sx, sy, sz = (float(v) for v in info["hfield_size"][4 * hid:4 * hid + 3])
    e = np.asarray(info["hfield_data"] if data is None else data, dtype=np.float64)[adr:adr + nrow * ncol].reshape(nrow, ncol)

    def vert(r, c):
        return [2 * sx * c / (ncol - 1) - sx, 2 * sy * r / (nrow - 1) - sy, e[r, c] * sz]
    tris = []
    for r in range(nrow - 1):
        for c in range(ncol - 1):
            tris.append([vert(r + 1, c), vert(r, c), vert(r + 1, c + 1)])
            tris.append([vert(r, c), vert(r + 1, c + 1), vert(r, c + 1)])
    return np.array(tris)


def _roots(o, d, r):
    """real roots t of |o + t d|^2 = r^2 (d need not be unit; none when d is zero or the line misses)"""
    a, b, c = d @ d, o @ d, o @ o - r * r
    if a < 1e-300 or b * b - a * c < 0:
        return []
    s = np.sqrt(b * b - a * c)
    return [(-b - s) / a, (-b + s) / a]


def _seg_seg(p, q, a, b):
    """smallest distance between the segments p-q and a-b"""
    u, v, w = q - p, b - a, p - a
    A, B, C, D, E = u @ u, u @ v, v @ v, u @ w, v @ w
    den = A * C - B * B
    best = np.inf
    cand = [0.0, 1.0]
    if den > 1e-300:
        cand.append(min(1.0, max(0.0, (B * E - C * D) / den)))
    for s in cand:  # the closest point of a-b to the point at s, and back
        t = min(1.0, max(0.0, ((p + s * u - a) @ v) / C)) if C > 1e-300 else 0.0
        s2 = min(1.0, max(0.0, ((a + t * v - p) @ u) / A)) if A > 1e-300 else 0.0
        t2 = min(1.0, max(0.0, ((p + s2 * u - a) @ v) / C)) if C > 1e-300 else 0.0
        best = min(best, np.linalg.norm(p + s * u - a - t * v), np.linalg.norm(p + s2 * u - a - t2 * v))
    return best


def _point_tri(p, tri):
    """distance from p to the triangle's face where p projects into it, else inf (its edges are measured as segments)"""
    e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
    n = np.cross(e1, e2)
    w = p - tri[0]
    M = np.array([[e1 @ e1, e1 @ e2], [e1 @ e2, e2 @ e2]])
    uv = np.linalg.solve(M, np.array([w @ e1, w @ e2]))
    if uv[0] >= 0 and uv[1] >= 0 and uv[0] + uv[1] <= 1:
        return abs(w @ n) / np.linalg.norm(n)
    return np.inf


def _geom_candidates(t, size, o, d, tris):
    """[(distance, |cos| of the incidence angle)] of every valid hit of the ray (geom frame) with one geom"""
    out = []
    if t == PLANE:
        if d[2] != 0:
            x = -o[2] / d[2]
            h = o + x * d
            if x >= 0 and (size[0] <= 0 or abs(h[0]) <= size[0]) and (size[1] <= 0 or abs(h[1]) <= size[1]):
                out.append((x, abs(d[2])))
    elif t == SPHERE:
        for x in _roots(o, d, size[0]):
            if x >= 0:
                out.append((x, abs((o + x * d) @ d) / size[0]))
    elif t == CAPSULE:
        r, half = size[0], size[1]
        for x in _roots(o * [1, 1, 0], d * [1, 1, 0], r):
            h = o + x * d
            if x >= 0 and abs(h[2]) <= half:
                out.append((x, abs(h[:2] @ d[:2]) / r))
        for sgn in (1.0, -1.0):
            c = np.array([0, 0, sgn * half])
            for x in _roots(o - c, d, r):
                h = o + x * d
                if x >= 0 and sgn * h[2] >= half:
                    out.append((x, abs((h - c) @ d) / r))
    elif t == HFIELD:
        e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
        pv = np.cross(d, e2)
        det = (e1 * pv).sum(1)
        ok = np.abs(det) > 1e-300
        inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
        tv = o - tris[:, 0]
        u = (tv * pv).sum(1) * inv
        qv = np.cross(tv, e1)
        v = (qv @ d) * inv
        x = (e2 * qv).sum(1) * inv
        n = np.cross(e1, e2)
        cosn = np.abs(n @ d) / np.linalg.norm(n, axis=1)
        for k in np.nonzero(ok & (u >= -1e-12) & (v >= -1e-12) & (u + v <= 1 + 1e-12) & (x >= 0))[0]:
            out.append((float(x[k]), float(cosn[k])))
    return out


def _geom_clearance(t, size, o, d, length, tris):
    """smallest distance between the segment o .. o + length d (geom frame) and the geom's surface, for a ray that does not hit it"""
    e = o + length * d
    if t == PLANE:
        if size[0] > 0 and size[1] > 0:  # a rectangle: its edges, and its face under the segment's ends
            c = [np.array([sx * size[0], sy * size[1], 0.0]) for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
            best = min(_seg_seg(o, e, c[k], c[(k + 1) % 4]) for k in range(4))
            for p in (o, e):
                if abs(p[0]) <= size[0] and abs(p[1]) <= size[1]:
                    best = min(best, abs(p[2]))
            return best
        if size[0] > 0 or size[1] > 0:  # a strip: bounded along one axis only
            k = 0 if size[0] > 0 else 1
            far = np.zeros(3); far[1 - k] = FAR * 10
            best = np.inf
            for s in (-1, 1):
                a = np.zeros(3); a[k] = s * size[k]
                best = min(best, _seg_seg(o, e, a - far, a + far))
            for p in (o, e):
                if abs(p[k]) <= size[k]:
                    best = min(best, abs(p[2]))
            return best
        return min(abs(o[2]), abs(e[2]))
    if t == SPHERE:
        return abs(_seg_seg(o, e, np.zeros(3), np.zeros(3)) - size[0])
    if t == CAPSULE:
        return abs(_seg_seg(o, e, np.array([0, 0, -size[1]]), np.array([0, 0, size[1]])) - size[0])
    best = np.inf
    for tri in tris:
        lo, hi = tri.min(0) - 1e-9, tri.max(0) + 1e-9
        # (skip triangles whose box the segment's box is farther from than the best so far)
        gap = np.maximum(0, np.maximum(lo - np.maximum(o, e), np.minimum(o, e) - hi))
        if np.linalg.norm(gap) >= best:
            continue
        for k in range(3):
            best = min(best, _seg_seg(o, e, tri[k], tri[(k + 1) % 3]))
        best = min(best, _point_tri(o, tri), _point_tri(e, tri))
    return best


def cast(info, geom_xpos, geom_xmat, pnt, vec, flags=STATIC | MOVING, bodyexclude=-1, cutoff=0.0, hfield_data=None):
    """World-frame rays (pnt [n, 3], vec [n, 3]) against the eligible geoms at the given world poses (geom_xpos [ngeom, 3], geom_xmat
    [ngeom, 3, 3]).  hfield_data: the env's own elevations (hb_env_get_domain_params' hfield_data block), default the model's.
    Returns a dict of arrays [n]: dist, geomid, second, second_geom, cosine, clearance (module docstring)."""
    pnt, vec = np.asarray(pnt, dtype=np.float64).reshape(-1, 3), np.asarray(vec, dtype=np.float64).reshape(-1, 3)
    vec = vec / np.linalg.norm(vec, axis=1, keepdims=True)
    geoms = eligible_geoms(info, flags, bodyexclude)
    gx, gm = np.asarray(geom_xpos, dtype=np.float64).reshape(-1, 3), np.asarray(geom_xmat, dtype=np.float64).reshape(-1, 3, 3)
    size = np.asarray(info["geom_size"], dtype=np.float64).reshape(-1, 3)
    tris = {g: hfield_triangles(info, int(info["geom_dataid"][g]), hfield_data) for g in geoms if int(info["geom_type"][g]) == HFIELD}
    n = len(pnt)
    out = dict(dist=np.full(n, -1.0), geomid=np.full(n, -1, dtype=np.int64), second=np.full(n, np.inf), second_geom=np.full(n, -1, dtype=np.int64),
               cosine=np.full(n, np.nan), clearance=np.full(n, np.nan))
    limit = cutoff if cutoff > 0 else np.inf
    for i in range(n):
        cands = []
        local = {}
        for g in geoms:
            o, d = gm[g].T @ (pnt[i] - gx[g]), gm[g].T @ vec[i]
            local[g] = (o, d)
            cands += [(x, g, c) for x, c in _geom_candidates(int(info["geom_type"][g]), size[g], o, d, tris.get(g))]
        cands.sort(key=lambda h: (h[0], h[1]))
        if cands and cands[0][0] <= limit:
            out["dist"][i], out["geomid"][i], out["cosine"][i] = cands[0]
            if len(cands) > 1:
                out["second"][i], out["second_geom"][i] = cands[1][0], cands[1][1]
            if limit - cands[0][0] < out["second"][i] - cands[0][0]:
                out["second"][i], out["second_geom"][i] = limit, -1
        else:
            length = limit if cutoff > 0 else FAR
            clear = min([_geom_clearance(int(info["geom_type"][g]), size[g], local[g][0], local[g][1], length, tris.get(g)) for g in geoms] + [np.inf])
            if cands:  # (beyond the cutoff)
                clear = min(clear, cands[0][0] - limit)
            out["clearance"][i] = clear
    return out


def reference(o, pnt, vec, frame=FRAME_WORLD, frame_body=0, flags=STATIC | MOVING, bodyexclude=-1, cutoff=0.0, hfield_data=None):
    """cast() of rays given in `frame` of the oracle's current data (after forward())"""
    nb, ng = o.nbody, o.ngeom
    pw, vw = world_rays(frame, o.xpos.reshape(nb, 3)[frame_body], o.xquat.reshape(nb, 4)[frame_body], pnt, vec)
    return cast(o.info, o.geom_xpos.reshape(ng, 3), o.geom_xmat.reshape(ng, 3, 3), pw, vw, flags, bodyexclude, cutoff, hfield_data)


def fragile(res):
    """mask [n] of the rays whose result a rounding error may flip: the second candidate within FRAGILE_DIST of the first, a grazing hit
    (|cos| < FRAGILE_COS), or a miss that clears a surface by less than FRAGILE_DIST"""
    hit = res["geomid"] >= 0
    with np.errstate(invalid="ignore"):
        return np.where(hit, (res["second"] - res["dist"] < FRAGILE_DIST) | (res["cosine"] < FRAGILE_COS), res["clearance"] < FRAGILE_DIST)


def height_scan(res, cutoff):
    """what VecEnv.height_scan reports of a downward scan's result: the distance below the origin, cutoff where nothing is hit"""
    return np.where(res["geomid"] >= 0, res["dist"], cutoff)
