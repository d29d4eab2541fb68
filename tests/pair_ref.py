"""A labelled fp64 restatement, in numpy, of the primitive colliders of oracle/mjstep_oracle.c (plane_sphere, sphere_sphere,
capsule_capsule and the dispatch of collision() over plane / sphere / capsule pairs).

TEST INFRASTRUCTURE.  Every collider also returns the BRANCH LABELS it took (general or parallel, which clamp, which of the
parallel branch's four candidates h0..h3 became contacts, the fallback normal) and every activation test it made (cdist against
margin + radii), so that tests/test_pair_cases_cpu.py can prove that the case table of tests/pair_cases.py covers the branches and
keeps clear of the activation boundaries.  The reference the device is held to remains the oracle; this module is held to it.
"""
import numpy as np

MINVAL = 1e-15
GEOM_PLANE, GEOM_HFIELD, GEOM_SPHERE, GEOM_CAPSULE = 0, 1, 2, 3
JNT_FREE = 0


def quat2mat(q):
    q00, q11, q22, q33 = q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3]
    q01, q02, q03, q12, q13, q23 = q[0] * q[1], q[0] * q[2], q[0] * q[3], q[1] * q[2], q[1] * q[3], q[2] * q[3]
    return np.array([[q00 + q11 - q22 - q33, 2 * (q12 - q03), 2 * (q13 + q02)],
                     [2 * (q12 + q03), q00 - q11 + q22 - q33, 2 * (q23 - q01)],
                     [2 * (q13 - q02), 2 * (q23 + q01), q00 - q11 - q22 + q33]])


def mulquat(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def geom_poses(info, qpos):
    """world position and orientation matrix of every geom: bodies are the world or free bodies (the pair scene has no others)"""
    nbody = len(info["body_jntnum"])
    xpos, xquat = np.zeros((nbody, 3)), np.zeros((nbody, 4))
    xquat[0, 0] = 1.0
    for b in range(1, nbody):
        j = info["body_jntadr"][b]
        assert info["body_jntnum"][b] == 1 and info["jnt_type"][j] == JNT_FREE
        qa = info["jnt_qposadr"][j]
        q = np.array(qpos[qa + 3:qa + 7], dtype=np.float64)
        n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
        xpos[b], xquat[b] = qpos[qa:qa + 3], (q / n if n >= MINVAL else [1, 0, 0, 0])
    gpos, gmat = [], []
    for g in range(len(info["geom_type"])):
        b = info["geom_bodyid"][g]
        gpos.append(xpos[b] + quat2mat(xquat[b]) @ info["geom_pos"][3 * g:3 * g + 3])
        gmat.append(quat2mat(mulquat(xquat[b], info["geom_quat"][4 * g:4 * g + 4])))
    return gpos, gmat


def plane_sphere(tests, margin, ppos, normal, spos, radius):
    cdist = dot3(spos - ppos, normal)
    tests.append(("plane", cdist, margin + radius))
    if cdist > margin + radius:
        return None
    dist = cdist - radius
    return dict(dist=dist, pos=spos + normal * (-dist / 2 - radius), normal=normal.copy())


def sphere_sphere(tests, labels, margin, p1, r1, p2, r2):
    dif = p2 - p1
    cdist = np.sqrt(dot3(dif, dif))
    tests.append(("sphere", cdist, margin + r1 + r2))
    if cdist > margin + r1 + r2:
        return None
    dist = cdist - r1 - r2
    if cdist < MINVAL:
        n = np.array([1.0, 0.0, 0.0])
        labels.append("normal:fallback")
    else:
        n = dif / cdist
        labels.append("normal:dif")
    return dict(dist=dist, pos=p1 + n * (r1 + dist / 2), normal=n)


def clip(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def capsule_capsule(tests, labels, margin, pos1, axis1, r1, len1, pos2, axis2, r2, len2):
    dif = pos1 - pos2
    ma, mb, mc = dot3(axis1, axis1), -dot3(axis1, axis2), dot3(axis2, axis2)
    u, v = -dot3(axis1, dif), dot3(axis2, dif)
    det = ma * mc - mb * mb
    if abs(det) >= MINVAL:
        labels.append("cc:general")
        x1, x2 = (mc * u - mb * v) / det, (ma * v - mb * u) / det
        c1 = c2 = "none"
        if x1 > len1:
            x1, x2, c1 = len1, (v - mb * len1) / mc, "x1>len1"
        elif x1 < -len1:
            x1, x2, c1 = -len1, (v + mb * len1) / mc, "x1<-len1"
        if x2 > len2:
            x2, x1, c2 = len2, clip((u - mb * len2) / ma, -len1, len1), "x2>len2"
        elif x2 < -len2:
            x2, x1, c2 = -len2, clip((u + mb * len2) / ma, -len1, len1), "x2<-len2"
        labels.append("clamp1:" + c1)
        labels.append("clamp2:" + c2)
        if c1 != "none" and c2 != "none":
            labels.append("clamp:double")
        c = sphere_sphere(tests, labels, margin, pos1 + axis1 * x1, r1, pos2 + axis2 * x2, r2)
        return [c] if c else []
    labels.append("cc:parallel")
    out = []

    def cand(name, v1, v2):
        c = sphere_sphere(tests, labels, margin, v1, r1, v2, r2)
        if c:
            out.append(c)
            labels.append("hit:" + name)
    cand("h0", pos1 + axis1 * len1, pos2 + axis2 * clip((v - mb * len1) / mc, -len2, len2))
    cand("h1", pos1 - axis1 * len1, pos2 + axis2 * clip((v + mb * len1) / mc, -len2, len2))
    if len(out) < 2:
        cand("h2", pos1 + axis1 * clip((u - mb * len2) / ma, -len1, len1), pos2 + axis2 * len2)
    if len(out) < 2:
        cand("h3", pos1 + axis1 * clip((u + mb * len2) / ma, -len1, len1), pos2 - axis2 * len2)
    labels.append("parallel:%d" % len(out))
    return out


def collide(info, qpos):
    """oracle collision() over the model's pair list from the state qpos (fp64): (contacts, labels, tests).  A contact is a dict
    of dist, pos, normal, geom1, geom2; labels are the branch labels in the order taken; tests are the activation tests made, as
    (kind, cdist, threshold, geom1, geom2) - the bounding test that stands in for the broadphase is "bound"."""
    gpos, gmat = geom_poses(info, qpos)
    gt, size, rb = info["geom_type"], info["geom_size"].reshape(-1, 3), info["geom_rbound"]
    contacts, labels, tests = [], [], []
    for g1, g2 in zip(info["pair_geom1"], info["pair_geom2"]):
        t1, t2 = gt[g1], gt[g2]
        margin = max(info["geom_margin"][g1], info["geom_margin"][g2])
        pos1, pos2, s1, s2 = gpos[g1], gpos[g2], size[g1], size[g2]
        tt, ll, con = [], [], []
        if t1 == GEOM_HFIELD:  # (the scene's height field is parked 50 m away: never a contact, tests/test_pair_cases_cpu.py holds the counts)
            continue
        if t1 == GEOM_PLANE:
            normal = gmat[g1][:, 2].copy()
            d = dot3(pos2 - pos1, normal)
            tt.append(("bound", d, margin + rb[g2]))
            if d <= margin + rb[g2]:
                if t2 == GEOM_SPHERE:
                    ll.append("plane-sphere")
                    con = [plane_sphere(tt, margin, pos1, normal, pos2, s2[0])]
                else:
                    assert t2 == GEOM_CAPSULE
                    axis = gmat[g2][:, 2]
                    con = [plane_sphere(tt, margin, pos1, normal, pos2 + axis * s2[1], s2[0]), plane_sphere(tt, margin, pos1, normal, pos2 - axis * s2[1], s2[0])]
                    ll.append("plane-capsule:%d%d" % (con[0] is not None, con[1] is not None))
        else:
            dp = pos2 - pos1
            bound = rb[g1] + rb[g2] + margin
            tt.append(("bound", np.sqrt(dot3(dp, dp)), bound))
            if dot3(dp, dp) <= bound * bound:
                if t1 == GEOM_SPHERE and t2 == GEOM_SPHERE:
                    ll.append("sphere-sphere")
                    con = [sphere_sphere(tt, ll, margin, pos1, s1[0], pos2, s2[0])]
                elif t1 == GEOM_SPHERE and t2 == GEOM_CAPSULE:
                    axis = gmat[g2][:, 2]
                    x = dot3(axis, pos1 - pos2)
                    ll.append("sphere-capsule:" + ("x<-len" if x < -s2[1] else "x>len" if x > s2[1] else "interior"))
                    ll.append("sphere-capsule:g1%sg2" % ("<" if g1 < g2 else ">"))
                    con = [sphere_sphere(tt, ll, margin, pos1, s1[0], pos2 + axis * clip(x, -s2[1], s2[1]), s2[0])]
                else:
                    assert t1 == GEOM_CAPSULE and t2 == GEOM_CAPSULE
                    con = capsule_capsule(tt, ll, margin, pos1, gmat[g1][:, 2], s1[0], s1[1], pos2, gmat[g2][:, 2], s2[0], s2[1])
        labels += ll
        tests += [t + (g1, g2) for t in tt]
        for c in con:
            if c is not None:
                c["geom1"], c["geom2"] = int(g1), int(g2)
                contacts.append(c)
    return contacts, labels, tests
