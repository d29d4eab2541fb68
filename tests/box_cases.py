"""The box scene, its MESH TWIN, the case table and its references (tests/test_box_cpu.py, tests/test_gpu_box.py).

TEST INFRASTRUCTURE.  The scene and the table are pure numpy.  scene_xml(variant, twin) is one MJCF text: a TILTED plane, a small flat height field 30 m away, a
static box W, and four free bodies in geom order P (box), S (sphere), Q (box of other proportions), X (a capsule; in the "mesh"
variant a small mesh hull).  A model may have 28 dofs, so the capsule and the hull take turns on the fourth body.  twin=True writes the
same scene with every box replaced by a mesh of its eight corners: the form the fp64 oracle can load.  Every body has an explicit
<inertial>, so that the mesh compiler's frame changes nothing in the dynamics, and every box three different half extents.

build_cases(info, variant): a case is a name, its kind, the two geoms under test, a full qpos rounded to fp32 and whether it is EXACT.
Exactly one pair is in range per case; the other bodies are parked along the plane's normal, 6 m apart.  Portal-search pairs are built on
a face of the first box: the second geom's deepest point (its support point along the face's inward normal) stands over the face's
interior at a chosen gap, which then is the true distance of the two geoms.

reference(hbmod, variant, directory) is what the device is held to: box_ref for the analytic kinds, the fp64 oracle on the mesh twin
(class Twin) for the portal-search kinds, each with its conditioning envelope (pair_cases.evaluations).
"""
import numpy as np

import box_ref
import pair_ref
from oracle_lib import Oracle, load_state, parse_hbm
from pair_cases import _f32, _q_z_to, _qaxis, _qmul, _qrand, evaluations, state_of

MARGIN = 0.01
HALF = {"W": (0.30, 0.20, 0.10), "P": (0.10, 0.06, 0.04), "Q": (0.05, 0.12, 0.08)}
SPHERE_R = 0.07
CAPSULE = (0.04, 0.15)
HULL = np.array([[0.06, 0.0, -0.03], [-0.05, 0.05, -0.03], [-0.04, -0.06, -0.02], [0.0, 0.01, 0.07], [0.03, 0.04, 0.04], [-0.02, -0.03, 0.05]])
BODIES = ("P", "S", "Q", "X")
FIELD_POS = np.array([30.0, 0.0, 0.0])
W_POS = np.array([-2.875, -0.25, 4.0])  # fp32 numbers (the device's pose of W is the oracle's exactly); 2.6 m above the plane, 4 m from the nearest parked body
VARIANTS = ("pgs", "mesh", "newton_cd6", "pgs_cd6", "xfirst", "xfirst_mesh")


def bodies_of(variant):
    """body (and geom) order: the sphere S between the boxes, so that sphere - box comes in both orders; the fourth body X (capsule or
    hull) behind the boxes or, in the xfirst variants, ahead of them - a capsule link ahead of a box foot, a hull ahead of a box"""
    return ("X", "P", "S", "Q") if variant.startswith("xfirst") else BODIES


def _box_geom(name, twin, extra=""):
    if twin:
        return '<geom name="%s" type="mesh" mesh="box%s"%s/>' % (name, name, extra)
    return '<geom name="%s" type="box" size="%g %g %g"%s/>' % ((name,) + HALF[name] + (extra,))


def scene_xml(variant, twin=False):
    """pgs: condim 3, PGS, X a capsule; mesh: the same with X a mesh hull; newton_cd6: condim 6, Newton, X a capsule; pgs_cd6: condim 6,
    PGS (the kPgsNefcMax-row family); xfirst, xfirst_mesh: pgs and mesh with the body X ahead of the boxes"""
    assert variant in VARIANTS, variant
    asset = '<hfield name="h" nrow="3" ncol="3" size="0.5 0.5 0.1 0.1" elevation="0 0 0 0 0 0 0 0 0"/>'
    if twin:
        asset += "".join('<mesh name="box%s" vertex="%s"/>' % (n, " ".join("%.17g" % v for v in box_ref.corners(HALF[n]).reshape(-1))) for n in ("W", "P", "Q"))
    if variant.endswith("mesh"):
        asset += '<mesh name="hull" vertex="%s"/>' % " ".join("%.17g" % v for v in HULL.reshape(-1))
        x = '<geom name="X" type="mesh" mesh="hull"/>'
    else:
        x = '<geom name="X" type="capsule" size="%g %g"/>' % CAPSULE
    opt = 'iterations="100" tolerance="1e-8" solver="Newton"' if variant == "newton_cd6" else 'iterations="50" tolerance="0" solver="PGS"'
    inertial = '<inertial pos="0 0 0" mass="%g" diaginertia="%g %g %g"/>'
    body = '<body name="%s" pos="0 0 %d"><freejoint/>' + inertial + "%s</body>"
    bodies = {"P": body % ("P", 7, 1.2, 0.004, 0.005, 0.006, _box_geom("P", twin)),
              "S": body % ("S", 13, 0.8, 0.002, 0.002, 0.002, '<geom name="S" type="sphere" size="%g"/>' % SPHERE_R),
              "Q": body % ("Q", 19, 1.5, 0.007, 0.004, 0.008, _box_geom("Q", twin)),
              "X": body % ("X", 25, 0.6, 0.003, 0.003, 0.001, x)}
    return ('<mujoco model="boxes"><compiler angle="degree"/><option timestep="0.002" %s/>'
            '<default><geom condim="%d" margin="%g" friction="0.8"/></default><asset>%s</asset><worldbody>'
            '<geom name="floor" type="plane" pos="0.1 -0.2 0.05" euler="10 20 0" size="0 0 1"/>'
            '<geom name="field" type="hfield" hfield="h" pos="%g %g %g"/>%s%s</worldbody></mujoco>'
            % (opt, 6 if variant.endswith("cd6") else 3, MARGIN, asset, FIELD_POS[0], FIELD_POS[1], FIELD_POS[2],
               _box_geom("W", twin, ' pos="%g %g %g"' % tuple(W_POS)), "".join(bodies[n] for n in bodies_of(variant))))


def _support_local(kind, ld):
    """support point of a geom of the scene in its own frame along ld"""
    if kind in HALF:
        return box_ref.support(HALF[kind], ld)
    if kind == "S":
        return SPHERE_R * ld
    if kind == "capsule":
        return CAPSULE[0] * ld + np.array([0, 0, CAPSULE[1] if ld[2] >= 0 else -CAPSULE[1]])
    return HULL[int(np.argmax(HULL @ ld))]  # (relative to the BODY: X's pose is the body's, whatever frame the mesh compiler gives the geom)


def build_cases(info, variant):
    bodies = bodies_of(variant)
    names = list(info["geom_name"])
    gid = {n: names.index(n) for n in ("floor", "field", "W") + bodies}
    body = {n: int(info["geom_bodyid"][gid[n]]) for n in bodies}
    qadr = {n: int(info["jnt_qposadr"][info["body_jntadr"][body[n]]]) for n in bodies}
    nq = 7 * len(bodies)
    p0 = info["geom_pos"][3 * gid["floor"]:3 * gid["floor"] + 3].copy()
    pm = pair_ref.quat2mat(info["geom_quat"][4 * gid["floor"]:4 * gid["floor"] + 4])
    e1, e2, nrm = pm[:, 0], pm[:, 1], pm[:, 2]
    rng = np.random.default_rng(20250611)
    qG = _qrand(rng)
    G = pair_ref.quat2mat(qG)
    centre = p0 + nrm * 1.5 + 0.45 * e1 - 0.35 * e2
    xkind = "hull" if variant.endswith("mesh") else "capsule"
    cases = []

    def add(name, kind, pair, poses, exact=False):
        q = np.zeros(nq)
        for k, n in enumerate(bodies):
            pos, quat = poses[n] if n in poses else (p0 + nrm * (7.0 + 6.0 * k) + 0.3 * k * e1, _qaxis([1, 2, 3], 0.4 + k))
            q[qadr[n]:qadr[n] + 3] = pos
            q[qadr[n] + 3:qadr[n] + 7] = np.asarray(quat) / np.linalg.norm(quat)
        cases.append(dict(name=name, kind=kind, pair=pair, geoms=tuple(gid[n] for n in pair), qpos=_f32(q), exact=exact))

    depths = (("penetrating", -0.008), ("in the margin", 0.5 * MARGIN), ("outside", 1.6 * MARGIN))
    # ------------------------------------------------------------------ plane - box: a face, an edge, a corner down (0.03 rad off: no two corners level)
    downs = {"face": [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)],
             "edge": [(1, 1, 0), (-1, 0, 1), (0, 1, -1), (1, 0, -1)], "corner": [(1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, 1)]}
    for b in ("P", "Q"):
        h = np.array(HALF[b])
        for what, dirs in downs.items():
            for k, s in enumerate(dirs):
                s = np.array(s, dtype=np.float64)
                dl = s if what == "face" else s * h  # the local direction that points down: the face's outward normal, or towards the edge / corner
                dl /= np.linalg.norm(dl)
                for tag, gap in depths if k < 2 else depths[:1]:
                    # carries dl onto -nrm, then 0.03 rad off it: no two corners level
                    qb = _qmul(_qaxis([1, 0.3, 0.2], 0.03), _qmul(_q_z_to(-nrm, spin=0.4 + k), _qconj(_q_z_to(dl))))
                    R = pair_ref.quat2mat(qb)
                    low = min((R @ c) @ nrm for c in box_ref.corners(h))
                    pos = p0 + (0.3 + 0.1 * k) * e1 - 0.2 * e2 + nrm * (gap - low)
                    add("plane-%s %s %d down, %s" % (b, what, k, tag), "plane-box", ("floor", b), {b: (pos, qb)})
    # ------------------------------------------------------------------ sphere - box: face / edge / corner region, inside, and the margin
    for b in ("P", "Q", "W"):
        h = np.array(HALF[b])
        qb = _qmul(qG, _qrand(rng)) if b != "W" else np.array([1.0, 0, 0, 0])
        pb = centre + 0.05 * rng.standard_normal(3) if b != "W" else W_POS
        R = pair_ref.quat2mat(qb)
        for region, sgn in (("face", (1, 0, 0)), ("face", (0, -1, 0)), ("edge", (0, 1, -1)), ("edge", (-1, 0, 1)), ("corner", (1, -1, 1)), ("corner", (-1, 1, -1))):
            sgn = np.array(sgn, dtype=np.float64)
            u = sgn + 0.15 * rng.standard_normal(3) * (sgn != 0)
            u /= np.linalg.norm(u)
            for tag, gap in depths if b != "W" else depths[:2]:
                foot = sgn * h + (sgn == 0) * h * rng.uniform(-0.6, 0.6, 3)
                c = foot + u * (SPHERE_R + gap)
                add("S-%s %s region %s, %s" % (b, region, sgn.astype(int).tolist(), tag), "sphere-box", ("S", b), {"S": (pb + R @ c, _qrand(rng)), **({b: (pb, qb)} if b != "W" else {})})
        for k in range(6):  # the centre inside, nearest to face k
            c = h * rng.uniform(-0.3, 0.3, 3)
            c[k // 2] = (1 if k % 2 else -1) * (h[k // 2] - 0.3 * h.min())
            add("S-%s centre inside, face %s" % (b, box_ref.FACES[k]), "sphere-box", ("S", b), {"S": (pb + R @ c, _qrand(rng)), **({b: (pb, qb)} if b != "W" else {})})
        pc = _f32(pb)  # exact: the same fp32 centre; -z and +z tie on the smallest half extent of P and W, -x and +x on Q's
        add("S-%s coincident centres" % b, "sphere-box", ("S", b), {"S": (pc, _qrand(rng)), **({b: (pc, qb)} if b != "W" else {})}, exact=True)
    # ------------------------------------------------------------------ the portal-search pairs, on a face of the first box
    def on_face(a, other, okind, face, gap, rot_other, lateral):
        """poses of box a (world pose pa, qa given by the caller) and `other`, whose support point along the face's inward normal stands
        `gap` off the face over its interior"""
        h = np.array(HALF[a])
        nl = np.zeros(3)
        nl[face // 2] = 1.0 if face % 2 else -1.0
        qa = np.array([1.0, 0, 0, 0]) if a == "W" else _qmul(qG, _qaxis([1, 2, 3], 0.3))
        pa = W_POS if a == "W" else centre
        Ra = pair_ref.quat2mat(qa)
        Ro = pair_ref.quat2mat(rot_other)
        sup = Ro @ _support_local(okind, Ro.T @ (Ra @ -nl))  # the other geom's deepest point towards the face, relative to its body
        foot = nl * h + lateral * h * (nl == 0)
        po = pa + Ra @ (foot + nl * gap) - sup
        poses = {other: (po, rot_other)}
        if a != "W":
            poses[a] = (pa, qa)
        return poses

    def hull_or_capsule_rot(k):
        return _qmul(qG, _qaxis([3, 1, 2], 0.5 + 0.9 * k))

    # (Q, P): the face owner is the HIGHER geom id - Q's face under P's corner; the others have it the lower
    pairs = [("W", "P", "P"), ("W", "Q", "Q"), ("P", "Q", "Q"), ("Q", "P", "P"), ("W", "X", xkind), ("P", "X", xkind), ("Q", "X", xkind)]
    for a, o, okind in pairs:
        kind = "box-box" if okind in HALF else ("box-mesh" if okind == "hull" else "capsule-box")
        for k, face in enumerate((5, 0, 3)):
            if (a, o) == ("P", "Q") and k == 2:
                continue
            for tag, gap in depths if k < 2 else depths[:1]:
                for cfg in (("corner", "edge") if k == 0 and (a, o) != ("Q", "P") else ("corner",)) if okind in HALF else ("generic",):
                    ro = hull_or_capsule_rot(k)
                    if cfg == "edge":  # an edge of the second box parallel to the face: turn it about the face normal's image only
                        ro = _qmul(np.array([1.0, 0, 0, 0]) if a == "W" else _qmul(qG, _qaxis([1, 2, 3], 0.3)), _qaxis([(face // 2 == 0) * 1.0, (face // 2 == 1) * 1.0, (face // 2 == 2) * 1.0], 0.6))
                        ro = _qmul(ro, _qaxis([(face // 2 != 0) * 1.0, 0.0, (face // 2 == 0) * 1.0], 0.7))
                    # the pair as build_pairs lists it: by geom type (capsule 3 < box 6 < mesh 7), two boxes by geom id
                    pair = (o, a) if kind == "capsule-box" else (a, o) if kind == "box-mesh" else tuple(sorted((a, o), key=lambda n: gid[n]))
                    add("%s-%s %s on face %s, %s" % (a, o, cfg, box_ref.FACES[face], tag), kind, pair, on_face(a, o, okind, face, gap, ro, np.array([0.3, -0.2, 0.25])))
    # axis-aligned EXACT cases: identity quaternions, dyadic offsets, a face of one box flat on a face of the other
    for k, (a, o) in enumerate((("W", "P"), ("W", "Q"), ("P", "Q"))):
        pa = W_POS if a == "W" else np.round(centre * 64) / 64
        ha, ho = np.array(HALF[a]), np.array(HALF[o])
        off = np.array([0.03125, -0.015625, ha[2] + ho[2] - 0.0078125])
        poses = {o: (pa + off, [1.0, 0, 0, 0])}
        if a != "W":
            poses[a] = (pa, [1.0, 0, 0, 0])
        add("%s-%s axis-aligned, face on face" % (a, o), "box-box", (a, o), poses, exact=True)
    # ------------------------------------------------------------------ height field - box: over the interior of a triangle of the flat field
    for b in ("P", "Q"):
        h = np.array(HALF[b])
        for k, what in enumerate(("corner", "edge", "face")):
            for tag, gap in depths:
                qb = _qrand(rng) if what == "corner" else (_qaxis([1, 0.1, 0.05], 0.8 + 0.05 * k) if what == "edge" else _qaxis([1, 0.4, 0.1], 0.02))
                low = box_ref.lowest_point(h, pair_ref.quat2mat(qb))  # (the field's frame is the world's)
                pos = FIELD_POS + np.array([0.13 + 0.05 * k, -0.21, gap - low])
                add("field-%s %s down, %s" % (b, what, tag), "hfield-box", ("field", b), {b: (pos, qb)})
    return cases


def _qconj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


# ---- the stairs model (tests/models/box_stairs.xml is stairs_xml() written out; tests/test_box_cpu.py holds the two together) ----
STEP_RISE, STEP_RUN, STEP_X0, NSTEPS = 0.1, 0.3, 0.45, 4
BRICK_HALF, BRICK_MASS = (0.12, 0.08, 0.04), 2.0


def stairs_xml(twin=False, solver="PGS", nsteps=NSTEPS):
    """A flight of four box steps (tops at 0.1 .. 0.4 m, 0.3 m deep, from x = 0.3 m) on a plane, a box-footed biped in front of it (free
    torso, hip and knee hinges held within a degree, box feet flat on the floor: 10 dofs) and a free brick lying face-down on the plane
    behind it (6 dofs).  twin: every box as the mesh of its eight corners.  nsteps: a longer flight (tools/gpu_box_bench.py)."""
    _STAIR_BOXES = dict([("step%d" % k, (0.5 * STEP_RUN, 0.6, 0.5 * STEP_RISE * (k + 1))) for k in range(nsteps)]
                        + [("torso", (0.08, 0.14, 0.12)), ("lfoot", (0.09, 0.045, 0.02)), ("rfoot", (0.09, 0.045, 0.02)), ("brick", BRICK_HALF)])

    def box(name, extra=""):
        if twin:
            return '<geom name="%s" type="mesh" mesh="m_%s"%s/>' % (name, name, extra)
        return '<geom name="%s" type="box" size="%g %g %g"%s/>' % ((name,) + _STAIR_BOXES[name] + (extra,))
    asset = "<asset>%s</asset>" % "".join('<mesh name="m_%s" vertex="%s"/>' % (n, " ".join("%.17g" % v for v in box_ref.corners(h).reshape(-1))) for n, h in _STAIR_BOXES.items()) if twin else ""
    steps = "".join(box("step%d" % k, ' pos="%g 0 %g"' % (STEP_X0 + STEP_RUN * k, 0.5 * STEP_RISE * (k + 1))) for k in range(nsteps))
    leg = ('<body name="%(s)sthigh" pos="0 %(y)g -0.12"><joint name="%(s)ship" type="hinge" axis="0 1 0" limited="true" range="-1 1"/>'
           '<inertial pos="0 0 -0.11" mass="1.2" diaginertia="0.006 0.006 0.001"/><geom name="%(s)sthigh" type="capsule" fromto="0 0 0 0 0 -0.22" size="0.035"/>'
           '<body name="%(s)sshin" pos="0 0 -0.22"><joint name="%(s)sknee" type="hinge" axis="0 1 0" limited="true" range="-1 1"/>'
           '<inertial pos="0 0 -0.12" mass="1.0" diaginertia="0.005 0.005 0.001"/><geom name="%(s)sshin" type="capsule" fromto="0 0 0 0 0 -0.2" size="0.03"/>%(foot)s</body></body>')
    legs = "".join(leg % dict(s=s, y=y, foot=box(s + "foot", ' pos="0.03 0 -0.24"')) for s, y in (("l", 0.09), ("r", -0.09)))
    motors = "".join('<motor name="m_%s" joint="%s" gear="20" ctrlrange="-1 1" ctrllimited="true"/>' % (j, j) for j in ("lhip", "lknee", "rhip", "rknee"))
    opt = 'iterations="100" tolerance="1e-8" solver="Newton"' if solver == "Newton" else 'iterations="50" tolerance="0" solver="PGS"'
    return ('<mujoco model="box_stairs"><compiler angle="degree"/><option timestep="0.002" %s/>'
            '<default><geom condim="3" friction="1" margin="0.002"/><joint damping="1" armature="0.01"/></default>%s<worldbody>'
            '<geom name="floor" type="plane" size="0 0 1"/>%s'
            '<body name="torso" pos="0 0 0.601"><freejoint name="root"/><inertial pos="0 0 0" mass="6" diaginertia="0.07 0.05 0.05"/>%s%s</body>'
            '<body name="brick" pos="-0.8 0.1 %g"><freejoint name="brick"/><inertial pos="0 0 0" mass="%g" diaginertia="0.006 0.012 0.014"/>%s</body>'
            '</worldbody><actuator>%s</actuator></mujoco>\n'
            % (opt, asset, steps, box("torso"), legs, BRICK_HALF[2] + 0.001, BRICK_MASS, box("brick"), motors))


# ---------------------------------------------------------------------------------------------------------------- the references
ANALYTIC = ("plane-box", "sphere-box")
ROWS_PER_CONTACT = {1: 1, 3: 4, 4: 6, 6: 10}
_cache = {}


def compiled(hbmod, variant, directory):
    """[model, .hbm path, parsed .hbm] of a scene variant, then the same three of its mesh twin"""
    out = []
    for twin in (False, True):
        m = hbmod.Model.from_xml_string(scene_xml(variant, twin))
        p = str(directory / ("boxes_%s%s.hbm" % (variant, "_twin" if twin else "")))
        m.save(p)
        out += [m, p, parse_hbm(p)]
    return out


def analytic(info, qpos, geoms, labels=None, tests=None):
    """box_ref on the pair under test of an analytic case, as Oracle.contacts() would list it"""
    gpos, gmat = pair_ref.geom_poses(info, qpos)
    g1, g2 = geoms
    size = info["geom_size"].reshape(-1, 3)
    margin = max(info["geom_margin"][g1], info["geom_margin"][g2])
    dim = int(max(info["geom_condim"][g1], info["geom_condim"][g2]))
    if info["geom_type"][g1] == box_ref.GEOM_PLANE:
        con = box_ref.plane_box(margin, gpos[g1], gmat[g1][:, 2], gpos[g2], gmat[g2], size[g2], labels, tests)
    else:
        c = box_ref.sphere_box(margin, gpos[g1], size[g1][0], gpos[g2], gmat[g2], size[g2], labels, tests)
        con = [c] if c else []
    return [dict(dist=c["dist"], pos=c["pos"], frame=c["normal"][None, :], dim=dim, geom1=int(g1), geom2=int(g2)) for c in con]


class Twin:
    """The fp64 oracle on a scene's mesh twin, spoken to in the BOX model's terms: states in the box model's qpos / qvel order, contacts
    with the box model's geom ids.  For most scenes the twin has the box model's bodies in the same order and nothing is permuted.  The
    xfirst_mesh scene (hull X ahead of the boxes) cannot use its own twin: the device collides (box, hull) - geom type order - and a twin
    made of meshes alone would collide (hull, box) - geom id order - and the portal search is not symmetric in its two objects (measured in
    the oracle: depth apart by up to 1e-2 on deep random overlaps).  Its twin is the "mesh" scene's, X behind the boxes, where the order
    is (box, hull) too; bodies and geoms are matched by name."""

    def __init__(self, info, tpath):
        self.o = Oracle(tpath)
        ti = self.o.info
        self.nv, self.nu = self.o.nv, self.o.nu
        self.geom = {g: list(info["geom_name"]).index(n) for g, n in enumerate(ti["geom_name"])}  # twin geom id -> box model's
        self.qmap, self.vmap = np.zeros(self.o.nq, dtype=int), np.zeros(self.o.nv, dtype=int)     # twin index -> box model's index
        for b, name in enumerate(ti["body_name"]):
            if b == 0:
                continue
            bb = list(info["body_name"]).index(name)
            jt, jb = ti["body_jntadr"][b], info["body_jntadr"][bb]
            self.qmap[ti["jnt_qposadr"][jt]:ti["jnt_qposadr"][jt] + 7] = np.arange(7) + info["jnt_qposadr"][jb]
            self.vmap[ti["jnt_dofadr"][jt]:ti["jnt_dofadr"][jt] + 6] = np.arange(6) + info["jnt_dofadr"][jb]
        self.same_order = bool((self.qmap == np.arange(self.o.nq)).all())

    def load(self, qpos):
        load_state(self.o, state_of(self.o, np.asarray(qpos)[self.qmap]), np.zeros(self.o.nu))

    def forward(self):
        self.o.forward()

    def step(self):
        self.o.step()

    @property
    def ncon(self):
        return self.o.ncon

    @property
    def nefc(self):
        return self.o.nefc

    def contacts(self):
        out = self.o.contacts()
        for c in out:
            c["geom1"], c["geom2"] = self.geom[c["geom1"]], self.geom[c["geom2"]]
        return out

    def _back(self, x, m):
        out = np.zeros(len(x))
        out[m] = x
        return out

    @property
    def qpos(self):
        return self._back(self.o.qpos, self.qmap)

    @property
    def qvel(self):
        return self._back(self.o.qvel, self.vmap)


def _evaluate(ref, case, qpos):
    if case["kind"] in ANALYTIC:
        con = analytic(ref["info"], qpos, case["geoms"])
        return dict(qpos=qpos, ncon=len(con), nefc=len(con) * ROWS_PER_CONTACT[con[0]["dim"]] if con else 0, con=con)
    o = ref["oracle"]
    o.load(qpos)
    o.forward()
    return dict(qpos=qpos, ncon=o.ncon, nefc=o.nefc, con=o.contacts())


def reference(hbmod, variant, directory):
    """dict(model, info, twin_info, oracle (on the twin), cases, evals, ill): evals[i] lists case i's reference evaluations, the unperturbed
    one first (an exact case has no other) - box_ref for the analytic kinds, the oracle on the mesh twin for the portal-search kinds"""
    if variant in _cache:
        return _cache[variant]
    m, p, info, _, tp, tinfo = compiled(hbmod, variant, directory)
    if variant == "xfirst_mesh":  # (class Twin: the twin with X behind the boxes)
        _, _, _, _, tp, tinfo = compiled(hbmod, "mesh", directory)
    ref = dict(model=m, path=p, info=info, twin_info=tinfo, oracle=Twin(info, tp), cases=build_cases(info, variant))
    evals, ill = evaluations(ref["cases"], lambda c, qpos: _evaluate(ref, c, qpos))
    ref.update(evals=evals, ill=ill)
    _cache[variant] = ref
    return ref


def twin_agreement(ref):
    """{case index: same order} of the plane - box cases whose box_ref contacts equal the oracle's plane - hull contacts on the twin to 1e-9
    as SETS; same order: also in the same order (the hull lists its support vertex first, then that vertex's neighbours; the box its
    corners in corner order - the PGS solver cut at 50 sweeps is sensitive to the order, DESIGN.md 2, the Newton solver is not)"""
    o = ref["oracle"]
    out = {}
    for i, c in enumerate(ref["cases"]):
        if c["kind"] != "plane-box":
            continue
        o.load(c["qpos"])
        o.forward()
        mine, theirs = ref["evals"][i][0]["con"], o.contacts()
        if len(mine) != len(theirs) or any((t["geom1"], t["geom2"]) != c["geoms"] for t in theirs):
            continue
        left = list(range(len(theirs)))
        order = []
        for a in mine:
            k = next((k for k in left if abs(a["dist"] - theirs[k]["dist"]) <= 1e-9 and np.abs(a["pos"] - theirs[k]["pos"]).max() <= 1e-9
                      and np.abs(a["frame"][0] - theirs[k]["frame"][0]).max() <= 1e-9), None)
            if k is None:
                break
            left.remove(k)
            order.append(k)
        else:
            out[i] = order == sorted(order)
    return out
