"""The pair scene and its case table: one plane, two capsules and two spheres on free bodies, every primitive pair placed in a
chosen configuration (tests/test_pair_cases_cpu.py, tests/test_gpu_narrow_pairs.py), and the oracle's side of it: reference().

TEST INFRASTRUCTURE.  The scene and the table are pure numpy.  scene_xml(variant) is one MJCF text with a TILTED plane, capsules A and B and spheres S and T
of different sizes and a positive geom margin, in four variants by text substitution (VARIANTS).  build_cases(info) returns the
table for a compiled variant (info: oracle_lib.parse_hbm of its .hbm): a case is a name, the two geoms under test, a full qpos
already rounded to fp32, the branch labels it is built to take (pair_ref's labels) and whether it is EXACT.  One env is one case.

Every case has exactly one pair in range; the two or three bodies not under test are parked along the plane's normal, 6 m apart
and at least 5 m from everything.  Pairs without the plane are built in a local frame and carried into the world by one fixed
random rotation and an offset of order 1 m, so that a capsule's world axis is a generic vector (its fp32 square norm is generally
not exactly 1).  EXACT cases are those whose decisive operands are bitwise identical on the device and in the oracle: capsules
that carry the same fp32 quaternion bit pattern (exactly parallel axes), coincident sphere centres, a sphere centre exactly on a
capsule's axis.  They get no conditioning envelope and no count allowance.

reference(hbmod, variant, directory) is what the device is held to: the oracle on every case, and - the CONDITIONING ENVELOPE - on NPERT
states whose qpos is perturbed by one fp32 rounding.  evaluations, envelope and state_of serve the box table (tests/box_cases.py) too.
"""
import numpy as np

import pair_ref
from oracle_lib import Oracle, load_state, parse_hbm

MARGIN = 0.01
SIZE = {"A": (0.05, 0.20), "B": (0.04, 0.15), "S": (0.07, 0.0), "T": (0.09, 0.0)}  # radius, half-length
BODIES = ("A", "S", "B", "T")  # body (and geom) order: the sphere S sits between the capsules, so that sphere - capsule pairs come in both geom orders
# "Along the normal" is 0.02 rad off it.  Exactly along it the reference's own contact frame is degenerate: the plane - capsule collider
# hands the capsule's axis to make_frame as the tangent hint, and a hint parallel to the normal leaves nothing but rounding residue to
# normalise (mju_makeFrame does the same).  0.02 rad keeps the fp32 residue, 6e-8 / 0.02, inside the 1e-5 the frames are held to.
ALONG = 0.02
SWEEP_ANGLES = (1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)

_SCENE = """<mujoco model="pairs">
  <compiler angle="degree"/>
  <option timestep="0.002" iterations="50" tolerance="0" solver="PGS"/>
  <default><geom condim="3" margin="%g" friction="0.8"/></default>
  <asset/>
  <worldbody>
    <geom name="floor" type="plane" pos="0.1 -0.2 0.05" euler="10 20 0" size="0 0 1"/>
    <body name="A" pos="0 0 7"><freejoint/><geom name="A" type="capsule" size="%g %g"/></body>
    <body name="S" pos="0 0 13"><freejoint/><geom name="S" type="sphere" size="%g"/></body>
    <body name="B" pos="0 0 19"><freejoint/><geom name="B" type="capsule" size="%g %g"/></body>
    <body name="T" pos="0 0 25"><freejoint/><geom name="T" type="sphere" size="%g"/></body>
  </worldbody>
</mujoco>
""" % ((MARGIN,) + SIZE["A"] + SIZE["S"][:1] + SIZE["B"] + SIZE["T"][:1])

_HFIELD_ASSET = '<asset><hfield name="h" nrow="3" ncol="3" size="0.5 0.5 0.1 0.1" elevation="0 0 0 0 0 0 0 0 0"/></asset>'
_HFIELD_GEOM = '<geom name="far" type="hfield" hfield="h" pos="50 0 0"/>'
VARIANTS = ("pgs", "newton", "hfield", "newton_cd6")


def scene_xml(variant):
    """pgs: condim 3, PGS (the classic PGS kernels); newton: condim 1, Newton (the classic Newton kernels); hfield: the pgs scene with
    a small flat height field parked 50 m away (every pair goes through the general collision path); newton_cd6: condim 6, Newton
    (the big-kernel family)"""
    x = _SCENE
    if variant in ("newton", "newton_cd6"):
        x = x.replace('iterations="50" tolerance="0" solver="PGS"', 'iterations="100" tolerance="1e-8" solver="Newton"')
        x = x.replace('condim="3"', 'condim="%d"' % (1 if variant == "newton" else 6))
    elif variant == "hfield":
        x = x.replace("<asset/>", _HFIELD_ASSET).replace('size="0 0 1"/>', 'size="0 0 1"/>\n    ' + _HFIELD_GEOM)
    else:
        assert variant == "pgs", variant
    return x


# ---- small quaternion kit (fp64)
def _qmul(a, b):
    return pair_ref.mulquat(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


def _qaxis(axis, ang):
    axis = np.asarray(axis, dtype=np.float64)
    return np.concatenate([[np.cos(0.5 * ang)], np.sin(0.5 * ang) * axis / np.linalg.norm(axis)])


def _qrand(rng):
    q = rng.standard_normal(4)
    return q / np.linalg.norm(q)


def _q_z_to(d, spin=0.0):
    """a quaternion that carries the z axis onto the unit vector d, after a spin about z"""
    d = np.asarray(d, dtype=np.float64) / np.linalg.norm(d)
    z = np.array([0.0, 0.0, 1.0])
    c = float(np.clip(d[2], -1, 1))
    if c > 1 - 1e-12:
        q = np.array([1.0, 0, 0, 0])
    elif c < -1 + 1e-12:
        q = np.array([0.0, 1, 0, 0])
    else:
        q = _qaxis(np.cross(z, d), np.arccos(c))
    return _qmul(q, _qaxis(z, spin))


_FLIP = np.array([0.0, 1.0, 0.0, 0.0])  # half a turn about the local x axis: reverses a capsule's axis


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _axis_of(q32):
    """the fp64 world z axis of a body whose qpos carries the (fp32-rounded) quaternion q32, as the oracle forms it"""
    q = np.asarray(q32, dtype=np.float64)
    return pair_ref.quat2mat(q / np.sqrt(q @ q))


def build_cases(info):
    names = list(info["geom_name"])
    gid = {n: names.index(n) for n in ("floor",) + BODIES}
    body = {n: int(info["geom_bodyid"][gid[n]]) for n in BODIES}
    qadr = {n: int(info["jnt_qposadr"][info["body_jntadr"][body[n]]]) for n in BODIES}
    nq = 7 * len(BODIES)
    p0 = info["geom_pos"][3 * gid["floor"]:3 * gid["floor"] + 3].copy()
    pm = pair_ref.quat2mat(info["geom_quat"][4 * gid["floor"]:4 * gid["floor"] + 4])
    e1, e2, nrm = pm[:, 0], pm[:, 1], pm[:, 2]
    rng = np.random.default_rng(20240229)
    qG = _qrand(rng)                     # the fixed global rotation ...
    G = pair_ref.quat2mat(qG)
    centre = p0 + nrm * 1.0 + 0.45 * e1 - 0.35 * e2  # ... and offset (order 1 m; 1 m above the plane: out of its range)
    cases = []

    def add(name, pair, poses, expect=(), exact=False):
        """poses: body -> (world position, world quaternion) of the bodies under test; the others are parked"""
        q = np.zeros(nq)
        for k, n in enumerate(BODIES):
            if n in poses:
                pos, quat = poses[n]
            else:
                pos, quat = p0 + nrm * (7.0 + 6.0 * k) + 0.3 * k * e1, _qaxis([1, 2, 3], 0.4 + k)
            q[qadr[n]:qadr[n] + 3] = pos
            q[qadr[n] + 3:qadr[n] + 7] = np.asarray(quat) / np.linalg.norm(quat)
        g = tuple(gid[n] for n in pair)
        cases.append(dict(name=name, pair=pair, geoms=g, qpos=_f32(q), expect=tuple(expect), exact=exact))

    def world(pl, ql):
        return centre + G @ np.asarray(pl, dtype=np.float64), _qmul(qG, ql)

    # ------------------------------------------------------------------ plane - sphere
    for s in ("S", "T"):
        r = SIZE[s][0]
        for tag, h in (("penetrating", r - 0.02), ("touching", r), ("shell", r + 0.5 * MARGIN), ("outside", r + 1.5 * MARGIN)):
            lat = 0.3 * e1 + (0.2 if s == "S" else -0.4) * e2
            add("plane-%s %s" % (s, tag), ("floor", s), {s: (p0 + lat + nrm * h, _qrand(rng))}, expect=() if tag == "outside" else ("plane-sphere",))
    # ------------------------------------------------------------------ plane - capsule: (tilt from the normal, centre height), both axis senses
    for c in ("A", "B"):
        r, L = SIZE[c]
        lim = MARGIN + r
        for tag, tilt, h, lab in (("both ends in", np.radians(80), lim - 0.04, "11"), ("one end in", np.radians(45), L * np.cos(np.radians(45)) + lim - 0.05, "01"),
                                  ("parallel to the plane", np.radians(90), lim - 0.02, "11"), ("along the normal", ALONG, L + lim - 0.03, "01"),
                                  ("both ends out", np.radians(45), L * np.cos(np.radians(45)) + lim + 0.01, "00")):
            d = np.cos(tilt) * nrm + np.sin(tilt) * (np.cos(0.7) * e1 + np.sin(0.7) * e2)
            for rev in (0, 1):
                q = _q_z_to(d, spin=0.3 + rev)
                if rev:
                    q = _qmul(q, _FLIP)
                label = "plane-capsule:" + (lab[::-1] if rev else lab)
                add("plane-%s %s%s" % (c, tag, ", axis reversed" if rev else ""), ("floor", c), {c: (p0 - 0.2 * e1 + 0.1 * e2 + nrm * h, q)}, expect=(label,))
    # ------------------------------------------------------------------ sphere - sphere
    rs = SIZE["S"][0] + SIZE["T"][0]
    for k, (tag, dd) in enumerate((("shell", rs + 0.5 * MARGIN), ("penetrating", rs - 0.01), ("deep", 0.03), ("outside", rs + 1.5 * MARGIN), ("1e-6 apart", 1e-6),
                                   ("shell 2", rs + 0.3 * MARGIN), ("deep 2", 0.005))):
        u = rng.standard_normal(3)
        u /= np.linalg.norm(u)
        pS, qS = world(-0.4 * dd * u, _qrand(rng))
        pT, qT = world(0.6 * dd * u, _qrand(rng))
        add("S-T %s" % tag, ("S", "T"), {"S": (pS, qS), "T": (pT, qT)}, expect=() if tag == "outside" else ("sphere-sphere", "normal:dif"))
    for k in range(2):
        p, _ = world(0.1 * rng.standard_normal(3), _qrand(rng))
        add("S-T coincident %d" % k, ("S", "T"), {"S": (p, _qrand(rng)), "T": (p, _qrand(rng))}, expect=("sphere-sphere", "normal:fallback"), exact=True)
    # ------------------------------------------------------------------ sphere - capsule (local frame: the capsule along z at the origin)
    for s in ("S", "T"):
        for c in ("A", "B"):
            (r1, _), (r2, L) = SIZE[s], SIZE[c]
            lim = MARGIN + r1 + r2
            for rev in (0, 1):
                ql = _qmul(_qrand(rng), _FLIP) if rev else _qrand(rng)
                ax = pair_ref.quat2mat(ql)
                for tag, x, lat, lab in (("interior", 0.35 * L, lim - 0.02, "interior"), ("interior, shell", -0.6 * L, lim - 0.3 * MARGIN, "interior"),
                                         ("beyond the + cap", L + 0.6 * lim, 0.5 * lim, "x>len"), ("beyond the - cap", -L - 0.5 * lim, 0.6 * lim, "x<-len"),
                                         ("at the + clamp boundary", L, lim - 0.03, None), ("at the - clamp boundary", -L, lim - 0.025, None),
                                         ("outside", 0.2 * L, lim + 0.5 * MARGIN, "interior"), ("on the axis beyond the + cap", L + 0.5 * lim, 0.0, "x>len")):
                    if rev and tag in ("interior, shell", "outside", "at the - clamp boundary"):
                        continue
                    pl = ax[:, 2] * x + ax[:, 0] * lat
                    pc, qc = world([0, 0, 0], ql)
                    ps, qs = world(pl, _qrand(rng))
                    add("%s-%s %s%s" % (s, c, tag, ", axis reversed" if rev else ""), (s, c), {s: (ps, qs), c: (pc, qc)},
                        expect=(("sphere-capsule:" + lab,) if lab else ()) + (("normal:dif",) if tag != "outside" else ()))
            # exact: the sphere's centre on the capsule's centre (any rotation), and on an axis that fp32 and fp64 form exactly
            pc, qc = world(0.1 * rng.standard_normal(3), _qrand(rng))
            add("%s-%s centre on the capsule's centre" % (s, c), (s, c), {s: (_f32(pc), _qrand(rng)), c: (_f32(pc), qc)}, expect=("sphere-capsule:interior", "normal:fallback"), exact=True)
            for qx, x in (([1.0, 0, 0, 0], 0.5 * L), ([0.0, 1, 0, 0], -0.25 * L)):  # world axis (0, 0, +-1) exactly
                pc = _f32(centre + 0.05 * rng.standard_normal(3))
                add("%s-%s centre on the axis, %+.3f" % (s, c, x), (s, c), {s: (pc + np.array([0, 0, _f32(x)]), _qrand(rng)), c: (pc, qx)},
                    expect=("sphere-capsule:interior", "normal:fallback"), exact=True)
    # ------------------------------------------------------------------ capsule - capsule, skew axes
    (r1, L1), (r2, L2) = SIZE["A"], SIZE["B"]
    lim = MARGIN + r1 + r2

    def skew(tag, x1, x2, sep, angle, expect):
        """axes `angle` apart whose lines come closest (distance sep) at abscissas x1 on A and x2 on B"""
        ql1 = _qrand(rng)
        m1 = pair_ref.quat2mat(ql1)
        ql2 = _qmul(ql1, _qaxis([1, 0, 0], angle))  # turned about A's local x: the common perpendicular
        m2 = pair_ref.quat2mat(ql2)
        pA, qA = world(-m1[:, 2] * x1, ql1)
        pB, qB = world(m1[:, 0] * sep - m2[:, 2] * x2, ql2)
        add("A-B " + tag, ("A", "B"), {"A": (pA, qA), "B": (pB, qB)}, expect=("cc:general",) + tuple(expect))

    for k, ang in enumerate((np.radians(60), np.radians(115))):
        cs = np.cos(ang)
        v = " (%d deg)" % round(np.degrees(ang))
        skew("skew, both interior" + v, 0.05, -0.04, lim - 0.02, ang, ("clamp1:none", "clamp2:none"))
        skew("skew, both interior, shell" + v, -0.1, 0.08, lim - 0.4 * MARGIN, ang, ("clamp1:none", "clamp2:none"))
        skew("skew, outside" + v, 0.02, 0.03, lim + MARGIN, ang, ("clamp1:none", "clamp2:none"))
        skew("axes pass within 2 mm" + v, 0.05, -0.04, 0.002, ang, ("clamp1:none", "clamp2:none"))
        skew("clamp x1 > len1" + v, L1 + 0.06, -0.02 * np.sign(cs), 0.03, ang, ("clamp1:x1>len1", "clamp2:none"))
        skew("clamp x1 < -len1" + v, -L1 - 0.06, 0.02 * np.sign(cs), 0.03, ang, ("clamp1:x1<-len1", "clamp2:none"))
        skew("clamp x2 > len2" + v, 0.03, L2 + 0.06, 0.03, ang, ("clamp1:none", "clamp2:x2>len2"))
        skew("clamp x2 < -len2" + v, -0.03, -L2 - 0.06, 0.03, ang, ("clamp1:none", "clamp2:x2<-len2"))
        # double clamps: after x1 is clamped the foot point on B, x2 + (+-L1 - x1) cos(angle), is still beyond B's end
        for s1 in (1, -1):
            for s2 in (1, -1):
                x1 = s1 * (L1 + 0.03)
                x2 = s2 * (L2 + 0.05) - (s1 * L1 - x1) * cs
                skew("double clamp x1 %s, x2 %s%s" % ("> len1" if s1 > 0 else "< -len1", "> len2" if s2 > 0 else "< -len2", v), x1, x2, 0.03, ang,
                     ("clamp1:" + ("x1>len1" if s1 > 0 else "x1<-len1"), "clamp2:" + ("x2>len2" if s2 > 0 else "x2<-len2"), "clamp:double"))
    # axes that intersect: under a generic rotation the distance between the lines is rounding noise of the positions (1e-8 m in fp32,
    # 1e-16 m in fp64) and so is the normal, in the oracle too.  Axis-aligned instead, with dyadic coordinates: A along z, B a quarter
    # turn away, the lines meeting in a point that every sum reaches exactly - the oracle's cdist is below its MINVAL and its normal the
    # fallback, whatever its compiler contracts.  (The device's fp32 residuals need not vanish: not an exact case.)
    h = np.sqrt(0.5)
    for k, (qB, off) in enumerate((([h, h, 0, 0], [0.0, 0.0625, 0.03125]), ([h, 0, h, 0], [-0.046875, 0.0, -0.0625]))):  # B along -y / along +x
        pA = np.round(centre * 1024) / 1024
        add("A-B axes intersect %d" % k, ("A", "B"), {"A": (pA, [1.0, 0, 0, 0]), "B": (pA + np.array(off), qB)}, expect=("cc:general", "clamp1:none", "clamp2:none", "normal:fallback"))
    # ------------------------------------------------------------------ capsule - capsule, exactly parallel: the same fp32 quaternion bits
    for k in range(2):
        q32 = _f32(_qmul(qG, _qrand(rng)))
        m = _axis_of(q32)
        a, e = m[:, 2], m[:, 0]
        pA = centre + 0.1 * rng.standard_normal(3)
        for tag, t, sep, hits in (("full overlap, the ends of A", 0.0, lim - 0.04, "h0 h1"), ("full overlap, the ends of B", 0.0, lim - 0.5 * MARGIN, "h2 h3"),
                                  ("partial overlap from the + side", L1, 0.06, "h0 h3"), ("partial overlap from the - side", -L1, 0.06, "h1 h2"),
                                  ("partial overlap, the + ends", 0.1, 0.06, "h0 h2"), ("partial overlap, the - end of A inside B", -0.1, 0.06, "h1 h2"),
                                  ("collinear end to end, +", L1 + L2 + r1 + r2 - 0.005, 0.0, "h0 h3"), ("collinear end to end, -", -(L1 + L2 + r1 + r2 + 0.5 * MARGIN), 0.0, "h1 h2"),
                                  ("side by side outside the margin", 0.02, lim + 2 * MARGIN, "")):
            exp = ("cc:parallel", "parallel:%d" % len(hits.split())) + tuple("hit:" + h for h in hits.split())
            add("A-B parallel %d, %s" % (k, tag), ("A", "B"), {"A": (pA, q32), "B": (pA + a * t + e * sep, q32)}, expect=exp, exact=True)
    # ------------------------------------------------------------------ antiparallel and the near-parallel sweep (conditioned by the angle: not exact)
    for k in range(2):
        ql = _qrand(rng)
        m = pair_ref.quat2mat(ql)
        pA, qA = world([0, 0, 0], ql)
        pB, qB = world(m[:, 2] * (0.05 - 0.1 * k) + m[:, 0] * (lim - 0.02), _qmul(ql, _FLIP))
        add("A-B antiparallel %d" % k, ("A", "B"), {"A": (pA, qA), "B": (pB, qB)})
    # The sweep.  "converging": B turned about the direction across both axes, so the lines meet (far) beyond one end and the foot points
    # are clamped - towards the + ends or, turned the other way, the - ends; the result does not depend on the size of det.  "crossing":
    # B turned about the common perpendicular, foot points interior, x = numerator / det with det = angle^2: in the ORACLE's own fp64 the
    # foot point then carries a relative error of 2e-16 / angle^2, so only angles of 1e-2 rad and more reproduce to the 1e-12 at which
    # tests/test_pair_cases_cpu.py holds the restatement to the oracle (0.03 m x 2e-16 / 1e-4 = 6e-14).
    ql = _qrand(rng)
    m = pair_ref.quat2mat(ql)
    for ang in SWEEP_ANGLES:
        for tag, ax, sgn in (("converging beyond the + ends", [0, 1, 0], 1), ("converging beyond the - ends", [0, 1, 0], -1), ("crossing at B's centre", [1, 0, 0], 1)):
            if ax[0] and ang < 1e-2:
                continue
            pA, qA = world([0, 0, 0], ql)
            pB, qB = world(m[:, 2] * 0.03 + m[:, 0] * (lim - 0.02), _qmul(ql, _qaxis(ax, sgn * ang)))
            add("A-B near-parallel %.0e rad, %s" % (ang, tag), ("A", "B"), {"A": (pA, qA), "B": (pB, qB)})
    return cases


# ---------------------------------------------------------------------------------------------------------------- the references
GUARD = 1e-4  # no case sits on an activation boundary: every activation test the reference makes is further than this off its threshold
NPERT = 32    # perturbed evaluations per case
_cache = {}


def state_of(o, qpos):
    """the mjSTATE_INTEGRATION record of a case: at rest at qpos, time 0 (o: anything with nv - an oracle, a model)"""
    return np.concatenate([[0.0], qpos, np.zeros(2 * o.nv)])


def evaluations(cases, evaluate):
    """(evals, ill) of a case table under evaluate(case, qpos) -> dict(qpos, ncon, nefc, con).  evals[i] lists case i's evaluations, the
    unperturbed one first; an exact case has no other, every other case NPERT more at qpos + 2^-24 max(1, |qpos|) N(0, 1) - one
    default_rng(7) per table, drawn in case order.  ill[i]: the evaluations of case i disagree on the contact count."""
    rng = np.random.default_rng(7)
    evals, ill = [], []
    for c in cases:
        ev = [evaluate(c, c["qpos"])]
        if not c["exact"]:
            for _ in range(NPERT):
                ev.append(evaluate(c, c["qpos"] + 2.0 ** -24 * np.maximum(1.0, np.abs(c["qpos"])) * rng.standard_normal(len(c["qpos"]))))
        evals.append(ev)
        ill.append(len({e["ncon"] for e in ev}) > 1)
    return evals, np.array(ill)


def _spread(ref, others):
    """largest deviation of dist, pos and normal of evaluations with ref's count from ref, per contact: [ncon, 3]"""
    env = np.zeros((ref["ncon"], 3))
    for ev in others:
        if ev["ncon"] != ref["ncon"]:
            continue
        for i, (a, b) in enumerate(zip(ref["con"], ev["con"])):
            env[i] = np.maximum(env[i], (abs(a["dist"] - b["dist"]), np.abs(a["pos"] - b["pos"]).max(), np.abs(a["frame"][0] - b["frame"][0]).max()))
    return env


def envelope(ref, i, ncon):
    """(the evaluation of case i that a device reporting ncon contacts is held to, its [ncon, 3] envelope), or None when no evaluation
    the rules allow has that count: the unperturbed reference, or for an ill-conditioned case any of its perturbed evaluations"""
    ev = ref["evals"][i]
    pick = next((e for e in ev if e["ncon"] == ncon), None)
    if pick is None:
        return None
    return pick, _spread(pick, [e for e in ev if e is not pick])


def compiled(hbmod, variant, directory):
    """(model, .hbm path, parsed .hbm) of a scene variant"""
    m = hbmod.Model.from_xml_string(scene_xml(variant))
    p = str(directory / ("pairs_%s.hbm" % variant))
    m.save(p)
    return m, p, parse_hbm(p)


def evaluate(o, qpos):
    """the oracle's contacts at rest at qpos"""
    load_state(o, state_of(o, qpos), np.zeros(o.nu))
    o.forward()
    return dict(qpos=qpos, ncon=o.ncon, nefc=o.nefc, con=o.contacts())


def reference(hbmod, variant, directory):
    """The oracle's side of a scene variant, computed once: dict(model, path, info, cases, evals, ill, oracle).  envelope(ref, i, n) gives
    the evaluation a device count n is held to and the spread around it."""
    if variant in _cache:
        return _cache[variant]
    m, p, info = compiled(hbmod, variant, directory)
    o = Oracle(p)
    cases = build_cases(info)
    evals, ill = evaluations(cases, lambda c, qpos: evaluate(o, qpos))
    ref = dict(model=m, path=p, info=info, cases=cases, evals=evals, ill=ill, oracle=o)
    _cache[variant] = ref
    return ref


# ---------------------------------------------------------------------------------------------------------------- the device's side
def launch(hbmod, gpu, ref, knobs, diag, tiles=1):
    """one step of a batch from the cases' states (tiled `tiles` times), one env per case, no controls: what it left.  knobs: Batch.tune's,
    and body_acc=1 for the body-acceleration read-out; diag: the diagnostic outputs, with the contact records"""
    m, cases = ref["model"], ref["cases"]
    st = np.tile(np.stack([state_of(m, c["qpos"]) for c in cases]), (tiles, 1))
    knobs = dict(knobs)
    acc = knobs.pop("body_acc", 0)
    b = hbmod.Batch(m, len(st), gpu)
    b.tune(**knobs)
    b.diag_enable(diag)
    if acc:
        b.body_acc_readout(True)
    if tiles > 1:
        b.pipeline(False)  # one launch over the whole batch: the two-envs-per-wave narrowphase (hb_narrow.hip: launch_pose_narrow)
    b.set_state(hbmod.STATE_INTEGRATION, st)
    b.step(np.zeros((len(st), m.nu), dtype=np.float32))
    out = dict(kernel=b.last_kernel(), counts=b.counts(), status=b.status(), state=b.get_state(hbmod.STATE_INTEGRATION), qpos=b.qpos.astype(np.float64), qvel=b.qvel.astype(np.float64),
               con=b.contacts().astype(np.float64) if diag else None)
    b.close()
    return out


def held_to(ref, i, ncon, nefc, bad, who):
    """the evaluation case i's device counts are held to and its envelope; None, and an entry in bad that names the reference `who`, if
    the counts match none"""
    c = ref["cases"][i]
    got = envelope(ref, i, ncon)
    if got is None:
        bad.append((c["name"], "contact count", ncon, who, sorted({e["ncon"] for e in ref["evals"][i]})))
    elif nefc != got[0]["nefc"]:
        bad.append((c["name"], "nefc", nefc, who, got[0]["nefc"]))
    else:
        return got
    return None
