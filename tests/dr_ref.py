"""Per-env model parameters (hb_env_domain_randomize) for the tests: the layout of an env's block, the draw restated in numpy, and
the block written into the fp64 oracle's model arrays.

layout(model, stride)      the DomainLayout offsets (hb_device.hpp) from the model's sizes, the limit candidates in constraint order
                           (hb_tables.cpp: build_limits) and the floor the friction scale applies to (the first plane geom)
snapshot / apply / restore one env's block into the oracle's model arrays and the originals back.  Derived constants (body_subtreemass,
                           dof_M0, the inverse weights) are left alone: the engine, like the reference, leaves them stale (include/hb.h)
draw(A, D, env, episode)   domain_draw (hb_env.hip) in np.float32 arithmetic, in the kernel's operation order, on env_ref.rng_uniform
family(D, name, ...)       a hb_domain_randomization that randomises one family of FAMILIES only (or "all", or "none"), with ranges
                           large enough that the effect on one step sits far above fp32 noise

Test infrastructure only.
"""
import numpy as np

from env_ref import rng_uniform
from humanoid_mujoco_amd.engine import HbDomainRandomization

RS_DR_MASS, RS_DR_EXTRA, RS_DR_FRIC, RS_DR_ARM, RS_DR_STIFF, RS_DR_MARGIN, RS_DR_RANGE, RS_DR_KP, RS_DR_FRC, RS_DR_FLOOR = range(16, 26)
GEOM_PLANE = 0
FAMILIES = ("mass", "arm_stiff", "limits", "actuator", "friction")
TABLES = ("mass", "arm", "stiff", "lmargin", "lrange", "gain", "bias1", "frc", "fric", "hfield")
f32 = np.float32
# the multipliers of the family "friction": at 1.2 .. 2 the state after one step (all that a launch without diagnostic outputs is compared
# in) moves by 10 x its bound in 11 of 32 cases on the condim-6 chains, at 2 .. 4 in 22 and 24 (tests/test_dr_ref_cpu.py)
FRICTION_RANGE = (2.0, 4.0)


def limit_candidates(model):
    """[(kind, id, side)]: lower and upper of every limited hinge / slide joint, then of every limited tendon"""
    jt, jl = model.array("jnt_type").astype(int), model.array("jnt_limited").astype(int)
    cand = [(0, j, s) for j in range(model.njnt) if jl[j] and jt[j] >= 2 for s in (-1, 1)]
    if model.ntendon:
        tl = model.array("tendon_limited").astype(int)
        cand += [(1, t, s) for t in range(model.ntendon) if tl[t] for s in (-1, 1)]
    return cand


def layout(model, stride):
    """offsets of the tables of an env's block (keys of TABLES), "stride", the sizes, "cand" and "floor" (geom id or -1).  nhfielddata
    is the model's; nlimcand is what the stride leaves, and must be the model's number of limit candidates."""
    nb, nv, nu = model.nbody, model.nv, model.nu
    nhf = len(model.array("hfield_data"))
    rest = stride - (nb + 2 * nv + 4 * nu + 1 + nhf)
    assert rest >= 0 and rest % 2 == 0, (stride, rest)
    nlim = rest // 2
    cand = limit_candidates(model)
    assert len(cand) == nlim, (len(cand), nlim)
    L = dict(mass=0, arm=nb, stiff=nb + nv, lmargin=nb + 2 * nv)
    L["lrange"] = L["lmargin"] + nlim
    L["gain"] = L["lrange"] + nlim
    L["bias1"] = L["gain"] + nu
    L["frc"] = L["bias1"] + nu
    L["fric"] = L["frc"] + 2 * nu
    L["hfield"] = L["fric"] + 1
    L["stride"] = L["hfield"] + nhf
    assert L["stride"] == stride
    gt = model.array("geom_type").astype(int)
    planes = np.flatnonzero(gt == GEOM_PLANE)
    L.update(nbody=nb, nv=nv, nu=nu, nlimcand=nlim, nhfielddata=nhf, cand=cand, floor=int(planes[0]) if len(planes) else -1,
             jnt_dofadr=model.array("jnt_dofadr").astype(int), jnt_type=model.array("jnt_type").astype(int))
    return L


def stride_of(model):
    return model.nbody + 2 * model.nv + 2 * len(limit_candidates(model)) + 4 * model.nu + 1 + len(model.array("hfield_data"))


def sizes(L):
    """table -> number of entries"""
    return dict(mass=L["nbody"], arm=L["nv"], stiff=L["nv"], lmargin=L["nlimcand"], lrange=L["nlimcand"], gain=L["nu"], bias1=L["nu"], frc=2 * L["nu"], fric=1,
                hfield=L["nhfielddata"])


def table(P, L, name):
    """the table `name` of one block or of a [n, stride] array of blocks"""
    return P[..., L[name]:L[name] + sizes(L)[name]]


ORACLE_ARRAYS = ("body_mass", "dof_armature", "jnt_stiffness", "jnt_margin", "jnt_range", "tendon_margin", "tendon_range", "actuator_gainprm", "actuator_biasprm",
                 "actuator_forcerange", "geom_friction", "hfield_data")


def snapshot(o):
    """copies of the oracle's model arrays that apply writes"""
    base = {}
    for k in ORACLE_ARRAYS:
        try:
            base[k] = o.marr(k).copy()
        except KeyError:  # (an array the model has no entries of: no tendons, no height field)
            pass
    return base


def restore(o, base):
    for k, v in base.items():
        o.marr(k)[:] = v


def apply(o, P_row, L, base):
    """one env's block (fp32 values, handed over exactly) into the oracle's model arrays"""
    P = np.asarray(P_row, dtype=np.float64)
    o.marr("body_mass")[:] = P[L["mass"]:L["mass"] + L["nbody"]]
    o.marr("dof_armature")[:] = P[L["arm"]:L["arm"] + L["nv"]]
    stiff = o.marr("jnt_stiffness")
    for j, t in enumerate(L["jnt_type"]):
        if t >= 2:  # (hinge / slide: the joints whose spring the kernels evaluate)
            stiff[j] = P[L["stiff"] + L["jnt_dofadr"][j]]
    for c, (kind, i, side) in enumerate(L["cand"]):
        margin, rng = (o.marr("jnt_margin"), o.marr("jnt_range")) if kind == 0 else (o.marr("tendon_margin"), o.marr("tendon_range"))
        if side < 0:
            margin[i] = P[L["lmargin"] + c]
        else:
            assert margin[i] == P[L["lmargin"] + c], "one margin per joint / tendon: the lower and the upper candidate carry the same"
        rng[2 * i + (side + 1) // 2] = P[L["lrange"] + c]
    nu = L["nu"]
    o.marr("actuator_gainprm")[:] = P[L["gain"]:L["gain"] + nu]
    o.marr("actuator_biasprm")[1::3] = P[L["bias1"]:L["bias1"] + nu]
    o.marr("actuator_forcerange")[:] = P[L["frc"]:L["frc"] + 2 * nu]
    if L["floor"] >= 0:  # (the scale applies to the first plane geom; a model without one ignores it)
        o.marr("geom_friction")[3 * L["floor"]] = base["geom_friction"][3 * L["floor"]] * P[L["fric"]]
    if L["nhfielddata"]:
        o.marr("hfield_data")[:] = P[L["hfield"]:L["hfield"] + L["nhfielddata"]]


def model_arrays(model):
    """what domain_draw reads of the model, as the device tables hold it (fp32)"""
    A = dict(nbody=model.nbody, nv=model.nv, nu=model.nu, cand=limit_candidates(model))
    for k in ("body_mass", "dof_armature", "jnt_stiffness", "jnt_margin", "jnt_range", "actuator_gainprm", "actuator_biasprm", "actuator_forcerange", "hfield_data"):
        A[k] = model.array(k).astype(f32)
    if model.ntendon:
        A["tendon_margin"], A["tendon_range"] = model.array("tendon_margin").astype(f32), model.array("tendon_range").astype(f32)
    for k in ("jnt_type", "dof_jntid", "hfield_nrow", "hfield_ncol"):
        A[k] = model.array(k).astype(int)
    return A


def draw(A, D, env_global, episode, want_gain=False):
    """the block domain_draw writes for (env_global, episode): np.float32 [stride]; want_gain: also the largest factor bump / (hi - lo)
    a height map's noise sum was scaled by (0 without a drawn map)"""
    nb, nv, nu, cand = A["nbody"], A["nv"], A["nu"], A["cand"]
    nlim, nhf = len(cand), len(A["hfield_data"])
    rf = f32(D.factor)

    def U(stream, idx, step=0):
        return rng_uniform(D.seed, env_global, episode, step, stream, idx)
    one, two = f32(1), f32(2)
    out = []
    # masses: +- max_mass_change per body, and up to max_external_mass on one body
    mass = np.zeros(nb, f32)
    bx = 1 + min(nb - 2, int(U(RS_DR_EXTRA, 0) * f32(nb - 1))) if nb > 1 else -1
    for b in range(1, nb):
        m = max(f32(1e-5), A["body_mass"][b] + (two * U(RS_DR_MASS, b) - one) * f32(D.max_mass_change) * rf)
        if b == bx:
            m = m + U(RS_DR_EXTRA, 1) * f32(D.max_external_mass) * rf
        mass[b] = m
    out.append(mass)
    arm, stiff = np.zeros(nv, f32), np.zeros(nv, f32)
    for i in range(nv):
        j = A["dof_jntid"][i]
        scalar = A["jnt_type"][j] >= 2
        arm[i] = A["dof_armature"][i] + (U(RS_DR_ARM, i) * f32(D.armature_max_change) * rf if scalar else f32(0))
        stiff[i] = A["jnt_stiffness"][j] + (U(RS_DR_STIFF, i) * f32(D.stiffness_max_change) * rf if scalar else f32(0))
    out += [arm, stiff]
    lmargin, lrange = np.zeros(nlim, f32), np.zeros(nlim, f32)
    for c, (kind, i, side) in enumerate(cand):
        if kind == 0:
            lmargin[c] = A["jnt_margin"][i] + U(RS_DR_MARGIN, i) * f32(D.margin_max_change) * rf
            lrange[c] = A["jnt_range"][2 * i + (side + 1) // 2] + (two * U(RS_DR_RANGE, c) - one) * f32(D.range_max_change) * rf
        else:
            lmargin[c], lrange[c] = A["tendon_margin"][i], A["tendon_range"][2 * i + (side + 1) // 2]
    out += [lmargin, lrange]
    gain, bias1, frc = np.zeros(nu, f32), np.zeros(nu, f32), np.zeros(2 * nu, f32)
    for a in range(nu):
        g, b1 = A["actuator_gainprm"][a], A["actuator_biasprm"][3 * a + 1]
        if D.kp_nominal > 0:
            g = f32(D.kp_nominal) + (two * U(RS_DR_KP, a) - one) * f32(D.kp_max_change) * rf
            if b1 != 0:
                b1 = -g
        gain[a], bias1[a] = g, b1
        for s in range(2):
            frc[2 * a + s] = A["actuator_forcerange"][2 * a + s] + (two * U(RS_DR_FRC, 2 * a + s) - one) * f32(D.force_limit_max_change) * rf
    out += [gain, bias1, frc]
    fmin, fmax = f32(D.friction_min_mult), f32(D.friction_max_mult)
    out.append(np.array([(one - rf) + (fmin + U(RS_DR_FRIC, 0) * (fmax - fmin)) * rf], f32))
    # height maps: three octaves of smooth value noise (lattices of 3x3, 5x5, 9x9 nodes), shifted and scaled to [0, bump]
    bump = f32(D.floor_bump_min) + rf * (f32(D.floor_bump_max) - f32(D.floor_bump_min))
    h = np.zeros(nhf, f32)
    adr, gain = 0, 0.0
    for hf in range(len(A["hfield_nrow"])):
        nr, nc = int(A["hfield_nrow"][hf]), int(A["hfield_ncol"][hf])
        n = nr * nc
        if not D.floor_bump_max > 0:
            h[adr:adr + n] = A["hfield_data"][adr:adr + n]
            adr += n
            continue
        v = np.zeros(n, f32)
        for i in range(n):
            r, c = divmod(i, nc)
            acc, amp, cells = f32(0), f32(1), 2
            for octv in range(3):
                x = f32(c) / f32(max(1, nc - 1)) * f32(cells)
                y = f32(r) / f32(max(1, nr - 1)) * f32(cells)
                x0, y0 = min(int(x), cells - 1), min(int(y), cells - 1)
                fx, fy = x - f32(x0), y - f32(y0)
                fx = fx * fx * (f32(3) - two * fx)
                fy = fy * fy * (f32(3) - two * fy)

                def node(ix, iy):
                    return U(RS_DR_FLOOR, (octv * 16 + iy) * 16 + ix, step=hf)
                a, b, cc, dd = node(x0, y0), node(x0 + 1, y0), node(x0, y0 + 1), node(x0 + 1, y0 + 1)
                acc = acc + amp * ((a * (one - fx) + b * fx) * (one - fy) + (cc * (one - fx) + dd * fx) * fy)
                cells *= 2
                amp = amp * f32(0.5)
            v[i] = acc
        lo, hi = v.min(), v.max()
        sc = bump / (hi - lo) if hi > lo else f32(0)
        gain = max(gain, float(sc))
        h[adr:adr + n] = (v - lo) * sc
        adr += n
    out.append(h)
    block = np.concatenate(out).astype(f32)
    return (block, gain) if want_gain else block


def draw_bounds(A, D, hfield_gain=1.0):
    """per table, 2 ulp of the largest term of the expression that fills it (what a contracted multiply-add may move an entry by):
    a dict table -> array of absolute bounds (zero where the entry is a plain copy)"""
    def ulp2(x):
        return 2.0 * np.spacing(np.abs(np.asarray(x, dtype=f32)).astype(f32)).astype(np.float64)
    nb, nv, nu, cand = A["nbody"], A["nv"], A["nu"], A["cand"]
    rf = abs(D.factor)
    scalar = A["jnt_type"][A["dof_jntid"]] >= 2
    B = {}
    B["mass"] = ulp2(np.maximum(np.abs(A["body_mass"]) + D.max_external_mass * rf, D.max_mass_change * rf) * (D.max_mass_change + D.max_external_mass > 0))
    B["mass"][0] = 0.0
    B["arm"] = ulp2(np.maximum(np.abs(A["dof_armature"]), D.armature_max_change * rf)) * (scalar & (D.armature_max_change > 0))
    B["stiff"] = ulp2(np.maximum(np.abs(A["jnt_stiffness"][A["dof_jntid"]]), D.stiffness_max_change * rf)) * (scalar & (D.stiffness_max_change > 0))
    joint = np.array([k == 0 for k, _, _ in cand], dtype=bool)
    m0 = np.array([A["jnt_margin"][i] if k == 0 else 0.0 for k, i, _ in cand])
    r0 = np.array([A["jnt_range"][2 * i + (s + 1) // 2] if k == 0 else 0.0 for k, i, s in cand])
    B["lmargin"] = ulp2(np.maximum(np.abs(m0), D.margin_max_change * rf)) * (joint & (D.margin_max_change > 0)) if len(cand) else np.zeros(0)
    B["lrange"] = ulp2(np.maximum(np.abs(r0), D.range_max_change * rf)) * (joint & (D.range_max_change > 0)) if len(cand) else np.zeros(0)
    kp = D.kp_nominal > 0
    B["gain"] = ulp2(np.full(nu, max(D.kp_nominal, D.kp_max_change * rf))) * kp
    B["bias1"] = B["gain"].copy()
    B["frc"] = ulp2(np.maximum(np.abs(A["actuator_forcerange"]), D.force_limit_max_change * rf)) * (D.force_limit_max_change > 0)
    B["fric"] = ulp2(np.array([max(1.0, D.friction_max_mult * rf)]))
    # a height: the noise sum (at most 1.75) is the largest term; the normalisation (v - lo) * bump / (hi - lo) carries its rounding on,
    # times hfield_gain = bump / (hi - lo) where that exceeds 1 (draw(..., want_gain=True) reports it)
    B["hfield"] = ulp2(np.full(len(A["hfield_data"]), 1.75)) * (D.floor_bump_max > 0) * max(1.0, hfield_gain)
    return B


def family(name, seed=9, kp=None, bump=0.0):
    """a hb_domain_randomization that randomises the family `name` only; "all": every family, and the
    height maps where bump > 0 (the maps' top, in the height field's own elevation units); "none": nothing (the block then holds the
    model's own fp32 values).  kp = (nominal, max change): the reference robot's gain path, part of the family "actuator"."""
    assert name in FAMILIES + ("all", "none"), name
    on = (lambda f: name in (f, "all"))
    D = HbDomainRandomization()
    D.factor, D.seed = 1.0, seed
    D.max_mass_change, D.max_external_mass = (0.5, 0.2) if on("mass") else (0.0, 0.0)
    D.armature_max_change, D.stiffness_max_change = (0.02, 2.0) if on("arm_stiff") else (0.0, 0.0)
    D.margin_max_change, D.range_max_change = (0.02, 0.015) if on("limits") else (0.0, 0.0)
    D.force_limit_max_change = 0.2 if on("actuator") else 0.0
    D.kp_nominal, D.kp_max_change = (kp if kp is not None and on("actuator") else (0.0, 0.0))
    # the mixed coefficient is the larger of the floor's and the other geom's: only a scale that lifts the floor's above the other's shows
    D.friction_min_mult, D.friction_max_mult = FRICTION_RANGE if on("friction") else (1.0, 1.0)
    D.floor_bump_min, D.floor_bump_max = 0.0, (bump if name == "all" else 0.0)
    return D
