"""fp64 reference of the dynamics read-out (include/hb.h: hb_dynamics): the oracle's products after forward(), in the read-out's layouts.

TEST INFRASTRUCTURE: the product package never imports this module.

    M            [nv, nv]      Oracle.dense_M(): mj_fullM of qM, armature included
    qfrc_bias    [nv]          the oracle's array (mj_rne with zero acceleration)
    qfrc_passive [nv]          the oracle's array (joint springs and dampers)
    jac          [n, 6, nv]    rows 0..2 jacp, rows 3..5 jacr of the spec's points, built from xanchor / xaxis / xpos / xmat:
                               hinge  jacr = axis, jacp = axis x (p - anchor);   slide  jacp = axis;
                               free   jacp = identity for the three translations; for rotation k the body's own axis k (column k of
                                      xmat) as jacr and axis x (p - xpos) as jacp
                               - each only for the dofs of the point's body and of its ancestors
    a subtree's centre of mass: the mass-weighted mean of the xipos Jacobians of the subtree's bodies (rotational rows zero)

tests/test_dyn_cpu.py holds these formulas to central differences of the oracle's own poses and to the oracle's velocities, energy and
smooth accelerations.
"""
import numpy as np

import kin_ref
from oracle_lib import load_state

JAC_POINT, JAC_SUBTREE_COM = 0, 1


def dof_moves_body(o):
    """[nbody, nv] bool: dof d belongs to body b or to one of its ancestors"""
    parent, dof_body = np.asarray(o.info["body_parentid"]), np.asarray(o.info["dof_bodyid"])
    out = np.zeros((o.nbody, o.nv), dtype=bool)
    for b in range(1, o.nbody):
        a = b
        while a > 0:
            out[b] |= dof_body == a
            a = parent[a]
    return out


def subtree_members(o, root):
    parent = np.asarray(o.info["body_parentid"])
    out = []
    for b in range(1, o.nbody):
        a = b
        while a > 0 and a != root:
            a = parent[a]
        if a == root:
            out.append(b)
    return out


def point_jacobian(o, body, point, moves=None):
    """[6, nv] = jacp | jacr of the world point `point` moving with `body`, from the oracle's current data"""
    nv = o.nv
    moves = dof_moves_body(o) if moves is None else moves
    jt, jdof, jbody = (np.asarray(o.info[k]) for k in ("jnt_type", "jnt_dofadr", "jnt_bodyid"))
    xanchor, xaxis = o.xanchor.reshape(-1, 3), o.xaxis.reshape(-1, 3)
    xpos, xmat = o.xpos.reshape(-1, 3), o.xmat.reshape(-1, 3, 3)
    J = np.zeros((6, nv))
    for j in range(o.njnt):
        d = jdof[j]
        if not moves[body, d]:
            continue
        if jt[j] == 0:  # free: translations along the world axes, rotations about the body's own axes
            b = jbody[j]
            J[0:3, d:d + 3] = np.eye(3)
            for k in range(3):
                axis = xmat[b][:, k]
                J[3:6, d + 3 + k] = axis
                J[0:3, d + 3 + k] = np.cross(axis, point - xpos[b])
        elif jt[j] == 2:  # slide
            J[0:3, d] = xaxis[j]
        else:  # hinge (ball joints do not occur: the engine has none)
            assert jt[j] == 3, jt[j]
            J[3:6, d] = xaxis[j]
            J[0:3, d] = np.cross(xaxis[j], point - xanchor[j])
    return J


def spec_points(spec):
    """[(kind, body, offset)] of an HbJacSpec"""
    return [(int(spec.kind[k]), int(spec.body[k]), np.array([spec.offset[k][i] for i in range(3)], dtype=np.float64)) for k in range(spec.n)]


def jacobians(o, points):
    """[len(points), 6, nv] of (kind, body, offset) points, from the oracle's current data"""
    moves = dof_moves_body(o)
    xpos, xmat, xipos = o.xpos.reshape(-1, 3), o.xmat.reshape(-1, 3, 3), o.xipos.reshape(-1, 3)
    mass = o.marr("body_mass")
    out = []
    for kind, body, off in points:
        if kind == JAC_POINT:
            out.append(point_jacobian(o, body, xpos[body] + xmat[body] @ off, moves))
        else:
            members = subtree_members(o, body) if body else list(range(1, o.nbody))
            J = np.zeros((6, o.nv))
            for c in members:
                J[0:3] += mass[c] * point_jacobian(o, c, xipos[c], moves)[0:3]
            out.append(J / sum(mass[c] for c in members))
    return np.array(out)


def point_positions(o, points):
    """[len(points), 3]: where the points are (a subtree's: its centre of mass), from the oracle's current data"""
    xpos, xmat, xipos = o.xpos.reshape(-1, 3), o.xmat.reshape(-1, 3, 3), o.xipos.reshape(-1, 3)
    mass = o.marr("body_mass")
    out = []
    for kind, body, off in points:
        if kind == JAC_POINT:
            out.append(xpos[body] + xmat[body] @ off)
        else:
            members = subtree_members(o, body) if body else list(range(1, o.nbody))
            out.append(sum(mass[c] * xipos[c] for c in members) / sum(mass[c] for c in members))
    return np.array(out)


def reference(o, points=None):
    """dict M, bias, passive (and jac) of the oracle's current data (after forward())"""
    out = dict(M=o.dense_M(), bias=o.qfrc_bias.copy(), passive=o.qfrc_passive.copy())
    if points is not None:
        out["jac"] = jacobians(o, points)
    return out


def references(o, states, points=None):
    """reference() of every [time, qpos, qvel, warm] record, stacked along a leading axis"""
    out = []
    for s in states:
        load_state(o, s, np.zeros(o.nu))
        o.forward()
        out.append(reference(o, points))
    return {k: np.array([r[k] for r in out]) for k in out[0]}


def errors(ref, dev, k):
    """State k of a device read-out (a dict as Batch.dynamics returns it) against state k of references(): quantity -> the largest
    deviation relative to max(1, max |reference|) of that quantity in that state"""
    return {q: float(np.abs(dev[q][k].astype(np.float64) - ref[q][k]).max()) / max(1.0, float(np.abs(ref[q][k]).max())) for q in dev}


def default_points(hbmod, m):
    """The sixteen points the parity cases read: body frames, sites, bodies' centres of mass and subtrees' centres of mass spread over
    the tree (the whole model's included), as arguments of Batch.jac_spec"""
    ids = list(range(1, m.nbody))
    n = len(ids)
    sel = lambda shift: [ids[min(n - 1, (i * n) // 4 + shift)] for i in range(4)]
    sites = [(b, (0.03 * (i + 1), -0.02, 0.05 - 0.01 * i)) for i, b in enumerate(sel(1))]
    return dict(bodies=sel(0), sites=sites, body_coms=sel(2), subtree_coms=[0, 1, ids[n // 3], ids[(2 * n) // 3]])


DYN_KERNEL = {"hb_kin16_kernel": "hb_dyn16_kernel", "hb_kin32_kernel": "hb_dyn32_kernel", "hb_kin64_kernel": "hb_dyn64_kernel"}


def parity_case(hbmod, name, tmp_path):
    """kin_ref.parity_case with the dynamics kernel the model's size asks for (the read-outs choose their lane counts alike)"""
    m, o, kernel, states = kin_ref.parity_case(hbmod, name, tmp_path)
    return m, o, DYN_KERNEL[kernel], states
