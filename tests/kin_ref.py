"""fp64 reference of the whole-body kinematics read-out (include/hb.h: hb_kinematics): the oracle's mj_kinematics / mj_comVel products
after forward(), stacked into the read-out's three layouts, and a model generator for the lane counts of its kernels.

TEST INFRASTRUCTURE: the product package never imports this module.

    body_pose [nbody, 10] = xpos | xquat | xipos
    body_vel  [nbody, 6]  = omega | v,   omega = cvel_ang,  v = cvel_lin + cvel_ang x (xipos - subtree_com[body_rootid])
    geom_pose: geom_xpos [ngeom, 3] and geom_xmat [ngeom, 3, 3] (the device returns the orientation as a quaternion)

cvel refers to the subtree centre of mass of the body's tree (mj_comVel); moved to the body's own xipos it is
mj_objectVelocity(objtype body, flg_local = 0).  tests/test_kin_cpu.py holds the formula to central differences of xipos / ximat.
"""
import numpy as np

from oracle_lib import load_state


def reference(o):
    """dict of pose [nbody, 10], vel [nbody, 6], geom_xpos [ngeom, 3], geom_xmat [ngeom, 3, 3] of the oracle's current data"""
    nb, ng = o.nbody, o.ngeom
    xpos, xquat, xipos = o.xpos.reshape(nb, 3), o.xquat.reshape(nb, 4), o.xipos.reshape(nb, 3)
    cvel, scom = o.cvel.reshape(nb, 6), o.subtree_com.reshape(nb, 3)
    root = np.asarray(o.info["body_rootid"])
    vel = np.zeros((nb, 6))
    vel[:, 0:3] = cvel[:, 0:3]
    vel[:, 3:6] = cvel[:, 3:6] + np.cross(cvel[:, 0:3], xipos - scom[root])
    vel[0] = 0.0
    return dict(pose=np.concatenate([xpos, xquat, xipos], axis=1), vel=vel, geom_xpos=o.geom_xpos.reshape(ng, 3).copy(),
                geom_xmat=o.geom_xmat.reshape(ng, 3, 3).copy())


def references(o, states):
    """reference() of every [time, qpos, qvel, warm] record, stacked along a leading axis"""
    out = []
    for s in states:
        load_state(o, s, np.zeros(o.nu))
        o.forward()
        out.append(reference(o))
    return {k: np.array([r[k] for r in out]) for k in out[0]}


def quat_to_mat(q):
    """fp64 rotation matrices [..., 3, 3] of quaternions [..., 4] (w x y z), normalised first"""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def errors(ref, dev, k):
    """State k of a device read-out (dict pose / vel / geoms as Batch.kinematics returns them) against state k of references():
    (pose error, velocity error), each the largest deviation relative to max(1, max |reference|) of the state.  The pose error covers
    xpos, xipos, geom_xpos, the quaternions up to sign and their | |q| - 1 |, and the geoms' orientation as matrices against
    geom_xmat."""
    p, rp = dev["pose"][k].astype(np.float64), ref["pose"][k]
    scale = max(1.0, float(np.abs(rp).max()), float(np.abs(ref["geom_xpos"][k]).max()))
    e = [np.abs(p[:, 0:3] - rp[:, 0:3]).max(), np.abs(p[:, 7:10] - rp[:, 7:10]).max()]
    q, rq = p[:, 3:7], rp[:, 3:7]
    sign = np.where((q * rq).sum(axis=1, keepdims=True) < 0, -1.0, 1.0)
    e += [np.abs(sign * q - rq).max(), np.abs(np.linalg.norm(q, axis=1) - 1).max()]
    if "geoms" in dev:
        g = dev["geoms"][k].astype(np.float64)
        gq = g[:, 3:7]
        w, x, y, z = gq[:, 0], gq[:, 1], gq[:, 2], gq[:, 3]
        mat = np.stack([np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                        np.stack([2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)], -1),
                        np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1)], -2)
        e += [np.abs(g[:, 0:3] - ref["geom_xpos"][k]).max(), np.abs(mat - ref["geom_xmat"][k]).max(), np.abs(np.linalg.norm(gq, axis=1) - 1).max()]
    pose_err = float(max(e)) / scale
    vel_err = None
    if "vel" in dev:
        rv = ref["vel"][k]
        vel_err = float(np.abs(dev["vel"][k].astype(np.float64) - rv).max()) / max(1.0, float(np.abs(rv).max()))
    return pose_err, vel_err


# ---- a model for every lane count of the kernels

AXES = ("0 1 0", "0 0 1", "1 0 0")


def bush_xml(branches, joint_every=1, timestep=0.004):
    """A free base carrying one capsule chain per entry of `branches` (its length in links), a hinge on every joint_every-th link on
    alternating axes (the links between are welded to their parents), the second hinge of the first branch a slide joint instead, the
    first link of the last branch with three joints (two hinges and a slide), a non-identity quat on every link, geoms offset from
    their body frames, a motor on every joint.  Only the base and every seventh link collide, and only with the floor.
    1 + sum(branches) moving bodies, one geom each, and the floor."""
    assert 1 <= len(branches) <= 8 and max(branches) <= 15  # (<= 8 children, tree depth <= 16)
    parts = ['<body name="base" pos="0 0 0.6" quat="0.96 0.1 -0.2 0.15"><freejoint name="root"/>'
             '<geom name="base" type="sphere" pos="0.01 -0.02 0.015" size="0.07" mass="1.5" contype="1"/>']
    joints, nj, link = [], 0, 0
    for bi, n in enumerate(branches):
        ang = 360.0 * bi / len(branches)
        for k in range(n):
            if k == 0:
                parts.append('<body name="b%d_%d" pos="%.4f %.4f 0" euler="%g %g %g">' % (bi, k, 0.08 * np.cos(np.radians(ang)), 0.08 * np.sin(np.radians(ang)), 10 + 3 * bi, -15, ang))
            else:
                parts.append('<body name="b%d_%d" pos="0.1 0 0" euler="%g %g %g">' % (bi, k, 4 + (link % 5), -7 + 2 * (link % 3), 5 - 3 * (link % 4)))
            triple = bi == len(branches) - 1 and k == 0
            if triple:
                for a, t in ((0, "hinge"), (1, "hinge"), (2, "slide")):
                    name = "j%d" % nj
                    rng = ' limited="true" range="-0.02 0.02"' if t == "slide" else ""
                    parts.append('<joint name="%s" type="%s" axis="%s" pos="0.01 0.005 %g"%s/>' % (name, t, AXES[a], 0.002 * a, rng))
                    joints.append(name); nj += 1
            elif k % joint_every == 0:
                name = "j%d" % nj
                if bi == 0 and k == joint_every:
                    parts.append('<joint name="%s" type="slide" axis="1 0 0" limited="true" range="-0.02 0.02"/>' % name)
                else:
                    lim = ' limited="true" range="-%d %d"' % (25 + 3 * (nj % 5), 25 + 3 * (nj % 5)) if nj % 3 == 1 else ""
                    parts.append('<joint name="%s" type="hinge" axis="%s" pos="0 0.004 -0.003"%s/>' % (name, AXES[nj % 2 if nj % 7 else 2], lim))
                joints.append(name); nj += 1
            parts.append('<geom name="g%d_%d" type="capsule" fromto="0.01 0.004 0 0.1 -0.004 0.006" size="0.02" mass="%g" contype="%d"/>' % (bi, k, 0.15 + 0.01 * (link % 7), 1 if link % 7 == 3 else 0))
            link += 1
        parts.append("</body>" * n)
    parts.append("</body>")
    motors = "".join('<motor name="m_%s" joint="%s" gear="2" ctrlrange="-1 1" ctrllimited="true"/>' % (n, n) for n in joints)
    return ('<mujoco model="bush"><compiler angle="degree"/><option timestep="%g" iterations="50" tolerance="0" solver="PGS"/>'
            '<default><joint damping="0.05" armature="0.01"/><geom conaffinity="0" condim="3"/></default>'
            '<worldbody><geom name="floor" type="plane" size="0 0 1" condim="3" friction="1 0.01 0.001" contype="1" conaffinity="1"/>%s</worldbody>'
            '<actuator>%s</actuator></mujoco>' % (timestep, "".join(parts), motors))


# ---- the parity cases of tests/test_gpu_kinematics.py and tools/gpu_kinematics_report.py

FL = (4.0, 0.05, 0.6, 0.02, 3.0)
BUSHES = {  # name -> (branches, joint_every, moving bodies, kernel)
    "bush17": ((8, 8), 1, 17, "hb_kin32_kernel"),              # the first size on 32 lanes
    "bush32": ((11, 10, 10), 2, 32, "hb_kin32_kernel"),        # the last
    "bush33": ((11, 11, 10), 2, 33, "hb_kin64_kernel"),        # the first on 64
    "bush63": ((15, 15, 15, 15, 2), 3, 63, "hb_kin64_kernel"),  # nbody = 64, the engine's maximum
}
CASES = ("humanoid27", "chain32", "team_robot", "fric_chain28", "humanoid27_rk4") + tuple(BUSHES)


def fric_chain_xml(nv=28):
    """kernel_models.chain_xml with frictionloss on the joints j0, j2, j4, ... (a model that steps in the friction-loss kernels)"""
    import re

    from kernel_models import chain_xml
    return re.sub(r'<joint name="j(\d+)"', lambda mo: mo.group(0) + (' frictionloss="%g"' % FL[(int(mo.group(1)) // 2) % len(FL)] if int(mo.group(1)) % 2 == 0 else ""),
                  chain_xml(nv))


def parity_case(hbmod, name, tmp_path, nstates=30):
    """(model, oracle, kernel the read-out must take, [time, qpos, qvel, warm] records along an oracle rollout of the model - contacts,
    joint limits and a tumbling free base included) of one entry of CASES"""
    import os

    from kernel_models import chain_xml, oracle_for, rollout_states
    from oracle_lib import HUMANOID_HBM, Oracle
    kernel = "hb_kin16_kernel"
    if name in ("humanoid27", "humanoid27_rk4", "team_robot"):
        path = HUMANOID_HBM if name != "team_robot" else os.path.join(os.path.dirname(HUMANOID_HBM), "team_robot.hbm")
        m, o = hbmod.Model.load(path), Oracle(path)
        if name == "humanoid27_rk4":
            m.set_opt(integrator=hbmod.INT_RK4)
    elif name == "chain32":
        m, _, o = oracle_for(hbmod, chain_xml(32), tmp_path, name + ".hbm")
    elif name == "fric_chain28":
        m, _, o = oracle_for(hbmod, fric_chain_xml(28), tmp_path, name + ".hbm")
    else:
        branches, every, moving, kernel = BUSHES[name]
        m, _, o = oracle_for(hbmod, bush_xml(branches, every), tmp_path, name + ".hbm")
        assert m.nbody == moving + 1, (name, m.nbody)
    states, _ = rollout_states(o, steps=10 * nstates, every=10, seed=3)
    return m, o, kernel, states


def split_state(o, states):
    """(qpos [n, nq], qvel [n, nv]) float32 of [time, qpos, qvel, warm] records"""
    s = np.asarray(states)
    return s[:, 1:1 + o.nq].astype(np.float32), s[:, 1 + o.nq:1 + o.nq + o.nv].astype(np.float32)
