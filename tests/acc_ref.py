"""fp64 reference of the body-acceleration read-out (include/hb.h: hb_body_acc_readout): mj_rnePostConstraint's cacc, the bodies'
accelerations at their own xipos (mj_objectAcceleration, objtype body, world axes) and the accelerometer / gyro / frame-acceleration
sensor entries, from the oracle's data after forward().

TEST INFRASTRUCTURE: the product package never imports this module.

    cacc[0] = (0, -gravity)                      (zero with mjDSBL_GRAVITY)
    cacc[b] = cacc[parent(b)] + sum over the dofs i of b, in order: cdof_dot[i] qvel[i] + cdof[i] qacc[i]

Spatial vectors are angular[3] | linear[3], refer to the subtree centre of mass of the body's tree (subtree_com[body_rootid[b]]) and are
in world axes.  The gravity pseudo-acceleration is part of the convention: at rest on the floor +|g| upward, in free fall 0.  qacc is
an ARGUMENT everywhere, so that the same functions take the oracle's qacc (parity) or the device's own (decode); None: the oracle's.
"""
import numpy as np

DSBL_GRAVITY = 1 << 6


def _sizes(o):
    return o.nbody, o.nv


def world_cacc(o):
    g = np.zeros(6)
    if not (int(o.opt("disableflags")) & DSBL_GRAVITY):
        g[3:6] = -np.asarray(o.marr("gravity"), dtype=np.float64)
    return g


def cacc(o, qacc=None):
    """[nbody, 6]: the recursion above, on the oracle's cdof, cdof_dot and qvel"""
    nb, nv = _sizes(o)
    qacc = np.asarray(o.qacc if qacc is None else qacc, dtype=np.float64)
    cdof, cdd, qvel = o.cdof.reshape(nv, 6), o.cdof_dot.reshape(nv, 6), np.asarray(o.qvel)
    parent, dof_body = o.info["body_parentid"], o.info["dof_bodyid"]
    a = np.zeros((nb, 6))
    a[0] = world_cacc(o)
    for b in range(1, nb):
        a[b] = a[parent[b]]
        for i in range(nv):
            if dof_body[i] == b:
                a[b] = a[b] + cdd[i] * qvel[i] + cdof[i] * qacc[i]
    return a


def point_acc(o, a, b, point):
    """(angular velocity, angular acceleration, linear acceleration) of the point `point` (world coordinates) moving with body b, world
    axes, given cacc `a`: cvel and cacc are moved from the subtree centre of mass to the point, and omega x v is added to the linear
    part (mj_objectAcceleration)"""
    nb = o.nbody
    r = np.asarray(point, dtype=np.float64) - o.subtree_com.reshape(nb, 3)[o.info["body_rootid"][b]]
    cv = o.cvel.reshape(nb, 6)[b]
    om, al = cv[0:3], a[b, 0:3]
    v = cv[3:6] + np.cross(om, r)
    return om.copy(), al.copy(), a[b, 3:6] + np.cross(al, r) + np.cross(om, v)


def body_acc(o, qacc=None, a=None):
    """[nbody, 6] = angular | linear acceleration of every body's xipos, world axes: what hb_get_body_acc returns"""
    nb = o.nbody
    a = cacc(o, qacc) if a is None else a
    out = np.zeros((nb, 6))
    xipos = o.xipos.reshape(nb, 3)
    for b in range(nb):
        _, al, li = point_acc(o, a, b, xipos[b])
        out[b, 0:3], out[b, 3:6] = al, li
    return out


def imu(o, body, offset, qacc=None, a=None):
    """[6] = accelerometer | gyro of a site at body frame + offset with the body's orientation: R' (linear acceleration of the point) |
    R' omega"""
    nb = o.nbody
    a = cacc(o, qacc) if a is None else a
    R = o.xmat.reshape(nb, 3, 3)[body]
    p = o.xpos.reshape(nb, 3)[body] + R @ np.asarray(offset, dtype=np.float64)
    om, _, li = point_acc(o, a, body, p)
    return np.concatenate([R.T @ li, R.T @ om])


def frameacc(o, body, qacc=None, a=None):
    """[6] = frameangacc | framelinacc, objtype body: row `body` of body_acc"""
    return body_acc(o, qacc, a)[body]


def readout(o, qacc=None, imus=(), frameacc_bodies=()):
    """dict of cacc, body_acc [nbody, 6], imu [len(imus), 6] and frameacc [len(frameacc_bodies), 6] of the oracle's current data"""
    a = cacc(o, qacc)
    acc = body_acc(o, a=a)
    return dict(cacc=a, body_acc=acc, imu=np.array([imu(o, b, off, a=a) for b, off in imus]).reshape(len(imus), 6),
                frameacc=acc[list(frameacc_bodies)].reshape(len(frameacc_bodies), 6))


def scale(acc):
    """what the errors of a state are relative to: max(1, max |read-out|)"""
    return max(1.0, float(np.abs(acc).max()))


# ---- the device's read-out against the reference (tests/test_gpu_body_acc.py, tools/gpu_body_acc_report.py)

def device_readout(hb, model, states, ctrls, device=0, tune=None, diag=True, forward=False):
    """One step (or forward pass) of the states on the device with the read-out on: a dict of body_acc, the device's own qacc (None
    without diag), counts, status and the kernel's name"""
    b = hb.Batch(model, len(states), device)
    if tune:
        b.tune(**tune)
    b.diag_enable(diag)
    b.body_acc_readout(True)
    b.set_state(hb.STATE_INTEGRATION, np.asarray(states))
    if forward:
        b.forward(np.asarray(ctrls, dtype=np.float32))
    else:
        b.step(np.asarray(ctrls, dtype=np.float32))
    ncon, nefc, _ = b.counts()
    out = dict(acc=b.body_acc().astype(np.float64), qacc=b.qacc().astype(np.float64) if diag else None, ncon=ncon, nefc=nefc, status=b.status(), kernel=b.last_kernel())
    b.close()
    return out


def compare_state(o, dev, k):
    """Env k of a device_readout against the oracle's CURRENT data (forward() done at that env's state), errors relative to
    max(1, max |reference read-out|):
      decode: against the reference fed with the DEVICE's own qacc on the oracle's kinematics (needs the diagnostics) - no state left out
      parity: against the reference on the oracle's qacc; None when the state's (ncon, nefc) differ from the oracle's"""
    out = {"decode": None, "parity": None}
    if dev["qacc"] is not None:
        ref = body_acc(o, dev["qacc"][k])
        out["decode"] = float(np.abs(dev["acc"][k] - ref).max()) / scale(ref)
    if (int(dev["ncon"][k]), int(dev["nefc"][k])) == (o.ncon, o.nefc):
        ref = body_acc(o)
        out["parity"] = float(np.abs(dev["acc"][k] - ref).max()) / scale(ref)
    return out


def compare(o, states, ctrls, dev, at_state=None):
    """compare_state over all states after the oracle's forward() at each (at_state(o, k): puts the oracle there instead, e.g. at the
    last RK4 stage): (decode errors of every state, or None without the diagnostics; parity errors of the states whose counts agree;
    number of states left out of the parity tier)"""
    from oracle_lib import load_state
    dec, par = [], []
    for k, (s, c) in enumerate(zip(states, ctrls)):
        if at_state is None:
            load_state(o, s, np.asarray(c, dtype=np.float64))
            o.forward()
        else:
            at_state(o, k)
        r = compare_state(o, dev, k)
        if r["decode"] is not None:
            dec.append(r["decode"])
        if r["parity"] is not None:
            par.append(r["parity"])
    return (np.array(dec) if dev["qacc"] is not None else None), np.array(par), len(states) - len(par)
