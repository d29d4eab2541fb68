"""fp64 reference of the contact-force read-out (include/hb.h: hb_contact_readout): mj_contactForce of every contact and the bodies'
contact wrenches, decoded from constraint-row forces with the oracle's row conventions (oracle/mjstep_oracle.c, mj_makeConstraint: a
condim-1 contact has one row, any other 2 (dim - 1) pyramid rows  normal +- friction[k - 1] * direction k, in that order).

TEST INFRASTRUCTURE: the product package never imports this module.

A contact is a dict as Oracle.contacts() returns it: pos, frame (rows n, t1, t2), dim, geom1, geom2, efc_address (< 0: no rows),
friction5.  The decode is a linear map of the row forces, so it applies to the oracle's own efc_force as well as to the device's.
"""
import numpy as np


def contact_forces(efc_force, contacts):
    """[ncon, 6] contact-frame force | torque of every contact."""
    f = np.zeros((len(contacts), 6))
    efc_force = np.asarray(efc_force, dtype=np.float64)
    for k, c in enumerate(contacts):
        a, d = int(c["efc_address"]), int(c["dim"])
        if a < 0:
            continue
        if d == 1:
            f[k, 0] = efc_force[a]
            continue
        r = efc_force[a:a + 2 * (d - 1)]
        f[k, 0] = r.sum()
        for i in range(d - 1):
            f[k, i + 1] = c["friction5"][i] * (r[2 * i] - r[2 * i + 1])
    return f


def body_wrenches(f, contacts, geom_bodyid, xipos, nbody):
    """[nbody, 6]: force | torque about xipos[b], world axes, of the contacts on every body (+ on geom2's body, - on geom1's),
    summed in contact order."""
    w = np.zeros((nbody, 6))
    xipos = np.asarray(xipos, dtype=np.float64).reshape(nbody, 3)
    for k, c in enumerate(contacts):
        frame = np.asarray(c["frame"], dtype=np.float64).reshape(3, 3)
        F, T = frame.T @ f[k, 0:3], frame.T @ f[k, 3:6]
        for g, sign in ((c["geom2"], 1.0), (c["geom1"], -1.0)):
            b = int(geom_bodyid[int(g)])
            w[b, 0:3] += sign * F
            w[b, 3:6] += sign * (np.cross(np.asarray(c["pos"], dtype=np.float64) - xipos[b], F) + T)
    return w


def touch(f, contacts, geom_bodyid, body):
    """the touch entry of a body: the normal forces of the contacts that involve it, summed"""
    return sum(f[k, 0] for k, c in enumerate(contacts) if body in (int(geom_bodyid[int(c["geom1"])]), int(geom_bodyid[int(c["geom2"])])))


def oracle_readout(o):
    """(f [ncon, 6], w [nbody, 6], contacts) of the oracle's current data (after forward())."""
    con = o.contacts()
    f = contact_forces(o.efc_force[:o.nefc], con)
    return f, body_wrenches(f, con, o.info["geom_bodyid"], o.xipos, o.nbody), con


def root_checks(o, w):
    """The three identities of the reference decode against the oracle's own J' efc_force, for a model whose body 1 hangs on a free
    joint (dofs 0..2: world-frame translation, 3..5: rotation in the body frame).  Returns the largest deviation relative to
    max(1, max |efc_force|)."""
    nv, ne, nb = o.nv, o.nefc, o.nbody
    force = o.efc_force[:ne]
    scale = max(1.0, float(np.abs(force).max(initial=0.0)))
    jtf = o.efc_J[:ne * nv].reshape(ne, nv).T @ force if ne else np.zeros(nv)
    xipos = o.xipos.reshape(nb, 3)
    root = o.xpos.reshape(nb, 3)[1]
    rmat = o.xmat.reshape(nb, 3, 3)[1]
    # only the root's tree carries the free joint's dofs: sum the bodies of that tree (every body but the world, in these models)
    tq = sum(w[b, 3:6] + np.cross(xipos[b] - root, w[b, 0:3]) for b in range(1, nb))
    dev = [np.abs(w[1:, 0:3].sum(axis=0) - jtf[0:3]).max(), np.abs(rmat.T @ tq - jtf[3:6]).max(),
           np.abs(w[:, 0:3].sum(axis=0)).max(), np.abs(sum(w[b, 3:6] + np.cross(xipos[b], w[b, 0:3]) for b in range(nb))).max()]
    return max(dev) / scale


def team_states(o, n=16, every=12):
    """n states of the team robot along an oracle rollout from its on-the-floor keyframe under small sinusoidal controls (it stays down
    and in contact, condim 6): [time, qpos, qvel, qacc_warmstart] rounded to fp32 (what hb_set_state leaves on the device) and the
    controls of the step that follows each."""
    o.reset(0)
    states, ctrls = [], []
    for t in range(n * every):
        o.ctrl[:] = 0.2 * np.sin(0.05 * t + np.arange(o.nu))
        if t % every == every - 1:
            states.append(np.concatenate([[o.time], o.qpos, o.qvel, o.qacc_warmstart]))
            ctrls.append(o.ctrl.copy())
        o.step()
    return np.array(states).astype(np.float32).astype(np.float64), np.array(ctrls, dtype=np.float32)


# ---- the device's read-out against the reference (tests/test_gpu_contact_force.py, tools/gpu_contact_force_report.py)

def device_readout(hb, model, states, ctrls, device=0, tune=None, diag=True, forward=False):
    """One step (or forward pass) of the states on the device with the read-out on: a dict of contact_force, body_contact, the
    diagnostics (efc_force, contacts; None without diag), counts, status and the kernel's name."""
    b = hb.Batch(model, len(states), device)
    if tune:
        b.tune(**tune)
    b.diag_enable(diag)
    b.contact_readout(True)
    b.set_state(hb.STATE_INTEGRATION, np.asarray(states))
    if forward:
        b.forward(np.asarray(ctrls, dtype=np.float32))
    else:
        b.step(np.asarray(ctrls, dtype=np.float32))
    ncon, nefc, _ = b.counts()
    out = dict(cf=b.contact_force().astype(np.float64), bc=b.body_contact().astype(np.float64), efc=b.efc_force().astype(np.float64) if diag else None,
               con=b.contacts().astype(np.float64) if diag else None, ncon=ncon, nefc=nefc, status=b.status(), kernel=b.last_kernel())
    b.close()
    return out


def compare_state(o, dev, k):
    """Env k of a device_readout against the oracle's CURRENT data (forward() done at that env's state).  Returns None when the row
    sets differ (counts, or a contact's geoms / dimension), else a dict of errors relative to max(1, max |efc_force|):
      decode_f / decode_w: the device's read-out against the reference decode of the DEVICE's own efc_force and contacts (friction and
                           row addresses from the oracle's contacts, xipos from the oracle) - needs the diagnostics
      parity_f / parity_w: against the reference decode of the oracle's efc_force and contacts."""
    nc, ne = int(dev["ncon"][k]), int(dev["nefc"][k])
    ocon = o.contacts()
    if (nc, ne) != (o.ncon, o.nefc):
        return None
    gb = o.info["geom_bodyid"]
    out = {}
    if dev["con"] is not None:
        dcon = []
        for i, c in enumerate(ocon):
            r = dev["con"][k, i]
            if (int(r[13]), int(r[14]), int(r[15])) != (c["dim"], c["geom1"], c["geom2"]):
                return None
            dcon.append(dict(pos=r[1:4], frame=r[4:13].reshape(3, 3), dim=c["dim"], geom1=c["geom1"], geom2=c["geom2"], efc_address=c["efc_address"], friction5=c["friction5"]))
        s = max(1.0, float(np.abs(dev["efc"][k, :ne]).max(initial=0.0)))
        f = contact_forces(dev["efc"][k, :ne], dcon)
        w = body_wrenches(f, dcon, gb, o.xipos, o.nbody)
        out["decode_f"] = float(np.abs(dev["cf"][k, :nc] - f).max(initial=0.0)) / s
        out["decode_w"] = float(np.abs(dev["bc"][k] - w).max()) / s
    s = max(1.0, float(np.abs(o.efc_force[:ne]).max(initial=0.0)))
    f, w, _ = oracle_readout(o)
    out["parity_f"] = float(np.abs(dev["cf"][k, :nc] - f).max(initial=0.0)) / s
    out["parity_w"] = float(np.abs(dev["bc"][k] - w).max()) / s
    out["beyond"] = float(np.abs(dev["cf"][k, nc:]).max(initial=0.0))  # rows beyond ncon: zeros
    return out


def compare(o, states, ctrls, dev):
    """compare_state over all states after the oracle's forward() at each: (dict of per-state error arrays over the states whose row
    sets agree, number of states whose row sets differ)"""
    from oracle_lib import load_state
    rows, differ = [], 0
    for k, (s, c) in enumerate(zip(states, ctrls)):
        load_state(o, s, np.asarray(c, dtype=np.float64))
        o.forward()
        r = compare_state(o, dev, k)
        if r is None:
            differ += 1
        else:
            rows.append(r)
    return {key: np.array([r[key] for r in rows]) for key in (rows[0] if rows else {})}, differ


# the models and states both the GPU tests and the report tool run: name -> (model, oracle, states, ctrls, tune knobs)
CASES = ("humanoid27_pgs", "humanoid27_newton", "humanoid27_pgs_unsized", "chain12_cd4", "chain12_cd6", "chain12_hfield", "team_robot")


def make_case(hb, name, tmp_path):
    import os
    from kernel_models import chain_xml, oracle_for, rollout_states
    from oracle_lib import GOLDEN, HUMANOID_HBM, TEAM_HBM, Oracle
    if name.startswith("humanoid27"):
        g = np.load(os.path.join(GOLDEN, "humanoid27_steps.npz"))
        st = np.concatenate([g["time"][:, None], g["qpos"], g["qvel"], g["warm"]], axis=1).astype(np.float32).astype(np.float64)
        m, o = hb.Model.load(HUMANOID_HBM), Oracle()
        if name == "humanoid27_newton":
            m.set_opt(solver=2, iterations=100)
            o.set_opt(solver=2, iterations=100)
        return m, o, st, g["ctrl"].astype(np.float32), (dict(sized=0) if name.endswith("unsized") else None)
    if name == "team_robot":
        p = TEAM_HBM
        o = Oracle(p)
        st, ct = team_states(o)
        return hb.Model.load(p), o, st, ct, None
    xml = {"chain12_cd4": chain_xml(12, condim=4), "chain12_cd6": chain_xml(12, condim=6), "chain12_hfield": chain_xml(12, floor="hfield")}[name]
    m, _, o = oracle_for(hb, xml, tmp_path, name + ".hbm")
    st, ct = rollout_states(o)
    return m, o, st, ct, None
