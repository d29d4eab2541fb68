"""fp64 reference of equality constraints (mj_instantiateEquality: scalar-joint couplings and connect anchors, and their unbounded force in
mj_solPGS / the primal solvers), in numpy over the oracle's forward() arrays.

TEST INFRASTRUCTURE, like fric_ref.py: the product package never imports it.

The oracle (oracle/mjstep_oracle.c) does not read the eq_* records: a model with equalities loads there as its unconstrained twin.  After
the oracle's forward pass this module builds the equality rows from the .hbm records (o.info) and the state - body poses from the
oracle's kinematics, point Jacobians from the joints' world axes and anchors, not from cdof - and puts them in FRONT of fric_ref.stacked's
problem: mj_makeConstraint's order, equality, friction loss, limits, contacts.  Every definition is MuJoCo's, from memory ([recall]):

    joint:    pos = (q1 - q1_0) - poly(q2 - q2_0), J = e_dof1 - poly'(q2 - q2_0) e_dof2; without joint2: pos = q1 - q1_0 - a0, J = e_dof1;
              diagApprox = dof_invweight0[dof1] (+ dof_invweight0[dof2])
    connect:  three rows, world x / y / z: pos = p1 - p2, p_k = xpos[b_k] + xmat[b_k] anchor_k, J = jacp(b1, p1) - jacp(b2, p2);
              diagApprox = body_invweight0[b1][0] + body_invweight0[b2][0]
    each row: margin 0, imp = impedance(solimp, pos) of the row's own pos, R = max(MINVAL, (1 - imp) / imp diagApprox),
              aref = -B (J qvel) - K imp pos (K, B of solref, with the 2 timestep floor unless mjDSBL_REFSAFE), -inf < f < inf:
              the dual does not project the row, the primal has it quadratic wherever jar is, f = -D jar
"""
import numpy as np

import fric_ref
from fric_ref import DSBL_CONSTRAINT, DSBL_REFSAFE, MAXIMP, MINIMP, MINVAL, euler, solve_pgs  # noqa: F401  (the solves that need no change)
from oracle_lib import load_state

DSBL_EQUALITY = 1 << 1
EQ_CONNECT, EQ_JOINT = 0, 2
NEQDATA = 11
CNSTR_EQUALITY = 0  # (mjCNSTR_EQUALITY: the type this module gives its rows in front of fric_ref's types)


def impedance(solimp, pos):
    """mj_makeImpedance's getimpedance at margin 0, clipped to [MINIMP, MAXIMP]"""
    d0, d1 = np.clip(solimp[0], MINIMP, MAXIMP), np.clip(solimp[1], MINIMP, MAXIMP)
    width, mid, power = max(0.0, solimp[2]), np.clip(solimp[3], MINIMP, MAXIMP), max(1.0, solimp[4])
    if d0 == d1 or width <= MINVAL:
        return float(np.clip(0.5 * (d0 + d1), MINIMP, MAXIMP))
    x = abs(pos) / width
    if x >= 1:
        y = 1.0
    elif x <= 0:
        y = 0.0
    elif x <= mid:
        y = x ** power / mid ** (power - 1)
    else:
        y = 1 - (1 - x) ** power / (1 - mid) ** (power - 1)
    return float(np.clip(d0 + y * (d1 - d0), MINIMP, MAXIMP))


def kb(solref, solimp, h, refsafe):
    dmax = np.clip(solimp[1], MINIMP, MAXIMP)
    if solref[0] > 0:
        tc = max(solref[0], 2 * h) if refsafe else solref[0]
        return 1 / max(MINVAL, dmax * dmax * tc * tc * solref[1] * solref[1]), 2 / max(MINVAL, dmax * tc)
    return -solref[0] / max(MINVAL, dmax * dmax), -solref[1] / max(MINVAL, dmax)


def point_jacobian(o, body, point):
    """jacp [3, nv] of `point` (world) moving with `body`, from the world axes and anchors of the joints between the body and the world"""
    info, nv = o.info, o.nv
    J = np.zeros((3, nv))
    xanchor, xaxis, xmat, xpos = o.xanchor.reshape(-1, 3), o.xaxis.reshape(-1, 3), o.xmat.reshape(-1, 3, 3), o.xpos.reshape(-1, 3)
    b = int(body)
    while b > 0:
        for j in range(int(info["body_jntadr"][b]), int(info["body_jntadr"][b]) + int(info["body_jntnum"][b])):
            t, da = int(info["jnt_type"][j]), int(info["jnt_dofadr"][j])
            if t == 0:  # free: world translations, then rotations about the body's own axes through its origin
                J[:, da:da + 3] = np.eye(3)
                for i in range(3):
                    J[:, da + 3 + i] = np.cross(xmat[b][:, i], point - xpos[b])
            elif t == 2:
                J[:, da] = xaxis[j]
            elif t == 3:
                J[:, da] = np.cross(xaxis[j], point - xanchor[j])
            else:
                raise ValueError("ball joints are not in the engine")
        b = int(info["body_parentid"][b])
    return J


def equality_pos(o):
    """(pos [ne], per-row element index) of the active equality rows at the oracle's current kinematics (forward() or kinematics done)"""
    return _rows(o, jac=False)


def _rows(o, jac=True, drop=False):
    info, nv = o.info, o.nv
    types = np.asarray(info.get("eq_type", []), dtype=np.int64)
    flags = o.opt("disableflags")
    out = dict(J=[], pos=[], elem=[], da=[])
    if drop or (flags & (DSBL_CONSTRAINT | DSBL_EQUALITY)):
        types = types[:0]
    data = np.asarray(info.get("eq_data", []), dtype=np.float64).reshape(-1, NEQDATA)
    xpos, xmat = o.xpos.reshape(-1, 3), o.xmat.reshape(-1, 3, 3)
    for e, t in enumerate(types):
        if not info["eq_active0"][e]:
            continue
        o1, o2 = int(info["eq_obj1id"][e]), int(info["eq_obj2id"][e])
        if t == EQ_JOINT:
            q1, d1 = int(info["jnt_qposadr"][o1]), int(info["jnt_dofadr"][o1])
            a = data[e, :5]
            J = np.zeros(nv)
            J[d1] = 1.0
            da = info["dof_invweight0"][d1]
            if o2 >= 0:
                q2, d2 = int(info["jnt_qposadr"][o2]), int(info["jnt_dofadr"][o2])
                x = o.qpos[q2] - info["qpos0"][q2]
                pos = (o.qpos[q1] - info["qpos0"][q1]) - (a[0] + a[1] * x + a[2] * x ** 2 + a[3] * x ** 3 + a[4] * x ** 4)
                J[d2] -= a[1] + 2 * a[2] * x + 3 * a[3] * x ** 2 + 4 * a[4] * x ** 3
                da = da + info["dof_invweight0"][d2]
            else:
                pos = o.qpos[q1] - info["qpos0"][q1] - a[0]
            out["J"].append(J); out["pos"].append(pos); out["elem"].append(e); out["da"].append(da)
        elif t == EQ_CONNECT:
            p1, p2 = xpos[o1] + xmat[o1] @ data[e, 0:3], xpos[o2] + xmat[o2] @ data[e, 3:6]
            Jc = point_jacobian(o, o1, p1) - point_jacobian(o, o2, p2) if jac else np.zeros((3, nv))
            da = info["body_invweight0"][2 * o1] + info["body_invweight0"][2 * o2]
            for k in range(3):
                out["J"].append(Jc[k]); out["pos"].append(p1[k] - p2[k]); out["elem"].append(e); out["da"].append(da)
        else:
            raise ValueError("equality type %d" % t)
    if not jac:
        return np.array(out["pos"]), np.array(out["elem"], dtype=np.int64)
    return out


def equality_rows(o, drop=False):
    """The model's active equality rows at the oracle's current forward() state: dict of J [ne, nv], pos, R, aref, imp, elem.  drop: none."""
    info, nv = o.info, o.nv
    r = _rows(o, True, drop)
    ne = len(r["pos"])
    J = np.array(r["J"]).reshape(ne, nv)
    pos = np.array(r["pos"], dtype=np.float64)
    h, refsafe = o.opt("timestep"), not (o.opt("disableflags") & DSBL_REFSAFE)
    R, aref, imps = np.zeros(ne), np.zeros(ne), np.zeros(ne)
    for i in range(ne):
        e = r["elem"][i]
        sr, si = np.asarray(info["eq_solref"][2 * e:2 * e + 2]), np.asarray(info["eq_solimp"][5 * e:5 * e + 5])
        imp = impedance(si, pos[i])
        K, B = kb(sr, si, h, refsafe)
        R[i] = max(MINVAL, (1 - imp) / imp * r["da"][i])
        aref[i] = -B * (J[i] @ o.qvel) - K * imp * pos[i]
        imps[i] = imp
    return dict(J=J, pos=pos, R=R, aref=aref, imp=imps, elem=np.array(r["elem"], dtype=np.int64))


def stacked(o, drop=False, drop_eq=False):
    """fric_ref.stacked's problem with the equality rows in front: J, R, aref, lo, hi (+-inf on an equality row), ne, nf, ..., contacts
    (efc_address shifted by ne + nf)"""
    p = fric_ref.stacked(o, drop)
    eq = equality_rows(o, drop_eq)
    ne = len(eq["pos"])
    if ne == 0:
        p["ne"] = 0
        return p
    p["J"] = np.vstack([eq["J"], p["J"]])
    p["R"] = np.concatenate([eq["R"], p["R"]])
    p["aref"] = np.concatenate([eq["aref"], p["aref"]])
    p["lo"] = np.concatenate([np.full(ne, -np.inf), p["lo"]])
    p["hi"] = np.concatenate([np.full(ne, np.inf), p["hi"]])
    p["types"] = np.concatenate([np.full(ne, CNSTR_EQUALITY, dtype=np.int64), p["types"]])
    for c in p["contacts"]:
        if c["efc_address"] >= 0:
            c["efc_address"] += ne
    p["ne"] = ne
    p["eq_pos"] = eq["pos"]
    return p


def primal_force(p, jar):
    """fric_ref.primal_force with the row kind taken from both bounds: (-inf, inf) always quadratic, [0, inf) active below zero"""
    R, lo, hi = p["R"], p["lo"], p["hi"]
    f = np.clip(-jar / R, lo, hi)
    quad = (f > lo) & (f < hi) if len(R) else np.zeros(0, dtype=bool)
    quad = np.where(np.isinf(hi) & np.isfinite(lo), jar < 0, quad)
    cost = np.where(quad, 0.5 * jar * jar / R, -f * jar - 0.5 * R * f * f)
    return f, quad, float(cost.sum())


def solve_newton(o, p, warm=None, maxiter=200):
    """fric_ref.solve_newton over this module's primal_force: exact Newton on the active set with an exact line search, run until the
    gradient stops shrinking.  Returns dict force, qacc, residual, quad."""
    J, R, M, qs = p["J"], p["R"], p["M"], p["qs"]
    n = len(R)
    a = qs.copy()
    if n == 0:
        return dict(force=np.zeros(0), qacc=a, residual=0.0, quad=np.zeros(0, dtype=bool))
    thr = []  # per row: the jar values at which its zone changes
    for i in range(n):
        lo, hi = p["lo"][i], p["hi"][i]
        thr.append(() if np.isinf(lo) and np.isinf(hi) else (-R[i] * hi, -R[i] * lo) if np.isfinite(hi) else (0.0,))
    best, stall = None, 0
    for _ in range(maxiter):
        jar = J @ a - p["aref"]
        f, quad, _ = primal_force(p, jar)
        grad = M @ (a - qs) - J.T @ f
        g = np.abs(grad).max()
        if best is None or g < best[0]:
            best, stall = (g, a.copy(), f.copy(), quad.copy()), 0
        else:
            stall += 1
        if g <= 1e-14 * max(1.0, float(np.abs(p["qfs"]).max())) or stall >= 3:
            break
        H = M + (J[quad].T * (1.0 / R[quad])) @ J[quad]
        s = -np.linalg.solve(H, grad)
        Jv, Ms = J @ s, M @ s
        d0, d1 = s @ (M @ (a - qs)), s @ Ms
        bps = np.array(sorted({(t - jar[i]) / Jv[i] for i in range(n) if Jv[i] != 0.0 for t in thr[i] if (t - jar[i]) / Jv[i] > 0}))
        lo_a, lo_d = 0.0, d0 - primal_force(p, jar)[0] @ Jv
        if lo_d >= 0:
            break
        alpha = None
        if len(bps):
            F = np.clip(-(jar[None, :] + bps[:, None] * Jv[None, :]) / R[None, :], p["lo"][None, :], p["hi"][None, :])
            ds = d0 + bps * d1 - F @ Jv
            up = np.flatnonzero(ds >= 0)
            k = int(up[0]) if len(up) else len(bps)
            if k > 0:
                lo_a, lo_d = float(bps[k - 1]), float(ds[k - 1])
            if k < len(bps):
                bp, d = float(bps[k]), float(ds[k])
                alpha = lo_a + (bp - lo_a) * (-lo_d) / (d - lo_d) if d > lo_d else bp
        if alpha is None:  # beyond the last breakpoint the derivative is linear with slope phi''
            _, qd, _ = primal_force(p, jar + (lo_a + 1.0) * Jv)
            alpha = lo_a - lo_d / (d1 + ((Jv[qd] ** 2) / R[qd]).sum())
        a = a + alpha * s
    g, a, f, quad = best
    return dict(force=f, qacc=a, residual=float(g), quad=quad)


def solve(o, p, warm):
    return solve_newton(o, p, warm) if o.opt("solver") == 2 else solve_pgs(o, p, warm)


def forward(o, state, ctrl, drop=False, drop_eq=False):
    """The oracle's forward pass at the record `state` under `ctrl`, then the stacked solve.  Returns (problem, solution)."""
    load_state(o, np.asarray(state, dtype=np.float64), np.asarray(ctrl, dtype=np.float64))
    o.forward()
    p = stacked(o, drop, drop_eq)
    return p, solve(o, p, o.qacc_warmstart.copy())


def step(o, state, ctrl, drop=False, drop_eq=False):
    """One mj_step (Euler) of the model with its equalities.  Returns (record after the step, problem, solution)."""
    p, sol = forward(o, state, ctrl, drop, drop_eq)
    return euler(o, p, sol), p, sol


def record(o):
    return np.concatenate([[o.time], o.qpos, o.qvel, o.qacc_warmstart])


def rollout_states(o, steps=300, every=10, seed=0):
    """fric_ref.rollout_states over this module's step: states every `every` steps under the same control schedule, rounded to fp32, and
    the controls of the step that follows each"""
    rng = np.random.default_rng(seed)
    o.reset()
    s = record(o)
    states, ctrls = [], []
    c = np.zeros(o.nu)
    for t in range(steps):
        if t % 25 == 0:
            c = rng.uniform(-1, 1, o.nu)
        if t % every == every - 1:
            states.append(s.copy())
            ctrls.append(c.copy())
        s, _, _ = step(o, s, c)
    return np.array(states).astype(np.float32).astype(np.float64), np.array(ctrls, dtype=np.float32)


def steps_ref(o, states, ctrls):
    """one reference step from each state: per-state qpos, qvel after the step; qacc, efc_force, contacts (efc_address shifted), counts,
    row types, sweep counts, residuals; zones: friction rows at +bound, at -bound, inside"""
    out = dict(qpos=[], qvel=[], qacc=[], force=[], ncon=[], nefc=[], ne=[], nf=[], con=[], types=[], niter=[], reverts=0, residual=[],
               zones=np.zeros(3, dtype=np.int64), xipos=[], qfs=[])
    nq, nv = o.nq, o.nv
    for s, c in zip(states, ctrls):
        rec, p, sol = step(o, s, c.astype(np.float64))
        out["qpos"].append(rec[1:1 + nq]); out["qvel"].append(rec[1 + nq:1 + nq + nv]); out["qacc"].append(sol["qacc"]); out["force"].append(sol["force"])
        out["ncon"].append(p["ncon"]); out["nefc"].append(len(p["R"])); out["ne"].append(p["ne"]); out["nf"].append(p["nf"])
        out["con"].append(p["contacts"]); out["types"].append(p["types"])
        out["niter"].append(sol.get("niter", -1)); out["reverts"] += sol.get("reverts", 0); out["residual"].append(sol.get("residual", 0.0))
        out["xipos"].append(o.xipos.copy()); out["qfs"].append(float(np.abs(p["qfs"]).max()))
        ff, fl = sol["force"][p["ne"]:p["ne"] + p["nf"]], p["fl"]
        out["zones"] += np.array([(ff >= fl).sum(), (ff <= -fl).sum(), (np.abs(ff) < fl).sum()])
    return out


def inverse_ref(o, qacc, discrete=False):
    """fric_ref.inverse_ref with the equality rows' force f = -D (J qacc - aref): the terms of qfrc_inverse at the oracle's current state"""
    t = fric_ref.inverse_ref(o, qacc, discrete)
    eq = equality_rows(o)
    qa = np.asarray(qacc, dtype=np.float64)
    if discrete:
        damping = o.marr("dof_damping")
        if not (o.opt("disableflags") & fric_ref.DSBL_EULERDAMP) and (damping > 0).any():
            qa = qa + np.linalg.solve(o.dense_M(), o.opt("timestep") * damping * qa)
    if len(eq["pos"]):
        f = -(eq["J"] @ qa - eq["aref"]) / eq["R"]
        t["constraint"] = t["constraint"] + eq["J"].T @ f
        t["active"] += len(f)
    return t


def anchor_gaps(o, qpos):
    """|p1 - p2| of every active connect (one value per connect) at `qpos`"""
    o.reset()
    o.qpos[:] = qpos
    o.forward()
    pos, elem = equality_pos(o)
    types = np.asarray(o.info["eq_type"])
    return np.array([np.linalg.norm(pos[elem == e]) for e in sorted(set(elem.tolist())) if types[e] == EQ_CONNECT])
