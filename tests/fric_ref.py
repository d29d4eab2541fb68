"""fp64 reference of joint friction loss (mj_instantiateFriction and the two-sided force bound in mj_solPGS / the primal solvers), in
numpy over the oracle's forward() arrays.

TEST INFRASTRUCTURE, like inverse_ref.py: the product package never imports it.

The oracle (oracle/mjstep_oracle.c) does not read dof_frictionloss: a friction model loads there as its frictionless twin.  After the
oracle's forward pass this module takes efc_J, efc_R, efc_aref, qacc_smooth, qfrc_smooth, the dense mass matrix, the contacts and the
row types, puts the friction rows (constants from parse_hbm, restated here) in FRONT - mj_makeConstraint's order without equality rows:
friction loss, limits, contacts - and solves the stacked problem:

    row i of dof d with fl = dof_frictionloss[d] > 0:  J = e_d, pos = margin = 0, diagApprox = dof_invweight0[d],
    imp = impedance(solimp, 0, 0), R = max(MINVAL, (1 - imp) / imp diagApprox), D = 1 / R, aref = -B qvel[d] (B of solref), -fl <= f <= fl
    dual (PGS):    f <- clip(f - res / AR_ii, -fl, fl); warm start clip(-D jar, -fl, fl), kept if its cost is <= 0
    primal:        jar <= -R fl: f = +fl, cost fl (-R fl / 2 - jar);  jar >= R fl: f = -fl, cost fl (-R fl / 2 + jar);  else f = -D jar, cost D jar^2 / 2
"""
import numpy as np

from oracle_lib import load_state
from rk4_ref import integrate_pos

MINVAL, MINIMP, MAXIMP = 1e-15, 0.0001, 0.9999
DSBL_CONSTRAINT, DSBL_FRICTIONLOSS, DSBL_WARMSTART, DSBL_REFSAFE, DSBL_EULERDAMP = 1 << 0, 1 << 2, 1 << 8, 1 << 11, 1 << 14
DEF_SOLREF, DEF_SOLIMP = (0.02, 1.0), (0.9, 0.95, 0.001, 0.5, 2.0)
CNSTR_FRICTION_DOF = 1  # (mjCNSTR_FRICTION_DOF, mjmodel.h: the type this module gives its rows in front of the oracle's types)


def friction_rows(o, drop=False):
    """The model's friction rows from its .hbm records (o.info) and the oracle's options: dict of dof [nf], fl, R, B.  drop: none."""
    info = o.info
    nv = o.nv
    fl_all = np.asarray(info.get("dof_frictionloss", np.zeros(nv)), dtype=np.float64)
    flags = o.opt("disableflags")
    dof = [d for d in range(nv) if fl_all[d] > 0]
    if drop or (flags & (DSBL_CONSTRAINT | DSBL_FRICTIONLOSS)):
        dof = []
    sr = np.asarray(info.get("dof_solref_friction", np.tile(DEF_SOLREF, nv)), dtype=np.float64).reshape(nv, 2)
    si = np.asarray(info.get("dof_solimp_friction", np.tile(DEF_SOLIMP, nv)), dtype=np.float64).reshape(nv, 5)
    h = o.opt("timestep")
    R, B = [], []
    for d in dof:
        d0, d1 = np.clip(si[d, 0], MINIMP, MAXIMP), np.clip(si[d, 1], MINIMP, MAXIMP)
        imp = 0.5 * (d0 + d1) if (d0 == d1 or max(0.0, si[d, 2]) <= MINVAL) else d0  # impedance(solimp, 0, 0)
        R.append(max(MINVAL, (1 - imp) / imp * info["dof_invweight0"][d]))
        if sr[d, 0] > 0:
            tc = sr[d, 0] if (flags & DSBL_REFSAFE) else max(sr[d, 0], 2 * h)
            B.append(2 / max(MINVAL, d1 * tc))
        else:
            B.append(-sr[d, 1] / max(MINVAL, d1))
    return dict(dof=np.array(dof, dtype=np.int64), fl=fl_all[dof] if dof else np.zeros(0), R=np.array(R), B=np.array(B))


def stacked(o, drop=False):
    """The stacked problem at the oracle's current forward() state: friction rows, then the oracle's rows.  Dict of J [n, nv], R, aref,
    lo, hi (force bounds), nf, M, qacc_smooth, qfrc_smooth, types, contacts (efc_address shifted by nf)."""
    nv, ne = o.nv, o.nefc
    fr = friction_rows(o, drop)
    nf = len(fr["dof"])
    Jf = np.zeros((nf, nv))
    Jf[np.arange(nf), fr["dof"]] = 1.0
    J = np.vstack([Jf, o.efc_J[:ne * nv].reshape(ne, nv)])
    R = np.concatenate([fr["R"], o.efc_R[:ne]])
    aref = np.concatenate([-fr["B"] * o.qvel[fr["dof"]] if nf else np.zeros(0), o.efc_aref[:ne]])
    lo = np.concatenate([-fr["fl"], np.zeros(ne)])
    hi = np.concatenate([fr["fl"], np.full(ne, np.inf)])
    con = o.contacts()
    for c in con:
        if c["efc_address"] >= 0:
            c["efc_address"] += nf
    types = np.concatenate([np.full(nf, CNSTR_FRICTION_DOF, dtype=np.int64), o.efc_types()[0]]) if ne else np.full(nf, CNSTR_FRICTION_DOF, dtype=np.int64)
    return dict(J=J, R=R, aref=aref, lo=lo, hi=hi, nf=nf, fl=fr["fl"], M=o.dense_M(), qs=o.qacc_smooth.copy(), qfs=o.qfrc_smooth.copy(),
                types=types, contacts=con, ncon=o.ncon)


def solve_pgs(o, p, warm):
    """mj_solPGS as the oracle restates it (fwd_constraint), with the two-sided clamp.  Returns dict force, qacc, niter, reverts."""
    J, R, lo, hi = p["J"], p["R"], p["lo"], p["hi"]
    n, nv = len(R), o.nv
    if n == 0:
        return dict(force=np.zeros(0), qacc=p["qs"].copy(), niter=0, reverts=0)
    MinvJt = np.linalg.solve(p["M"], J.T)
    AR = J @ MinvJt + np.diag(R)
    b = J @ p["qs"] - p["aref"]
    f = np.zeros(n)
    if not (o.opt("disableflags") & DSBL_WARMSTART):
        jar = J @ np.asarray(warm, dtype=np.float64) - p["aref"]
        f = np.clip(-jar / R, lo, hi)
        if f @ (0.5 * (AR @ f) + b) > 0:
            f = np.zeros(n)
    scale = 1.0 / (o.info["meaninertia"] * max(1, nv))
    tol, maxiter = o.opt("tolerance"), o.opt("iterations")
    it = reverts = 0
    while it < maxiter:
        improvement = 0.0
        for i in range(n):
            res = b[i] + AR[i] @ f
            old = f[i]
            new = min(max(old - res / AR[i, i], lo[i]), hi[i])
            delta = new - old
            change = 0.5 * delta * delta * AR[i, i] + delta * res
            if change > 1e-10:
                new, change = old, 0.0
                reverts += 1
            f[i] = new
            improvement -= change
        it += 1
        if improvement * scale < tol:
            break
    return dict(force=f, qacc=p["qs"] + MinvJt @ f, niter=it, reverts=reverts)


def primal_force(p, jar):
    """(force, rows in the quadratic zone, cost) of the stacked rows at jar"""
    R, lo, hi = p["R"], p["lo"], p["hi"]
    f = np.clip(-jar / R, lo, hi)
    quad = (f > lo) & (f < hi) if len(R) else np.zeros(0, dtype=bool)
    quad = np.where(np.isinf(hi), jar < 0, quad)  # (a unilateral row: active below zero)
    # cost: quadratic zone D jar^2 / 2; at a bound b the linear continuation  -b jar - R b^2 / 2  (b = fl: fl (-R fl / 2 - jar); b = -fl: fl (-R fl / 2 + jar); b = 0: 0)
    cost = np.where(quad, 0.5 * jar * jar / R, -f * jar - 0.5 * R * f * f)
    return f, quad, float(cost.sum())


def solve_newton(o, p, warm=None, maxiter=200):
    """The primal problem  min_a 1/2 (a - a_s)' M (a - a_s) + sum_rows s_i(J_i a - aref_i)  by Newton steps on the active set with an EXACT
    line search (the derivative along the search direction is piecewise linear: walked breakpoint by breakpoint), run until the gradient
    M (a - a_s) - J' f(a) stops shrinking.  Iteration counts are no part of the contract.  Returns dict force, qacc, residual, quad."""
    J, R, M, qs = p["J"], p["R"], p["M"], p["qs"]
    n = len(R)
    a = qs.copy()
    if n == 0:
        return dict(force=np.zeros(0), qacc=a, residual=0.0, quad=np.zeros(0, dtype=bool))
    thr = []  # per row: the jar values at which its zone changes
    for i in range(n):
        thr.append((-R[i] * p["hi"][i], -R[i] * p["lo"][i]) if np.isfinite(p["hi"][i]) else (0.0,))
    best = None
    for _ in range(maxiter):
        jar = J @ a - p["aref"]
        f, quad, _ = primal_force(p, jar)
        grad = M @ (a - qs) - J.T @ f
        g = np.abs(grad).max()
        if best is None or g < best[0]:
            best, stall = (g, a.copy(), f.copy(), quad.copy()), 0
        else:
            stall += 1
        if g <= 1e-14 * max(1.0, float(np.abs(p["qfs"]).max())) or stall >= 3:  # (at fp64 rounding of its own terms, or no longer shrinking)
            break
        H = M + (J[quad].T * (1.0 / R[quad])) @ J[quad]
        s = -np.linalg.solve(H, grad)
        Jv, Ms = J @ s, M @ s
        # phi'(alpha) = s'M(a - qs) + alpha s'Ms - sum_i f_i(jar_i + alpha Jv_i) Jv_i: increasing and piecewise linear in alpha
        d_gauss0, d_gauss1 = s @ (M @ (a - qs)), s @ Ms

        def dphi(al):
            ff, _, _ = primal_force(p, jar + al * Jv)
            return d_gauss0 + al * d_gauss1 - ff @ Jv
        bps = np.array(sorted({(t - jar[i]) / Jv[i] for i in range(n) if Jv[i] != 0.0 for t in thr[i] if (t - jar[i]) / Jv[i] > 0}))
        lo_a, lo_d = 0.0, dphi(0.0)
        if lo_d >= 0:
            break
        alpha = None
        if len(bps):  # the derivative at every breakpoint at once: the first one at which it is no longer negative ends the walk
            F = np.clip(-(jar[None, :] + bps[:, None] * Jv[None, :]) / R[None, :], p["lo"][None, :], p["hi"][None, :])
            ds = d_gauss0 + bps * d_gauss1 - F @ Jv
            up = np.flatnonzero(ds >= 0)
            k = int(up[0]) if len(up) else len(bps)
            if k > 0:
                lo_a, lo_d = float(bps[k - 1]), float(ds[k - 1])
            if k < len(bps):
                bp, d = float(bps[k]), float(ds[k])
                alpha = lo_a + (bp - lo_a) * (-lo_d) / (d - lo_d) if d > lo_d else bp
        if alpha is None:  # beyond the last breakpoint the derivative is linear with slope phi''
            ff, qd, _ = primal_force(p, jar + (lo_a + 1.0) * Jv)
            curv = d_gauss1 + ((Jv[qd] ** 2) / R[qd]).sum()
            alpha = lo_a - lo_d / curv
        a = a + alpha * s
    g, a, f, quad = best
    return dict(force=f, qacc=a, residual=float(g), quad=quad)


def solve(o, p, warm):
    return solve_newton(o, p, warm) if o.opt("solver") == 2 else solve_pgs(o, p, warm)


def forward(o, state, ctrl, drop=False):
    """The oracle's forward pass at the record `state` under `ctrl`, then the stacked solve.  Returns (problem, solution)."""
    load_state(o, np.asarray(state, dtype=np.float64), np.asarray(ctrl, dtype=np.float64))
    o.forward()
    p = stacked(o, drop)
    return p, solve(o, p, o.qacc_warmstart.copy())


def euler(o, p, sol):
    """mj_Euler with implicit joint damping from the solution: (M + h diag(damping))^-1 (qfrc_smooth + J' f), mj_advance, warm start = qacc.
    Returns the record [time, qpos, qvel, qacc_warmstart] after the step."""
    h = o.opt("timestep")
    damping = o.marr("dof_damping")
    qfrc = p["qfs"] + (p["J"].T @ sol["force"] if len(sol["force"]) else 0.0)
    if not (o.opt("disableflags") & DSBL_EULERDAMP) and (damping > 0).any():
        qa = np.linalg.solve(p["M"] + h * np.diag(damping), qfrc)
    else:
        qa = sol["qacc"].copy()
    qvel = o.qvel + h * qa
    qpos = integrate_pos(o, o.qpos.copy(), qvel, h)
    return np.concatenate([[o.time + h], qpos, qvel, sol["qacc"]])


def step(o, state, ctrl, drop=False):
    """One mj_step of the friction model.  Returns (record after the step, problem, solution)."""
    p, sol = forward(o, state, ctrl, drop)
    return euler(o, p, sol), p, sol


def rollout_states(o, steps=300, every=10, seed=0):
    """kernel_models.rollout_states over this module's step: states every `every` steps under the same control schedule, rounded to fp32,
    and the controls of the step that follows each"""
    rng = np.random.default_rng(seed)
    o.reset()
    s = np.concatenate([[o.time], o.qpos, o.qvel, o.qacc_warmstart])
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
    """one reference step from each state (kernel_models.oracle_steps for a friction model): per-state qpos, qvel after the step; qacc,
    efc_force, contacts, counts, row types, sweep counts, reverts, residuals, zone counts of the friction rows of the step"""
    out = dict(qpos=[], qvel=[], qacc=[], force=[], ncon=[], nefc=[], nf=[], con=[], types=[], niter=[], reverts=0, residual=[], zones=np.zeros(3, dtype=np.int64),
               xipos=[], qfs=[])
    for s, c in zip(states, ctrls):
        rec, p, sol = step(o, s, c.astype(np.float64))
        nq, nv = o.nq, o.nv
        out["qpos"].append(rec[1:1 + nq]); out["qvel"].append(rec[1 + nq:1 + nq + nv]); out["qacc"].append(sol["qacc"]); out["force"].append(sol["force"])
        out["ncon"].append(p["ncon"]); out["nefc"].append(len(p["R"])); out["nf"].append(p["nf"]); out["con"].append(p["contacts"]); out["types"].append(p["types"])
        out["niter"].append(sol.get("niter", -1)); out["reverts"] += sol.get("reverts", 0); out["residual"].append(sol.get("residual", 0.0))
        out["xipos"].append(o.xipos.copy()); out["qfs"].append(float(np.abs(p["qfs"]).max()))
        ff, fl = sol["force"][:p["nf"]], p["fl"]
        out["zones"] += np.array([(ff >= fl).sum(), (ff <= -fl).sum(), (np.abs(ff) < fl).sum()])
    return out


def inverse_ref(o, qacc, discrete=False):
    """inverse_ref.inverse_terms with the friction rows' force: the terms of qfrc_inverse at the oracle's current forward() state"""
    from inverse_ref import inverse_terms
    t = inverse_terms(o, qacc, discrete)
    fr = friction_rows(o)
    qa = np.asarray(qacc, dtype=np.float64)
    if discrete:
        damping = o.marr("dof_damping")
        if not (o.opt("disableflags") & DSBL_EULERDAMP) and (damping > 0).any():
            qa = qa + np.linalg.solve(o.dense_M(), o.opt("timestep") * damping * qa)
    if len(fr["dof"]):
        jar = qa[fr["dof"]] + fr["B"] * o.qvel[fr["dof"]]
        f = np.clip(-jar / fr["R"], -fr["fl"], fr["fl"])
        t["constraint"] = t["constraint"].copy()
        np.add.at(t["constraint"], fr["dof"], f)
        t["active"] += len(f)
    return t
