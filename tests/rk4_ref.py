"""fp64 reference of the RK4 step (mj_RungeKutta with N = 4) on top of the oracle's mj_forward (oracle/mjstep_oracle.c: om_forward).

TEST INFRASTRUCTURE: the product package never imports this module, and the oracle itself is not touched - the recurrence is restated
here in numpy over Oracle.forward():

    stage i = 0..3:  F_i = qacc of mj_forward at (Q_i, V_i)      (collision, constraint rows, solver: everything, every stage)
                     Q_0 = q0, V_0 = v0;  Q_i = integratePos(q0, V_{i-1}, a_i h),  V_i = v0 + a_i h F_{i-1},  a = (1/2, 1/2, 1)
    end:             qvel' = v0 + h (F_0 + 2 F_1 + 2 F_2 + F_3) / 6
                     qpos' = integratePos(q0, (V_0 + 2 V_1 + 2 V_2 + V_3) / 6, h)
                     time' = time + h,  qacc_warmstart' = F_3

ctrl and the step's incoming qacc_warmstart are held for all four stages; no implicit joint damping (that is mj_Euler's).
"""
import numpy as np

from oracle_lib import load_state

A = (0.5, 0.5, 1.0)
B = (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)
JNT_FREE = 0


def quat_mul(a, b):
    return np.array([a[0]*b[0]-a[1]*b[1]-a[2]*b[2]-a[3]*b[3], a[0]*b[1]+a[1]*b[0]+a[2]*b[3]-a[3]*b[2],
                     a[0]*b[2]-a[1]*b[3]+a[2]*b[0]+a[3]*b[1], a[0]*b[3]+a[1]*b[2]-a[2]*b[1]+a[3]*b[0]])


def integrate_pos(o, qpos, vel, h):
    """mj_integratePos for free, hinge and slide joints: qpos advanced along vel for the time h, the free joint's quaternion through
    the tangent space (normalise, then multiply by the rotation h |w| about w / |w|), as mj_advance does"""
    q = np.array(qpos, dtype=np.float64)
    jt, qa, da = o.info["jnt_type"], o.info["jnt_qposadr"], o.info["jnt_dofadr"]
    for j in range(o.njnt):
        if jt[j] == JNT_FREE:
            q[qa[j]:qa[j] + 3] += h * vel[da[j]:da[j] + 3]
            w = vel[da[j] + 3:da[j] + 6]
            n = np.linalg.norm(w)
            quat = q[qa[j] + 3:qa[j] + 7] / np.linalg.norm(q[qa[j] + 3:qa[j] + 7])
            if n > 1e-15:
                rot = np.concatenate([[np.cos(0.5 * h * n)], np.sin(0.5 * h * n) * w / n])
            else:
                rot = np.array([1.0, 0.0, 0.0, 0.0])
            q[qa[j] + 3:qa[j] + 7] = quat_mul(quat, rot)
        else:
            q[qa[j]] += h * vel[da[j]]
    return q


def rk4_step(o, state, ctrl, h=None, want_stages=False):
    """One RK4 step of the [time, qpos, qvel, qacc_warmstart] record `state` under `ctrl` (xfrc_applied zero).  Returns a dict: the
    record after the step (`state`), qpos / qvel / warm of it, `counts` = per stage (ncon, nefc, solver_niter), and what the LAST
    forward pass left: qacc, efc_force, contacts, types (the oracle itself is left in that state).  want_stages: also per-stage qacc."""
    nq, nv = o.nq, o.nv
    h = o.opt("timestep") if h is None else h
    state = np.asarray(state, dtype=np.float64)
    ctrl = np.asarray(ctrl, dtype=np.float64)
    q0, v0, warm = state[1:1 + nq].copy(), state[1 + nq:1 + nq + nv].copy(), state[1 + nq + nv:1 + nq + 2 * nv].copy()
    Q, V, F, counts = [q0], [v0], [], []
    for i in range(4):
        load_state(o, np.concatenate([[state[0]], Q[i], V[i], warm]), ctrl)
        o.forward()
        F.append(o.qacc.copy())
        counts.append((o.ncon, o.nefc, o.dint("solver_niter")))
        if i < 3:
            Q.append(integrate_pos(o, q0, V[i], A[i] * h))
            V.append(v0 + A[i] * h * F[i])
    dv = sum(b * f for b, f in zip(B, F))
    dq = sum(b * v for b, v in zip(B, V))
    qpos, qvel = integrate_pos(o, q0, dq, h), v0 + h * dv
    out = dict(qpos=qpos, qvel=qvel, warm=F[3].copy(), time=state[0] + h, counts=counts, qacc=F[3].copy(),
               efc_force=o.efc_force[:o.nefc].copy(), contacts=o.contacts(), types=o.efc_types()[0],
               state=np.concatenate([[state[0] + h], qpos, qvel, F[3]]))
    if want_stages:
        out["F"] = F
    return out


def euler_step(o, state, ctrl):
    """the oracle's own (Euler) step from the same kind of record"""
    load_state(o, np.asarray(state, dtype=np.float64), np.asarray(ctrl, dtype=np.float64))
    o.step()
    return np.concatenate([[o.time], o.qpos, o.qvel, o.qacc_warmstart])


def trajectory(o, state, ctrl, h, n, kind="rk4"):
    """n steps of size h under constant ctrl; returns the list of records after each step.  Sets the oracle's timestep to h."""
    o.set_opt(timestep=h)
    s, out = np.asarray(state, dtype=np.float64), []
    for _ in range(n):
        s = rk4_step(o, s, ctrl, h)["state"] if kind == "rk4" else euler_step(o, s, ctrl)
        out.append(s)
    return out


def convergence_case(o, env, horizon=0.04, fine=256):
    """The start record of env `env` (om_init_env: what Batch.reset(perturb=True) gives that env; zero warm start), the held control
    0.3 * ctrl_env(0, env), and the fine RK4 trajectory's end [qpos, qvel] at h = horizon / fine"""
    o.init_env(env)
    ctrl = 0.3 * o.ctrl_env(0, env)
    s0 = np.concatenate([[0.0], o.qpos.copy(), o.qvel.copy(), np.zeros(o.nv)])
    ref = trajectory(o, s0, ctrl, horizon / fine, fine)[-1][1:1 + o.nq + o.nv]
    return s0, ctrl, ref


def end_error(o, s0, ctrl, ref, h, kind, horizon=0.04):
    """max |delta| over qpos and qvel at the horizon, stepping with size h, against the fine trajectory's end"""
    x = trajectory(o, s0, ctrl, h, int(round(horizon / h)), kind)[-1][1:1 + o.nq + o.nv]
    return np.abs(x - ref).max()


def rk4_transition_fd(o, x, u, warm, eps):
    """mjd_transitionFD (centered) restated over rk4_step, in tangent coordinates, for models with at most one free joint at the root
    followed by scalar joints (the chains and the humanoid)"""
    nq, nv, nu = o.nq, o.nv, o.nu
    free = nq == nv + 1

    def step(q, v, uu):
        r = rk4_step(o, np.concatenate([[0.0], q, v, warm]), uu)
        return r["qpos"], r["qvel"]

    def integrate(q, dq):
        q = q.copy()
        if not free:
            return q + dq
        q[:3] += dq[:3]
        ang = np.linalg.norm(dq[3:6])
        if ang > 0:
            r = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * dq[3:6] / ang])
            q[3:7] = quat_mul(q[3:7], r); q[3:7] /= np.linalg.norm(q[3:7])
        q[7:] += dq[6:]
        return q

    def differentiate(q1, q2):
        if not free:
            return q2 - q1
        d = np.zeros(nv)
        d[:3] = q2[:3] - q1[:3]
        c = quat_mul(q1[3:7] * np.array([1, -1, -1, -1]), q2[3:7])
        sn = np.linalg.norm(c[1:])
        ang = 2 * np.arctan2(sn, c[0])
        if ang > np.pi:
            ang -= 2 * np.pi
        d[3:6] = c[1:] * (ang / sn if sn > 1e-15 else 0.0)
        d[6:] = q2[7:] - q1[7:]
        return d

    q0, v0 = x[:nq], x[nq:]
    qn, vn = step(q0, v0, u)
    Am = np.zeros((2 * nv, 2 * nv)); Bm = np.zeros((2 * nv, nu))
    for col in range(2 * nv + nu):
        out = []
        for sgn in (1.0, -1.0):
            q, v, uu = q0, v0.copy(), u.copy()
            if col < nv:
                dq = np.zeros(nv); dq[col] = sgn * eps
                q = integrate(q0, dq)
            elif col < 2 * nv:
                v[col - nv] += sgn * eps
            else:
                uu[col - 2 * nv] += sgn * eps
            q2, v2 = step(q, v, uu)
            out.append(np.concatenate([differentiate(qn, q2), v2 - vn]))
        d = (out[0] - out[1]) / (2 * eps)
        if col < 2 * nv:
            Am[:, col] = d
        else:
            Bm[:, col - 2 * nv] = d
    return Am, Bm


def device_one_step_errors(hbmod, b, o, states, ctrls):
    """One teacher-forced RK4 step of batch b (diag outputs on) from `states` under `ctrls` against rk4_step from the same fp32-rounded
    records.  Returns (errors, info): errors = dict quantity -> per-state array (qpos: max relative to max(1, |qpos|); qvel, qacc,
    warm, force: max |delta| / max(1, max |reference|); time: |delta|), info = dict(kernel, status, dev_counts = (ncon, nefc) arrays of
    the device, ref_counts = per state the reference's four (ncon, nefc, niter), types = the reference's row types of the last stage).
    Asserts nothing: the tests and tools/gpu_rk4_parity_report.py both read it."""
    nq, nv = o.nq, o.nv
    states = np.asarray(states, dtype=np.float32).astype(np.float64)
    b.diag_enable(True)
    b.set_state(hbmod.STATE_INTEGRATION, states)
    b.step(np.asarray(ctrls, dtype=np.float32))
    kernel = b.last_kernel()
    after = b.get_state(hbmod.STATE_INTEGRATION).astype(np.float64)
    a, f = b.qacc().astype(np.float64), b.efc_force().astype(np.float64)
    nc, ne, _ = b.counts()
    status = b.status()
    b.diag_enable(False)
    err = dict(qpos=[], qvel=[], qacc=[], warm=[], force=[], time=[])
    ref_counts, types = [], []
    for k in range(len(states)):
        r = rk4_step(o, states[k], np.asarray(ctrls[k], dtype=np.float32).astype(np.float64))
        ref_counts.append(r["counts"]); types.append(r["types"])
        q, v, w = after[k, 1:1 + nq], after[k, 1 + nq:1 + nq + nv], after[k, 1 + nq + nv:]
        err["time"].append(abs(after[k, 0] - r["time"]))
        err["qpos"].append((np.abs(q - r["qpos"]) / np.maximum(1.0, np.abs(r["qpos"]))).max())
        err["qvel"].append(np.abs(v - r["qvel"]).max() / max(1.0, np.abs(r["qvel"]).max()))
        err["qacc"].append(np.abs(a[k] - r["qacc"]).max() / max(1.0, np.abs(r["qacc"]).max()))
        err["warm"].append(np.abs(w - r["warm"]).max() / max(1.0, np.abs(r["warm"]).max()))
        n = r["counts"][3][1]
        same = (nc[k], ne[k]) == r["counts"][3][:2]
        err["force"].append(np.abs(f[k, :n] - r["efc_force"]).max() / max(1.0, np.abs(r["efc_force"]).max()) if n and same else 0.0)
    return {k: np.array(v) for k, v in err.items()}, dict(kernel=kernel, status=status, dev_counts=(nc, ne), ref_counts=ref_counts, types=types)
