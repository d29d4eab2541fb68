"""The RK4 integrator (mjINT_RK4; hb_step.hip: step_body's INTEG, the INTEG rows of HB_KERNELS) on the GPU, against the fp64 reference of
tests/rk4_ref.py (the RK4 recurrence restated over the oracle's mj_forward).

KERNELS (step_lib.RK4_KERNELS) names every RK4 kernel and the model that must run it (Batch.last_kernel): the benchmark humanoid under PGS/50 and Newton/100,
and the capsule chains of tests/kernel_models.py at 28 and 32 dofs with `integrator="RK4"` in their <option>.

One-step bounds (BOUNDS): the project's rule is at most 3 x the measured maximum, against the fp64 reference, and for these kernels no
more than twice the Euler step's bound of the same quantity (tests/test_gpu_parity.py: qpos 4e-5 relative, qvel / qacc / force
4e-4 * max(1, max|.|)).  The measurement is quoted at bounds.RK4_BOUNDS (profiles/rk4_parity_report.txt, from tools/gpu_rk4_parity_report.py).
"""
import os

import numpy as np
import pytest

import rk4_ref
import step_lib
from bounds import RK4_BOUNDS as BOUNDS
from kernel_models import CNSTR_CONTACT_FRICTIONLESS, CNSTR_CONTACT_PYRAMIDAL, CNSTR_LIMIT_JOINT, chain_xml, oracle_for, rollout_states
from oracle_lib import ASSETS, HUMANOID_HBM, Oracle, golden_states
from step_lib import RK4_KERNELS as KERNELS, T, everything

pytestmark = pytest.mark.gpu

CHAINS = {name: step_lib.CHAINS[name] for name in ("chain28_cd3_pgs", "chain32_cd3_pgs", "chain28_cd1_newton", "chain32_cd1_newton")}


def _humanoid(hbmod, solver, iterations, integrator=1, **opt):
    m = hbmod.Model.load(HUMANOID_HBM)
    m.set_opt(solver=solver, iterations=iterations, integrator=integrator, **opt)
    o = Oracle()
    o.set_opt(solver=solver, iterations=iterations, **opt)
    return m, o


def _golden_states():
    st, ctrl, _ = golden_states()
    return st.astype(np.float32).astype(np.float64), ctrl.astype(np.float32)


def _rk4_chain(hbmod, name, tmp_path):
    xml = chain_xml(*CHAINS[name])
    assert xml.count("<option ") == 1
    m, p, o = oracle_for(hbmod, xml.replace("<option ", '<option integrator="RK4" '), tmp_path)
    assert m.opt.integrator == hbmod.INT_RK4
    st, ct = rollout_states(o)
    return m, o, st, ct


def _hold_to_reference(hbmod, gpu, m, o, st, ct, label, kernel):
    b = hbmod.Batch(m, len(st), gpu)
    err, info = rk4_ref.device_one_step_errors(hbmod, b, o, st, ct)
    b.close()
    for k, v in err.items():
        print("  %-22s %-6s median %.2e  max %.2e" % (label, k, np.median(v), v.max()))
    assert info["kernel"] == kernel, (label, info["kernel"])
    assert not info["status"].any(), (label, info["status"])
    nc, ne = info["dev_counts"]
    for k, rc in enumerate(info["ref_counts"]):
        assert (nc[k], ne[k]) == rc[3][:2], (label, k, "counts are not the last stage's", (nc[k], ne[k]), rc)
    for k, v in err.items():
        assert v.max() <= BOUNDS[k], (label, k, v.max(), BOUNDS[k])
    return info


@pytest.mark.parametrize("name,solver,iterations", [("humanoid27_pgs", 0, 50), ("humanoid27_newton", 2, 100)])
def test_one_step_parity_on_the_golden_states(hbmod, gpu, name, solver, iterations):
    """the 128 golden states, teacher-forced: kernel by name, status zero, (ncon, nefc) those of the reference's LAST stage for all 128,
    qpos', qvel', qacc and efc_force (last stage), qacc_warmstart' = F_3 and time' within BOUNDS"""
    m, o = _humanoid(hbmod, solver, iterations)
    st, ct = _golden_states()
    info = _hold_to_reference(hbmod, gpu, m, o, st, ct, name, KERNELS[name])
    differ = sum(rc[3][:2] != rc[0][:2] for rc in info["ref_counts"])
    print("  %s: (ncon, nefc) of the last stage differ from the first stage's in %d of %d states" % (name, differ, len(st)))
    assert differ >= 20  # (the read-out rule is exercised: 63 in the fp64 reference)
    assert max(x[0] for rc in info["ref_counts"] for x in rc) <= 24 and max(x[1] for rc in info["ref_counts"] for x in rc) <= 63


@pytest.mark.parametrize("name", list(CHAINS))
def test_one_step_parity_of_the_other_kernels_and_sizes(hbmod, gpu, tmp_path, name):
    """capsule chains at 28 and 32 dofs, condim 3 under PGS and condim 1 under Newton, compiled with integrator="RK4": the four RK4
    kernels by name, each held to the reference as above, on states of which at least 10 have contact rows and 10 limit rows"""
    m, o, st, ct = _rk4_chain(hbmod, name, tmp_path)
    info = _hold_to_reference(hbmod, gpu, m, o, st, ct, name, KERNELS[name])
    con = sum(bool(np.isin(t, (CNSTR_CONTACT_FRICTIONLESS, CNSTR_CONTACT_PYRAMIDAL)).any()) for t in info["types"])
    lim = sum(bool((t == CNSTR_LIMIT_JOINT).any()) for t in info["types"])
    assert con >= 10 and lim >= 10, (name, con, lim)


def test_launch_shapes_are_the_same_arithmetic(hbmod, gpu):
    """T steps as one rollout, as T step calls, as T folded step_dev calls on a pipelined batch, each with the diagnostic outputs on
    and off: one instantiation serves them all, so state, counts and status are bit-identical"""
    m, _ = _humanoid(hbmod, 0, 50)
    st, _ = _golden_states()
    n = len(st)
    ctrl = np.random.default_rng(5).uniform(-1, 1, (T, n, m.nu)).astype(np.float32)
    got = {}
    for diag in (False, True):
        for shape in ("rollout", "steps", "folded"):
            b = hbmod.Batch(m, n, gpu)
            b.diag_enable(diag)
            b.set_state(hbmod.STATE_INTEGRATION, st)
            if shape == "rollout":
                b.rollout(ctrl)
            elif shape == "steps":
                for t in range(T):
                    b.step(ctrl[t])
            else:
                b.tune(fold=64)
                b.pipeline(True)
                p = b.dev_alloc(ctrl.nbytes)
                b.to_dev(p, ctrl)
                for t in range(T):
                    b.step_dev(p + t * ctrl[0].nbytes)
                b.sync()
                b.dev_free(p)
            assert b.last_kernel() == "hb_rk4_kernel", (shape, diag, b.last_kernel())
            got[shape, diag] = everything(hbmod, b)
            b.close()
    ref = got["rollout", False]
    assert ref[2].max() > 0 and not ref[4].any()
    assert np.allclose(ref[0][:, 0], st[:, 0] + T * 0.005, atol=1e-5)
    for key, x in got.items():
        assert all(np.array_equal(u, w) for u, w in zip(x, ref)), key


def test_order_of_convergence_on_the_device(hbmod, gpu):
    """The benchmark humanoid under Newton/100 over the contact-free first 0.04 s, envs 0 and 3 of a reset(perturb=True) batch under the
    held control 0.3 * ctrl_env(0, e), against the fp64 RK4 trajectory at h = 0.04 / 256 from the same start: halving h from 0.01 to
    0.005 divides the device's RK4 error by at least 8 (fourth order: 16 and more) and its Euler error by at most 3; the device's
    free-running RK4 qpos stays within 1e-4 relative of the fp64 reference stepping at the same h."""
    envs, horizon = (0, 3), 0.04
    _, o = _humanoid(hbmod, 2, 100)
    ctrl = np.zeros((8, o.nu), np.float32)
    for e in envs:
        ctrl[e] = 0.3 * o.ctrl_env(0, e)
    err, start, fine = {}, None, {}
    for integrator in (1, 0):
        for h in (0.01, 0.005):
            m, _ = _humanoid(hbmod, 2, 100, integrator=integrator, timestep=h)
            b = hbmod.Batch(m, 8, gpu)
            b.reset(perturb=True)
            s0 = b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
            if start is None:
                start = s0
                for e in envs:
                    o.init_env(e)  # (the batch's start is the oracle's env e, rounded to fp32)
                    assert np.abs(s0[e, 1:1 + o.nq + o.nv] - np.concatenate([o.qpos, o.qvel])).max() < 1e-6 and not s0[e, 1 + o.nq + o.nv:].any() and s0[e, 0] == 0
                    fine[e] = rk4_ref.trajectory(o, s0[e], ctrl[e].astype(np.float64), horizon / 256, 256)[-1][1:1 + o.nq + o.nv]
            assert np.array_equal(s0, start)
            n = int(round(horizon / h))
            traj = []
            for _ in range(n):
                b.step(ctrl)
                traj.append(b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64))
            assert b.last_kernel().startswith("hb_rk4_newton28_kernel" if integrator else "hb_step_newton28_"), b.last_kernel()
            assert not b.status().any() and not b.counts()[1][list(envs)].any()  # (contact-free, no limit rows)
            b.close()
            for e in envs:
                err[integrator, h, e] = np.abs(traj[-1][e, 1:1 + o.nq + o.nv] - fine[e]).max()
                if integrator:  # free-running against the reference at the same h
                    ref = rk4_ref.trajectory(o, start[e], ctrl[e].astype(np.float64), h, n)
                    drift = max((np.abs(traj[t][e, 1:1 + o.nq] - ref[t][1:1 + o.nq]) / np.maximum(1.0, np.abs(ref[t][1:1 + o.nq]))).max() for t in range(n))
                    print("  env %d h %g: free-running qpos drift against the fp64 reference %.2e" % (e, h, drift))
                    assert drift <= 1e-4, (e, h, drift)
    for e in envs:
        print("  env %d: RK4 error %.2e (h=0.01) %.2e (h=0.005), Euler %.2e %.2e" % (e, err[1, 0.01, e], err[1, 0.005, e], err[0, 0.01, e], err[0, 0.005, e]))
        assert err[1, 0.01, e] / err[1, 0.005, e] >= 8, (e, err[1, 0.01, e], err[1, 0.005, e])
        assert err[0, 0.01, e] / err[0, 0.005, e] <= 3, (e, err[0, 0.01, e], err[0, 0.005, e])


def test_bad_first_stage_qacc_resets_and_steps_from_the_reset_state(hbmod, gpu):
    """mj_checkAcc after the first stage (as tests/test_gpu_parity.py::test_bad_state_is_flagged_and_reset builds the state): the env is
    flagged, reset, and ends at the RK4 step from the reset state (qpos0, zero velocity, warm start, ctrl, xfrc_applied, time 0)"""
    m, o = _humanoid(hbmod, 0, 50)
    n = 8
    b = hbmod.Batch(m, n, gpu)
    b.reset(perturb=True)
    b.rollout_halton(30)
    spec = hbmod.STATE_INTEGRATION | hbmod.STATE_XFRC_APPLIED
    st = b.get_state(spec, dtype=np.float64)
    nint = 1 + m.nq + 2 * m.nv
    st[6, nint + 6 * 1 + 2] = 1e14  # xfrc_applied on the torso: |qacc| > 1e10 -> mjWARN_BADQACC
    b.set_state(spec, st)
    ctrl = np.full((n, m.nu), 0.7, np.float32)
    b.step(ctrl)
    s = b.status()
    assert s[6] == hbmod.WARN_BADQACC and not s[[0, 1, 2, 3, 4, 5, 7]].any(), s
    after = b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
    o.reset()
    reset = np.concatenate([[0.0], o.qpos.copy(), np.zeros(2 * m.nv)])
    for e in range(n):
        r = rk4_ref.rk4_step(o, reset if e == 6 else st[e, :nint], np.zeros(m.nu) if e == 6 else ctrl[e])
        assert abs(after[e, 0] - r["time"]) < 1e-6 and (abs(r["time"] - 0.005) < 1e-12) == (e == 6)
        assert (np.abs(after[e, 1:1 + m.nq] - r["qpos"]) / np.maximum(1, np.abs(r["qpos"]))).max() <= BOUNDS["qpos"], e
        assert np.abs(after[e, 1 + m.nq:1 + m.nq + m.nv] - r["qvel"]).max() <= BOUNDS["qvel"] * max(1.0, np.abs(r["qvel"]).max()), e
    assert np.abs(after[6, 1 + m.nq:1 + m.nq + m.nv]).max() > 1e-3  # (not simply qpos0: gravity acted)
    assert not b.get_state(spec, dtype=np.float64)[6, nint:].any()  # (xfrc_applied of the reset env is zero)
    b.close()


def test_rollout_sensors_are_those_of_the_first_stage(hbmod, gpu):
    """hb_rollout_sensors under RK4 returns, per step, what hb_sensors reads at the state before that step (MuJoCo evaluates no
    sensors in the later stages) - bit for bit: the same kernel's first forward pass"""
    m, _ = _humanoid(hbmod, 0, 50)
    st, ct = _golden_states()
    n = len(st)
    torso = m.name2id("body", "torso")
    spec = hbmod.Batch.sensor_spec([m.name2id("body", "head"), m.name2id("body", "foot_right")], subtree_body=torso, linvel_bodies=[torso])
    ctrl = np.random.default_rng(9).uniform(-1, 1, (3, n, m.nu)).astype(np.float32)
    ctrl[0] = ct
    a, b = hbmod.Batch(m, n, gpu), hbmod.Batch(m, n, gpu)
    a.set_state(hbmod.STATE_INTEGRATION, st); b.set_state(hbmod.STATE_INTEGRATION, st)
    sens, _ = a.rollout_sensors(ctrl, spec)
    assert a.last_kernel() == "hb_rk4_kernel"
    for t in range(3):
        before = b.sensors(spec, ctrl[t])
        assert np.array_equal(sens[t], before), (t, np.abs(sens[t] - before).max())
        b.step(ctrl[t])
        assert np.abs(b.sensors(spec, ctrl[t]) - before).max() > 1e-4  # (and not those of the state the step ends in)
    assert np.array_equal(a.get_state(hbmod.STATE_INTEGRATION), b.get_state(hbmod.STATE_INTEGRATION))
    a.close(); b.close()


def test_discrete_inverse_is_refused_and_the_continuous_one_unchanged(hbmod, gpu):
    """hb_inverse(HB_INV_DISCRETE) is the inverse of the Euler step: refused on an RK4 model; the continuous inverse of hb_forward's
    qacc still returns the actuator forces (the bound of tests/test_gpu_inverse.py::test_continuous_round_trip)"""
    from inverse_ref import forward_at
    m, o = _humanoid(hbmod, 2, 100)
    st, ct = _golden_states()
    idx = np.arange(0, 128, 2)
    nq, nv = m.nq, m.nv
    qpos, qvel = st[idx, 1:1 + nq].astype(np.float32), st[idx, 1 + nq:1 + nq + nv].astype(np.float32)
    ctrl = (0.5 * ct[idx]).astype(np.float32)
    b = hbmod.Batch(m, len(idx), gpu)
    b.set_state(hbmod.STATE_INTEGRATION, np.concatenate([np.zeros((len(idx), 1)), qpos, qvel, np.zeros_like(qvel)], axis=1))
    b.diag_enable(True)
    b.forward(ctrl)
    assert b.last_kernel() == "hb_rk4_newton28_kernel"
    qacc = b.qacc()
    with pytest.raises(hbmod.HbError):
        b.inverse(qacc, discrete=True)
    got = b.inverse(qacc)
    assert b.last_kernel() == "hb_inverse_kernel"
    err = []
    for k in range(len(idx)):
        forward_at(o, qpos[k], qvel[k], ctrl[k])
        err.append(np.abs(got[k] - o.qfrc_actuator).max() / max(1.0, np.abs(o.qfrc_bias).max(), np.abs(o.qfrc_actuator).max()))
    print("  continuous round trip on an RK4 model: worst %.2e" % max(err))
    assert max(err) < 5e-5, max(err)
    b.close()


def test_staged_models_are_refused_not_stepped_with_euler(hbmod, gpu):
    for name in ("team_robot.hbm", "humanoid27_hfield.hbm"):
        m = hbmod.Model.load(os.path.join(ASSETS, name))
        m.set_opt(integrator=hbmod.INT_RK4)
        with pytest.raises(hbmod.HbError, match="RK4: only models that step in one kernel"):
            hbmod.Batch(m, 4, gpu)
        m.set_opt(integrator=hbmod.INT_EULER)
        hbmod.Batch(m, 4, gpu).close()


def test_transition_fd_differentiates_the_rk4_step(hbmod, gpu, tmp_path):
    """hb_transition_fd on the 28-dof chain, contact-free states, centered, eps 1e-3, against central differences of the fp64 RK4
    reference (tolerances of tests/test_gpu_planner.py::test_transition_derivatives_by_batched_finite_differences)"""
    xml = chain_xml(*CHAINS["chain28_cd3_pgs"]).replace("<option ", '<option integrator="RK4" ')
    m, p, o = oracle_for(hbmod, xml, tmp_path)
    st, ct = rollout_states(o, steps=40, every=4)
    nq, nv, nu = m.nq, m.nv, m.nu
    free = [k for k in range(len(st)) if all(c[1] == 0 for c in rk4_ref.rk4_step(o, st[k], ct[k].astype(np.float64))["counts"])][:3]
    assert len(free) == 3
    xs = st[free, 1:1 + nq + nv]; us = 0.5 * ct[free].astype(np.float64); ws = st[free, 1 + nq + nv:]
    eps = 1e-3
    b = hbmod.Batch(m, len(free) * (1 + 2 * (2 * nv + nu)) + 5, gpu)
    A, B = b.transition_fd(xs, us, ws, eps=eps, centered=True)
    assert b.last_kernel() == "hb_rk4_kernel"
    b.close()
    for t in range(len(free)):
        Ao, Bo = rk4_ref.rk4_transition_fd(o, xs[t], us[t], ws[t], eps)
        sa, sb = np.abs(Ao).max(), np.abs(Bo).max()
        print("  point %d: A worst %.2e median %.2e of %.2e, B worst %.2e of %.2e" % (t, np.abs(A[t] - Ao).max(), np.median(np.abs(A[t] - Ao)), sa, np.abs(B[t] - Bo).max(), sb))
        assert np.abs(A[t] - Ao).max() <= 5e-3 * sa, (t, np.abs(A[t] - Ao).max(), sa)
        assert np.abs(B[t] - Bo).max() <= 5e-3 * max(sb, 1e-3), (t, np.abs(B[t] - Bo).max(), sb)
        assert np.median(np.abs(A[t] - Ao)) <= 2e-4 * sa and np.median(np.abs(B[t] - Bo)) <= 2e-4 * max(sb, 1e-3)


def test_vecenv_steps_on_rk4(hbmod, gpu):
    m, _ = _humanoid(hbmod, 0, 50)
    env = hbmod.VecEnv(m, 256, gpu)
    env.reset()
    rng = np.random.default_rng(4)
    bad = hbmod.WARN_BADQPOS | hbmod.WARN_BADQVEL | hbmod.WARN_BADQACC
    for _ in range(50):
        obs = env.step(rng.uniform(-1, 1, (256, m.nu)).astype(np.float32))[0]
        assert np.isfinite(obs).all()
        assert env.batch.last_kernel().startswith("hb_rk4_"), env.batch.last_kernel()
    assert not (env.batch.status() & bad).any()
    env.close()


@pytest.mark.parametrize("solver,iterations", [(0, 50), (2, 100)])
def test_soak(hbmod, gpu, solver, iterations):
    """256 envs x 1000 RK4 steps of the Halton workload: finite, time = 1000 h where no bad-state reset happened, and no more envs with a
    HB_WARN_BAD* bit than the same run under Euler shows"""
    bad = hbmod.WARN_BADQPOS | hbmod.WARN_BADQVEL | hbmod.WARN_BADQACC
    nbad = {}
    for integrator in (1, 0):
        m, _ = _humanoid(hbmod, solver, iterations, integrator=integrator)
        b = hbmod.Batch(m, 256, gpu)
        b.reset(perturb=True)
        b.rollout_halton(1000)
        st, s = b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64), b.status()
        assert b.last_kernel().startswith("hb_rk4_") == bool(integrator), b.last_kernel()
        b.close()
        assert np.isfinite(st).all()
        ok = (s & bad) == 0
        assert np.abs(st[ok, 0] - 1000 * 0.005).max() < 1e-3, np.abs(st[ok, 0] - 5.0).max()
        nbad[integrator] = int((~ok).sum())
    print("  solver %d: envs with a bad-state bit after 1000 steps: RK4 %d, Euler %d" % (solver, nbad[1], nbad[0]))
    assert nbad[1] <= nbad[0], nbad
