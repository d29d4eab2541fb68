"""Inverse dynamics on the GPU (include/hb.h: hb_inverse / hb_inverse_dev, engine.Batch.inverse) against the fp64 restatement of
tests/inverse_ref.py on the oracle's forward() arrays, and the call's contract: purity, ordering behind held step calls, warnings.

Bounds are relative to the force scale of the env: the largest entry of any term of the sum (M qacc, qfrc_bias, qfrc_passive, J' f; at
least 1) in the fp64 reference (inverse_ref.force_scale); the measured
worst and median values are written beside each bound (the tests print them: pytest -s)."""
import os

import numpy as np
import pytest

from inverse_ref import force_scale, forward_at, inverse_ref, inverse_terms
from oracle_lib import ASSETS, GOLDEN, HUMANOID_HBM, Oracle, MODELS_DIR as MODELS

pytestmark = pytest.mark.gpu
SOL_NEWTON = 2


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "humanoid27_steps.npz"))


def _hbm(tmp_path, name):
    """a test model's path: assets as they are, tests/models/*.xml compiled to .hbm for the oracle"""
    import humanoid_mujoco_amd as hb
    if name.endswith(".hbm"):
        return os.path.join(ASSETS, name)
    p = str(tmp_path / (name + ".hbm"))
    hb.Model.load(os.path.join(MODELS, name + ".xml")).save(p)
    return p


def _ref_errors(o, qpos, qvel, qacc, got, discrete=False):
    """relative error of every env's qfrc_inverse against the reference, the reference's force scale, and its active rows"""
    err, active = [], 0
    for e in range(len(qpos)):
        forward_at(o, qpos[e], qvel[e])
        t = inverse_terms(o, qacc[e].astype(np.float64), discrete)
        ref = t["Mqacc"] + t["bias"] - t["passive"] - t["constraint"]
        err.append(np.abs(got[e] - ref).max() / force_scale(t))
        active += t["active"]
    return np.array(err), active


def _batch_at(hb, model, qpos, qvel, gpu):
    b = hb.Batch(model, len(qpos), gpu)
    st = np.concatenate([np.zeros((len(qpos), 1)), qpos, qvel, np.zeros_like(qvel)], axis=1)
    b.set_state(hb.STATE_INTEGRATION, st)
    return b


def test_parity_on_golden_states(hbmod, humanoid_model, gpu, golden):
    """128 golden states, (a) their forward qacc, (b) that qacc plus noise that switches rows on and off (classic variant)."""
    g = golden
    qpos, qvel = g["qpos"].astype(np.float32), g["qvel"].astype(np.float32)
    b = _batch_at(hbmod, humanoid_model, qpos, qvel, gpu)
    o = Oracle()
    rng = np.random.default_rng(3)
    qa = g["qacc"].astype(np.float32)
    qb = (qa + rng.normal(size=qa.shape) * 0.3 * np.maximum(1.0, np.abs(qa).max(axis=1, keepdims=True))).astype(np.float32)
    res = {}
    for tag, qacc in (("golden", qa), ("noisy", qb)):
        got = b.inverse(qacc)
        assert b.last_kernel() == "hb_inverse_kernel"
        res[tag] = _ref_errors(o, qpos, qvel, qacc, got)
    print("inverse parity, golden qacc: worst %.2e median %.2e (%d active rows); noisy: worst %.2e median %.2e (%d active rows)"
          % (res["golden"][0].max(), np.median(res["golden"][0]), res["golden"][1], res["noisy"][0].max(), np.median(res["noisy"][0]), res["noisy"][1]))
    assert res["golden"][1] > 100 and res["noisy"][1] != res["golden"][1]
    # measured: golden qacc worst 1.85e-3, median 1.8e-5; noisy worst 8.6e-5, median 1.0e-6.  The worst states are stiff contacts whose
    # force D (aref - J qacc) follows the penetration depth: the fp64 reference itself moves by up to 2.6e-3 of the force scale when
    # qpos moves by 6e-7 relative (the few fp32 ulps the device's kinematics accumulate; oracle_lib.FENCE_MAGNITUDES), 2.4e-4 at 6e-8
    assert res["golden"][0].max() < 4e-3 and np.median(res["golden"][0]) < 1e-4, res["golden"][0].max()
    assert res["noisy"][0].max() < 3e-4 and np.median(res["noisy"][0]) < 1e-5, res["noisy"][0].max()


@pytest.mark.parametrize("name,solver,kernel", [("pendulum_limit", None, "hb_inverse_kernel"), ("chain", None, "hb_inverse_kernel"),
                                                ("capsules", None, "hb_inverse_kernel"), ("maxsize", None, "hb_inverse32_kernel"),
                                                ("ball_hfield", None, "hb_inverse_gen_kernel"), ("humanoid27_hfield.hbm", None, "hb_inverse_gen_kernel"),
                                                ("humanoid27_hfield.hbm", SOL_NEWTON, "hb_inverse_big28_kernel"),
                                                ("team_robot.hbm", None, "hb_inverse_big20_kernel"), ("team_robot.hbm", 0, "hb_inverse_pgs_big_kernel")])
def test_parity_on_other_models(hbmod, gpu, tmp_path, name, solver, kernel):
    """limits, a fixed tendon, multi-tree contacts, 32 dofs, height fields (general path), the team robot (meshes, condim 6, 256 rows with
    Newton, 128 with PGS); continuous and discrete"""
    p = _hbm(tmp_path, name)
    o = Oracle(p)
    if solver is not None:
        o.set_opt(solver=solver)
    o.reset(0 if name in ("chain", "team_robot.hbm") else -1)
    qpos, qvel = [], []
    for t in range(16 * 25):
        o.ctrl[:] = np.sign(np.sin(0.01 * t + 1.0 + np.arange(o.nu)))
        o.step()
        if t % 25 == 24:
            qpos.append(o.qpos.copy()); qvel.append(o.qvel.copy())
    qpos, qvel = np.array(qpos, np.float32), np.array(qvel, np.float32)
    if name == "pendulum_limit":  # (across the range [-0.5, 0.3] and beyond)
        qpos[:, 0] = np.linspace(-0.6, 0.4, len(qpos))
    if name == "chain":  # (the rail's range and the tendon's, h1 - h2 / 2 in [-0.5, 0.5], from end to end)
        qpos[:, 0] = np.linspace(-1.05, 1.05, len(qpos))
        qpos[:, 1], qpos[:, 2] = np.linspace(-0.8, 0.8, len(qpos)), np.linspace(0.6, -0.6, len(qpos))
    qacc = np.random.default_rng(7).normal(size=qvel.shape).astype(np.float32) * 5.0
    model = hbmod.Model.load(p)
    if solver is not None:
        model.set_opt(solver=solver)
    b = _batch_at(hbmod, model, qpos, qvel, gpu)
    spec = hbmod.STATE_INTEGRATION | hbmod.STATE_XFRC_APPLIED
    before = (b.get_state(spec), b.status(), *b.collision_counts(want_cycles=True), *b.counts())
    got = b.inverse(qacc)
    assert b.last_kernel() == kernel
    after = (b.get_state(spec), b.status(), *b.collision_counts(want_cycles=True), *b.counts())
    assert all(np.array_equal(x, y) for x, y in zip(before, after))  # (general variants: the narrowphase's counts and bits as well)
    err, active = _ref_errors(o, qpos.astype(np.float64), qvel.astype(np.float64), qacc, got)
    errd, _ = _ref_errors(o, qpos.astype(np.float64), qvel.astype(np.float64), qacc, b.inverse(qacc, discrete=True), discrete=True)
    print("inverse parity %s (solver %s): worst %.2e median %.2e, %d active rows; discrete: worst %.2e median %.2e"
          % (name, solver, err.max(), np.median(err), active, errd.max(), np.median(errd)))
    # measured (worst / median, the discrete reading within 1e-7 of these): pendulum_limit 4.3e-7 / 1.0e-7, chain 1.4e-6 / 1.1e-7, capsules
    # 2.0e-5 / 3.3e-6, maxsize 1.3e-5 / 8.0e-7, ball_hfield 2.0e-5 / 3.3e-6, humanoid27_hfield 2.5e-4 / 1.0e-5 (Newton: 5.8e-5 / 8.3e-6),
    # team_robot 2.3e-4 / 1.0e-4 with either solver (stiff contacts: see test_parity_on_golden_states)
    assert active > 0 and err.max() < 1e-3 and errd.max() < 1e-3, (name, err, errd)


def _newton_model(hb, path=HUMANOID_HBM):
    m = hb.Model.load(path)
    m.set_opt(solver=SOL_NEWTON, iterations=100, tolerance=1e-10)
    return m


def test_continuous_round_trip(hbmod, gpu, golden):
    """forward (Newton) -> qacc -> inverse recovers qfrc_actuator (xfrc_applied, qfrc_applied zero), also with per-env parameters"""
    g = golden
    idx = np.arange(0, 128, 2)
    qpos, qvel = g["qpos"][idx].astype(np.float32), g["qvel"][idx].astype(np.float32)
    ctrl = (0.5 * g["ctrl"][idx]).astype(np.float32)
    b = _batch_at(hbmod, _newton_model(hbmod), qpos, qvel, gpu)
    b.diag_enable(True)
    b.forward(ctrl)
    got = b.inverse(b.qacc())
    o = Oracle()
    err = []
    for k in range(len(idx)):
        forward_at(o, qpos[k], qvel[k], ctrl[k])
        err.append(np.abs(got[k] - o.qfrc_actuator).max() / max(1.0, np.abs(o.qfrc_bias).max(), np.abs(o.qfrc_actuator).max()))
    err = np.array(err)
    print("continuous round trip: worst %.2e median %.2e" % (err.max(), np.median(err)))
    assert err.max() < 5e-5, err.max()  # (measured: worst 1.5e-5, median 1.6e-6)
    # per-env model parameters (masses, armature, limits, friction, force ranges): motors inside their force range
    env = hbmod.VecEnv(_newton_model(hbmod), 32, gpu, auto_reset=0, max_time=0.0, target_z=10.0)
    d = env.batch.env_default_domain_randomization()
    d.seed = 5
    d.max_mass_change = 0.5
    env.batch.env_domain_randomize(d)
    env.reset()
    bb = env.batch
    assert bb.env_domain_params() is not None
    c = np.tile(0.2 * np.sin(np.arange(bb.model.nu)), (bb.n_env, 1)).astype(np.float32)
    bb.diag_enable(True)
    bb.forward(c)
    got = bb.inverse(bb.qacc())
    o.reset()
    o.ctrl[:] = c[0]
    o.forward()
    want = o.qfrc_actuator.copy()  # (motors: gear * gain * ctrl, the same in every env and state)
    errd = np.abs(got - want).max(axis=1) / max(1.0, np.abs(want).max())
    print("continuous round trip with per-env parameters: worst %.2e median %.2e" % (errd.max(), np.median(errd)))
    assert errd.max() < 2e-3, errd.max()  # (measured: worst 6.5e-4, median 2.9e-5: Newton's fp32 tolerance on heavier / lighter bodies)


def test_discrete_round_trip(hbmod, gpu, golden):
    """one Newton step, (qvel' - qvel) / h, inverse(discrete) at the state before the step: the forces that drove the step"""
    g = golden
    idx = np.arange(1, 128, 2)
    qpos, qvel = g["qpos"][idx].astype(np.float32), g["qvel"][idx].astype(np.float32)
    ctrl = (0.5 * g["ctrl"][idx]).astype(np.float32)
    m = _newton_model(hbmod)
    b = _batch_at(hbmod, m, qpos, qvel, gpu)
    st0 = b.get_state(hbmod.STATE_INTEGRATION)
    b.step(ctrl)
    qacc_d = (b.qvel.astype(np.float64) - qvel) / m.opt.timestep
    b.set_state(hbmod.STATE_INTEGRATION, st0)
    got = b.inverse(qacc_d.astype(np.float32), discrete=True)
    got_c = b.inverse(qacc_d.astype(np.float32))
    o = Oracle()
    err, err_c = [], []
    for k in range(len(idx)):
        forward_at(o, qpos[k], qvel[k], ctrl[k])
        s = max(1.0, np.abs(o.qfrc_bias).max(), np.abs(o.qfrc_actuator).max())
        err.append(np.abs(got[k] - o.qfrc_actuator).max() / s)
        err_c.append(np.abs(got_c[k] - o.qfrc_actuator).max() / s)
    err, err_c = np.array(err), np.array(err_c)
    print("discrete round trip: worst %.2e median %.2e (continuous reading of the same qacc: median %.2e)" % (err.max(), np.median(err), np.median(err_c)))
    assert err.max() < 1e-3, err.max()  # (measured: worst 2.8e-4, median 3.8e-6; the continuous reading of the same qacc is 0.41 off)
    assert np.median(err) < np.median(err_c)  # (the humanoid's joints are damped: the conversion matters)


def test_purity_and_ordering(hbmod, humanoid_model, gpu):
    n = 64
    spec = hbmod.STATE_INTEGRATION | hbmod.STATE_XFRC_APPLIED  # (ctrl: nothing on the inverse's path writes the control buffer)
    a = hbmod.Batch(humanoid_model, n, gpu)
    a.reset(perturb=True)
    a.rollout_halton(60)
    before = (a.get_state(spec), a.status(), a.counts())
    qacc = np.random.default_rng(1).normal(size=(n, humanoid_model.nv)).astype(np.float32)
    f1, w1 = a.inverse(qacc, want_warnings=True)
    f2 = a.inverse(qacc, discrete=True)
    after = (a.get_state(spec), a.status(), a.counts())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert all(np.array_equal(x, y) for x, y in zip(before[2], after[2]))
    assert np.isfinite(f1).all() and np.isfinite(f2).all() and not w1.any()
    # step, inverse, step == step, step
    c = np.random.default_rng(2).uniform(-1, 1, size=(n, humanoid_model.nu)).astype(np.float32)
    x = hbmod.Batch(humanoid_model, n, gpu)
    y = hbmod.Batch(humanoid_model, n, gpu)
    for bb in (x, y):
        bb.set_state(hbmod.STATE_INTEGRATION, after[0][:, :x.state_size(hbmod.STATE_INTEGRATION)])
    x.step(c); x.inverse(qacc); x.step(c)
    y.step(c); y.step(c)
    assert np.array_equal(x.get_state(spec), y.get_state(spec)) and np.array_equal(x.status(), y.status())
    # a pipelined batch with held step_dev calls: the inverse runs behind them, on the state they leave
    p = hbmod.Batch(humanoid_model, n, gpu)
    u = hbmod.Batch(humanoid_model, n, gpu)
    p.pipeline(True)
    cd = p.dev_alloc(c.nbytes)
    p.to_dev(cd, c)
    for bb in (p, u):
        bb.set_state(hbmod.STATE_INTEGRATION, after[0][:, :x.state_size(hbmod.STATE_INTEGRATION)])
    n0 = p.step_launches()
    p.step_dev(cd); p.step_dev(cd)
    fp = p.inverse(qacc)
    assert p.step_launches() > n0
    u.step(c); u.step(c)
    assert np.array_equal(fp, u.inverse(qacc))
    assert np.array_equal(p.get_state(spec), u.get_state(spec))
    # the device entry point: same numbers, asynchronous
    qd, od = p.dev_alloc(qacc.nbytes), p.dev_alloc(qacc.nbytes)
    p.to_dev(qd, qacc)
    p.inverse_dev(qd, od)
    p.sync()
    assert np.array_equal(p.from_dev(od, qacc.shape), fp)
    with pytest.raises(hbmod.HbError):
        p.inverse_dev(0, od)  # (NULL qacc: HB_EINVAL)
    L = hbmod.lib()
    assert L.hb_inverse(p._h, None, 0, None, None) == -1 and L.hb_inverse(p._h, qacc.ctypes.data, 2, qacc.ctypes.data, None) == -1
    for ptr in (cd, qd, od):
        p.dev_free(ptr)


def test_overflow_warnings(hbmod, gpu, tmp_path):
    """overflow.xml: 30 contacts / 120 rows at rest, above the capacities; the per-env bits come back, the batch status stays"""
    p = _hbm(tmp_path, "overflow")
    m = hbmod.Model.load(p)
    b = hbmod.Batch(m, 4, gpu)
    b.reset()
    st = b.get_state(hbmod.STATE_INTEGRATION)
    st[2:, 3:1 + m.nq:7] += 5.0  # envs 2, 3: every raft lifted clear of the floor
    b.set_state(hbmod.STATE_INTEGRATION, st)
    s0 = b.status()
    f, w = b.inverse(np.zeros((4, m.nv), np.float32), want_warnings=True)
    assert np.array_equal(b.status(), s0)
    assert all(w[e] & hbmod.WARN_CONTACTFULL for e in (0, 1)) and not w[2:].any(), w
    assert not (w & ~(hbmod.WARN_CONTACTFULL | hbmod.WARN_CNSTRFULL)).any()
    assert np.isfinite(f).all()


def test_height_sweep(hbmod, humanoid_model, gpu):
    """The reference's set_mujoco_state (controllers/mpc_utils.py:36-56): keyframe, 200 root-height offsets, qacc = 0; the vertical
    force picks the height.  One inverse call of a 200-env batch."""
    n = 200
    offsets = np.linspace(-0.001, 0.001, n)
    b = hbmod.Batch(humanoid_model, n, gpu)
    b.reset(keyframe=0)
    st = b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
    st[:, 1 + 2] += offsets
    st[:, 1 + humanoid_model.nq:] = 0.0
    b.set_state(hbmod.STATE_INTEGRATION, st)
    fz = b.inverse(np.zeros((n, humanoid_model.nv), np.float32))[:, 2]
    st = b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
    o = Oracle()
    ref = np.empty(n)
    for e in range(n):
        forward_at(o, st[e, 1:1 + o.nq], np.zeros(o.nv))
        ref[e] = inverse_ref(o, np.zeros(o.nv))[2]
    scale = np.abs(ref).max()
    worst = np.abs(fz - ref).max() / scale
    print("height sweep: best offset %.3e (GPU) / %.3e (reference), worst |dfz| / max|fz| %.2e" % (offsets[np.argmin(np.abs(fz))], offsets[np.argmin(np.abs(ref))], worst))
    assert worst < 2e-5 and np.ptp(ref) > 0.1 * scale  # (measured: 5.2e-6)
    assert np.argmin(np.abs(fz)) == np.argmin(np.abs(ref))
