"""Joint friction loss on the GPU (step_body's FRIC instantiations, hb_step.hip: the FRIC rows of HB_KERNELS) against the fp64 reference of
tests/fric_ref.py: the oracle's forward pass with the friction rows stacked in front and the two-sided force bound.

Models: the capsule chains of tests/kernel_models.py at the two dense orders (nv 28 and 32), PGS condim 3 and Newton condim 1, with
frictionloss on every other joint in mixed magnitudes - some far above what a motor (gear 2) can push, so that the joint sticks, some far
below, so that it slips - and solreffriction / solimpfriction of their own on some.  States: every 10th of a 300-step reference
rollout, rounded to fp32.  tests/test_fric_cpu.py holds the reference to the oracle and checks what these state sets cover.
The bounds are bounds.BOUNDS, test_gpu_inverse.py's and the contact-force read-out's (tests/bounds.py): imported, never wider.
"""
import numpy as np
import pytest

import fric_ref
from bounds import BOUNDS, CONTACT_DECODE_BOUND as DECODE_BOUND, CONTACT_PARITY_BOUND as PARITY_BOUND
from contact_ref import body_wrenches, contact_forces
from fric_models import MODELS, PLAIN_KERNEL, add_friction, fric_chain_xml, fric_tmp, pendulum_xml, reference  # noqa: F401  (fric_tmp: a fixture)
from inverse_ref import force_scale, forward_at
from kernel_models import chain_xml
from oracle_lib import Oracle
from step_lib import T, diag_step, report, result, same


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_one_step_against_the_reference(hbmod, gpu, fric_tmp, name):
    """Teacher-forced, diagnostics on: the expected kernel, counts and PGS sweep counts identical, qacc / efc_force / state / contacts
    within bounds.BOUNDS, friction-row forces inside their bound, status zero.  Worst deviations: profiles/fric_parity.txt."""
    p, o, st, ct, ref = reference(name, fric_tmp)
    m = hbmod.Model.load(p)
    d = diag_step(hbmod, m, st, ct, gpu)
    assert d["kernel"] == MODELS[name][3], d["kernel"]
    assert not d["status"].any(), d["status"]
    fr = fric_ref.friction_rows(o)
    nf = len(fr["dof"])
    assert nf > 0
    worst = dict(qpos=0.0, qvel=0.0, qacc=0.0, force=0.0, dist=0.0, pos=0.0, frame=0.0, bound=0.0)
    for k in range(len(st)):
        assert (d["ncon"][k], d["nefc"][k]) == (ref["ncon"][k], ref["nefc"][k]), (name, k, (d["ncon"][k], d["nefc"][k]), (ref["ncon"][k], ref["nefc"][k]))
        if MODELS[name][2] == "PGS":
            assert d["niter"][k] == ref["niter"][k], (name, k, d["niter"][k], ref["niter"][k])
        ne = ref["nefc"][k]
        for i, c in enumerate(ref["con"][k]):
            r = d["con"][k, i]
            assert (int(r[14]), int(r[15])) == (c["geom1"], c["geom2"]), (name, k, i)
            worst["dist"] = max(worst["dist"], abs(r[0] - c["dist"]))
            worst["pos"] = max(worst["pos"], np.abs(r[1:4] - c["pos"]).max())
            worst["frame"] = max(worst["frame"], np.abs(r[4:13] - c["frame"].reshape(-1)).max())
        worst["qacc"] = max(worst["qacc"], np.abs(d["qacc"][k] - ref["qacc"][k]).max() / max(1.0, np.abs(ref["qacc"][k]).max()))
        worst["force"] = max(worst["force"], np.abs(d["force"][k, :ne] - ref["force"][k]).max() / max(1.0, np.abs(ref["force"][k]).max()))
        worst["qpos"] = max(worst["qpos"], (np.abs(d["qpos"][k] - ref["qpos"][k]) / np.maximum(1.0, np.abs(ref["qpos"][k]))).max())
        worst["qvel"] = max(worst["qvel"], np.abs(d["qvel"][k] - ref["qvel"][k]).max() / max(1.0, np.abs(ref["qvel"][k]).max()))
        worst["bound"] = max(worst["bound"], (np.abs(d["force"][k, :nf]) / fr["fl"]).max())
        assert not d["force"][k, ne:].any()
    line = "%-20s %-26s nf %2d, rows <= %2d: %s" % (name, d["kernel"], nf, max(ref["nefc"]), " ".join("%s %.2e" % kv for kv in worst.items()))
    report(line, "HB_FRIC_PARITY_OUT")  # (set to collect the lines of profiles/fric_parity.txt)
    assert worst.pop("bound") <= 1.0 + 1e-6
    for key, x in worst.items():
        assert x <= BOUNDS[key], (name, key, x, BOUNDS[key])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_launch_shapes_are_bit_identical(hbmod, gpu, fric_tmp, name):
    """a plain step (the lean request falls back to the friction kernel), T single step calls, a T-step rollout and a pipelined batch of
    two segments with fold at its default: state, counts and status equal the diagnostic step's / the rollout's, by the same kernel"""
    p, o, st, ct, ref = reference(name, fric_tmp)
    m = hbmod.Model.load(p)
    kernel = MODELS[name][3]
    n = len(st)
    ref1 = diag_step(hbmod, m, st, ct, gpu)["result"]
    ctrlT = np.random.default_rng(5).uniform(-1, 1, (T, n, m.nu)).astype(np.float32)
    ctrlT[0] = ct
    b = hbmod.Batch(m, n, gpu)
    b.set_state(hbmod.STATE_INTEGRATION, st); b.step(ct)
    same(result(hbmod, b), ref1, name + " step")
    assert b.last_kernel() == kernel
    b.set_state(hbmod.STATE_INTEGRATION, st)
    b.rollout(ctrlT)
    refT = result(hbmod, b)
    assert b.last_kernel() == kernel and not refT[2].any()
    b.set_state(hbmod.STATE_INTEGRATION, st)
    for t in range(T):
        b.step(ctrlT[t])
    same(result(hbmod, b), refT, name + " steps")
    assert b.last_kernel() == kernel
    b.close()
    # two segments: the library cuts a batch into segments of at least 64 envs, so the states are tiled to 128 (the only batch here above 64)
    idx = np.arange(128) % n
    res = []
    for pipe in (0, 2):
        b = hbmod.Batch(m, 128, gpu)
        if pipe:
            b.pipeline(pipe)
        b.set_state(hbmod.STATE_INTEGRATION, st[idx])
        for t in range(T):
            b.step(ctrlT[t][idx])
        b.join()
        assert b.segments == (pipe or 1), b.segments
        res.append(result(hbmod, b))
        assert b.last_kernel() == kernel
        b.close()
    same(res[1], res[0], name + " pipelined")
    assert np.array_equal(res[0][0][:n], refT[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fric28_cd3_pgs", "fric28_cd1_newton"])
@pytest.mark.parametrize("how", ["flag", "zero"])
def test_disabled_or_zero_friction_is_an_ordinary_model(hbmod, gpu, tmp_path, name, how):
    """<flag frictionloss="disable"/>, or frictionloss 0 on every joint: today's kernel by name, and the oracle's own step within BOUNDS"""
    from kernel_models import oracle_steps, rollout_states
    xml = fric_chain_xml(name, flag="disable") if how == "flag" else fric_chain_xml(name, value=0.0)
    m = hbmod.Model.from_xml_string(xml)
    p = str(tmp_path / "m.hbm")
    m.save(p)
    o = Oracle(p)
    st, ct = rollout_states(o, steps=100)
    ref = oracle_steps(o, st, ct)
    d = diag_step(hbmod, m, st, ct, gpu)
    assert d["kernel"] == PLAIN_KERNEL[name], d["kernel"]
    assert not d["status"].any()
    for k in range(len(st)):
        assert (d["ncon"][k], d["nefc"][k]) == (ref["ncon"][k], ref["nefc"][k])
        ne = ref["nefc"][k]
        assert np.abs(d["qacc"][k] - ref["qacc"][k]).max() / max(1.0, np.abs(ref["qacc"][k]).max()) <= BOUNDS["qacc"]
        if ne:
            assert np.abs(d["force"][k, :ne] - ref["force"][k]).max() / max(1.0, np.abs(ref["force"][k]).max()) <= BOUNDS["force"]
        assert (np.abs(d["qpos"][k] - ref["qpos"][k]) / np.maximum(1.0, np.abs(ref["qpos"][k]))).max() <= BOUNDS["qpos"]
        assert np.abs(d["qvel"][k] - ref["qvel"][k]).max() / max(1.0, np.abs(ref["qvel"][k]).max()) <= BOUNDS["qvel"]


@pytest.mark.gpu
def test_stick_and_slip(hbmod, gpu):
    """No reference needed.  The horizontal pendulum (gravity torque 1.962 N m) held by frictionloss 2.5 moves less than 1e-3 rad in 500
    steps; with frictionloss 1 it starts at (tau_g - fl) / I.  A chain with frictionloss 5 on every hinge and no controls keeps its joint
    angles within 1e-2 rad over 300 steps while it falls and lands: the 12-dof chain with a friction impedance of 0.999, for which the
    fp64 reference gives 2.2e-4 rad.  (Friction loss is a soft constraint: a held joint creeps at tau R / B, 2.3e-2 rad on this chain
    with MuJoCo's default impedance of 0.9; and the landing of the 28-dof chain takes its inner hinges past 5 N m - the reference gives
    0.112 rad there with the default impedance, 0.073 with 0.999, and the device 0.112.  Neither is a kernel's doing.)"""
    for sign in (1, -1):
        m = hbmod.Model.from_xml_string(pendulum_xml(2.5, sign))
        b = hbmod.Batch(m, 2, gpu)
        for _ in range(500):
            b.step(np.zeros((2, 0), dtype=np.float32))
        assert np.abs(b.qpos).max() < 1e-3, b.qpos
        assert b.last_kernel() == "hb_fric_newton28_kernel" and not b.status().any()
        b.close()
        m = hbmod.Model.from_xml_string(pendulum_xml(1.0, sign))
        b = hbmod.Batch(m, 2, gpu)
        b.diag_enable(True)
        b.step(np.zeros((2, 0), dtype=np.float32))
        I = m.array("dof_M0")[0]
        want = sign * (0.5 * 0.4 * 9.81 - 1.0) / I  # (+x arm: gravity turns it about +y, qacc > 0)
        assert np.abs(b.qacc()[:, 0] - want).max() <= 1e-3 * abs(want), (b.qacc(), want)
        b.close()
    m = hbmod.Model.from_xml_string(add_friction(chain_xml(12), value=5.0, solimp=0.999))
    b = hbmod.Batch(m, 4, gpu)
    q0 = b.qpos.copy()
    zc = np.zeros((4, m.nu), dtype=np.float32)
    z0 = b.qpos[:, 2].copy()
    for _ in range(300):
        b.step(zc)
    jtype = m.array("jnt_type").astype(int)
    hinge_q = [int(a) for a, t in zip(m.array("jnt_qposadr"), jtype) if t == 3]
    assert np.abs(b.qpos[:, hinge_q] - q0[:, hinge_q]).max() < 1e-2
    assert (b.qpos[:, 2] < z0 - 0.02).all() and b.counts()[0].min() > 0 and not b.status().any()  # (fell, and lies on the floor)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_inverse_dynamics(hbmod, gpu, fric_tmp, name):
    """hb_inverse on a friction model, continuous and HB_INV_DISCRETE, by the friction kernel of its dense order: against the fp64
    restatement on random accelerations (the 1e-3 of test_gpu_inverse.py / test_gpu_kernel_matrix.py), and - Newton models - the
    round trips forward -> inverse (5e-5) and step -> inverse(discrete) (1e-3), which recover qfrc_actuator"""
    p, o, st, ct, ref = reference(name, fric_tmp)
    m = hbmod.Model.load(p)
    nq, nv, n = m.nq, m.nv, len(st)
    qpos, qvel = st[:, 1:1 + nq].astype(np.float32), st[:, 1 + nq:1 + nq + nv].astype(np.float32)
    zst = np.concatenate([np.zeros((n, 1)), qpos, qvel, np.zeros_like(qvel)], axis=1)
    b = hbmod.Batch(m, n, gpu)
    b.set_state(hbmod.STATE_INTEGRATION, zst)
    qacc = np.random.default_rng(7).normal(size=qvel.shape).astype(np.float32) * 5.0
    for discrete in (False, True):
        got = b.inverse(qacc, discrete=discrete)
        assert b.last_kernel() == MODELS[name][4], b.last_kernel()
        err = []
        for e in range(n):
            forward_at(o, qpos[e].astype(np.float64), qvel[e].astype(np.float64))
            t = fric_ref.inverse_ref(o, qacc[e].astype(np.float64), discrete)
            err.append(np.abs(got[e] - (t["Mqacc"] + t["bias"] - t["passive"] - t["constraint"])).max() / force_scale(t))
        print("inverse %s discrete=%d: worst %.2e median %.2e" % (name, discrete, max(err), np.median(err)))
        assert max(err) < 1e-3, (name, discrete, max(err))
    if MODELS[name][2] == "Newton":
        b.diag_enable(True)
        b.forward(ct)
        got = b.inverse(b.qacc())
        b.diag_enable(False)
        b.set_state(hbmod.STATE_INTEGRATION, zst)
        b.step(ct)
        qd = ((b.qvel.astype(np.float64) - qvel) / m.opt.timestep).astype(np.float32)
        b.set_state(hbmod.STATE_INTEGRATION, zst)
        gotd = b.inverse(qd, discrete=True)
        ec, ed = [], []
        for e in range(n):
            forward_at(o, qpos[e].astype(np.float64), qvel[e].astype(np.float64), ct[e].astype(np.float64))
            s = max(1.0, np.abs(o.qfrc_bias).max(), np.abs(o.qfrc_actuator).max())
            ec.append(np.abs(got[e] - o.qfrc_actuator).max() / s)
            ed.append(np.abs(gotd[e] - o.qfrc_actuator).max() / s)
        print("round trips %s: continuous worst %.2e, discrete worst %.2e" % (name, max(ec), max(ed)))
        assert max(ec) < 5e-5 and max(ed) < 1e-3, (name, max(ec), max(ed))
    b.close()


@pytest.mark.gpu
def test_contact_force_readout(hbmod, gpu, fric_tmp):
    """the contact-force read-out of the PGS model against the reference's decoded forces (rows shifted by the friction rows), within
    test_gpu_contact_force.py's bounds: the decode of the device's own rows, and parity with the reference's"""
    name = "fric28_cd3_pgs"
    p, o, st, ct, ref = reference(name, fric_tmp)
    m = hbmod.Model.load(p)
    d = diag_step(hbmod, m, st, ct, gpu, readout=True)
    assert d["kernel"] == "hb_fric_kernel"
    gb = o.info["geom_bodyid"]
    seen = 0
    for k in range(len(st)):
        nc, ne, con = ref["ncon"][k], ref["nefc"][k], ref["con"][k]
        assert (d["ncon"][k], d["nefc"][k]) == (nc, ne)
        if not nc:
            continue
        seen += 1
        dcon = [dict(c, pos=d["con"][k, i, 1:4], frame=d["con"][k, i, 4:13].reshape(3, 3)) for i, c in enumerate(con)]
        s = max(1.0, np.abs(d["force"][k, :ne]).max())
        f = contact_forces(d["force"][k, :ne], dcon)
        w = body_wrenches(f, dcon, gb, ref["xipos"][k], o.nbody)
        assert np.abs(d["cf"][k, :nc] - f).max() / s <= DECODE_BOUND and np.abs(d["bc"][k] - w).max() / s <= DECODE_BOUND, (k, "decode")
        s = max(1.0, np.abs(ref["force"][k]).max())
        f = contact_forces(ref["force"][k], con)
        w = body_wrenches(f, con, gb, ref["xipos"][k], o.nbody)
        assert np.abs(d["cf"][k, :nc] - f).max() / s <= PARITY_BOUND and np.abs(d["bc"][k] - w).max() / s <= PARITY_BOUND, (k, "parity")
        assert not d["cf"][k, nc:].any()
    assert seen >= 10


@pytest.mark.gpu
def test_refusals(hbmod, gpu):
    """Each refusal names friction loss, nothing faults, and a batch that refused a read-out still steps"""
    for xml in (add_friction(chain_xml(12, floor="hfield")), add_friction(chain_xml(12, condim=6)), add_friction(chain_xml(12, condim=6, solver="Newton"))):
        with pytest.raises(hbmod.HbError, match="friction loss"):
            hbmod.Batch(hbmod.Model.from_xml_string(xml), 4, gpu)
    m = hbmod.Model.from_xml_string(add_friction(chain_xml(12)))
    m.set_opt(integrator=hbmod.INT_RK4)
    with pytest.raises(hbmod.HbError, match="friction loss"):
        hbmod.Batch(m, 4, gpu)
    m = hbmod.Model.from_xml_string(add_friction(chain_xml(12)))
    b = hbmod.Batch(m, 4, gpu)
    c = np.zeros((4, m.nu), dtype=np.float32)
    with pytest.raises(hbmod.HbError, match="friction loss"):
        b.body_acc_readout(True)
    b.step(c)
    with pytest.raises(hbmod.HbError, match="friction loss"):
        b.sensors(hbmod.Batch.sensor_spec(framepos_bodies=(1,), imu=((1, (0, 0, 0)),)), c)
    b.step(c)
    assert b.last_kernel() == "hb_fric_kernel" and not b.status().any() and np.isfinite(b.qpos).all()
    b.close()


@pytest.mark.gpu
def test_env_adapter_runs_on_a_friction_model(hbmod, gpu):
    """VecEnv on the nv = 28 friction chain: 20 steps, finite rewards, by the friction kernel (the adapter reads the joint torques)"""
    m = hbmod.Model.from_xml_string(fric_chain_xml("fric28_cd3_pgs"))
    env = hbmod.VecEnv(m, 16, gpu, seed=1)
    env.reset()
    rng = np.random.default_rng(0)
    for _ in range(20):
        obs, rew, done, info = env.step(rng.uniform(-1, 1, (16, m.nu)).astype(np.float32))
        assert np.isfinite(rew).all() and np.isfinite(obs).all()
    assert env.batch.last_kernel() == "hb_fric_kernel"
    env.close()
