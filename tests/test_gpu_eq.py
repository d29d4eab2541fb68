"""Equality constraints on the GPU (step_body's FRIC == 2 instantiations, hb_step.hip: the hb_eq_* rows of HB_KERNELS) against the fp64
reference of tests/eq_ref.py: the oracle's forward pass with the equality and friction rows stacked in front.

Models: tests/eq_models.py.  States of the chains: every 10th of a 300-step reference rollout, rounded to fp32; tests/test_eq_cpu.py
holds the reference to things it does not define and checks what these state sets cover.  The bounds are bounds.BOUNDS,
test_gpu_inverse.py's, the contact-force read-out's and the free-running bound (tests/bounds.py): imported, never wider.
"""
import numpy as np
import pytest

import eq_ref
from bounds import BOUNDS, FREE_RUNNING_BOUND, CONTACT_DECODE_BOUND as DECODE_BOUND, CONTACT_PARITY_BOUND as PARITY_BOUND
from contact_ref import body_wrenches, contact_forces
from eq_models import (DISABLED_KERNEL, FOURBAR_BENT, MODELS, NE, SLIDER_A0, SLIDER_SOLIMP, SLIDER_SOLREF, add_equality, eq_chain_xml, eq_tmp,  # noqa: F401  (eq_tmp: a fixture)
                       fourbar_xml, geared_xml, plain_chain_xml, reference, scissors_xml, slider_xml)
from fric_models import add_friction
from inverse_ref import force_scale, forward_at
from kernel_models import chain_xml, oracle_for
from step_lib import T, diag_step, report, result, same


def _report(line):
    report(line, "HB_EQ_PARITY_OUT")  # (set to collect the lines of profiles/eq_parity.txt)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_one_step_against_the_reference(hbmod, gpu, eq_tmp, name):
    """Teacher-forced, diagnostics on: the expected kernel, counts and PGS sweep counts identical, qacc / efc_force / state / contacts
    within bounds.BOUNDS, status zero.  Worst deviations: profiles/eq_parity.txt."""
    p, o, st, ct, ref = reference(name, eq_tmp)
    m = hbmod.Model.load(p)
    assert m.equality_rows() == NE
    d = diag_step(hbmod, m, st, ct, gpu)
    assert d["kernel"] == MODELS[name][3], d["kernel"]
    assert not d["status"].any(), d["status"]
    worst = dict(qpos=0.0, qvel=0.0, qacc=0.0, force=0.0, dist=0.0, pos=0.0, frame=0.0)
    for k in range(len(st)):
        assert (d["ncon"][k], d["nefc"][k]) == (ref["ncon"][k], ref["nefc"][k]), (name, k, (d["ncon"][k], d["nefc"][k]), (ref["ncon"][k], ref["nefc"][k]))
        if MODELS[name][2] == "PGS":
            assert d["niter"][k] == ref["niter"][k] == 50, (name, k, d["niter"][k], ref["niter"][k])
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
        assert not d["force"][k, ne:].any()
    _report("%-18s %-24s ne %d nf %2d, rows <= %2d: %s" % (name, d["kernel"], NE, ref["nf"][0], max(ref["nefc"]), " ".join("%s %.2e" % kv for kv in worst.items())))
    for key, x in worst.items():
        assert x <= BOUNDS[key], (name, key, x, BOUNDS[key])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_inverse_dynamics(hbmod, gpu, eq_tmp, name):
    """hb_inverse on a model with equality rows, continuous and HB_INV_DISCRETE, by the equality kernel of its dense order: against the fp64
    restatement on random accelerations (the 1e-3 of test_gpu_inverse.py / test_gpu_kernel_matrix.py), and - Newton models - the
    round trips forward -> inverse (5e-5) and step -> inverse(discrete) (1e-3), which recover qfrc_actuator, and forward -> inverse
    with a wrench on two bodies, which recovers qfrc_actuator + J' xfrc_applied (5e-5; the oracle's qfrc_smooth - qfrc_passive +
    qfrc_bias under the same wrench).  The round trips need a converged forward solve: the Newton models."""
    p, o, st, ct, ref = reference(name, eq_tmp)
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
            t = eq_ref.inverse_ref(o, qacc[e].astype(np.float64), discrete)
            err.append(np.abs(got[e] - (t["Mqacc"] + t["bias"] - t["passive"] - t["constraint"])).max() / force_scale(t))
        _report("inverse %s discrete=%d: worst %.2e median %.2e" % (name, discrete, max(err), np.median(err)))
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
        _report("round trips %s: continuous worst %.2e, discrete worst %.2e" % (name, max(ec), max(ed)))
        assert max(ec) < 5e-5 and max(ed) < 1e-3, (name, max(ec), max(ed))
        # the same identity with xfrc_applied: a force and a torque on a link inside the loop and on the last link
        xfrc = np.zeros((n, m.nbody, 6), dtype=np.float32)
        xfrc[:, 4] = (0.5, -0.3, 0.8, 0.02, 0.01, -0.03)
        xfrc[:, m.nbody - 1] = (-0.2, 0.4, 0.3, 0.0, -0.02, 0.01)
        b.set_state(hbmod.STATE_INTEGRATION, zst)
        b.set_state(hbmod.STATE_XFRC_APPLIED, xfrc.reshape(n, -1))
        b.diag_enable(True)
        b.forward(ct)
        got = b.inverse(b.qacc())
        ex = []
        for e in range(n):
            o.reset()
            o.qpos[:] = qpos[e]; o.qvel[:] = qvel[e]; o.ctrl[:] = ct[e]; o.xfrc_applied[:] = xfrc[e].reshape(-1)
            o.forward()
            want = o.qfrc_smooth - o.qfrc_passive + o.qfrc_bias
            assert np.abs(want - o.qfrc_actuator).max() > 0.05  # (the wrench is in it)
            ex.append(np.abs(got[e] - want).max() / max(1.0, np.abs(o.qfrc_bias).max(), np.abs(want).max()))
        _report("round trip with xfrc_applied %s: worst %.2e" % (name, max(ex)))
        assert max(ex) < 5e-5, (name, max(ex))
    b.close()


@pytest.mark.gpu
def test_contact_force_readout(hbmod, gpu, eq_tmp):
    """the contact-force read-out of a PGS chain against the reference's decoded forces (rows shifted by ne + nf), within
    test_gpu_contact_force.py's bounds: the decode of the device's own rows, and parity with the reference's"""
    name = "eq28_cd3_pgs"
    p, o, st, ct, ref = reference(name, eq_tmp)
    m = hbmod.Model.load(p)
    d = diag_step(hbmod, m, st, ct, gpu, readout=True)
    assert d["kernel"] == "hb_eq_kernel"
    gb = o.info["geom_bodyid"]
    seen = 0
    for k in range(len(st)):
        nc, ne, con = ref["ncon"][k], ref["nefc"][k], ref["con"][k]
        assert (d["ncon"][k], d["nefc"][k]) == (nc, ne)
        if not nc:
            continue
        seen += 1
        assert all(c["efc_address"] < 0 or c["efc_address"] >= NE + ref["nf"][k] for c in con)
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
@pytest.mark.parametrize("name", ["eq28_cd3_pgs", "eq32_cd1_newton"])
def test_launch_shapes_are_bit_identical(hbmod, gpu, eq_tmp, name):
    """a plain step, T single step calls, a T-step rollout, the same rollout with sensors, and a pipelined batch of two segments: state,
    counts and status equal the diagnostic step's / the rollout's, by the same kernel (the env mask: test_a_masked_env_keeps_its_state)"""
    p, o, st, ct, ref = reference(name, eq_tmp)
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
    b.set_state(hbmod.STATE_INTEGRATION, st)
    sens = b.rollout_sensors(ctrlT, hbmod.Batch.sensor_spec(framepos_bodies=(1, m.nbody - 1), linvel_bodies=(2,)))
    same(result(hbmod, b), refT, name + " rollout with sensors")
    assert b.last_kernel() == kernel and np.isfinite(np.asarray(sens[0] if isinstance(sens, tuple) else sens)).all()
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
def test_a_masked_env_keeps_its_state(hbmod, gpu):
    """An env mask leaves skipped envs untouched.  hb_env_reset with reset_collision_mode = 2 steps every env once and then re-draws and
    steps, under an env mask, only the envs that ended in a self-collision (the scissors model: its two tip spheres overlap after
    about 40 % of the perturbed resets).  An env whose first draw stood is skipped by those later launches: its state, counts and
    status are the plain reset's advanced by one zero-control step, bit for bit; and the envs that were drawn again are exactly those
    whose first draw the plain batch sees colliding."""
    m, n = hbmod.Model.from_xml_string(scissors_xml()), 128
    assert m.equality_rows() == 4
    kw = dict(randomization_factor=1.0, auto_reset=0, max_time=0.0, target_z=10.0)
    a = hbmod.VecEnv(m, n, gpu, reset_collision_mode=2, **kw)
    a.reset()
    b = hbmod.VecEnv(m, n, gpu, **kw)
    b.reset()
    b.step_arrays(np.zeros((n, m.nu), np.float32))
    assert a.batch.last_kernel() == b.batch.last_kernel() == "hb_eq_kernel"
    sa, sb = a.batch.get_state(hbmod.STATE_INTEGRATION), b.batch.get_state(hbmod.STATE_INTEGRATION)
    first_draw = (sa == sb).all(axis=1)
    collided = b.batch.counts()[0] > 0  # (the plain batch's one step ran at the first draw: its contacts are that draw's)
    print("\n  %d envs kept their first draw, %d were re-drawn under a mask" % (first_draw.sum(), (~first_draw).sum()))
    assert (~first_draw).sum() >= 8 and first_draw.sum() >= 8
    assert np.array_equal(~first_draw, collided), (np.flatnonzero(~first_draw), np.flatnonzero(collided))
    for x, y in zip(a.batch.counts(), b.batch.counts()):
        assert np.array_equal(x[first_draw], y[first_draw])
    assert (a.batch.counts()[1] >= 4).all()  # (every env has its equality rows)
    assert not a.batch.status().any() and not b.batch.status().any() and np.isfinite(sa).all()
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["eq28_cd3_pgs", "eq28_cd1_newton"])
@pytest.mark.parametrize("how", ["flag", "inactive"])
def test_disabled_means_absent(hbmod, gpu, eq_tmp, name, how):
    """<flag equality="disable"/>, or active="false" on every element: the kernel the model runs without its <equality> section, by
    name, and bit for bit that model's result"""
    p, o, st, ct, ref = reference(name, eq_tmp)
    off = hbmod.Model.from_xml_string(eq_chain_xml(name, flag="disable") if how == "flag" else eq_chain_xml(name, inactive=True))
    plain = hbmod.Model.from_xml_string(plain_chain_xml(name))
    assert off.neq == 6 and off.equality_rows() == 0 and plain.neq == 0
    a, b = diag_step(hbmod, off, st, ct, gpu), diag_step(hbmod, plain, st, ct, gpu)
    assert a["kernel"] == b["kernel"] == DISABLED_KERNEL[name], (a["kernel"], b["kernel"])
    same(a["result"], b["result"], name + " " + how)
    assert np.array_equal(a["qacc"], b["qacc"]) and np.array_equal(a["force"], b["force"]) and np.array_equal(a["con"], b["con"])
    # (and with nothing always active at all: the kernel of a plain chain)
    nv, condim, solver = MODELS[name][:3]
    bare = hbmod.Model.from_xml_string(add_equality(chain_xml(nv, condim=condim, solver=solver), flag="disable"))
    bb = hbmod.Batch(bare, 4, gpu)
    bb.diag_enable(True)
    bb.step(np.zeros((4, bare.nu), dtype=np.float32))
    assert bb.last_kernel() == ("hb_step_kernel" if solver == "PGS" else "hb_step_newton28_kernel"), bb.last_kernel()
    bb.close()


def _small(hbmod, xml, tmp, name):
    m, _, o = oracle_for(hbmod, xml, tmp, name)
    return m, o


def _free_run(hbmod, gpu, m, o, q0, steps):
    """(device qpos trajectory [steps, nq] of env 0, reference trajectory) from rest at q0, no controls"""
    st = np.concatenate([[0.0], q0, np.zeros(2 * m.nv)])
    b = hbmod.Batch(m, 2, gpu)
    b.set_state(hbmod.STATE_INTEGRATION, np.tile(st.astype(np.float32), (2, 1)))
    q = b.rollout(np.zeros((steps, 2, m.nu), dtype=np.float32), want_qpos=True)
    assert b.last_kernel() == "hb_eq_newton28_kernel" and not b.status().any()
    assert np.array_equal(q[:, 0], q[:, 1])
    b.close()
    s = st.astype(np.float32).astype(np.float64)
    want = []
    for _ in range(steps):
        s, _, _ = eq_ref.step(o, s, np.zeros(m.nu))
        want.append(s[1:1 + m.nq])
    return q[:, 0].astype(np.float64), np.array(want)


@pytest.mark.gpu
def test_fourbar_stays_closed(hbmod, gpu, eq_tmp):
    """The four-bar released from a sheared pose under Newton, 400 steps: the anchor gap |p1 - p2| at every step stays at or below twice
    the largest gap of the reference's own rollout, the final qpos agrees with it within test_gpu_parity.py's free-running bound, and
    the linkage has moved"""
    m, o = _small(hbmod, fourbar_xml(), eq_tmp, "fourbar.hbm")
    got, want = _free_run(hbmod, gpu, m, o, np.array(FOURBAR_BENT), 400)
    gap_ref = max(eq_ref.anchor_gaps(o, q)[0] for q in want)
    gap_dev = max(eq_ref.anchor_gaps(o, q)[0] for q in got)
    drift = (np.abs(got[-1] - want[-1]) / np.maximum(1.0, np.abs(want[-1]))).max()
    _report("four-bar, 400 steps: largest anchor gap %.3e m (reference %.3e m), final qpos off by %.2e, crank moved %.2f rad" % (gap_dev, gap_ref, drift, abs(want[-1][0] - FOURBAR_BENT[0])))
    assert 0 < gap_ref < 5e-3 and np.abs(want[:, 0] - FOURBAR_BENT[0]).max() > 0.3
    assert gap_dev <= 2 * gap_ref, (gap_dev, gap_ref)
    assert drift <= FREE_RUNNING_BOUND, drift


@pytest.mark.gpu
def test_geared_pair_keeps_its_ratio(hbmod, gpu, eq_tmp):
    """two pendulums geared 1 : -2, released 0.6 / -0.3 rad from their reference: |dq1 + 2 dq2| under the four-bar's rule"""
    m, o = _small(hbmod, geared_xml(), eq_tmp, "geared.hbm")
    got, want = _free_run(hbmod, gpu, m, o, np.array([0.6, -0.3]), 400)
    v_ref, v_dev = np.abs(want[:, 0] + 2 * want[:, 1]).max(), np.abs(got[:, 0] + 2 * got[:, 1]).max()
    drift = (np.abs(got[-1] - want[-1]) / np.maximum(1.0, np.abs(want[-1]))).max()
    _report("geared pair, 400 steps: largest |dq1 + 2 dq2| %.3e rad (reference %.3e rad), final qpos off by %.2e" % (v_dev, v_ref, drift))
    assert 0 < v_ref < 2e-2 and np.abs(want[:, 0] - 0.6).max() > 0.3
    assert v_dev <= 2 * v_ref, (v_dev, v_ref)
    assert drift <= FREE_RUNNING_BOUND, drift


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["Newton", "PGS"])
def test_slider_closed_form(hbmod, gpu, solver):
    """one dof, one row: qacc = (1 - d) qacc_smooth + d aref on the device, d / K / B written out here (fp32: 1e-5 relative to the
    largest term of the sum)"""
    m = hbmod.Model.from_xml_string(slider_xml(solver))
    (tc, dr), (d0, d1, width, mid, power) = SLIDER_SOLREF, SLIDER_SOLIMP
    K, B = 1 / (d1 * d1 * tc * tc * dr * dr), 2 / (d1 * tc)
    qv = np.array([(0.0, 0.0), (0.03, 0.5), (0.045, -1.0), (-0.2, 0.3), (SLIDER_A0, 2.0)])
    b = hbmod.Batch(m, len(qv), gpu)
    b.diag_enable(True)
    b.set_state(hbmod.STATE_INTEGRATION, np.concatenate([np.zeros((len(qv), 1)), qv, np.zeros((len(qv), 1))], axis=1).astype(np.float32))
    b.forward()
    got = b.qacc()[:, 0].astype(np.float64)
    assert b.last_kernel() == ("hb_eq_newton28_kernel" if solver == "Newton" else "hb_eq_kernel") and (b.counts()[1] == 1).all()
    for k, (q, v) in enumerate(qv.astype(np.float32).astype(np.float64)):
        pos = q - SLIDER_A0
        x = abs(pos) / width
        y = 1.0 if x >= 1 else x * x / mid if x <= mid else 1 - (1 - x) ** 2 / (1 - mid)
        d = d0 + y * (d1 - d0)
        aref = -B * v - K * d * pos
        want = (1 - d) * -9.81 + d * aref
        assert abs(got[k] - want) <= 1e-5 * max(9.81, abs(aref)), (k, got[k], want)
    b.close()


@pytest.mark.gpu
def test_refusals(hbmod, gpu):
    """Each refusal names equality constraints (the compiler: what it does not support), nothing faults, and a batch that refused a
    read-out still steps"""
    eq = '<equality><joint joint1="j5" joint2="j9"/></equality>'
    for xml in (chain_xml(12, floor="hfield"), chain_xml(12, condim=6), chain_xml(12, condim=6, solver="Newton")):
        with pytest.raises(hbmod.HbError, match="equality constraints: only models that step in one kernel"):
            hbmod.Batch(hbmod.Model.from_xml_string(add_equality(xml, eq.replace("j9", "j3").replace("j5", "j1"))), 4, gpu)
    m = hbmod.Model.from_xml_string(add_equality(chain_xml(12), eq.replace("j9", "j3")))
    m.set_opt(integrator=hbmod.INT_RK4)
    with pytest.raises(hbmod.HbError, match="equality constraints: the RK4 integrator"):
        hbmod.Batch(m, 4, gpu)
    # 33 always-active rows: 13 friction rows of the nv = 32 chain and 20 locks
    locks = "<equality>" + "".join('<joint joint1="j%d"/>' % j for j in range(20)) + "</equality>"
    with pytest.raises(hbmod.HbError, match="20 equality rows and 13 friction-loss rows: a model may have at most 32"):
        hbmod.Batch(hbmod.Model.from_xml_string(add_equality(add_friction(chain_xml(32)), locks)), 4, gpu)
    ok = hbmod.Batch(hbmod.Model.from_xml_string(add_equality(add_friction(chain_xml(32)), locks.replace('<joint joint1="j19"/>', ""))), 4, gpu)  # (32 fit)
    ok.step(np.zeros((4, ok.model.nu), dtype=np.float32))
    assert ok.last_kernel() == "hb_eq32_kernel" and (ok.counts()[1] >= 32).all() and not ok.status().any()
    ok.close()
    with pytest.raises(hbmod.HbError, match="equality <weld> is not supported"):
        hbmod.Model.from_xml_string(add_equality(chain_xml(12), '<equality><weld body1="l1" body2="l2"/></equality>'))
    b = hbmod.Batch(m.__class__.from_xml_string(add_equality(chain_xml(12), eq.replace("j9", "j3"))), 4, gpu)
    c = np.zeros((4, b.model.nu), dtype=np.float32)
    with pytest.raises(hbmod.HbError, match="equality constraints"):
        b.body_acc_readout(True)
    b.step(c)
    with pytest.raises(hbmod.HbError, match="equality constraints"):
        b.sensors(hbmod.Batch.sensor_spec(framepos_bodies=(1,), imu=((1, (0, 0, 0)),)), c)
    b.step(c)
    assert b.last_kernel() == "hb_eq_kernel" and not b.status().any() and np.isfinite(b.qpos).all()
    b.close()


@pytest.mark.gpu
def test_env_adapter_runs_on_a_model_with_equalities(hbmod, gpu):
    """VecEnv on the nv = 28 chain with equalities: 20 steps, finite, status zero, by the equality kernel"""
    m = hbmod.Model.from_xml_string(eq_chain_xml("eq28_cd3_pgs"))
    env = hbmod.VecEnv(m, 16, gpu, seed=1)
    env.reset()
    rng = np.random.default_rng(0)
    for _ in range(20):
        obs, rew, done, info = env.step(rng.uniform(-1, 1, (16, m.nu)).astype(np.float32))
        assert np.isfinite(rew).all() and np.isfinite(obs).all()
    assert env.batch.last_kernel() == "hb_eq_kernel" and not env.batch.status().any()
    env.close()
