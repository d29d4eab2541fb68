"""The dynamics read-out (include/hb.h: hb_dynamics*; csrc/hb_dyn.hip) on the GPU against the fp64 oracle's mass matrix, bias and passive
forces and the Jacobians built from its kinematics (tests/dyn_ref.py), and its contract as a pure function of the state: the same bits
whatever the packing, the batch size, a state's place in a wave or the form of the call, nothing of the batch written.

Bounds (bounds.DYN_BOUND; errors relative to max(1, max |reference|) of the quantity in the state): the project's convention, 3 x the maxima of
profiles/dynamics_parity.txt (tools/gpu_dynamics_report.py, the same cases and the same sixteen points), rounded down.  All maxima are
far below the 4e-4 qacc bound of tests/test_gpu_parity.py.
    M             measured maximum 2.814e-7 (chain32),    3 x = 8.442e-7  -> 8.44e-7
    qfrc_bias     measured maximum 1.675e-6 (team_robot), 3 x = 5.026e-6  -> 5.02e-6
    qfrc_passive  measured maximum 6.825e-8 (bush32),     3 x = 2.047e-7  -> 2.04e-7
    Jacobians     measured maximum 5.563e-7 (bush32),     3 x = 1.669e-6  -> 1.66e-6

The cross-API identities propagate these bounds through the products they form (each test's docstring says how).
"""
import ctypes
import itertools
import os

import numpy as np
import pytest

import dr_ref
import dyn_ref
import kin_ref
from bounds import DYN_BOUND as BOUND
from bounds import VEL_BOUND  # the velocities of Batch.kinematics against the same oracle
from oracle_lib import ASSETS, HUMANOID_HBM, load_state
from step_lib import same_dict, snapshot

pytestmark = pytest.mark.gpu

QUANT = ("M", "bias", "passive", "jac")

_cache = {}


def _case(hbmod, name, tmp_path_factory):
    """dyn_ref.parity_case(name), its sixteen points and its references, computed once per session and left unchanged"""
    if name not in _cache:
        m, o, kernel, states = dyn_ref.parity_case(hbmod, name, tmp_path_factory.mktemp(name))
        spec = m.jac_spec(**dyn_ref.default_points(hbmod, m))
        ref = dyn_ref.references(o, states, dyn_ref.spec_points(spec))
        for a in ref.values():
            a.setflags(write=False)
        states.setflags(write=False)
        _cache[name] = (m, o, kernel, states, spec, ref)
    return _cache[name]


def _readout(hbmod, m, states, spec, gpu, **tune):
    b = hbmod.Batch(m, len(states), gpu)
    if tune:
        b.tune(**tune)
    b.set_state(hbmod.STATE_INTEGRATION, np.asarray(states))
    out = b.dynamics(jac=spec)
    kernel = b.last_kernel()
    b.close()
    return out, kernel


@pytest.mark.parametrize("name", kin_ref.CASES)
def test_parity(hbmod, gpu, tmp_path_factory, name):
    """every state of every case inside the four bounds, on the kernel the model's size asks for; M symmetric bit for bit"""
    m, o, kernel, states, spec, ref = _case(hbmod, name, tmp_path_factory)
    dev, ran = _readout(hbmod, m, states, spec, gpu)
    assert ran == kernel
    n, nv = len(states), m.nv
    assert dev["M"].shape == (n, nv, nv) and dev["bias"].shape == dev["passive"].shape == (n, nv) and dev["jac"].shape == (n, 16, 6, nv)
    err = {q: max(dyn_ref.errors(ref, dev, k)[q] for k in range(n)) for q in QUANT}
    print("%s: %s" % (name, " ".join("%s %.3g" % kv for kv in err.items())))
    for q in QUANT:
        assert err[q] <= BOUND[q], (name, q, err[q])
    assert np.array_equal(dev["M"], dev["M"].transpose(0, 2, 1))


@pytest.mark.parametrize("name", ["humanoid27", "bush17"])
def test_packing_and_place_are_bit_identical(hbmod, gpu, tmp_path_factory, name):
    """kin_pack 1 against 0; n = 1 and n = 64 / L + 1 (a wave part filled); the same state in every slot of a wave"""
    m, o, kernel, states, spec, ref = _case(hbmod, name, tmp_path_factory)
    per = 64 // int(kernel[6:8])
    packed, k1 = _readout(hbmod, m, states, spec, gpu)
    plain, k0 = _readout(hbmod, m, states, spec, gpu, kin_pack=0)
    assert (k1, k0) == (kernel, "hb_dyn64_kernel")
    same_dict(packed, plain, "kin_pack")
    for n in (1, per + 1):
        out, _ = _readout(hbmod, m, states[:n], spec, gpu)
        same_dict(out, {k: a[:n] for k, a in packed.items()}, "n %d" % n)
    qpos, qvel = kin_ref.split_state(o, states)
    b = hbmod.Batch(m, 2, gpu)
    for k in (0, 7):
        rep = b.dynamics_states(np.tile(qpos[k], (2 * per + 1, 1)), np.tile(qvel[k], (2 * per + 1, 1)), jac=spec)
        for q in QUANT:
            assert all(np.array_equal(rep[q][i], packed[q][k]) for i in range(2 * per + 1)), (k, q)
    b.close()


def test_forms_agree(hbmod, gpu, tmp_path_factory):
    """the _states form on get_state(), the _dev forms, and every subset of the outputs give the bits of the full host call"""
    m, o, _, states, spec, _ = _case(hbmod, "humanoid27", tmp_path_factory)
    n = 7
    b = hbmod.Batch(m, n, gpu)
    b.set_state(hbmod.STATE_INTEGRATION, np.asarray(states[:n]))
    full = b.dynamics(jac=spec)
    st = b.get_state(hbmod.STATE_INTEGRATION)
    qpos, qvel = st[:, 1:1 + m.nq].copy(), st[:, 1 + m.nq:1 + m.nq + m.nv].copy()
    same_dict(b.dynamics_states(qpos, qvel, jac=spec), full, "dynamics_states on get_state")
    tape = b.dynamics_states(np.stack([qpos, qpos[::-1]]), np.stack([qvel, qvel[::-1]]), jac=spec)
    assert tape["M"].shape == (2, n, m.nv, m.nv) and tape["jac"].shape == (2, n, 16, 6, m.nv)
    same_dict({k: a[1, ::-1] for k, a in tape.items()}, full, "leading shape")
    nov = b.dynamics_states(qpos, None, bias=False, passive=False, jac=spec)
    same_dict(nov, {k: full[k] for k in ("M", "jac")}, "qvel=None")
    for r in range(1, 4):
        for keep in itertools.combinations(QUANT, r):
            kw = dict(M="M" in keep, bias="bias" in keep, passive="passive" in keep, jac=spec if "jac" in keep else None)
            same_dict(b.dynamics(**kw), {k: full[k] for k in QUANT if k in keep}, "subset %s" % (keep,))
            same_dict(b.dynamics_states(qpos, qvel, **kw), {k: full[k] for k in QUANT if k in keep}, "states subset %s" % (keep,))
    # device forms
    ptr = {k: b.dev_alloc(full[k].nbytes) for k in QUANT}
    b.dynamics_dev(ptr["M"], ptr["bias"], ptr["passive"], spec, ptr["jac"])
    b.sync()
    same_dict({k: b.from_dev(ptr[k], full[k].shape) for k in QUANT}, full, "dynamics_dev")
    dq, dv = b.dev_alloc(qpos.nbytes), b.dev_alloc(qvel.nbytes)
    b.to_dev(dq, qpos); b.to_dev(dv, qvel)
    for k in QUANT:
        b.to_dev(ptr[k], np.zeros_like(full[k]))
    b.dynamics_states_dev(dq, dv, n, ptr["M"], ptr["bias"], ptr["passive"], spec, ptr["jac"])
    b.sync()
    same_dict({k: b.from_dev(ptr[k], full[k].shape) for k in QUANT}, full, "dynamics_states_dev")
    for p in list(ptr.values()) + [dq, dv]:
        b.dev_free(p)
    b.close()


def test_pure_function(hbmod, gpu, tmp_path_factory):
    """nothing of the batch is written (state with its warm start, status, counts, the step launches counted, the last step's results),
    the batch steps on as its twin does, and a free joint's quaternion is normalised for the computation only"""
    m, o, _, states, spec, ref = _case(hbmod, "humanoid27", tmp_path_factory)
    n = 8
    ctrl = np.random.default_rng(2).uniform(-1, 1, (n, m.nu)).astype(np.float32)
    a, twin = hbmod.Batch(m, n, gpu), hbmod.Batch(m, n, gpu)
    for b in (a, twin):
        b.diag_enable(True)
        b.set_state(hbmod.STATE_INTEGRATION, np.asarray(states[:n]))
        b.step(ctrl)
    before = snapshot(hbmod, a, extra=[a.qpos.copy(), a.qvel.copy(), a.qacc(), a.efc_force()])
    a.dynamics(jac=spec)
    for x, y in zip(before, snapshot(hbmod, a, extra=[a.qpos.copy(), a.qvel.copy(), a.qacc(), a.efc_force()])):
        assert np.array_equal(x, y)
    for b in (a, twin):
        b.step(ctrl)
    assert np.array_equal(a.get_state(hbmod.STATE_INTEGRATION), twin.get_state(hbmod.STATE_INTEGRATION))
    a.close(); twin.close()
    b = hbmod.Batch(m, 1, gpu)
    s = np.array(states[:1])
    s[0, 4:8] *= 1.3
    b.set_state(hbmod.STATE_INTEGRATION, s)
    out = b.dynamics(jac=spec)
    err = dyn_ref.errors(ref, out, 0)
    assert all(err[q] <= BOUND[q] for q in QUANT), err
    assert np.array_equal(b.get_state(hbmod.STATE_INTEGRATION)[0, 4:8], s[0, 4:8].astype(np.float32))
    b.close()


def test_held_steps_come_first(hbmod, gpu, tmp_path_factory):
    """after hb_step_dev calls on a pipelined, folding batch dynamics() sees the state those steps leave: get_state fed to dynamics_states"""
    m, o, _, states, spec, _ = _case(hbmod, "humanoid27", tmp_path_factory)
    n = 256
    big = np.tile(states, (9, 1))[:n]
    ctrl = np.random.default_rng(3).uniform(-1, 1, (n, m.nu)).astype(np.float32)
    b = hbmod.Batch(m, n, gpu)
    b.pipeline(True)
    b.set_state(hbmod.STATE_INTEGRATION, big)
    d = b.dev_alloc(ctrl.nbytes)
    b.to_dev(d, ctrl)
    n0 = b.step_launches()
    for _ in range(3):
        b.step_dev(d)
    out = b.dynamics(jac=spec)
    assert b.last_kernel() == "hb_dyn16_kernel"
    launches = b.step_launches() - n0
    st = b.get_state(hbmod.STATE_INTEGRATION)
    assert launches >= 1 and b.step_launches() - n0 == launches  # (the read-out is not counted)
    assert not np.array_equal(st[:, 1:1 + m.nq], big[:, 1:1 + m.nq].astype(np.float32))
    same_dict(b.dynamics_states(st[:, 1:1 + m.nq].copy(), st[:, 1 + m.nq:1 + m.nq + m.nv].copy(), jac=spec), out, "held step calls")
    b.dev_free(d)
    b.close()


def test_jacobians_give_the_kinematics_velocities(hbmod, gpu, tmp_path_factory):
    """jac(body_com) @ qvel against Batch.kinematics()["vel"], both on the device.  Propagation: the Jacobian is within JAC = BOUND["jac"]
    max(1, max |J|) of the true one entry by entry, so its product with qvel is within JAC sum |qvel| of the true velocity; the
    kinematics read-out is within VEL_BOUND max(1, max |vel|) of it (tests/test_gpu_kinematics.py); the product itself is formed in fp64."""
    m, o, _, states, _, _ = _case(hbmod, "humanoid27", tmp_path_factory)
    assert m.nbody == 17
    spec = m.jac_spec(body_coms=range(1, 17))
    b = hbmod.Batch(m, len(states), gpu)
    b.set_state(hbmod.STATE_INTEGRATION, np.asarray(states))
    J = b.dynamics(M=False, bias=False, passive=False, jac=spec)["jac"].astype(np.float64)
    vel = b.kinematics()["vel"].astype(np.float64)
    qvel = b.qvel.astype(np.float64)
    b.close()
    worst = 0.0
    for k in range(len(states)):
        v = J[k] @ qvel[k]  # [16, 6] = linear | angular
        tol = BOUND["jac"] * max(1.0, np.abs(J[k]).max()) * np.abs(qvel[k]).sum() + VEL_BOUND * max(1.0, np.abs(vel[k]).max())
        err = max(np.abs(v[:, 0:3] - vel[k, 1:, 3:6]).max(), np.abs(v[:, 3:6] - vel[k, 1:, 0:3]).max())
        worst = max(worst, err / tol)
        assert err <= tol, (k, err, tol)
    print("jac @ qvel against kinematics: worst error / bound %.3f" % worst)


def test_equation_of_motion_against_inverse(hbmod, gpu, tmp_path_factory):
    """M qacc + qfrc_bias - qfrc_passive against Batch.inverse(qacc) for the qacc of forward(), contacts and limits switched off (no
    constraint force).  Propagation: each term of the read-out is within its parity bound of the true term - M qacc within BOUND["M"]
    max(1, max |M|) sum |qacc|, the other two within BOUND[.] max(1, max |.|) - and the inverse kernel forms the same three terms in
    the same precision from the same kinematics, so it is held to the same sum: twice the sum in all; the products are formed in fp64."""
    _, o, _, states, _, _ = _case(hbmod, "humanoid27", tmp_path_factory)
    m = hbmod.Model.load(HUMANOID_HBM)
    m.set_opt(disableflags=m.opt.disableflags | (1 << 4) | (1 << 3))  # mjDSBL_CONTACT, mjDSBL_LIMIT
    n = len(states)
    b = hbmod.Batch(m, n, gpu)
    b.set_state(hbmod.STATE_INTEGRATION, np.asarray(states))
    b.diag_enable(True)
    b.forward(np.random.default_rng(4).uniform(-1, 1, (n, m.nu)).astype(np.float32))
    nc, ne, _ = b.counts()
    assert not nc.any() and not ne.any()
    qacc = b.qacc()
    inv = b.inverse(qacc).astype(np.float64)
    d = {k: a.astype(np.float64) for k, a in b.dynamics().items()}
    b.close()
    worst = 0.0
    for k in range(n):
        a = qacc[k].astype(np.float64)
        lhs = d["M"][k] @ a + d["bias"][k] - d["passive"][k]
        tol = 2 * (BOUND["M"] * max(1.0, np.abs(d["M"][k]).max()) * np.abs(a).sum() + BOUND["bias"] * max(1.0, np.abs(d["bias"][k]).max())
                   + BOUND["passive"] * max(1.0, np.abs(d["passive"][k]).max()))
        err = np.abs(lhs - inv[k]).max()
        worst = max(worst, err / tol)
        assert err <= tol, (k, err, tol)
    print("M qacc + bias - passive against inverse: worst error / bound %.3f" % worst)


def test_per_env_parameters(hbmod, gpu, tmp_path_factory):
    """with hb_env_domain_randomize installed every env's M, qfrc_bias, qfrc_passive and subtree-COM Jacobians are those of the oracle
    carrying that env's masses, armature and stiffness (dr_ref.apply); the _states form keeps the nominal model"""
    m, o, _, states, spec, ref = _case(hbmod, "humanoid27", tmp_path_factory)
    n = 16
    b = hbmod.Batch(m, n, gpu)
    b.env_domain_randomize(dr_ref.family("all", seed=9))
    P = b.env_domain_params()
    L = dr_ref.layout(m, P.shape[1])
    b.set_state(hbmod.STATE_INTEGRATION, np.asarray(states[:n]))
    dev = b.dynamics(jac=spec)
    qpos, qvel = kin_ref.split_state(o, states[:n])
    nominal = b.dynamics_states(qpos, qvel, jac=spec)
    b.close()
    base = dr_ref.snapshot(o)
    points = dyn_ref.spec_points(spec)
    moved = 0
    try:
        for e in range(n):
            dr_ref.apply(o, P[e], L, base)
            load_state(o, states[e], np.zeros(o.nu))
            o.forward()
            r = {k: a[None] for k, a in dyn_ref.reference(o, points).items()}
            err = dyn_ref.errors(r, {k: a[e:e + 1] for k, a in dev.items()}, 0)
            assert all(err[q] <= BOUND[q] for q in QUANT), (e, err)
            moved += np.abs(dev["M"][e].astype(np.float64) - ref["M"][e]).max() > BOUND["M"] * max(1.0, np.abs(ref["M"][e]).max())
            assert np.abs(dev["passive"][e].astype(np.float64) - ref["passive"][e]).max() > BOUND["passive"] * max(1.0, np.abs(ref["passive"][e]).max())
    finally:
        dr_ref.restore(o, base)
    assert moved >= 1  # (the test sees the parameters)
    for e in range(n):
        err = dyn_ref.errors(ref, nominal, e)
        assert all(err[q] <= BOUND[q] for q in QUANT), (e, err)


def test_every_kind_of_model_is_taken(hbmod, gpu, tmp_path):
    """a friction-loss model, an equality model, the humanoid on a height field and the reference's robot: HB_OK, and each steps in
    the same kernel after the call as before it"""
    import eq_models
    models = {"fric_chain28": hbmod.Model.from_xml_string(kin_ref.fric_chain_xml(28)), "eq28_cd3_pgs": hbmod.Model.from_xml_string(eq_models.eq_chain_xml("eq28_cd3_pgs")),
              "humanoid27_hfield": hbmod.Model.load(os.path.join(ASSETS, "humanoid27_hfield.hbm")), "team_robot": hbmod.Model.load(os.path.join(ASSETS, "team_robot.hbm"))}
    for name, m in models.items():
        b = hbmod.Batch(m, 8, gpu)
        b.reset(perturb=True)
        ctrl = np.zeros((8, m.nu), dtype=np.float32)
        b.step(ctrl); b.step(ctrl)
        b.sync()
        before = b.last_kernel()
        out = b.dynamics(jac=m.jac_spec(bodies=[1], subtree_coms=[0]))
        assert b.last_kernel().startswith("hb_dyn") and all(np.isfinite(a).all() for a in out.values()), name
        assert np.array_equal(out["M"], out["M"].transpose(0, 2, 1)) and (np.linalg.eigvalsh(out["M"].astype(np.float64)) > 0).all(), name
        b.step(ctrl)
        b.sync()
        assert b.last_kernel() == before and not before.startswith("hb_dyn"), (name, before, b.last_kernel())
        assert not b.status().any(), name
        b.close()


def test_argument_errors(hbmod, gpu, humanoid_model):
    """every HB_EINVAL case, and a refused call leaves the batch stepping"""
    import humanoid_mujoco_amd.engine as eng
    m = humanoid_model
    L = hbmod.lib()
    n = 4
    b = hbmod.Batch(m, n, gpu)
    b.reset()
    q, v = np.zeros((n, m.nq), dtype=np.float32), np.zeros((n, m.nv), dtype=np.float32)
    q[:, 3] = 1
    M, f, J = np.zeros((n, m.nv, m.nv), dtype=np.float32), np.zeros((n, m.nv), dtype=np.float32), np.zeros((n, 16, 6, m.nv), dtype=np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    spec = m.jac_spec(bodies=[1, 2])
    S = ctypes.byref
    EINVAL = -1
    h = b._h
    # NULL batch
    assert L.hb_dynamics(None, P(M), None, None, None, None) == L.hb_dynamics_dev(None, P(M), None, None, None, None) == EINVAL
    assert L.hb_dynamics_states(None, P(q), P(v), n, P(M), None, None, None, None) == L.hb_dynamics_states_dev(None, P(q), P(v), n, P(M), None, None, None, None) == EINVAL
    # all outputs NULL
    assert L.hb_dynamics(h, None, None, None, None, None) == L.hb_dynamics_dev(h, None, None, None, None, None) == EINVAL
    assert L.hb_dynamics_states(h, P(q), P(v), n, None, None, None, None, None) == L.hb_dynamics_states_dev(h, P(q), P(v), n, None, None, None, None, None) == EINVAL
    # exactly one of jac and spec
    assert L.hb_dynamics(h, P(M), None, None, S(spec), None) == L.hb_dynamics(h, P(M), None, None, None, P(J)) == EINVAL
    assert L.hb_dynamics_dev(h, P(M), None, None, S(spec), None) == L.hb_dynamics_dev(h, P(M), None, None, None, P(J)) == EINVAL
    assert L.hb_dynamics_states(h, P(q), P(v), n, P(M), None, None, S(spec), None) == L.hb_dynamics_states(h, P(q), P(v), n, P(M), None, None, None, P(J)) == EINVAL
    assert L.hb_dynamics_states_dev(h, P(q), P(v), n, P(M), None, None, S(spec), None) == L.hb_dynamics_states_dev(h, P(q), P(v), n, P(M), None, None, None, P(J)) == EINVAL
    # spec.n outside 1..16, a body or a kind out of range
    for field, idx, value in (("n", None, 0), ("n", None, 17), ("n", None, -1), ("body", 1, m.nbody), ("body", 0, -1), ("kind", 1, 2), ("kind", 0, -1)):
        bad = eng.HbJacSpec.from_buffer_copy(spec)
        if idx is None:
            setattr(bad, field, value)
        else:
            getattr(bad, field)[idx] = value
        assert L.hb_dynamics(h, None, None, None, S(bad), P(J)) == EINVAL, (field, value)
        assert L.hb_dynamics_dev(h, None, None, None, S(bad), P(J)) == EINVAL, (field, value)
        assert L.hb_dynamics_states(h, P(q), None, n, None, None, None, S(bad), P(J)) == EINVAL, (field, value)
        assert L.hb_dynamics_states_dev(h, P(q), None, n, None, None, None, S(bad), P(J)) == EINVAL, (field, value)
    # n <= 0, NULL qpos, bias or passive without qvel
    for bad_n in (0, -3):
        assert L.hb_dynamics_states(h, P(q), P(v), bad_n, P(M), None, None, None, None) == L.hb_dynamics_states_dev(h, P(q), P(v), bad_n, P(M), None, None, None, None) == EINVAL
    assert L.hb_dynamics_states(h, None, P(v), n, P(M), None, None, None, None) == L.hb_dynamics_states_dev(h, None, P(v), n, P(M), None, None, None, None) == EINVAL
    for outs in ((None, P(f), None), (None, None, P(f)), (P(M), P(f), P(f))):
        assert L.hb_dynamics_states(h, P(q), None, n, outs[0], outs[1], outs[2], None, None) == EINVAL
        assert L.hb_dynamics_states_dev(h, P(q), None, n, outs[0], outs[1], outs[2], None, None) == EINVAL
    with pytest.raises(hbmod.HbError):
        b.dynamics(M=False, bias=False, passive=False)
    with pytest.raises(hbmod.HbError):
        b.dynamics_states(q, None, M=True, bias=True, passive=False)
    # the batch steps on, and a valid call still works
    b.step(np.zeros((n, m.nu), dtype=np.float32))
    assert not b.status().any()
    assert b.dynamics()["M"].shape == (n, m.nv, m.nv)
    b.close()


def test_bad_row_stays_alone(hbmod, gpu, tmp_path_factory):
    """a NaN joint angle in one of five states (all in two waves) leaves the other four rows and the batch's status as they are"""
    m, o, _, states, spec, _ = _case(hbmod, "humanoid27", tmp_path_factory)
    qpos, qvel = kin_ref.split_state(o, states[:5])
    b = hbmod.Batch(m, 2, gpu)
    status = b.status()
    good = b.dynamics_states(qpos, qvel, jac=spec)
    bad_q = qpos.copy()
    bad_q[2, 10] = np.nan
    bad = b.dynamics_states(bad_q, qvel, jac=spec)
    keep = [0, 1, 3, 4]
    same_dict({k: a[keep] for k, a in bad.items()}, {k: a[keep] for k, a in good.items()}, "rows beside the bad one")
    assert np.array_equal(b.status(), status)
    b.close()


def test_vecenv(hbmod, gpu, humanoid_model):
    """VecEnv.dynamics() and dynamics_torch() are the batch's, bit for bit, at the state the returned observation describes"""
    m = humanoid_model
    env = hbmod.VecEnv(m, 32, device=gpu)
    env.reset()
    rng = np.random.default_rng(5)
    for _ in range(4):
        env.step(rng.uniform(-1, 1, (32, m.nu)).astype(np.float32))
    spec = env.batch.jac_spec(bodies=["torso"], subtree_coms=[0, "torso"])
    want = env.batch.dynamics(jac=spec)
    assert want["M"].shape == (32, 27, 27) and want["jac"].shape == (32, 3, 6, 27)
    same_dict(env.dynamics(jac=spec), want, "VecEnv.dynamics")
    t = env.dynamics_torch(jac=spec)
    same_dict({k: a.cpu().numpy() for k, a in t.items()}, want, "VecEnv.dynamics_torch")
    t = env.dynamics_torch(M=True, bias=False, passive=False)
    assert set(t) == {"M"} and np.array_equal(t["M"].cpu().numpy(), want["M"])
    env.close()
