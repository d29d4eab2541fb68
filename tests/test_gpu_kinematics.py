"""The whole-body kinematics read-out (include/hb.h: hb_kinematics*; csrc/hb_kin.hip) on the GPU against the fp64 oracle's mj_kinematics /
mj_comVel products (tests/kin_ref.py), and its contract as a pure function of the state: the same bits whatever the packing, the batch
size, a state's place in a wave or the form of the call, nothing of the batch written.

Bounds (bounds.POSE_BOUND, VEL_BOUND; errors relative to max(1, max |reference|) of the state): the project's convention is 3 x the maxima of
profiles/kinematics_parity.txt (tools/gpu_kinematics_report.py, the same cases), capped at the 1.8e-6 DECODE_BOUND of
tests/test_gpu_body_acc.py, which covers the same fp32 kinematics plus a longer sum.
    poses       measured maximum 5.146e-7 (chain32), 3 x = 1.5438e-6          -> 1.54e-6 (rounded down)
    velocities  measured maximum 7.874e-7 (chain32), 3 x = 2.362e-6 > the cap -> 1.8e-6 (2.3 x the maximum)
"""
import ctypes

import numpy as np
import pytest

import kin_ref
from bounds import POSE_BOUND, VEL_BOUND
from step_lib import same_dict, snapshot

pytestmark = pytest.mark.gpu

_cache = {}


def _case(hbmod, name, tmp_path_factory):
    """parity_case(name) and its references, computed once per session and left unchanged"""
    if name not in _cache:
        m, o, kernel, states = kin_ref.parity_case(hbmod, name, tmp_path_factory.mktemp(name))
        ref = kin_ref.references(o, states)
        for a in ref.values():
            a.setflags(write=False)
        states.setflags(write=False)
        _cache[name] = (m, o, kernel, states, ref)
    return _cache[name]


def _readout(hbmod, m, states, gpu, **tune):
    b = hbmod.Batch(m, len(states), gpu)
    if tune:
        b.tune(**tune)
    b.set_state(hbmod.STATE_INTEGRATION, np.asarray(states))
    out = b.kinematics(pose=True, vel=True, geoms=True)
    kernel = b.last_kernel()
    b.close()
    return out, kernel


@pytest.mark.parametrize("name", kin_ref.CASES)
def test_parity(hbmod, gpu, tmp_path_factory, name):
    """1: every state of every case inside both bounds, on the kernel the model's size asks for"""
    m, o, kernel, states, ref = _case(hbmod, name, tmp_path_factory)
    dev, ran = _readout(hbmod, m, states, gpu)
    assert ran == kernel
    assert dev["pose"].shape == (len(states), m.nbody, 10) and dev["vel"].shape == (len(states), m.nbody, 6) and dev["geoms"].shape == (len(states), m.ngeom, 7)
    err = np.array([kin_ref.errors(ref, dev, k) for k in range(len(states))])
    print("%s: pose %.3g vel %.3g" % (name, err[:, 0].max(), err[:, 1].max()))
    assert err[:, 0].max() <= POSE_BOUND, (name, err[:, 0])
    assert err[:, 1].max() <= VEL_BOUND, (name, err[:, 1])


@pytest.mark.parametrize("name", ["humanoid27", "bush17"])
def test_packing_is_bit_identical(hbmod, gpu, tmp_path_factory, name):
    """2: kin_pack 1 against 0; batches that leave a wave part filled; a state's row whatever batch it is in"""
    m, o, kernel, states, ref = _case(hbmod, name, tmp_path_factory)
    packed, k1 = _readout(hbmod, m, states, gpu)
    plain, k0 = _readout(hbmod, m, states, gpu, kin_pack=0)
    assert (k1, k0) == (kernel, "hb_kin64_kernel")
    same_dict(packed, plain, "kin_pack")
    for n in (1, 3, 5):
        out, _ = _readout(hbmod, m, states[:n], gpu)
        same_dict(out, {k: a[:n] for k, a in packed.items()}, "n_env %d" % n)
    big = np.tile(states, (137, 1))[:4097]
    out, _ = _readout(hbmod, m, big, gpu)
    for pack in (1, 0):
        for e in (0, 1, 4095, 4096):
            one, _ = _readout(hbmod, m, big[e:e + 1], gpu, kin_pack=pack)
            same_dict(one, {k: a[e:e + 1] for k, a in out.items()}, "row %d of 4097, kin_pack %d" % (e, pack))
    same_dict({k: a[:len(states)] for k, a in out.items()}, packed, "4097")


def test_states_permuted(hbmod, gpu, tmp_path_factory):
    """2: the result of state k does not depend on where it stands among the states"""
    m, o, _, states, _ = _case(hbmod, "humanoid27", tmp_path_factory)
    qpos, qvel = kin_ref.split_state(o, states)
    b = hbmod.Batch(m, 4, gpu)
    a = b.kinematics_states(qpos, qvel, geoms=True)
    perm = np.random.default_rng(0).permutation(len(qpos))
    p = b.kinematics_states(qpos[perm], qvel[perm], geoms=True)
    same_dict({k: v[perm] for k, v in a.items()}, p, "permuted")
    b.close()


def test_states_form(hbmod, gpu, tmp_path_factory):
    """3: a [T, n_env] trajectory tape in one call against set_state + kinematics per step; n not tied to n_env; no qvel; device forms"""
    m, o, _, states, _ = _case(hbmod, "humanoid27", tmp_path_factory)
    T, n = 3, 5
    b = hbmod.Batch(m, n, gpu)
    b.set_state(hbmod.STATE_INTEGRATION, np.asarray(states[:n]))
    ctrl = np.random.default_rng(1).uniform(-1, 1, (T, n, m.nu)).astype(np.float32)
    q, v, _ = b.rollout_trajectory(ctrl)
    tape = b.kinematics_states(q, v, geoms=True)
    assert tape["pose"].shape == (T, n, m.nbody, 10) and tape["vel"].shape == (T, n, m.nbody, 6) and tape["geoms"].shape == (T, n, m.ngeom, 7)
    rec = b.get_state(hbmod.STATE_INTEGRATION)
    for t in range(T):
        rec[:, 1:1 + m.nq], rec[:, 1 + m.nq:1 + m.nq + m.nv] = q[t], v[t]
        b.set_state(hbmod.STATE_INTEGRATION, rec)
        same_dict(b.kinematics(geoms=True), {k: a[t] for k, a in tape.items()}, "step %d" % t)
    b.close()
    b = hbmod.Batch(m, 4, gpu)
    qpos, qvel = kin_ref.split_state(o, states[:7])
    seven = b.kinematics_states(qpos, qvel, geoms=True)
    assert seven["pose"].shape == (7, m.nbody, 10)
    full, _ = _readout(hbmod, m, states[:7], gpu)
    same_dict(seven, full, "n = 7 on 4 envs")
    nov = b.kinematics_states(qpos, None, vel=False, geoms=True)
    assert set(nov) == {"pose", "geoms"}
    same_dict(nov, {k: seven[k] for k in nov}, "qvel=None")
    # device forms
    sizes = {"pose": m.nbody * 10, "vel": m.nbody * 6, "geoms": m.ngeom * 7}
    ptr = {k: b.dev_alloc(4 * 7 * s) for k, s in sizes.items()}
    dq, dv = b.dev_alloc(qpos.nbytes), b.dev_alloc(qvel.nbytes)
    b.to_dev(dq, qpos); b.to_dev(dv, qvel)
    b.kinematics_states_dev(dq, dv, 7, ptr["pose"], ptr["vel"], ptr["geoms"])
    b.sync()
    same_dict({k: b.from_dev(ptr[k], seven[k].shape) for k in sizes}, seven, "kinematics_states_dev")
    b.set_state(hbmod.STATE_INTEGRATION, np.asarray(states[:4]))
    host = b.kinematics(geoms=True)
    b.kinematics_dev(ptr["pose"], ptr["vel"], ptr["geoms"])
    b.sync()
    same_dict({k: b.from_dev(ptr[k], host[k].shape) for k in sizes}, host, "kinematics_dev")
    for p in list(ptr.values()) + [dq, dv]:
        b.dev_free(p)
    b.close()


def test_pure_function(hbmod, gpu, tmp_path_factory):
    """4: nothing of the batch is written, held step calls come first, a free joint's quaternion is normalised for the computation only"""
    m, o, _, states, ref = _case(hbmod, "humanoid27", tmp_path_factory)
    n = 8
    ctrl = np.random.default_rng(2).uniform(-1, 1, (n, m.nu)).astype(np.float32)
    a, twin = hbmod.Batch(m, n, gpu), hbmod.Batch(m, n, gpu)
    for b in (a, twin):
        b.set_state(hbmod.STATE_INTEGRATION, np.asarray(states[:n]))
        b.step(ctrl)
    before = snapshot(hbmod, a)
    a.kinematics(geoms=True)
    for x, y in zip(before, snapshot(hbmod, a)):
        assert np.array_equal(x, y)
    for b in (a, twin):
        b.step(ctrl)
    assert np.array_equal(a.get_state(hbmod.STATE_INTEGRATION), twin.get_state(hbmod.STATE_INTEGRATION))
    a.close(); twin.close()
    # held back, folded step calls on a pipelined batch
    n = 256
    big = np.tile(states, (9, 1))[:n]
    ctrl = np.random.default_rng(3).uniform(-1, 1, (n, m.nu)).astype(np.float32)
    outs = []
    for sync_first in (False, True):
        b = hbmod.Batch(m, n, gpu)
        b.pipeline(True)
        b.set_state(hbmod.STATE_INTEGRATION, big)
        d = b.dev_alloc(ctrl.nbytes)
        b.to_dev(d, ctrl)
        for _ in range(3):
            b.step_dev(d)
        if sync_first:
            b.sync()
        outs.append(b.kinematics(geoms=True))
        b.sync()
        outs.append({"state": b.get_state(hbmod.STATE_INTEGRATION)})
        b.dev_free(d)
        b.close()
    same_dict(outs[0], outs[2], "held step calls")
    same_dict(outs[1], outs[3], "state after")
    assert not np.array_equal(outs[1]["state"][:, 1:1 + m.nq], big[:, 1:1 + m.nq].astype(np.float32))
    # a free joint's quaternion of norm 1.3
    b = hbmod.Batch(m, 1, gpu)
    s = np.array(states[:1])
    s[0, 4:8] *= 1.3
    b.set_state(hbmod.STATE_INTEGRATION, s)
    out = b.kinematics(geoms=True)
    pe, ve = kin_ref.errors(ref, out, 0)
    assert pe <= POSE_BOUND and ve <= VEL_BOUND, (pe, ve)
    assert np.array_equal(b.get_state(hbmod.STATE_INTEGRATION)[0, 4:8], s[0, 4:8].astype(np.float32))
    assert abs(np.linalg.norm(b.get_state(hbmod.STATE_INTEGRATION)[0, 4:8].astype(np.float64)) - 1.3) < 1e-6
    b.close()


def test_agrees_with_the_sensors(hbmod, gpu, tmp_path_factory):
    """5: framepos, framelinvel and framezaxis of the step kernels' sensor read-out against xpos, v and the third column of xmat"""
    m, o, _, states, _ = _case(hbmod, "humanoid27", tmp_path_factory)
    b = hbmod.Batch(m, len(states), gpu)
    b.set_state(hbmod.STATE_INTEGRATION, np.asarray(states))
    spec = hbmod.engine.HbSensorSpec()
    spec.n_framepos, spec.subtree_body = 16, -1
    for i in range(16):
        spec.framepos_body[i] = i + 1
    spec.n_frameaxis = spec.n_framelinvel = 8
    for i in range(8):
        spec.frameaxis_body[i], spec.frameaxis_which[i], spec.framelinvel_body[i] = 2 * i + 1, 2, 2 * i + 2
    sens = b.sensors(spec, np.zeros((len(states), m.nu), dtype=np.float32)).astype(np.float64)
    kin = b.kinematics()
    b.close()
    pose, vel = kin["pose"].astype(np.float64), kin["vel"].astype(np.float64)
    lay = hbmod.Batch.sensor_layout(spec)
    fpos, axes, linvel = (sens[:, o:o + c].reshape(len(states), -1, 3) for o, c in (lay["framepos"], lay["axis"], lay["linvel"]))
    assert (fpos.shape[1], axes.shape[1], linvel.shape[1], lay["width"]) == (16, 8, 8, sens.shape[1])
    zcol = hbmod.quat_to_mat(pose[:, :, 3:7])[:, :, :, 2]
    for k in range(len(states)):
        ps = max(1.0, np.abs(pose[k]).max())
        assert np.abs(fpos[k] - pose[k, 1:17, 0:3]).max() / ps <= POSE_BOUND
        assert np.abs(axes[k] - zcol[k, 1:17:2]).max() / ps <= POSE_BOUND
        assert np.abs(linvel[k] - vel[k, 2:18:2, 3:6]).max() / max(1.0, np.abs(vel[k]).max()) <= VEL_BOUND
    assert np.array_equal(kin["pose"][:, 0], np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0], dtype=np.float32), (len(states), 1)))
    assert not kin["vel"][:, 0].any()


def test_argument_errors(hbmod, gpu, humanoid_model):
    """6: every HB_EINVAL case raises, nothing faults, the batch steps afterwards"""
    m = humanoid_model
    L = hbmod.lib()
    b = hbmod.Batch(m, 4, gpu)
    q, v = np.zeros((4, m.nq), dtype=np.float32), np.zeros((4, m.nv), dtype=np.float32)
    q[:, 3] = 1
    out = np.zeros((4, m.nbody, 10), dtype=np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    EINVAL = L.hb_kinematics(None, P(out), None, None)
    assert EINVAL != 0
    assert L.hb_kinematics_dev(None, P(out), None, None) == EINVAL
    assert L.hb_kinematics_states(None, P(q), P(v), 4, P(out), None, None) == EINVAL
    assert L.hb_kinematics_states_dev(None, P(q), P(v), 4, P(out), None, None) == EINVAL
    with pytest.raises(hbmod.HbError):
        b.kinematics(pose=False, vel=False, geoms=False)
    with pytest.raises(hbmod.HbError):
        b.kinematics_dev(None, None, None)
    with pytest.raises(hbmod.HbError):
        b.kinematics_states(q, v, pose=False, vel=False)
    with pytest.raises(hbmod.HbError):
        b.kinematics_states(q, None, vel=True)
    with pytest.raises(hbmod.HbError):
        b.kinematics_states_dev(1 << 20, None, 4, None, 1 << 20, None)
    with pytest.raises(hbmod.HbError):
        b.kinematics_states_dev(1 << 20, 1 << 20, 4)
    for n in (0, -3):
        assert L.hb_kinematics_states(b._h, P(q), P(v), n, P(out), None, None) == EINVAL
        assert L.hb_kinematics_states_dev(b._h, P(q), P(v), n, P(out), None, None) == EINVAL
    with pytest.raises(hbmod.HbError):
        b.tune(kin_pack=2)
    b.reset()
    b.step(np.zeros((4, m.nu), dtype=np.float32))
    assert not b.status().any()
    assert b.kinematics()["pose"].shape == (4, m.nbody, 10)
    b.close()


def test_bad_row_stays_alone(hbmod, gpu, tmp_path_factory):
    """7: a NaN joint angle in one of five states (all in one wave) leaves the other four rows and the batch's status as they are"""
    m, o, _, states, _ = _case(hbmod, "humanoid27", tmp_path_factory)
    qpos, qvel = kin_ref.split_state(o, states[:5])
    b = hbmod.Batch(m, 2, gpu)
    status = b.status()
    good = b.kinematics_states(qpos, qvel, geoms=True)
    bad_q = qpos.copy()
    bad_q[2, 10] = np.nan
    bad = b.kinematics_states(bad_q, qvel, geoms=True)
    keep = [0, 1, 3, 4]
    same_dict({k: a[keep] for k, a in bad.items()}, {k: a[keep] for k, a in good.items()}, "rows beside the bad one")
    assert np.array_equal(b.status(), status)
    b.close()


def test_vecenv(hbmod, gpu, humanoid_model):
    """8: the VecEnv's read-outs are the batch's, at the state the returned observation describes"""
    env = hbmod.VecEnv(humanoid_model, 16, device=gpu)
    env.reset()
    rng = np.random.default_rng(4)
    for _ in range(5):
        env.step(rng.uniform(-1, 1, (16, humanoid_model.nu)).astype(np.float32))
    poses, vels, geoms = env.body_poses(), env.body_velocities(), env.geom_poses()
    assert poses.shape == (16, 17, 10) and vels.shape == (16, 17, 6) and geoms.shape == (16, 20, 7)
    kin = env.batch.kinematics(geoms=True)
    assert np.array_equal(poses, kin["pose"]) and np.array_equal(vels, kin["vel"]) and np.array_equal(geoms, kin["geoms"])
    assert np.array_equal(poses[:, 1, 0:3], env.batch.qpos[:, :3])
    env.close()
