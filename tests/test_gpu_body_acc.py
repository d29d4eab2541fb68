"""The body-acceleration read-out (include/hb.h: hb_body_acc_readout; hb_step.hip: the epilogue behind the solver) on the GPU.

Two tiers, kept apart as in tests/test_gpu_contact_force.py:
  DECODE  the read-out against the fp64 reference (tests/acc_ref.py) fed with the DEVICE's own qacc on the oracle's kinematics.  What is
          left is the fp32 kinematics (cdof, cvel, the bias acceleration) and the fp32 sum over the body's dofs.  No state is left out.
  PARITY  the read-out against the reference on the ORACLE's qacc at the same state: carries the solver's fp32 error.  Only states whose
          (ncon, nefc) agree with the oracle's; a case may leave out at most 2.
Both relative to max(1, max |read-out|) of the state.  Measured on MI355X (tools/gpu_body_acc_report.py,
profiles/body_acc_parity_report.txt), maxima over every model and kernel below; each bound is at most 3 x its maximum:
  decode: 6.19e-7 (humanoid, Newton; chains <= 4.9e-7, team robot 3.0e-7; the RK4 kernels' forward passes the same 5.9e-7 / 6.2e-7)
          - fp32 rounding of a sum of up to 27 terms                                                    -> DECODE_BOUND 1.8e-6
  parity: 9.97e-5 (last stage of RK4 Newton; humanoid 8.9e-5 PGS, 9.0e-5 Newton; chains <= 3.0e-6, team robot 4.7e-6)
                                                                                                         -> PARITY_BOUND 2.7e-4
The last stage of an RK4 step has a tier of its own, ADDITIONAL to the two above (which the RK4 kernels' forward passes are held to).
The device reaches that stage's state through three fp32 stages of its own, the reference through its own fp64 ones, and no call hands out the device's stage state: fed with the device's qacc, the reference there
still differs by the two stage states' kinematics.  Measured 3.96e-6 (PGS; Newton 3.65e-6, the typical state 3e-7) -> RK4_STAGE_BOUND
1.1e-5.  That the RK4 kernels' epilogue itself is exact to rounding is what their forward passes show, under DECODE_BOUND.
"""
import numpy as np
import pytest

import acc_ref
import contact_ref
import rk4_ref
from bounds import ACC_DECODE_BOUND as DECODE_BOUND, ACC_PARITY_BOUND as PARITY_BOUND
from oracle_lib import HUMANOID_HBM, Oracle, load_state
from step_lib import ACC_KERNELS as KERNELS, ACC_RK4_KERNELS as RK4_KERNELS

pytestmark = pytest.mark.gpu
RK4_STAGE_BOUND = 1.1e-5
MAX_LEFT_OUT = 2
# (KERNELS and RK4_KERNELS, which kernels may write a model's read-out: step_lib.ACC_KERNELS, ACC_RK4_KERNELS)
# the staged steps whose fast pass runs on a one-group layout: [kernel with the diagnostics, which switch that pass off; kernel without]
FAST_PASS = {"chain12_cd4": ["hb_acc_gen_big_kernel", "hb_acc_gen_fast1_kernel"], "chain12_cd6": ["hb_acc_gen_big_kernel", "hb_acc_gen_fast1_kernel"],
             "team_robot": ["hb_acc_newton_big20_kernel", "hb_acc_newton_gen20_kernel"]}
TORSO, FOOT_R, FOOT_L = 1, 7, 10  # bodies of humanoid27.hbm
IMUS = ((TORSO, (0.0, 0.0, 0.1)), (FOOT_R, (0.05, 0.02, -0.03)))  # the second: a non-zero offset on a limb body
FRAMEACC = (TORSO, FOOT_L)


def _show(label, dev, dec, par, left):
    print("\n  %-34s %-30s left out %d | decode %s  parity %s" % (label, dev["kernel"], left, "%.2e" % dec.max() if dec is not None else "-", "%.2e" % par.max() if len(par) else "-"))


def _check(name, dev, dec, par, left, n, kernels, decode_bound=DECODE_BOUND):
    assert dev["kernel"] in kernels, dev["kernel"]
    assert not dev["status"].any()
    assert np.isfinite(dev["acc"]).all()
    if dec is not None:
        assert len(dec) == n  # the decode tier leaves out no state
        assert dec.max() <= decode_bound, (name, dec.max())
    assert left <= MAX_LEFT_OUT and len(par) == n - left
    assert par.max() <= PARITY_BOUND, (name, par.max())


@pytest.mark.parametrize("name", contact_ref.CASES)
def test_every_step_kernel(hbmod, gpu, tmp_path, name):
    """Every kernel variant by name: the classic kernels (sized and with the size-specialised instantiations switched off), PGS on two row
    groups (condim 4 / 6 chains), the height-field chain (variant 1) and the team robot (Newton on four row groups).  Without the
    diagnostics a staged step runs its one-group fast pass first: that run has no device qacc to read, so the parity tier only."""
    m, o, st, ct, tune = contact_ref.make_case(hbmod, name, tmp_path)
    runs = [("", acc_ref.device_readout(hbmod, m, st, ct, gpu, tune))]
    if name in FAST_PASS:
        runs.append((" (fast pass)", acc_ref.device_readout(hbmod, m, st, ct, gpu, tune, diag=False)))
    g = acc_ref.world_cacc(o)
    for label, dev in runs:
        dec, par, left = acc_ref.compare(o, st, ct, dev)
        _show(name + label, dev, dec, par, left)
        _check(name + label, dev, dec, par, left, len(st), KERNELS[name])
        assert np.array_equal(dev["acc"][:, 0], np.broadcast_to(g.astype(np.float32), (len(st), 6)))  # the world row is (0, -gravity)
        assert np.abs(dev["acc"][:, 1:]).max() > 1.0
    if name in FAST_PASS:
        assert [dev["kernel"] for _, dev in runs] == FAST_PASS[name]


@pytest.mark.parametrize("name", sorted(RK4_KERNELS))
def test_rk4_kernels(hbmod, gpu, name):
    """a forward pass of the RK4 kernel - one pass at the given state: both tiers as for every other kernel - and a step, after which
    the getter holds the last stage"""
    m, o, st, ct, _ = contact_ref.make_case(hbmod, name, None)
    m.set_opt(integrator=hbmod.INT_RK4)
    dev = acc_ref.device_readout(hbmod, m, st, ct, gpu, forward=True)
    dec, par, left = acc_ref.compare(o, st, ct, dev)
    _show(name + " rk4 forward", dev, dec, par, left)
    _check(name + " rk4 forward", dev, dec, par, left, len(st), (RK4_KERNELS[name],))
    dev = acc_ref.device_readout(hbmod, m, st, ct, gpu)
    dec, par, left = acc_ref.compare(o, st, ct, dev, at_state=lambda oo, k: rk4_ref.rk4_step(oo, st[k], ct[k]))  # leaves the oracle at the last stage
    _show(name + " rk4 last stage", dev, dec, par, left)
    _check(name + " rk4 last stage", dev, dec, par, left, len(st), (RK4_KERNELS[name],), RK4_STAGE_BOUND)


def test_rk4_sensors_hold_the_first_stage_and_the_getter_the_last(hbmod, gpu):
    m, o, st, ct, _ = contact_ref.make_case(hbmod, "humanoid27_pgs", None)
    m.set_opt(integrator=hbmod.INT_RK4)
    n = len(st)
    first, last, scale = np.zeros((n, 2, 6)), np.zeros((n, 2, 6)), np.ones(n)
    for k in range(n):
        load_state(o, st[k], ct[k].astype(np.float64))
        o.forward()
        a0 = acc_ref.body_acc(o)
        rk4_ref.rk4_step(o, st[k], ct[k])  # leaves the oracle at the last stage
        a3 = acc_ref.body_acc(o)
        scale[k] = max(acc_ref.scale(a0), acc_ref.scale(a3))
        first[k], last[k] = a0[list(FRAMEACC)], a3[list(FRAMEACC)]
    apart = np.abs(first - last).max(axis=(1, 2)) / scale
    pick = np.flatnonzero(apart > 10 * PARITY_BOUND)  # chosen on the reference alone: the two stages differ by far more than the bound
    print("\n  rk4: %d of %d states whose first and last stage differ by more than 10 x the bound" % (len(pick), n))
    assert len(pick) >= 20, len(pick)
    b = hbmod.Batch(m, n, gpu)
    b.body_acc_readout(True)
    b.set_state(hbmod.STATE_INTEGRATION, st)
    rows, _ = b.rollout_sensors(ct[None], hbmod.Batch.sensor_spec(frameacc_bodies=FRAMEACC))
    got_first = rows[0].astype(np.float64).reshape(n, 2, 6)
    got_last = b.body_acc().astype(np.float64)[:, FRAMEACC]
    assert b.last_kernel() == "hb_acc_rk4_kernel" and not b.status().any()
    b.close()
    e_first = np.abs(got_first - first).max(axis=(1, 2)) / scale
    e_last = np.abs(got_last - last).max(axis=(1, 2)) / scale
    print("  rk4: sensor row vs first stage %.2e, getter vs last stage %.2e; stages apart by >= %.2e on %d states" % (e_first[pick].max(), e_last[pick].max(), apart[pick].min(), len(pick)))
    assert e_first[pick].max() <= PARITY_BOUND and e_last[pick].max() <= PARITY_BOUND


def test_sensor_rows_are_the_single_steps_getter(hbmod, gpu):
    """T = 3 steps of hb_rollout_sensors in one launch, with accelerometer / gyro and frame-acceleration entries behind a framepos and a
    contact-force entry, against three single steps each followed by the getter: the frame-acceleration entries are body_acc's rows bit
    for bit; the accelerometer / gyro entries are R' applied to the reference (fed with the device's own qacc) within the decode bound.
    hb_sensors (a forward pass) and hb_transition_fd_sensors take the entries as well."""
    m, o, st, _, _ = contact_ref.make_case(hbmod, "humanoid27_pgs", None)
    n, T = len(st), 3
    spec = hbmod.Batch.sensor_spec(framepos_bodies=(TORSO,), contactforce_bodies=(FOOT_R,), imu=IMUS, frameacc_bodies=FRAMEACC)
    lay = hbmod.Batch.sensor_layout(spec)
    CFRC, IMU, FACC = (slice(o, o + c) for o, c in (lay["cfrc"], lay["imu"], lay["facc"]))
    assert (CFRC, IMU, FACC, lay["width"]) == (slice(3, 6), slice(6, 18), slice(18, 30), 30)
    ctrl = np.random.default_rng(3).uniform(-1, 1, (T, n, m.nu)).astype(np.float32)
    b = hbmod.Batch(m, n, gpu)
    b.set_state(hbmod.STATE_INTEGRATION, st)
    rows, _ = b.rollout_sensors(ctrl, spec)
    with pytest.raises(hbmod.HbError):
        b.body_acc()  # a sensor spec does not switch the getter on
    end = b.get_state(hbmod.STATE_INTEGRATION)
    b.close()
    assert rows.shape == (T, n, 3 + 3 + 12 + 12)
    s = hbmod.Batch(m, n, gpu)
    s.diag_enable(True)
    s.body_acc_readout(True)
    s.contact_readout(True)
    s.set_state(hbmod.STATE_INTEGRATION, st)
    worst = 0.0
    for t in range(T):
        before = s.get_state(hbmod.STATE_INTEGRATION).astype(np.float64)
        s.step(ctrl[t])
        acc, qacc = s.body_acc(), s.qacc().astype(np.float64)
        assert np.array_equal(rows[t, :, FACC], acc[:, FRAMEACC].reshape(n, 12)), t
        assert np.array_equal(rows[t, :, CFRC], s.body_contact()[:, FOOT_R, 0:3]), t
        for k in range(n):
            load_state(o, before[k], ctrl[t, k].astype(np.float64))
            o.forward()
            a = acc_ref.cacc(o, qacc[k])
            ref = np.concatenate([acc_ref.imu(o, bd, off, a=a) for bd, off in IMUS])
            worst = max(worst, float(np.abs(rows[t, k, IMU] - ref).max()) / acc_ref.scale(acc_ref.body_acc(o, a=a)))
    print("\n  accelerometer / gyro entries against R' of the reference: %.2e" % worst)
    assert worst <= DECODE_BOUND, worst
    assert np.array_equal(s.get_state(hbmod.STATE_INTEGRATION), end)
    r = s.sensors(spec, ctrl[0])
    assert np.array_equal(r[:, FACC], s.body_acc()[:, FRAMEACC].reshape(n, 12)) and np.abs(r[:, IMU]).max() > 0
    x = np.concatenate([s.qpos[:1], s.qvel[:1]], axis=1).astype(np.float64)
    eps, j = 1e-3, 6 + int(np.argmin(np.abs(x[0, m.nq + 6:])))  # the joint that moves slowest in this state
    C = s.transition_fd(x, ctrl[0, :1].astype(np.float64), eps=eps, centered=False, sensor_spec=spec)[2]  # (1 + 2 nv + nu = 76 envs of the 128)
    assert C.shape == (1, 30, 2 * m.nv) and np.isfinite(C).all()
    # ... with the new entries where the row has them: the column of that joint's velocity is the forward difference of two hb_sensors
    # rows, at (x, u) and with that velocity nudged by eps (zero warm start, as hb_transition_fd uses without one).  Both sides difference
    # fp32 rows of the same kernel; what may differ is the fp32 rounding of the nudged velocity against eps, 1.2e-7 |v| / eps <= 1e-3 of
    # the column for |v| <= 8 (asserted): bound 1e-3 of max(1, max |column|).  A shifted entry misses it by the column's own size.
    two = np.zeros((n, 1 + m.nq + 2 * m.nv))
    two[:, 1:1 + m.nq + m.nv] = x[0]
    two[1, 1 + m.nq + j] += eps
    assert abs(x[0, m.nq + j]) <= 8.0
    s.set_state(hbmod.STATE_INTEGRATION, two)
    r = s.sensors(spec, np.repeat(ctrl[0, :1], n, axis=0)).astype(np.float64)
    fd = (r[1] - r[0]) / eps
    print("  transition_fd column of qvel[%d] against two hb_sensors rows: %.2e of max |column| %.3g" % (j, np.abs(C[0, :, m.nv + j] - fd).max() / max(1.0, np.abs(fd).max()), np.abs(fd).max()))
    assert np.abs(fd[IMU]).max() > 0 and np.abs(fd[FACC]).max() > 0
    assert np.abs(C[0, :, m.nv + j] - fd).max() <= 1e-3 * max(1.0, np.abs(fd).max())
    s.close()


def _run_steps(hbmod, gpu, m, st, ctrl, readout, duo=None):
    b = hbmod.Batch(m, len(st), gpu)
    if duo is not None:
        b.tune(duo=duo)
    b.set_state(hbmod.STATE_INTEGRATION, st)
    b.step(ctrl[0])
    plain = b.last_kernel()  # the kernel of a launch without any read-out
    b.set_state(hbmod.STATE_INTEGRATION, st)
    b.diag_enable(True)
    b.contact_readout(True)
    if readout:
        b.body_acc_readout(True)
    for t in range(len(ctrl)):
        b.step(ctrl[t])
    out = dict(state=b.get_state(hbmod.STATE_INTEGRATION), status=b.status(), qacc=b.qacc(), cf=b.contact_force(), bc=b.body_contact(), kernel=b.last_kernel(), plain=plain,
               acc=b.body_acc() if readout else None)
    b.close()
    return out


def test_nothing_else_moves(hbmod, gpu):
    """a 3-step run with the read-out on and off: states, qacc, contact read-out and sensor rows bit for bit; a launch without the
    read-out still names the lean / two-envs-per-wave kernel, and the two-envs-per-wave knob changes no read-out"""
    m, _, st, _, _ = contact_ref.make_case(hbmod, "humanoid27_pgs", None)
    ctrl = np.random.default_rng(7).uniform(-1, 1, (3, len(st), m.nu)).astype(np.float32)
    off, on, duo = _run_steps(hbmod, gpu, m, st, ctrl, False), _run_steps(hbmod, gpu, m, st, ctrl, True), _run_steps(hbmod, gpu, m, st, ctrl, True, duo=2)
    assert (off["plain"], on["plain"], duo["plain"]) == ("hb_step_h27_kernel", "hb_step_h27_kernel", "hb_step_duo_kernel")
    assert off["kernel"] == "hb_step_kernel" and on["kernel"] == duo["kernel"] == "hb_acc_kernel"  # (the full kernel and its twin with the read-out)
    for key in ("state", "status", "qacc", "cf", "bc"):
        assert np.array_equal(off[key], on[key]) and np.array_equal(off[key], duo[key]), key
    assert np.array_equal(on["acc"], duo["acc"]) and np.abs(on["acc"]).max() > 20.0
    # the sensor rows a spec without acceleration entries gives are those of the same spec with them
    spec0 = hbmod.Batch.sensor_spec(framepos_bodies=(TORSO,), touch_bodies=(FOOT_R,), linvel_bodies=(TORSO,))
    spec1 = hbmod.Batch.sensor_spec(framepos_bodies=(TORSO,), touch_bodies=(FOOT_R,), linvel_bodies=(TORSO,), imu=IMUS[:1])
    got = []
    for spec in (spec0, spec1):
        b = hbmod.Batch(m, len(st), gpu)
        b.set_state(hbmod.STATE_INTEGRATION, st)
        got.append((b.rollout_sensors(ctrl, spec)[0], b.get_state(hbmod.STATE_INTEGRATION)))
        b.close()
    assert np.array_equal(got[0][0], got[1][0][:, :, :7]) and np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][1], off["state"])


def test_edges(hbmod, gpu, humanoid_model):
    m = humanoid_model
    b = hbmod.Batch(m, 8, gpu)
    for getter in (b.body_acc, b.body_acc_readout_dev):
        with pytest.raises(hbmod.HbError):
            getter()  # before body_acc_readout
    b.body_acc_readout(True)
    b.reset()
    q = b.get_state(hbmod.STATE_QPOS)
    q[:, 2] += 5.0  # free flight from rest, no controls: internal forces only, so the centre of mass falls with gravity and reads 0
    b.set_state(hbmod.STATE_QPOS, q)
    b.step(np.zeros((8, m.nu), np.float32))
    acc = b.body_acc()
    g = acc_ref.world_cacc(Oracle(HUMANOID_HBM)).astype(np.float32)
    assert acc.shape == (8, m.nbody, 6) and not b.counts()[0].any()
    assert np.array_equal(acc[:, 0], np.broadcast_to(g, (8, 6))) and g[5] > 9.0  # the world row: (0, -gravity)
    # rows refer to the bodies' own centres of mass (xipos): their mass-weighted mean is the acceleration of the whole body's centre of
    # mass, 0 in free flight - to the fp32 rounding of a 16-term sum of entries of the size of the largest row (6e-8 each: bound 1e-5)
    mass = Oracle(HUMANOID_HBM).marr("body_mass")
    com = np.einsum("b,ebi->ei", mass, acc[:, :, 3:6].astype(np.float64)) / mass.sum()
    print("\n  free flight: centre-of-mass reading %.2e, largest row %.3g" % (np.abs(com).max(), np.abs(acc[:, 1:]).max()))
    assert np.abs(com).max() <= 1e-5 * max(1.0, float(np.abs(acc[:, 1:]).max()))
    p = b.body_acc_readout_dev()
    assert p and np.array_equal(b.from_dev(p, (8, m.nbody, 6)), acc)
    b.body_acc_readout(False)
    with pytest.raises(hbmod.HbError):
        b.body_acc()
    b.close()
    import ctypes
    assert hbmod.lib().hb_sensor_size(ctypes.byref(hbmod.Batch.sensor_spec(imu=IMUS, frameacc_bodies=FRAMEACC))) == 24
    bad = hbmod.Batch.sensor_spec(frameacc_bodies=FRAMEACC)
    bad.n_imu = 5
    assert hbmod.lib().hb_sensor_size(ctypes.byref(bad)) < 0


def test_vecenv_body_accelerations(hbmod, gpu, humanoid_model):
    m = humanoid_model
    env = hbmod.VecEnv(m, 32, gpu, randomization_factor=0.0, auto_reset=0, max_time=0.0, body_accelerations=True)
    env.reset()
    for _ in range(10):  # the unperturbed reset pose stands on its feet
        env.step_arrays(np.zeros((32, m.nu), np.float32))
    a = env.body_accelerations()
    assert np.array_equal(a, env.batch.body_acc()) and a.shape == (32, m.nbody, 6)
    print("\n  standing humanoid: torso reads %.2f m/s^2 upward" % a[0, TORSO, 5])
    assert (a[:, 0, 5] > 9.0).all() and np.isfinite(a).all()
    plain = hbmod.VecEnv(m, 4, gpu)
    with pytest.raises(RuntimeError):
        plain.body_accelerations()
    env.close()
    plain.close()


def test_a_masked_env_keeps_its_rows(hbmod, gpu, humanoid_model):
    """hb_env_reset with reset_collision_mode = 2 steps every env once and then re-draws and steps, under an env mask, only the envs that
    ended in a self-collision.  An env whose first draw stood is skipped by those later launches; its state is then the plain reset's
    advanced by one zero-control step, bit for bit - and so must its read-out rows be, which the masked launches around it may not have
    touched (tests/test_gpu_contact_force.py does the same for the contact read-out)."""
    m, n = humanoid_model, 128
    kw = dict(randomization_factor=1.0, auto_reset=0, max_time=0.0, target_z=10.0, body_accelerations=True)
    a = hbmod.VecEnv(m, n, gpu, reset_collision_mode=2, **kw)
    a.reset()
    b = hbmod.VecEnv(m, n, gpu, **kw)
    b.reset()
    b.step_arrays(np.zeros((n, m.nu), np.float32))
    first_draw = (a.batch.get_state(hbmod.STATE_INTEGRATION) == b.batch.get_state(hbmod.STATE_INTEGRATION)).all(axis=1)
    wa, wb = a.body_accelerations(), b.body_accelerations()
    print("\n  %d envs kept their first draw, %d were re-drawn under a mask" % (first_draw.sum(), (~first_draw).sum()))
    assert (~first_draw).sum() >= 8 and first_draw.sum() >= 8
    assert np.array_equal(wa[first_draw], wb[first_draw]) and np.abs(wa[first_draw, 1:]).max() > 0
    assert not np.array_equal(wa[~first_draw], wb[~first_draw])  # (the re-drawn envs did move on)
    a.close()
    b.close()
