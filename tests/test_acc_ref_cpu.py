"""The fp64 reference of the body-acceleration read-out (tests/acc_ref.py) against the oracle itself and against closed forms, on the CPU.

Three kinds of evidence, none of which uses the device:
  (1) with qacc = 0 the reference's cacc is the oracle's own cacc array - the forward pass of mj_rne, which runs with flg_acc = 0 - to
      rounding: 1e-12 relative to max(1, max |cacc|);
  (2) independent of every spatial-algebra formula: the read-out of body b is the time derivative of the velocity of the material point
      xipos[b] and of the body's angular velocity, taken by central differences through the oracle's kinematics;
  (3) closed forms on one-body models written with the MJCF compiler: free fall, rest on the floor, a spinning hinge.
"""
import os
import re

import numpy as np

import acc_ref
import rk4_ref
from kernel_models import KERNEL_COLUMNS, chain_xml, kernel_table, oracle_for, rollout_states
from oracle_lib import HUMANOID_HBM, Oracle, golden_states, load_state, MODELS_DIR as MODELS
from step_lib import ACC_KERNELS, ACC_RK4_KERNELS

TOL = 1e-12
FD_H = 5e-7
FD_BOUND = 3 * 9.7e-11  # three times the worst deviation measured on the oracle: see test_readout_is_the_time_derivative_of_point_velocities


def worst_bias_deviation(o, states, ctrls):
    worst, moving = 0.0, 0
    for s, c in zip(states, ctrls):
        load_state(o, s, np.asarray(c, dtype=np.float64))
        o.forward()
        own = o.cacc.reshape(o.nbody, 6)
        worst = max(worst, float(np.abs(acc_ref.cacc(o, np.zeros(o.nv)) - own).max()) / max(1.0, float(np.abs(own).max())))
        moving += bool(np.abs(o.qvel).max() > 0.1)
    return worst, moving


def test_bias_cacc_is_the_oracles_rne_pass_on_golden_states():
    st, ctrl, _ = golden_states()
    o = Oracle(HUMANOID_HBM)
    worst, moving = worst_bias_deviation(o, st, ctrl)
    print("\ngolden states: worst deviation of cacc(qacc = 0) from the oracle's cacc %.2e over %d states (%d moving)" % (worst, len(st), moving))
    assert moving >= 100
    assert worst <= TOL, worst


def test_bias_cacc_is_the_oracles_rne_pass_on_a_chain(hbmod, tmp_path):
    _, _, o = oracle_for(hbmod, chain_xml(12), tmp_path)
    st, ct = rollout_states(o)
    worst, moving = worst_bias_deviation(o, st, ct)
    print("\nchain12: worst %.2e over %d states (%d moving)" % (worst, len(st), moving))
    assert moving >= 20
    assert worst <= TOL, worst


def point_state(o, q, v):
    """(velocity of every body's material point xipos, every body's angular velocity) from the oracle's kinematics at (q, v)"""
    nb = o.nbody
    load_state(o, np.concatenate([[0.0], q, v, np.zeros(o.nv)]), np.zeros(o.nu))
    o.forward()
    cv = o.cvel.reshape(nb, 6)
    r = o.xipos.reshape(nb, 3) - o.subtree_com.reshape(nb, 3)[o.info["body_rootid"]]
    return cv[:, 3:6] + np.cross(cv[:, 0:3], r), cv[:, 0:3].copy()


def fd_deviation(o, state, ctrl, h):
    """largest deviation of the reference read-out at `state` from the central differences with step h, relative to
    max(1, max |read-out|)"""
    nq, nv = o.nq, o.nv
    load_state(o, state, np.asarray(ctrl, dtype=np.float64))
    o.forward()
    q, v, a = o.qpos.copy(), o.qvel.copy(), o.qacc.copy()
    ref = acc_ref.body_acc(o)
    g = acc_ref.world_cacc(o)[3:6]
    vp, wp = point_state(o, rk4_ref.integrate_pos(o, q, v, h), v + h * a)
    vm, wm = point_state(o, rk4_ref.integrate_pos(o, q, v, -h), v - h * a)
    lin, ang = (vp - vm) / (2 * h), (wp - wm) / (2 * h)
    dev = max(float(np.abs(ref[:, 3:6] - g - lin).max()), float(np.abs(ref[:, 0:3] - ang).max()))
    return dev / acc_ref.scale(ref), acc_ref.scale(ref)


def fd_cases(hbmod, tmp_path):
    st, ctrl, _ = golden_states()
    yield "humanoid27", Oracle(HUMANOID_HBM), st[::4], ctrl[::4]
    _, _, o = oracle_for(hbmod, chain_xml(12), tmp_path)
    cs, cc = rollout_states(o)
    yield "chain12", o, cs, cc


def test_readout_is_the_time_derivative_of_point_velocities(hbmod, tmp_path):
    """Row b of the read-out, minus the world's (0, -gravity), against d/dt of the velocity of the point xipos[b] and of omega[b], by
    central differences over the oracle's kinematics at (integratePos(q, v, +-h), v +- h qacc), qacc the oracle's own at the state (32
    golden humanoid states with their contacts, 30 chain states).  The difference quotient's truncation error falls with h^2, its
    rounding error rises with 1 / h.  Scanned on the oracle, the worst deviation relative to max(1, max |read-out|) (read-outs up to
    3.1e3 on the humanoid, 4.8e2 on the chain):
        h        1e-3     1e-4     1e-5     1e-6     5e-7     3e-7     1e-7     3e-8
        humanoid 1.7e-4   1.7e-6   1.7e-8   1.7e-10  4.3e-11  2.3e-11  5.5e-11  2.5e-10
        chain12  9.7e-5   9.7e-7   9.7e-9   1.2e-10  9.7e-11  1.2e-10  3.5e-10  1.6e-9
    exactly h^2 on the left, 1 / h on the right, as a correct derivative must; the two balance at h = 5e-7, where the worst of both
    models is 9.7e-11.  Bound: 3 x 9.7e-11."""
    for name, o, states, ctrls in fd_cases(hbmod, tmp_path):
        worst, big = 0.0, 0.0
        for s, c in zip(states, ctrls):
            d, sc = fd_deviation(o, s, c, FD_H)
            worst, big = max(worst, d), max(big, sc)
        print("\n%s: worst deviation from the central differences %.2e over %d states (largest read-out %.3g)" % (name, worst, len(states), big))
        assert big > 50.0  # accelerations well above gravity are among the states
        assert worst <= FD_BOUND, (name, worst)


def _oracle_of(hbmod, tmp_path, xml, name, **opt):
    m = hbmod.Model.from_xml_string(xml) if xml.lstrip().startswith("<") else hbmod.Model.load(xml)
    if opt:
        m.set_opt(**opt)
    p = str(tmp_path / name)
    m.save(p)
    return Oracle(p)


BALL_AIR = ('<mujoco><option timestep="0.002"/><worldbody><geom type="plane" size="0 0 1"/>'
            '<body pos="0 0 3"><freejoint/><geom type="sphere" size="0.1" mass="2"/></body></worldbody></mujoco>')
G = 9.81


def test_free_fall_reads_zero(hbmod, tmp_path):
    """a ball in the air, moving and spinning: every entry of its row, its frame acceleration and an accelerometer at its centre read 0
    (the gravity pseudo-acceleration cancels its fall); the world's row is (0, -gravity)"""
    o = _oracle_of(hbmod, tmp_path, BALL_AIR, "air.hbm")
    o.reset()
    o.qvel[:] = [0.3, -0.2, 1.0, 2.0, -1.0, 0.5]
    o.forward()
    r = acc_ref.readout(o, imus=[(1, (0.0, 0.0, 0.0))], frameacc_bodies=[1])
    assert o.ncon == 0 and abs(o.qacc[2] + G) < 1e-12
    assert np.abs(r["body_acc"][1]).max() <= 1e-12 and np.abs(r["frameacc"][0]).max() <= 1e-12 and np.abs(r["imu"][0, 0:3]).max() <= 1e-12
    assert np.allclose(r["body_acc"][0], [0, 0, 0, 0, 0, G], atol=0)
    assert np.allclose(r["imu"][0, 3:6], [2.0, -1.0, 0.5], atol=1e-12)  # the gyro: the free joint's angular velocity is in body axes


def test_resting_ball_reads_plus_g(hbmod, tmp_path):
    """tests/models/ball_plane.xml, settled on the floor: +|g| upward.  The row is exactly g + qacc_z (the identity, to rounding) and
    the ball has settled to |qacc_z| <= 1e-6 g (tests/test_contact_ref_cpu.py), which together put the reading within 1.1e-6 g of g."""
    o = _oracle_of(hbmod, tmp_path, os.path.join(MODELS, "ball_plane.xml"), "ball.hbm", solver=2, iterations=100)
    o.reset()
    o.step(2000)
    o.forward()
    g = -float(o.marr("gravity")[2])
    r = acc_ref.readout(o, imus=[(1, (0.0, 0.0, 0.0))], frameacc_bodies=[1])
    az = float(o.qacc[2])
    print("\nresting ball: framelinacc z %.12g, g %.12g, qacc_z %.3e" % (r["frameacc"][0, 5], g, az))
    assert o.ncon == 1 and abs(az) <= 1e-6 * g
    assert abs(r["frameacc"][0, 5] - (g + az)) <= 1e-10 * g
    assert abs(r["frameacc"][0, 5] - g) <= 1.1e-6 * g and np.abs(r["frameacc"][0, [0, 1, 2, 3, 4]]).max() <= 1e-4 * g
    R = o.xmat.reshape(o.nbody, 3, 3)[1]
    assert np.allclose(R @ r["imu"][0, 0:3], r["frameacc"][0, 3:6], atol=1e-12)  # the accelerometer: the same vector in body axes


HINGE = ('<mujoco><option timestep="0.002" gravity="0 0 0"/><worldbody>'
         '<body pos="0 0 1"><joint type="hinge" axis="0 0 1"/><geom type="sphere" size="0.05" pos="0.4 0 0" mass="1"/></body></worldbody></mujoco>')


def test_spinning_hinge_reads_the_centripetal_acceleration(hbmod, tmp_path):
    """one hinge about z spinning at omega without gravity, its mass r = 0.4 from the axis: framelinacc (at xipos, world axes) is
    omega^2 r toward the axis, the accelerometer at the offset (r, 0, 0) reads (-omega^2 r, 0, 0) in body axes at every angle, the gyro
    omega on the axis, and frameangacc 0"""
    o = _oracle_of(hbmod, tmp_path, HINGE, "hinge.hbm")
    om, r0 = 3.0, 0.4
    for angle in (0.0, 0.7, 2.5):
        o.reset()
        o.qpos[0] = angle
        o.qvel[0] = om
        o.forward()
        assert abs(o.qacc[0]) <= 1e-12
        r = acc_ref.readout(o, imus=[(1, (r0, 0.0, 0.0)), (1, (0.0, 0.0, 0.0))], frameacc_bodies=[1])
        toward = -np.array([np.cos(angle), np.sin(angle), 0.0])
        assert np.allclose(r["frameacc"][0, 3:6], om * om * r0 * toward, atol=1e-12) and np.abs(r["frameacc"][0, 0:3]).max() <= 1e-12
        assert np.allclose(r["imu"][0], [-om * om * r0, 0, 0, 0, 0, om], atol=1e-12)
        assert np.allclose(r["imu"][1], [0, 0, 0, 0, 0, om], atol=1e-12)  # on the axis: no acceleration, the same rate


def test_every_full_kernel_has_a_twin_with_the_readout():
    """hb_step.hip's kernel table (HB_KERNELS): the read-out's instantiations (ACC = 1) repeat, parameter for parameter, exactly the
    rows that are full kernels (LEAN = 0, INV = 0, FRIC = 0) of the same INTEG - so that a launch with the read-out finds its kernel
    whatever the model - under names the step-kernel matrix does not collect; tests/test_gpu_body_acc.py names the ones it runs"""
    def rows(integ, acc):  # (every column but ACC itself)
        return {n: tuple(c[k] for k in KERNEL_COLUMNS if k != "ACC") for n, c in kernel_table()
                if c["INTEG"] == integ and c["ACC"] == acc and (acc == "1" or (c["LEAN"] == "0" and c["INV"] == "0" and c["FRIC"] == "0"))}
    full, rk4 = rows("0", "0"), rows("1", "0")
    acc, acc_rk4 = rows("0", "1"), rows("1", "1")
    assert len(full) == 12 and len(rk4) == 4
    assert {n.replace("hb_step", "hb_acc", 1): r for n, r in full.items()} == acc
    assert {n.replace("hb_rk4", "hb_acc_rk4", 1): r for n, r in rk4.items()} == acc_rk4
    assert not any(re.match(r"hb_step\w*_kernel$", n) for n in list(acc) + list(acc_rk4))
    used = {k for v in ACC_KERNELS.values() for k in v} | set(ACC_RK4_KERNELS.values())
    assert used <= set(acc) | set(acc_rk4) and len(used) >= 10
