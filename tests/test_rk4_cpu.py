"""The RK4 integrator (mjINT_RK4) without a GPU: the option through every host layer (C-ABI, MJCF compiler, .hbm loader and writer), the
fp64 reference tests/rk4_ref.py itself (order of convergence, exactness on a constant acceleration), and the naming of the RK4 kernels."""
import os
import re

import numpy as np
import pytest

import rk4_ref
from kernel_models import chain_xml, kernel_table
from oracle_lib import CSRC, HUMANOID_HBM, Oracle, parse_hbm
from step_lib import RK4_KERNELS, kernel_names_in_source


def _hbm_with_integrator(tmp_path, value):
    text = open(HUMANOID_HBM).read()
    assert text.count("\ni integrator 0\n") == 1
    p = str(tmp_path / ("integrator%d.hbm" % value))
    with open(p, "w") as f:
        f.write(text.replace("\ni integrator 0\n", "\ni integrator %d\n" % value))
    return p


def test_hbm_loader_holds_the_integrator_to_the_implemented_values(hbmod, tmp_path):
    m = hbmod.Model.load(_hbm_with_integrator(tmp_path, 1))
    assert m.opt.integrator == 1 == hbmod.INT_RK4
    for bad in (2, 7):
        with pytest.raises(hbmod.HbError, match="integrator"):
            hbmod.Model.load(_hbm_with_integrator(tmp_path, bad))


def test_option_through_api_compiler_and_model_file(hbmod, tmp_path):
    m = hbmod.Model.load(HUMANOID_HBM)
    assert m.opt.integrator == hbmod.INT_EULER == 0
    m.set_opt(integrator=hbmod.INT_RK4)
    assert m.opt.integrator == 1
    p = str(tmp_path / "rk4.hbm")
    m.save(p)
    assert parse_hbm(p)["integrator"] == 1
    assert hbmod.Model.load(p).opt.integrator == 1
    for bad in (2, 3):
        with pytest.raises(hbmod.HbError):
            m.set_opt(integrator=bad)
    assert m.opt.integrator == 1  # (a refused call changes nothing)
    m.set_opt(integrator=hbmod.INT_EULER)
    assert m.opt.integrator == 0
    xml = chain_xml(28)
    assert xml.count("<option ") == 1
    assert hbmod.Model.from_xml_string(xml).opt.integrator == 0
    assert hbmod.Model.from_xml_string(xml.replace("<option ", '<option integrator="Euler" ')).opt.integrator == 0
    assert hbmod.Model.from_xml_string(xml.replace("<option ", '<option integrator="RK4" ')).opt.integrator == 1
    for name in ("implicit", "implicitfast"):
        with pytest.raises(hbmod.HbError, match="RK4"):
            hbmod.Model.from_xml_string(xml.replace("<option ", '<option integrator="%s" ' % name))


def test_reference_integrate_pos_is_the_oracles_advance():
    """rk4_ref.integrate_pos against the oracle's own Euler advance: qpos' = integratePos(qpos, qvel', h)"""
    o = Oracle()
    h = o.opt("timestep")
    for e in (0, 3, 7):
        o.init_env(e)
        for t in range(20):
            o.ctrl[:] = o.ctrl_env(t, e)
            q0 = o.qpos.copy()
            o.step()
            assert np.abs(rk4_ref.integrate_pos(o, q0, o.qvel, h) - o.qpos).max() < 1e-14


def test_reference_is_fourth_order_and_euler_is_first():
    """the benchmark humanoid's contact-free opening, Newton/100, horizon 0.04 s, against RK4 at h = 0.04 / 256: halving h from 0.01 to
    0.005 divides the RK4 error by at least 8 (fourth order: 16 and more) and the Euler error by at most 3 (first order: 2)"""
    o = Oracle()
    o.set_opt(solver=2, iterations=100)
    for e in (0, 3):
        s0, ctrl, ref = rk4_ref.convergence_case(o, e)
        err = {(k, h): rk4_ref.end_error(o, s0, ctrl, ref, h, k) for k in ("rk4", "euler") for h in (0.01, 0.005)}
        print("env %d: rk4 %.2e %.2e, euler %.2e %.2e" % (e, err["rk4", 0.01], err["rk4", 0.005], err["euler", 0.01], err["euler", 0.005]))
        assert err["rk4", 0.01] / err["rk4", 0.005] >= 8
        assert err["euler", 0.01] / err["euler", 0.005] <= 3
        assert err["rk4", 0.005] < 0.01 * err["euler", 0.005]


def test_reference_is_exact_on_a_constant_acceleration(hbmod, tmp_path):
    """a free body under gravity, no contact, no rotation: one RK4 step is q0 + h v0 + h^2 g / 2 and v0 + h g to fp64 rounding"""
    xml = ('<mujoco><option timestep="0.01" gravity="0.5 0 -9.81"/><worldbody><body pos="0 0 1"><freejoint/>'
           '<geom type="sphere" size="0.1" mass="1" contype="0" conaffinity="0"/></body></worldbody></mujoco>')
    m = hbmod.Model.from_xml_string(xml)
    p = str(tmp_path / "ball.hbm")
    m.save(p)
    o = Oracle(p)
    h, g = 0.01, np.array([0.5, 0.0, -9.81])
    q0 = np.array([0.1, -0.2, 1.0, 1.0, 0.0, 0.0, 0.0]); v0 = np.array([0.3, 0.7, -1.1, 0.0, 0.0, 0.0])
    r = rk4_ref.rk4_step(o, np.concatenate([[0.0], q0, v0, np.zeros(6)]), np.zeros(0))
    assert np.abs(r["qpos"][:3] - (q0[:3] + h * v0[:3] + 0.5 * h * h * g)).max() < 1e-15
    assert np.abs(r["qvel"][:3] - (v0[:3] + h * g)).max() < 1e-15
    assert np.array_equal(r["qpos"][3:], q0[3:]) and r["time"] == h and np.abs(r["warm"][:3] - g).max() < 1e-13
    # (the Euler step of the same body is off by h^2 g / 2 in position)
    e = rk4_ref.euler_step(o, np.concatenate([[0.0], q0, v0, np.zeros(6)]), np.zeros(0))
    assert np.abs(e[1:4] - r["qpos"][:3]).max() > 0.4 * h * h * 9.81


def test_rk4_kernels_are_named_outside_the_step_kernel_pattern_and_all_tested():
    """the RK4 kernels - the rows of the kernel table with INTEG = 1 and no read-out - have names that the step-kernel matrix
    (test_gpu_kernel_matrix.py) does not collect; each is in the table test_gpu_rk4.py runs (step_lib.RK4_KERNELS)"""
    names = [n for n, c in kernel_table() if c["INTEG"] == "1" and c["ACC"] == "0"]
    assert sorted(names) == ["hb_rk4_32_kernel", "hb_rk4_kernel", "hb_rk4_newton28_kernel", "hb_rk4_newton32_kernel"]
    assert not set(names) & kernel_names_in_source()
    assert not any(re.match(r"hb_step\w*_kernel$", n) for n in names)
    assert set(names) == set(RK4_KERNELS.values())
    src = open(os.path.join(CSRC, "hb_step.hip")).read()
    assert "kStepKernels[] = {HB_KERNELS(HB_ROW)};" in src  # (every row of the table is in the dispatch's array)
