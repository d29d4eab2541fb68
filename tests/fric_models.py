"""Models with joint friction loss for tests/test_fric_cpu.py and tests/test_gpu_fric.py, and - add_friction - for every model that
stacks something on top of them (tests/eq_models.py, tests/dr_rows.py, tests/test_device_tables_cpu.py).

TEST INFRASTRUCTURE: the product package never imports this module.

The chains: kernel_models.chain_xml at the two dense orders (nv 28 and 32), PGS condim 3 and Newton condim 1, with frictionloss on every
other joint in mixed magnitudes - some far above what a motor (gear 2) can push, so that the joint sticks, some far below, so that it
slips - and solreffriction / solimpfriction of their own on some.  The small model: a horizontal hinge pendulum.
"""
import functools
import os
import re

import pytest

import fric_ref
from kernel_models import chain_xml
from oracle_lib import Oracle

FL = (4.0, 0.05, 0.6, 0.02, 3.0)  # frictionloss of the chain's joints 0, 2, 4, ...: above the motors' 2 N m (sticks) and below (slips)
MODELS = {  # name -> (nv, condim, solver, step kernel, inverse kernel)
    "fric28_cd3_pgs": (28, 3, "PGS", "hb_fric_kernel", "hb_fric_inverse_kernel"),
    "fric32_cd3_pgs": (32, 3, "PGS", "hb_fric32_kernel", "hb_fric_inverse32_kernel"),
    "fric28_cd1_newton": (28, 1, "Newton", "hb_fric_newton28_kernel", "hb_fric_inverse_kernel"),
    "fric32_cd1_newton": (32, 1, "Newton", "hb_fric_newton32_kernel", "hb_fric_inverse32_kernel"),
}
PLAIN_KERNEL = {"fric28_cd3_pgs": "hb_step_kernel", "fric32_cd3_pgs": "hb_step32_kernel", "fric28_cd1_newton": "hb_step_newton28_kernel",
                "fric32_cd1_newton": "hb_step_newton32_kernel"}


def add_friction(xml, value=None, flag=None, solimp=None):
    """chain_xml's MJCF with frictionloss on joints j0, j2, j4, ... (FL in turn, or `value` on EVERY joint, with the impedance `solimp`
    if given), solreffriction on every fourth and solimpfriction on every sixth of them; flag: a <flag frictionloss=.../> value"""
    def joint(mo):
        j = int(mo.group(1))
        if value is not None:
            return '<joint name="j%d" frictionloss="%g"%s' % (j, value, ' solimpfriction="%g %g 0.001 0.5 2"' % (solimp, solimp) if solimp else "")
        if j % 2:
            return mo.group(0)
        extra = ' frictionloss="%g"' % FL[(j // 2) % len(FL)]
        if j % 4 == 0:
            extra += ' solreffriction="0.03 1.2"'
        if j % 6 == 0:
            extra += ' solimpfriction="0.8 0.9 0.002 0.5 2"'
        return '<joint name="j%d"%s' % (j, extra)
    xml = re.sub(r'<joint name="j(\d+)"', joint, xml)
    if flag:
        xml = re.sub(r"(<option [^>]*?)/>", r'\1><flag frictionloss="%s"/></option>' % flag, xml, count=1)
    return xml


def fric_chain_xml(name, **kw):
    nv, condim, solver = MODELS[name][:3]
    return add_friction(chain_xml(nv, condim=condim, solver=solver), **kw)


@functools.lru_cache(maxsize=None)
def reference(name, tmp):
    """(model .hbm path, oracle, states, ctrls, reference steps) of a model: computed once per session and shared, never changed"""
    import humanoid_mujoco_amd as hb
    p = os.path.join(tmp, name + ".hbm")
    hb.Model.from_xml_string(fric_chain_xml(name)).save(p)
    o = Oracle(p)
    st, ct = fric_ref.rollout_states(o)
    return p, o, st, ct, fric_ref.steps_ref(o, st, ct)


@pytest.fixture(scope="session")
def fric_tmp(tmp_path_factory):
    """where reference() keeps its models: imported by name into the test files that use it"""
    return str(tmp_path_factory.mktemp("fric"))


# (armature 1 and a friction impedance of 0.99: R = 0.0101 / 1.0533 = 0.0096, B = 2 / (0.99 * 0.02) = 101 - a held joint creeps at
# tau R / B = 1.9e-4 rad / s, a fifth of test_stick_and_slip's 1e-3 rad in the 1 s it runs)
PENDULUM = ('<mujoco><option timestep="0.002" solver="Newton" tolerance="1e-10"/><worldbody><body pos="0 0 1">'
            '<joint name="h" type="hinge" axis="0 1 0" armature="1" frictionloss="%g" solimpfriction="0.99 0.99 0.001 0.5 2"/><geom type="capsule" fromto="0 0 0 %g 0 0" size="0.02" mass="1"/>'
            '</body></worldbody></mujoco>')


def pendulum_xml(fl, sign=1):
    """a horizontal hinge pendulum at rest (a 0.4 m capsule of 1 kg along +-x about the y axis): gravity torque m g l / 2 = 1.962 N m"""
    return PENDULUM % (fl, 0.4 * sign)
