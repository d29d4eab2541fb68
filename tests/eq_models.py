"""Models with equality constraints for tests/test_eq_cpu.py and tests/test_gpu_eq.py.

TEST INFRASTRUCTURE: the product package never imports this module.

The chains: kernel_models.chain_xml at the two dense orders (nv 28 and 32), PGS condim 3 and Newton condim 1, with fric_models'
friction loss on top and an <equality> section of nine rows: a linear joint coupling, one with quadratic and cubic terms, a joint1-only
lock with a0 != 0, a connect between two links six bodies apart, a connect of a late link to the world, and one inactive element.
The small models: a one-dof slider, a planar four-bar (three hinges, the loop closed by a connect to the world), a geared pendulum pair.
"""
import functools
import os

import pytest

import eq_ref
from fric_models import add_friction
from kernel_models import chain_xml
from oracle_lib import Oracle

MODELS = {  # name -> (nv, condim, solver, step kernel, inverse kernel)
    "eq28_cd3_pgs": (28, 3, "PGS", "hb_eq_kernel", "hb_eq_inverse_kernel"),
    "eq32_cd3_pgs": (32, 3, "PGS", "hb_eq32_kernel", "hb_eq_inverse32_kernel"),
    "eq28_cd1_newton": (28, 1, "Newton", "hb_eq_newton28_kernel", "hb_eq_inverse_kernel"),
    "eq32_cd1_newton": (32, 1, "Newton", "hb_eq_newton32_kernel", "hb_eq_inverse32_kernel"),
}
# what the same model runs with its equalities disabled or inactive: the friction-loss kernels (the chains keep their frictionloss)
DISABLED_KERNEL = {"eq28_cd3_pgs": "hb_fric_kernel", "eq32_cd3_pgs": "hb_fric32_kernel", "eq28_cd1_newton": "hb_fric_newton28_kernel",
                   "eq32_cd1_newton": "hb_fric_newton32_kernel"}
NE = 9  # rows of EQUALITY: 1 + 1 + 1 + 3 + 3, the inactive element none

EQUALITY = ('<equality>'
            '<joint name="lin" joint1="j5" joint2="j9" polycoef="0 0.5 0 0 0"/>'
            '<joint name="poly" joint1="j11" joint2="j13" polycoef="0.01 -0.8 0.3 0.2 0" solref="0.03 1.1"/>'
            '<joint name="lock" joint1="j15" polycoef="0.05 0 0 0 0" solimp="0.8 0.92 0.002 0.4 3"/>'
            '<connect name="loop" body1="l1" body2="l7" anchor="0.3 0 0.05" solref="0.025 1" solimp="0.85 0.97 0.003 0.5 2"/>'
            '<connect name="pin" body1="l9" anchor="0.05 0 0"/>'
            '<joint name="off" joint1="j17" joint2="j19" active="false"/>'
            '</equality>')


def add_equality(xml, section=EQUALITY, flag=None, inactive=False):
    """the MJCF with `section` appended; flag: a <flag equality=.../> value; inactive: every element active="false" """
    if inactive:
        section = section.replace(' active="false"', "").replace('" joint1=', '" active="false" joint1=').replace('" body1=', '" active="false" body1=')
    xml = xml.replace("</mujoco>", section + "</mujoco>")
    if flag:
        assert "<option " in xml
        head, tail = xml.split("<option ", 1)
        opt, rest = tail.split("/>", 1)
        xml = head + "<option " + opt + '><flag equality="%s"/></option>' % flag + rest
    return xml


def eq_chain_xml(name, **kw):
    nv, condim, solver = MODELS[name][:3]
    return add_equality(add_friction(chain_xml(nv, condim=condim, solver=solver)), **kw)


def plain_chain_xml(name):
    """the same chain with the <equality> section deleted"""
    nv, condim, solver = MODELS[name][:3]
    return add_friction(chain_xml(nv, condim=condim, solver=solver))


@functools.lru_cache(maxsize=None)
def reference(name, tmp):
    """(model .hbm path, oracle, states, ctrls, reference steps) of a chain model: computed once per session and shared, never changed"""
    import humanoid_mujoco_amd as hb
    p = os.path.join(tmp, name + ".hbm")
    hb.Model.from_xml_string(eq_chain_xml(name)).save(p)
    o = Oracle(p)
    st, ct = eq_ref.rollout_states(o)
    return p, o, st, ct, eq_ref.steps_ref(o, st, ct)


@pytest.fixture(scope="session")
def eq_tmp(tmp_path_factory):
    """where reference() and the small models keep their files: imported by name into the test files that use it"""
    return str(tmp_path_factory.mktemp("eq"))


# ---- the small models
SLIDER_SOLREF, SLIDER_SOLIMP, SLIDER_A0, SLIDER_MASS = (0.04, 0.8), (0.7, 0.9, 0.05, 0.3, 2.0), 0.02, 1.5


def slider_xml(solver="Newton"):
    """one vertical slide joint carrying 1.5 kg, locked at q = 0.02 by a joint1-only equality: qacc = (1 - d) qacc_smooth + d aref"""
    return ('<mujoco><option timestep="0.002" solver="%s" iterations="100" tolerance="1e-12"/><worldbody><body pos="0 0 1">'
            '<joint name="s" type="slide" axis="0 0 1"/><geom type="sphere" size="0.05" mass="%g" contype="0" conaffinity="0"/></body></worldbody>'
            '<equality><joint joint1="s" polycoef="%g 0 0 0 0" solref="%g %g" solimp="%g %g %g %g %g"/></equality></mujoco>'
            % ((solver, SLIDER_MASS, SLIDER_A0) + SLIDER_SOLREF + SLIDER_SOLIMP))


FOURBAR_BENT = (0.3, -0.3, 0.3)  # a sheared parallelogram: the loop stays closed


def fourbar_xml():
    """A planar four-bar: crank 0.3 m up, coupler 0.4 m across, rocker 0.3 m down, hinges about y, the rocker's end pinned to the world by a
    connect.  At qpos0 it is a rectangle; (t, -t, t) is the same linkage sheared by t.  Nothing collides."""
    return ('<mujoco><option timestep="0.002" solver="Newton" iterations="100" tolerance="1e-10"/>'
            '<default><geom type="capsule" size="0.015" contype="0" conaffinity="0"/><joint type="hinge" axis="0 1 0" damping="0.02" armature="0.002"/></default>'
            '<worldbody><body name="crank" pos="0 0 0.5"><joint name="a"/><geom fromto="0 0 0 0 0 0.3" mass="0.3"/>'
            '<body name="coupler" pos="0 0 0.3"><joint name="b"/><geom fromto="0 0 0 0.4 0 0" mass="0.4"/>'
            '<body name="rocker" pos="0.4 0 0"><joint name="c"/><geom fromto="0 0 0 0 0 -0.3" mass="0.3"/></body></body></body></worldbody>'
            '<equality><connect name="close" body1="rocker" anchor="0 0 -0.3"/></equality></mujoco>')


def geared_xml():
    """two pendulums side by side, geared 1 : -2 by a joint coupling: dq1 + 2 dq2 = 0"""
    return ('<mujoco><option timestep="0.002" solver="Newton" iterations="100" tolerance="1e-10"/>'
            '<default><geom type="capsule" size="0.02" contype="0" conaffinity="0"/><joint type="hinge" axis="0 1 0" damping="0.01" armature="0.005"/></default>'
            '<worldbody><body pos="0 0 1"><joint name="p1"/><geom fromto="0 0 0 0.3 0 0" mass="0.5"/></body>'
            '<body pos="0 0.2 1"><joint name="p2"/><geom fromto="0 0 0 0.2 0 0" mass="0.8"/></body></worldbody>'
            '<equality><joint name="gear" joint1="p1" joint2="p2" polycoef="0 -2 0 0 0"/></equality></mujoco>')


def scissors_xml():
    """A free base carrying two arms that face each other, hinged about y, with a sphere at each tip 0.05 m apart at qpos0: after a
    perturbed reset (+-0.2 rad per joint) the tips overlap in about half of the envs - a self-collision, which makes
    reset_collision_mode = 2 draw those envs again under an env mask.  A third arm is geared to the first, a fourth pinned to the base
    by a connect: four equality rows.  A motor on every joint; nothing touches the floor in one step."""
    arm = '<body name="%s" pos="%g %g 0" euler="0 0 %d"><joint name="%s" type="hinge" axis="0 1 0"/><geom type="capsule" fromto="0 0 0 0.3 0 0" size="0.01" mass="0.2"/>%s</body>'
    tip = '<geom name="%s" type="sphere" pos="0.3 0 0" size="0.03" mass="0.05" contype="1" conaffinity="1"/>'
    return ('<mujoco><compiler angle="degree"/><option timestep="0.002" solver="PGS" iterations="50" tolerance="0"/>'
            '<default><joint damping="0.05" armature="0.01"/><geom contype="0" conaffinity="0"/></default>'
            '<worldbody><geom name="floor" type="plane" size="0 0 1" contype="1" conaffinity="1"/>'
            '<body name="base" pos="0 0 1"><freejoint name="root"/><geom name="base" type="sphere" size="0.05" mass="2"/>'
            + arm % ("a1", -0.325, 0, 0, "h1", tip % "t1") + arm % ("a2", 0.325, 0, 180, "h2", tip % "t2")
            + arm % ("a3", -0.325, 0.2, 0, "h3", "") + arm % ("a4", -0.325, -0.2, 0, "h4", "") +
            '</body></worldbody>'
            '<actuator>' + "".join('<motor name="m%d" joint="h%d" gear="1" ctrlrange="-1 1" ctrllimited="true"/>' % (k, k) for k in (1, 2, 3, 4)) + '</actuator>'
            '<equality><joint name="gear" joint1="h3" joint2="h1"/><connect name="pin" body1="a4" body2="base" anchor="0.3 0 0"/></equality></mujoco>')
