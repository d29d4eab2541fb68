"""Joint friction loss without a GPU: the MJCF compiler and the .hbm records, the fp64 reference of tests/fric_ref.py pinned to the oracle
and certified on its own, known answers, what the state sets of tests/test_gpu_fric.py cover, and the kernel list of hb_step.hip."""
import os
import re

import numpy as np
import pytest

import fric_ref
from fric_models import MODELS, add_friction, fric_chain_xml, fric_tmp, pendulum_xml, reference  # noqa: F401  (fric_tmp: a fixture)
from kernel_models import CNSTR_LIMIT_JOINT, chain_xml, kernel_table, oracle_for, oracle_steps, rollout_states, row_kinds
from oracle_lib import ASSETS, CSRC, Oracle, load_state, parse_hbm
from step_lib import kernel_names_in_source

FRIC_KERNELS = ["hb_fric_kernel", "hb_fric32_kernel", "hb_fric_newton28_kernel", "hb_fric_newton32_kernel", "hb_fric_inverse_kernel", "hb_fric_inverse32_kernel"]
TWO_DOF = ('<mujoco><option timestep="0.002" solver="%s" iterations="%d" tolerance="0"/><worldbody><body pos="0 0 1">'
           '<joint name="h" type="hinge" axis="0 1 0" frictionloss="0.3" damping="0.1"/><geom type="capsule" fromto="0 0 0 0.4 0 0" size="0.02" mass="1"/>'
           '<body pos="0.2 0 0"><joint name="s" type="slide" axis="1 0 0" frictionloss="0.8" solreffriction="0.05 1"/><geom type="sphere" size="0.04" mass="0.5"/></body>'
           '</body></worldbody></mujoco>')


def _xml(joint_attrs="", default="", tendon="", extra_joint=""):
    return ('<mujoco><default>%s<default class="geared"><joint frictionloss="0.7" solreffriction="0.01 0.9" solimpfriction="0.8 0.85 0.002 0.4 3"/></default></default>'
            '<worldbody><body pos="0 0 1">%s<joint name="a" type="hinge" axis="0 1 0" %s/><geom type="capsule" fromto="0 0 0 0.3 0 0" size="0.02"/>'
            '<body pos="0.3 0 0"><joint name="b" class="geared" type="slide" axis="1 0 0"/><geom type="sphere" size="0.03"/>'
            '<body pos="0.1 0 0"><joint name="c" type="hinge" axis="0 0 1"/><geom type="sphere" size="0.03"/></body></body></body></worldbody>%s</mujoco>'
            % (default, extra_joint, joint_attrs, tendon))


def test_compiler_and_model_file(hbmod, tmp_path):
    """the three attributes directly and through a defaults class, MuJoCo's defaults, the .hbm round trip, the refusals by message, and
    the files of models without friction loss: byte for byte what they were, without the optional records"""
    m = hbmod.Model.from_xml_string(_xml('frictionloss="0.25"'))  # (the parent commit fails here: "joint frictionloss is not supported")
    assert np.array_equal(m.array("dof_frictionloss"), [0.25, 0.7, 0.0])
    assert np.array_equal(m.array("dof_solref_friction"), [0.02, 1, 0.01, 0.9, 0.02, 1])  # (a: MuJoCo's defaults; b: its class; c: defaults)
    assert np.array_equal(m.array("dof_solimp_friction"), [0.9, 0.95, 0.001, 0.5, 2, 0.8, 0.85, 0.002, 0.4, 3, 0.9, 0.95, 0.001, 0.5, 2])
    m = hbmod.Model.from_xml_string(_xml('frictionloss="0.25" solreffriction="-100 -5" solimpfriction="0.5 0.6 0.01 0.5 1"'))
    assert np.array_equal(m.array("dof_solref_friction")[:2], [-100, -5]) and np.array_equal(m.array("dof_solimp_friction")[:5], [0.5, 0.6, 0.01, 0.5, 1])
    p = str(tmp_path / "f.hbm")
    m.save(p)
    rec = parse_hbm(p)
    assert len(rec["dof_solref_friction"]) == 2 * m.nv and len(rec["dof_solimp_friction"]) == 5 * m.nv
    m2 = hbmod.Model.load(p)
    for f in ("dof_frictionloss", "dof_solref_friction", "dof_solimp_friction"):
        assert np.array_equal(m.array(f), m2.array(f)), f
    p2 = str(tmp_path / "f2.hbm")
    m2.save(p2)
    assert open(p, "rb").read() == open(p2, "rb").read()
    Oracle(p)  # (the oracle skips the records it does not know)
    # a truncated optional record is an error, not a read out of bounds
    bad = str(tmp_path / "bad.hbm")
    open(bad, "w").write(re.sub(r"^D dof_solref_friction \d+ \S+", "D dof_solref_friction %d" % (2 * m.nv - 1), open(p).read(), flags=re.M))
    with pytest.raises(hbmod.HbError, match="dof_solref_friction"):
        hbmod.Model.load(bad)
    # the refusals
    with pytest.raises(hbmod.HbError, match="frictionloss on a free joint"):
        hbmod.Model.from_xml_string('<mujoco><worldbody><body><joint type="free" frictionloss="0.1"/><geom type="sphere" size="0.1"/></body></worldbody></mujoco>')
    with pytest.raises(hbmod.HbError, match="tendon frictionloss"):
        hbmod.Model.from_xml_string(_xml(tendon='<tendon><fixed name="t" frictionloss="0.1"><joint joint="a" coef="1"/><joint joint="c" coef="-1"/></fixed></tendon>'))
    with pytest.raises(hbmod.HbError, match="negative joint frictionloss"):
        hbmod.Model.from_xml_string(_xml('frictionloss="-0.25"'))
    # models without friction loss: no optional records, and the same bytes on every save
    plain = hbmod.Model.from_xml_string(chain_xml(28))
    a, b = str(tmp_path / "a.hbm"), str(tmp_path / "b.hbm")
    plain.save(a); hbmod.Model.load(a).save(b)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert "dof_solref_friction" not in parse_hbm(a) and "dof_solimp_friction" not in parse_hbm(a) and not plain.array("dof_frictionloss").any()
    assert len(plain.array("dof_solref_friction")) == 2 * plain.nv  # (served with the defaults all the same)
    for asset in sorted(os.listdir(ASSETS)):
        if asset.endswith(".hbm"):
            out = str(tmp_path / asset)
            hbmod.Model.load(os.path.join(ASSETS, asset)).save(out)
            assert open(out, "rb").read() == open(os.path.join(ASSETS, asset), "rb").read(), asset
            assert "dof_solref_friction" not in parse_hbm(out)
    # <flag frictionloss="disable"/> is the option bit 2
    assert hbmod.Model.from_xml_string(fric_chain_xml("fric28_cd3_pgs", flag="disable")).opt.disableflags & 4


def test_reference_reproduces_the_oracle_without_friction_rows(hbmod, tmp_path):
    """fric_ref's PGS restatement with the friction rows dropped: the oracle's efc_force, qacc, sweep count and next state on
    chain28_cd3_pgs states to 1e-12 relative; its Newton: the oracle's Newton qacc to 1e-8"""
    m, p, o = oracle_for(hbmod, chain_xml(28, condim=3, solver="PGS"), tmp_path)
    st, ct = rollout_states(o)
    ref = oracle_steps(o, st, ct)
    rows = 0
    for k in range(len(st)):
        rec, prob, sol = fric_ref.step(o, st[k], ct[k].astype(np.float64), drop=True)
        assert len(prob["R"]) == ref["nefc"][k] and sol["niter"] == (o.dint("solver_niter") if ref["nefc"][k] else 0)
        rows += ref["nefc"][k]
        rel = lambda x, y: np.abs(x - y).max(initial=0.0) / max(1.0, np.abs(y).max(initial=0.0))
        assert rel(sol["force"], ref["force"][k]) < 1e-12 and rel(sol["qacc"], ref["qacc"][k]) < 1e-12, k
        assert rel(rec[1:1 + o.nq], ref["qpos"][k]) < 1e-12 and rel(rec[1 + o.nq:1 + o.nq + o.nv], ref["qvel"][k]) < 1e-12, k
        assert sol["reverts"] == 0
    assert rows > 100
    m, p, o = oracle_for(hbmod, chain_xml(28, condim=1, solver="Newton"), tmp_path, "n.hbm")
    st, ct = rollout_states(o)
    ref = oracle_steps(o, st, ct)
    for k in range(len(st)):
        prob, sol = fric_ref.forward(o, st[k], ct[k].astype(np.float64), drop=True)
        assert np.abs(sol["qacc"] - ref["qacc"][k]).max() / max(1.0, np.abs(ref["qacc"][k]).max()) < 1e-8, k


def test_reference_is_certified_on_its_own(hbmod, fric_tmp, tmp_path):
    """the Newton solution's stationarity residual |M (a - a_s) - J' f(a)| on every state of the GPU tests' friction models, and PGS run
    to convergence against it on a 2-dof model (a hinge pendulum with a sliding block on it, no contacts)"""
    for name in MODELS:
        p, o, st, ct, ref = reference(name, fric_tmp)
        for k in range(len(st)):
            load_state(o, st[k], ct[k].astype(np.float64))
            o.forward()
            prob = fric_ref.stacked(o)
            sol = fric_ref.solve_newton(o, prob)
            f, _, _ = fric_ref.primal_force(prob, prob["J"] @ sol["qacc"] - prob["aref"])
            res = np.abs(prob["M"] @ (sol["qacc"] - prob["qs"]) - prob["J"].T @ f).max()
            assert res < 1e-10 * max(1.0, np.abs(prob["qfs"]).max()), (name, k, res)
    m = hbmod.Model.from_xml_string(TWO_DOF % ("PGS", 20000))
    p = str(tmp_path / "two.hbm")
    m.save(p)
    o = Oracle(p)
    rng = np.random.default_rng(1)
    for k in range(6):
        o.reset()
        o.qpos[:] = rng.uniform(-0.5, 0.5, 2); o.qvel[:] = rng.uniform(-1, 1, 2) * (k % 3)
        o.forward()
        prob = fric_ref.stacked(o)
        assert prob["nf"] == 2 and len(prob["R"]) == 2
        nw, pg = fric_ref.solve_newton(o, prob), fric_ref.solve_pgs(o, prob, np.zeros(2))
        assert np.abs(nw["qacc"] - pg["qacc"]).max() < 1e-9 * max(1.0, np.abs(nw["qacc"]).max()), (k, nw["qacc"], pg["qacc"])
        assert np.abs(nw["force"] - pg["force"]).max() < 1e-9 * max(1.0, np.abs(nw["force"]).max())


def test_known_answers(hbmod, tmp_path):
    """the horizontal pendulum at rest: above the breakaway torque qacc = (tau_g - fl) / I exactly; below it |qacc| = |a_s| R / (R + 1 / I)
    with |f| < fl - both directions"""
    tau = 0.5 * 0.4 * 9.81
    for sign in (1, -1):
        for fl in (1.0, 2.5):
            m = hbmod.Model.from_xml_string(pendulum_xml(fl, sign))
            p = str(tmp_path / "p.hbm")
            m.save(p)
            o = Oracle(p)
            o.reset()
            o.forward()
            prob = fric_ref.stacked(o)
            I, a_s, R = prob["M"][0, 0], prob["qs"][0], prob["R"][0]
            assert abs(a_s - sign * tau / I) < 1e-12 * abs(a_s)
            for sol in (fric_ref.solve_newton(o, prob), fric_ref.solve_pgs(o, dict(prob), np.zeros(1))):
                if fl < tau:
                    assert abs(sol["qacc"][0] - sign * (tau - fl) / I) <= 4e-16 * abs(a_s) * 8 and sol["force"][0] == -sign * fl
                else:
                    want = abs(a_s) * R / (R + 1 / I)
                    assert abs(abs(sol["qacc"][0]) - want) < 1e-12 * abs(a_s) and abs(sol["force"][0]) < fl and np.sign(sol["qacc"][0]) == sign


def test_gpu_state_sets_cover_the_zones(hbmod, fric_tmp):
    """what the GPU tests' states exercise, by the reference alone: friction rows at +fl, at -fl and strictly inside, states that also
    have contact rows / joint-limit rows, and nothing above the kernels' capacities"""
    for name in MODELS:
        p, o, st, ct, ref = reference(name, fric_tmp)
        assert len(st) == 30
        assert (ref["zones"] >= 20).all(), (name, ref["zones"])
        con, lim = row_kinds(ref)
        assert con >= 10 and lim >= 10, (name, con, lim)
        assert max(ref["nefc"]) <= 63 and max(ref["ncon"]) <= 24, (name, max(ref["nefc"]), max(ref["ncon"]))
        assert ref["reverts"] == 0  # (the cost-revert the kernel leaves out never fires for a two-sided scalar row either)
        assert all(t[:n].tolist() == [fric_ref.CNSTR_FRICTION_DOF] * n for t, n in zip(ref["types"], ref["nf"]))  # friction rows first


def test_kernel_list():
    names = [n for n, c in kernel_table() if c["FRIC"] == "1"]
    assert names == FRIC_KERNELS, names
    assert not any(re.fullmatch(r"hb_step\w*_kernel", n) for n in names)
    assert not set(names) & kernel_names_in_source()
    src = open(os.path.join(CSRC, "hb_step.hip")).read()
    assert re.search(r"kStepKernels\[\] = \{(.*?)\};", src, re.S).group(1) == "HB_KERNELS(HB_ROW)"  # (every row of the table)
