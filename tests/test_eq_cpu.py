"""Equality constraints without a GPU: the MJCF compiler and the .hbm records, the fp64 reference of tests/eq_ref.py held to things it does
not itself define (central differences, a closed form, the stationarity of its own solution, fric_ref), what the state sets of
tests/test_gpu_eq.py cover, and the kernel list of hb_step.hip."""
import os
import re

import numpy as np
import pytest

import eq_ref
import fric_ref
from eq_models import (EQUALITY, FOURBAR_BENT, MODELS, NE, SLIDER_A0, SLIDER_MASS, SLIDER_SOLIMP, SLIDER_SOLREF, add_equality, eq_chain_xml, eq_tmp,  # noqa: F401  (eq_tmp: a fixture)
                       fourbar_xml, geared_xml, plain_chain_xml, reference, slider_xml)
from kernel_models import chain_xml, kernel_table, oracle_for, row_kinds
from oracle_lib import ASSETS, CSRC, MODELS_DIR, Oracle, load_state, parse_hbm
from rk4_ref import integrate_pos
from step_lib import kernel_names_in_source

EQ_KERNELS = ["hb_eq_kernel", "hb_eq32_kernel", "hb_eq_newton28_kernel", "hb_eq_newton32_kernel", "hb_eq_inverse_kernel", "hb_eq_inverse32_kernel"]


def _xml(equality, default="", free=False):
    """three scalar joints a (hinge), b (slide), c (hinge) on a chain of three bodies with non-trivial frames, optionally under a free base"""
    base = '<body name="base" pos="0 0 1"><freejoint name="root"/><geom type="sphere" size="0.05"/>' if free else ""
    return ('<mujoco><default>%s<default class="stiff"><equality solref="0.01 0.9" solimp="0.8 0.85 0.002 0.4 3"/></default></default>'
            '<worldbody>%s<body name="A" pos="0.1 0.2 1" euler="10 20 30"><joint name="a" type="hinge" axis="0 1 0" ref="15"/><geom type="capsule" fromto="0 0 0 0.3 0 0" size="0.02"/>'
            '<body name="B" pos="0.3 0 0" euler="0 -25 5"><joint name="b" type="slide" axis="1 0 0"/><geom type="sphere" size="0.03"/>'
            '<body name="C" pos="0.1 0.05 0" euler="40 0 0"><joint name="c" type="hinge" axis="0 0 1"/><geom type="sphere" size="0.03"/></body></body></body>%s</worldbody>'
            '<equality>%s</equality></mujoco>' % (default, base, "</body>" if free else "", equality))


def test_compiler_and_model_file(hbmod, tmp_path):
    """every attribute directly and through a defaults class, MuJoCo's defaults, the anchor in body2's frame, names, the .hbm round trip,
    and the files of models without equalities: byte for byte what they were, without the optional records"""
    eqs = ('<joint name="ab" joint1="a" joint2="b" polycoef="0.1 -2 0.3 0.4 0.5" solref="0.05 0.7" solimp="0.5 0.6 0.01 0.3 1"/>'
           '<joint joint1="c"/>'
           '<joint name="cls" class="stiff" joint1="b" joint2="c" active="false"/>'
           '<connect name="cw" body1="C" anchor="0.01 0.02 0.03"/>'
           '<connect name="ca" body1="C" body2="A" anchor="-0.2 0.1 0.05" class="stiff" solref="-500 -20"/>')
    m = hbmod.Model.from_xml_string(_xml(eqs))  # (the parent commit fails here: "equality constraints are not supported")
    assert m.neq == 5 and len(m.array("eq_type")) == 5
    assert np.array_equal(m.array("eq_type"), [2, 2, 2, 0, 0]) and np.array_equal(m.array("eq_active0"), [1, 1, 0, 1, 1])
    assert np.array_equal(m.array("eq_obj1id"), [0, 2, 1, 3, 3]) and np.array_equal(m.array("eq_obj2id"), [1, -1, 2, 0, 1])
    data = m.array("eq_data").reshape(5, 11)
    assert np.array_equal(data[0], [0.1, -2, 0.3, 0.4, 0.5, 0, 0, 0, 0, 0, 0]) and np.array_equal(data[1][:5], [0, 1, 0, 0, 0])
    assert np.array_equal(data[3][:3], [0.01, 0.02, 0.03]) and np.array_equal(data[4][:3], [-0.2, 0.1, 0.05]) and not data[:, 6:].any()
    assert np.array_equal(m.array("eq_solref"), [0.05, 0.7, 0.02, 1, 0.01, 0.9, 0.02, 1, -500, -20])
    assert np.array_equal(m.array("eq_solimp").reshape(5, 5), [[0.5, 0.6, 0.01, 0.3, 1], [0.9, 0.95, 0.001, 0.5, 2], [0.8, 0.85, 0.002, 0.4, 3],
                                                               [0.9, 0.95, 0.001, 0.5, 2], [0.8, 0.85, 0.002, 0.4, 3]])
    assert [m.name2id("equality", n) for n in ("ab", "cls", "cw", "ca", "nope")] == [0, 2, 3, 4, -1]
    e = m.equalities()
    assert [x["name"] for x in e] == ["ab", "", "cls", "cw", "ca"] and [x["type"] for x in e] == ["joint"] * 3 + ["connect"] * 2
    assert [x["active"] for x in e] == [True, True, False, True, True] and e[4]["obj2"] == 1 and len(e[0]["data"]) == 5 and len(e[3]["data"]) == 6
    assert m.equality_rows() == 1 + 1 + 3 + 3
    m.set_opt(disableflags=m.opt.disableflags | 2)
    assert m.equality_rows() == 0
    m.set_opt(disableflags=m.opt.disableflags & ~2)
    # a main-class default
    m3 = hbmod.Model.from_xml_string(_xml('<joint joint1="a"/>', default='<equality solref="0.07 1.3"/>'))
    assert np.array_equal(m3.array("eq_solref"), [0.07, 1.3])
    # the round trip, and the oracle, which skips the records it does not know
    p, p2 = str(tmp_path / "e.hbm"), str(tmp_path / "e2.hbm")
    m.save(p)
    rec = parse_hbm(p)
    assert len(rec["eq_type"]) == 5 and len(rec["eq_data"]) == 55 and rec["eq_name"] == ["ab", "", "cls", "cw", "ca"]
    m2 = hbmod.Model.load(p)
    for f in ("eq_type", "eq_obj1id", "eq_obj2id", "eq_active0", "eq_data", "eq_solref", "eq_solimp"):
        assert np.array_equal(m.array(f), m2.array(f)), f
    m2.save(p2)
    assert open(p, "rb").read() == open(p2, "rb").read()
    o = Oracle(p)
    # anchor2: the two points of every connect coincide at qpos0
    o.reset()
    o.forward()
    pos, elem = eq_ref.equality_pos(o)
    assert len(pos) == 8 and np.abs(pos[elem >= 3]).max() <= 1e-12, pos
    assert np.abs(data[3][3:6]).max() > 0.5  # (body2 = world: the anchor's world position)
    # a truncated or out-of-range record is an error, not a read out of bounds
    text = open(p).read()
    for pat, sub, msg in ((r"^D eq_data \d+ \S+", "D eq_data 54", "eq_data"), (r"^I eq_obj1id 5 0", "I eq_obj1id 5 7", "joint id out of range"),
                          (r"^I eq_type 5 2", "I eq_type 5 1", "equality type 1")):
        bad = str(tmp_path / "bad.hbm")
        assert re.search(pat, text, flags=re.M), pat
        open(bad, "w").write(re.sub(pat, sub, text, flags=re.M))
        with pytest.raises(hbmod.HbError, match=msg):
            hbmod.Model.load(bad)
    # models without equalities: no optional records, and every asset saves to the bytes it has
    plain = hbmod.Model.from_xml_string(chain_xml(28))
    a = str(tmp_path / "a.hbm")
    plain.save(a)
    assert not any(k.startswith("eq_") for k in parse_hbm(a)) and plain.neq == 0 and plain.equalities() == [] and plain.equality_rows() == 0
    empty = hbmod.Model.from_xml_string(chain_xml(28).replace("</mujoco>", "<equality/></mujoco>"))
    b = str(tmp_path / "b.hbm")
    empty.save(b)
    assert open(a, "rb").read() == open(b, "rb").read()
    for asset in sorted(os.listdir(ASSETS)):
        if asset.endswith(".hbm"):
            out = str(tmp_path / asset)
            mm = hbmod.Model.load(os.path.join(ASSETS, asset))
            assert mm.neq == 0
            mm.save(out)
            assert open(out, "rb").read() == open(os.path.join(ASSETS, asset), "rb").read(), asset
    # <flag equality="disable"/> is the option bit 1
    assert hbmod.Model.from_xml_string(eq_chain_xml("eq28_cd3_pgs", flag="disable")).opt.disableflags & 2
    assert hbmod.Model.from_xml_string(eq_chain_xml("eq28_cd3_pgs")).equality_rows() == NE
    assert hbmod.Model.from_xml_string(eq_chain_xml("eq28_cd3_pgs", inactive=True)).equality_rows() == 0


@pytest.mark.parametrize("eq,msg", [
    ('<weld body1="A" body2="B"/>', "equality <weld> is not supported"),
    ('<tendon tendon1="t"/>', "equality <tendon> is not supported"),
    ('<flex flex="f"/>', "equality <flex> is not supported"),
    ('<distance geom1="g" geom2="h"/>', "equality <distance> is not supported"),
    ('<connect site1="s" site2="t"/>', "site1 / site2 form of connect is not supported"),
    ('<joint joint1="root"/>', "joint equality on a free joint is not supported"),
    ('<joint joint1="a" joint2="root"/>', "joint equality on a free joint is not supported"),
    ('<joint joint1="nope"/>', "valid joint1"),
    ('<joint joint1="a" joint2="nope"/>', "unknown joint2"),
    ('<connect body1="nope" anchor="0 0 0"/>', "valid body1"),
    ('<connect body1="A" body2="nope" anchor="0 0 0"/>', "unknown body2"),
    ('<connect body1="A"/>', "needs anchor"),
])
def test_compiler_refusals(hbmod, eq, msg):
    with pytest.raises(hbmod.HbError, match=msg):
        hbmod.Model.from_xml_string(_xml(eq, free=True))


def test_kernel_list():
    names = [n for n, c in kernel_table() if c["FRIC"] == "2"]
    assert names == EQ_KERNELS, names
    assert not any(re.fullmatch(r"hb_step\w*_kernel", n) for n in names)
    assert not set(names) & kernel_names_in_source()
    cfg = {n: c for n, c in kernel_table()}
    for n in names:  # (the friction row of the same place in its list, but for the FRIC cell)
        twin = dict(cfg[n.replace("hb_eq", "hb_fric")], FRIC="2")
        assert cfg[n] == twin, n
    src = open(os.path.join(CSRC, "hb_step.hip")).read()
    assert re.search(r"kStepKernels\[\] = \{(.*?)\};", src, re.S).group(1) == "HB_KERNELS(HB_ROW)"  # (every row of the table)


def _random_states(o, n, seed, scale=0.4):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        o.reset()
        v = rng.normal(size=o.nv) * scale
        out.append(integrate_pos(o, o.qpos.copy(), v, 1.0))
    return out


def _small(hbmod, xml, tmp_path, name):
    return oracle_for(hbmod, xml, tmp_path, name)[2]


def test_jacobian_against_central_differences(hbmod, eq_tmp, tmp_path):
    """J of every equality row is the derivative of its pos along every dof: central differences of pos through integrate_pos, h = 1e-6,
    on the nv = 28 chain (free base, slide joint, both connects, the polynomial coupling) and the four-bar"""
    h = 1e-6
    for o in (Oracle(reference("eq28_cd3_pgs", eq_tmp)[0]), _small(hbmod, fourbar_xml(), tmp_path, "fb.hbm")):
        rows = 0
        for q in _random_states(o, 3, 2):
            o.reset(); o.qpos[:] = q; o.forward()
            J = eq_ref.equality_rows(o)["J"]
            num = np.zeros_like(J)
            for d in range(o.nv):
                e = np.zeros(o.nv); e[d] = 1.0
                pm = []
                for s in (1, -1):
                    o.reset(); o.qpos[:] = integrate_pos(o, q, s * e, h); o.forward()
                    pm.append(eq_ref.equality_pos(o)[0])
                num[:, d] = (pm[0] - pm[1]) / (2 * h)
            assert np.abs(J - num).max() < 1e-8 * max(1.0, np.abs(J).max()), np.abs(J - num).max()
            assert np.abs(J).max() > 0.1
            rows += len(J)
        assert rows >= 9


def test_slider_closed_form(hbmod, tmp_path):
    """one dof, one row: qacc = (1 - d) qacc_smooth + d aref, with d, K, B written out from solref / solimp here"""
    o = _small(hbmod, slider_xml(), tmp_path, "s.hbm")
    (tc, dr), (d0, d1, width, mid, power) = SLIDER_SOLREF, SLIDER_SOLIMP
    assert power == 2.0 and tc > 2 * 0.002
    K, B = 1 / (d1 * d1 * tc * tc * dr * dr), 2 / (d1 * tc)
    seen = set()
    for q, v in ((0.0, 0.0), (0.03, 0.5), (0.045, -1.0), (-0.2, 0.3), (SLIDER_A0, 2.0)):
        pos = q - SLIDER_A0
        x = abs(pos) / width
        y = 1.0 if x >= 1 else x * x / mid if x <= mid else 1 - (1 - x) ** 2 / (1 - mid)
        seen.add("end" if x >= 1 else "low" if x <= mid else "high")
        d = d0 + y * (d1 - d0)
        aref = -B * v - K * d * pos
        want = (1 - d) * -9.81 + d * aref
        o.reset(); o.qpos[:] = q; o.qvel[:] = v; o.forward()
        prob = eq_ref.stacked(o)
        assert prob["ne"] == 1 and len(prob["R"]) == 1 and abs(prob["M"][0, 0] - SLIDER_MASS) < 1e-12
        for sol in (eq_ref.solve_newton(o, prob), eq_ref.solve_pgs(o, dict(prob, ), np.zeros(1))):
            assert abs(sol["qacc"][0] - want) < 1e-10 * max(1.0, abs(want)), (q, v, sol["qacc"], want)
    assert seen == {"end", "low", "high"}


def test_reference_is_certified_on_its_own(hbmod, eq_tmp, tmp_path):
    """converged Newton satisfies M qacc - qfrc_smooth = J' f with f = -D jar on the equality rows, on every state of the GPU tests'
    models; PGS run to convergence agrees with it (the four-bar and the geared pair: no unilateral rows, a unique dual solution)"""
    for name in MODELS:
        p, o, st, ct, ref = reference(name, eq_tmp)
        for k in range(len(st)):
            load_state(o, st[k], ct[k].astype(np.float64))
            o.forward()
            prob = eq_ref.stacked(o)
            sol = eq_ref.solve_newton(o, prob)
            ne = prob["ne"]
            assert ne == NE
            jar = prob["J"] @ sol["qacc"] - prob["aref"]
            assert np.array_equal(sol["force"][:ne], -jar[:ne] / prob["R"][:ne]) and sol["quad"][:ne].all()
            res = np.abs(prob["M"] @ sol["qacc"] - prob["qfs"] - prob["J"].T @ sol["force"]).max()
            assert res < 1e-12 * max(1.0, np.abs(prob["qfs"]).max()), (name, k, res)  # (measured: 4e-14 at worst)
    for xml, q0 in ((fourbar_xml(), FOURBAR_BENT), (geared_xml(), (0.4, -0.1))):
        o = _small(hbmod, xml.replace('tolerance="1e-10"', 'tolerance="1e-12"').replace('iterations="100"', 'iterations="200000"'), tmp_path, "c.hbm")
        rng = np.random.default_rng(3)
        for k in range(4):
            o.reset()
            o.qpos[:] = np.array(q0) + 0.02 * k; o.qvel[:] = rng.uniform(-1, 1, o.nv) * k
            o.forward()
            prob = eq_ref.stacked(o)
            nw, pg = eq_ref.solve_newton(o, prob), eq_ref.solve_pgs(o, prob, np.zeros(o.nv))
            assert nw["residual"] < 1e-12 * max(1.0, np.abs(prob["qfs"]).max())
            assert np.abs(nw["qacc"] - pg["qacc"]).max() < 1e-8 * max(1.0, np.abs(nw["qacc"]).max()), (k, nw["qacc"], pg["qacc"])
            assert np.abs(nw["force"] - pg["force"]).max() < 1e-8 * max(1.0, np.abs(nw["force"]).max())


def test_inactive_equalities_are_fric_ref(hbmod, tmp_path):
    """with every element inactive, or the flag set, eq_ref's step is fric_ref's, bit for bit"""
    for i, kw in enumerate((dict(inactive=True), dict(flag="disable"))):
        for name in ("eq28_cd3_pgs", "eq28_cd1_newton"):
            o = _small(hbmod, eq_chain_xml(name, **kw), tmp_path, "i%d%s.hbm" % (i, name))
            st, ct = fric_ref.rollout_states(o, steps=60)
            for k in range(len(st)):
                a, pa, sa = eq_ref.step(o, st[k], ct[k].astype(np.float64))
                b, pb, sb = fric_ref.step(o, st[k], ct[k].astype(np.float64))
                assert pa["ne"] == 0 and np.array_equal(a, b) and np.array_equal(sa["force"], sb["force"]), (name, kw, k)


def test_gpu_state_sets_cover_the_rows(hbmod, eq_tmp):
    """what the GPU tests' states exercise, by the reference alone"""
    for name in MODELS:
        p, o, st, ct, ref = reference(name, eq_tmp)
        assert len(st) == 30
        assert max(ref["nefc"]) <= 63 and max(ref["ncon"]) <= 24, (name, max(ref["nefc"]), max(ref["ncon"]))
        con, lim = row_kinds(ref)
        assert con >= 10 and lim >= 10, (name, con, lim)
        assert all(n == NE for n in ref["ne"]) and all(n > 0 for n in ref["nf"]) and max(ref["ne"][0] + ref["nf"][0], 0) <= 32
        assert all(t[:NE].tolist() == [eq_ref.CNSTR_EQUALITY] * NE and t[NE:NE + n].tolist() == [fric_ref.CNSTR_FRICTION_DOF] * n for t, n in zip(ref["types"], ref["nf"]))
        assert (ref["zones"][0] + ref["zones"][1] > 0) and ref["zones"][2] > 0, (name, ref["zones"])  # some friction row at its bound, some inside
        assert ref["reverts"] == 0
        for k in range(len(st)):  # (the shifted contact addresses: a contact's first row is a contact row)
            for c in ref["con"][k]:
                assert c["efc_address"] < 0 or ref["types"][k][c["efc_address"]] in (5, 6)


def test_the_sanitizer_pass_model(hbmod, tmp_path):
    """tests/models/equalities.xml (what tools/asan_host.sh takes through compile -> save -> load -> save): every accepted form, five rows"""
    m = hbmod.Model.load(os.path.join(MODELS_DIR, "equalities.xml"))
    assert m.neq == 4 and m.equality_rows() == 3 + 1 + 1 and [e["name"] for e in m.equalities()] == ["close", "tether", "gear", "lock"]
    assert np.array_equal(m.array("eq_solref"), [0.03, 1, 0.01, 1, 0.03, 1, 0.01, 1])
    a, b = str(tmp_path / "a.hbm"), str(tmp_path / "b.hbm")
    m.save(a); hbmod.Model.load(a).save(b)
    assert open(a, "rb").read() == open(b, "rb").read()
    o = Oracle(a)
    o.reset(); o.forward()
    pos, elem = eq_ref.equality_pos(o)
    assert len(pos) == 5 and np.abs(pos[:3]).max() <= 1e-12 and abs(pos[4] + 0.01) < 1e-15


def test_id2name(hbmod):
    """hb_model_id2name, the inverse of hb_model_name2id that Model.equalities() reads its names through: every kind, an unnamed
    element, and the error returns (unknown kind, id out of range, a buffer without room for the terminator)"""
    import ctypes
    m = hbmod.Model.load(os.path.join(MODELS_DIR, "equalities.xml"))
    for kind, names in (("body", ["frame", "crank", "rod"]), ("joint", ["root", "a", "s"]), ("geom", ["floor", "frame"]), ("equality", ["close", "lock"])):
        for n in names:
            i = m.name2id(kind, n)
            assert i >= 0 and m.id2name(kind, i) == n, (kind, n)
    chain = hbmod.Model.from_xml_string(chain_xml(12).replace("</mujoco>", '<keyframe><key name="k0"/></keyframe></mujoco>'))
    assert chain.id2name("actuator", chain.name2id("actuator", "m_j3")) == "m_j3" and chain.id2name("key", 0) == "k0"
    tend = hbmod.Model.from_xml_string(_xml("").replace("<equality>", '<tendon><fixed name="t"><joint joint="a" coef="1"/></fixed></tendon><equality>'))
    assert tend.id2name("tendon", 0) == "t"
    assert m.id2name("geom", m.ngeom - 1) == ""  # (an unnamed geom)
    L, buf = hbmod.lib(), ctypes.create_string_buffer(8)
    assert L.hb_model_id2name(m._h, b"body", 1, buf, 8) == 5 and buf.value == b"frame"
    assert L.hb_model_id2name(m._h, b"body", 1, buf, 5) < 0 and L.hb_model_id2name(m._h, b"body", 1, buf, 6) == 5  # ("frame" needs six bytes)
    for kind, i in ((b"body", -1), (b"body", m.nbody), (b"equality", 4), (b"site", 0)):
        assert L.hb_model_id2name(m._h, kind, i, buf, 8) < 0, (kind, i)
    with pytest.raises(hbmod.HbError):
        m.id2name("equality", 99)
