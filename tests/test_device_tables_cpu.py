"""The device model tables as the host builds them (csrc/hb_tables.cpp), through the build/hb_tables tool: no GPU.

(a) every refusal of build_model_tables that a model file can reach, with its exact message, each from a minimal model that breaks that
one rule only; (b) for the two flagship models and tests/models/equalities.xml the sizes and flags the kernel constants state
(hb_device.hpp: kSizedHumanoid27, kSizedTeamV1), every pointer fix-up inside its array, and the dense view of the mass matrix.

Refusals this file cannot reach, and why:
  - "sparse mass matrix too large for the packed index tables" (nM > 1023): nv <= 32 is checked first, and 32 dofs give at most 528 entries;
  - "general collision: more than 65535 candidate pairs": 64 geoms, checked first, give at most 2016 pairs;
  - "contact dimension N does not exist": the compiler accepts condim 1, 3, 4, 6 only, and an .hbm with another one is a compiler bug;
  - the two LDS-layout refusals: no model within the size limits above needs more LDS than a CU has;
  - "mesh edge graph too large for the packed link words": a hull of more than 2040 neighbours on one vertex.
More than 64 bodies, a ball joint and an unknown integrator cannot come from MJCF: the compiler refuses them first ("model: nbody must be
1..64", "joint type 'ball' is not supported", "integrator 'implicit' is not implemented").  The body limit is held by its other half, 65
geoms.  The loader refuses an .hbm with another integrator as well, so that refusal is reached the way a caller could reach it if
hb_options_set let the value through: the tool's --integrator option, which sets the field behind the loader.  The ball joint is not
reached at all: an .hbm edited to jnt_type 1 fails the loader's "nq / nv do not match the joints", and a consistent one needs the dof
tables of a joint type nothing in this project writes.
"""
import os

import numpy as np
import pytest

from eq_models import add_equality
from fric_models import add_friction
from kernel_models import chain_xml
from oracle_lib import ASSETS, MODELS_DIR
from tables_lib import GENERAL_28, STAGED, fields, read_dump, run


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return p


def model(body, option="", asset="", tail=""):
    return ('<mujoco model="t"><option timestep="0.004" %s/>%s<worldbody><geom name="floor" type="plane" size="0 0 1"/>%s</worldbody>%s</mujoco>'
            % (option, asset, body, tail))


def link(k, joints=1, children=""):
    """one body with `joints` hinges and a capsule; children: the MJCF of its child bodies"""
    j = "".join('<joint name="j%d_%d" type="hinge" axis="%s" armature="0.01"/>' % (k, i, ("0 1 0", "0 0 1", "1 0 0", "1 1 0")[i]) for i in range(joints))
    return '<body name="b%d" pos="0.1 0 0.5">%s<geom type="capsule" fromto="0 0 0 0.1 0 0" size="0.02" mass="0.1"/>%s</body>' % (k, j, children)


def nested(n):
    """a chain of n links, one hinge each"""
    xml = ""
    for k in reversed(range(n)):
        xml = link(k, 1, xml)
    return xml


EQ = '<equality><joint joint1="j1" joint2="j3"/></equality>'
LOCKS = "<equality>" + "".join('<joint joint1="j%d"/>' % j for j in range(20)) + "</equality>"
HFIELD_ASSET = '<asset><hfield name="h" nrow="2" ncol="2" size="1 1 0.1 0.1" elevation="0 0.1 0.2 0"/></asset>'
# name -> (the model's MJCF, tool options, the message)
XML_REFUSALS = {
    "nv_33": (chain_xml(33), (), "this build supports nv <= 32 degrees of freedom"),
    # (more than 64 bodies: the model loader's own validation refuses the file first, "model: nbody must be 1..64"; the same rule, by its geoms)
    "geoms_66": (model('<body name="b" pos="0 0 1"><joint type="hinge" axis="0 1 0"/>%s</body>' % "".join('<geom type="sphere" size="0.01" pos="%g 0 0" mass="0.01"/>' % (0.03 * g) for g in range(65))),
                 (), "this build supports at most 64 bodies and 64 geoms"),
    "hfield_on_a_body": (model('<body name="b" pos="0 0 1"><joint type="hinge" axis="0 1 0" armature="0.01"/><geom type="sphere" size="0.05" mass="1"/><geom type="hfield" hfield="h"/></body>', asset=HFIELD_ASSET),
                         (), "height fields must be attached to the world body"),
    "joints_4": (model(link(0, joints=4)), (), "at most 3 joints per body are supported (body 'b0')"),
    "children_9": (model(link(0, 1, "".join(link(1 + c) for c in range(9)))), (), "at most 8 child bodies per body are supported (body 'b0')"),
    "depth_17": (model(nested(17)), (), "kinematic trees deeper than 16 bodies are not supported"),
    # tests/test_gpu_kernel_matrix.py::test_general_model_past_28_dofs_is_refused
    "general_29_newton_cd6": (chain_xml(29, True, "plane", 6, "Newton"), (), GENERAL_28),
    "general_29_pgs_cd4": (chain_xml(29, True, "plane", 4, "PGS"), (), GENERAL_28),
    "general_29_hfield": (chain_xml(29, True, "hfield", 3, "PGS"), (), GENERAL_28),
    # tests/test_gpu_fric.py::test_refusals
    "fric_hfield": (add_friction(chain_xml(12, floor="hfield")), (), "friction loss: " + STAGED + "remove the joints' frictionloss or set <flag frictionloss=\"disable\"/>"),
    "fric_cd6": (add_friction(chain_xml(12, condim=6)), (), "friction loss: " + STAGED + "remove the joints' frictionloss or set <flag frictionloss=\"disable\"/>"),
    "fric_cd6_newton": (add_friction(chain_xml(12, condim=6, solver="Newton")), (), "friction loss: " + STAGED + "remove the joints' frictionloss or set <flag frictionloss=\"disable\"/>"),
    "fric_rk4": (add_friction(chain_xml(12)), ("--integrator", 1), "friction loss: the RK4 integrator is not implemented for a model with joint frictionloss: use the Euler integrator"),
    # tests/test_gpu_eq.py::test_refusals
    "eq_hfield": (add_equality(chain_xml(12, floor="hfield"), EQ), (), "equality constraints: " + STAGED + "remove the <equality> section or set <flag equality=\"disable\"/>"),
    "eq_cd6": (add_equality(chain_xml(12, condim=6), EQ), (), "equality constraints: " + STAGED + "remove the <equality> section or set <flag equality=\"disable\"/>"),
    "eq_cd6_newton": (add_equality(chain_xml(12, condim=6, solver="Newton"), EQ), (), "equality constraints: " + STAGED + "remove the <equality> section or set <flag equality=\"disable\"/>"),
    "eq_rk4": (add_equality(chain_xml(12), EQ), ("--integrator", 1), "equality constraints: the RK4 integrator is not implemented for a model with equality rows: use the Euler integrator"),
    "rows_33": (add_equality(add_friction(chain_xml(32)), LOCKS), (), "equality constraints: 20 equality rows and 13 friction-loss rows: a model may have at most 32 always-active rows"),
}


@pytest.mark.parametrize("name", sorted(XML_REFUSALS))
def test_refusal_from_mjcf(name, tmp_path):
    xml, options, message = XML_REFUSALS[name]
    rc, out = run(write(tmp_path, name + ".xml", xml), *options)
    assert (rc, out) == (1, "refused: " + message + "\n")


def test_32_always_active_rows_fit(tmp_path):
    """one lock fewer than rows_33: accepted, 19 + 13 rows"""
    rc, out = run(write(tmp_path, "m.xml", add_equality(add_friction(chain_xml(32)), LOCKS.replace('<joint joint1="j19"/>', ""))))
    f = fields(out)
    assert rc == 0 and (f["neq_rows"], f["nfric"]) == (19, 13)


@pytest.mark.parametrize("name", ["team_robot.hbm", "humanoid27_hfield.hbm"])
def test_rk4_on_a_staged_model_is_refused(name):
    """tests/test_gpu_rk4.py::test_staged_models_are_refused_not_stepped_with_euler"""
    rc, out = run(os.path.join(ASSETS, name), "--integrator", 1)
    assert (rc, out) == (1, "refused: RK4: " + STAGED + "use the Euler integrator\n")
    assert run(os.path.join(ASSETS, name))[0] == 0


def test_unknown_integrator():
    assert run(os.path.join(MODELS_DIR, "pendulum.xml"), "--integrator", 2) == (1, "refused: integrator 2 is not implemented (Euler = 0, RK4 = 1)\n")


# ---- (b)
# the sizes of kSizedHumanoid27 and kSizedTeamV1 (hb_device.hpp), and what the reference models are besides
EXPECT = {
    "humanoid27": dict(nq=28, nv=27, nu=21, nbody=17, njnt=22, ngeom=20, ntendon=2, nM=243, ntree=1, npair=159, nlevel=7, nlimcand=46, nstate=83,
                       variant=0, nfric=0, neq_rows=0, sized_h27=1, sized_team=0, fast_lds_floats=0),
    "team_robot": dict(nq=19, nv=18, nu=12, nbody=15, njnt=13, ngeom=13, ntendon=0, nM=117, ntree=1, npair=37, nlevel=5, nlimcand=24, nstate=56,
                       variant=2, nfric=0, neq_rows=0, sized_h27=0, sized_team=1),
    # tests/models/equalities.xml: the rows its own header lists; no size-specialised kernel
    "equalities": dict(variant=0, sized_h27=0, sized_team=0, fast_lds_floats=0),
}
PATHS = {"humanoid27": os.path.join(ASSETS, "humanoid27.hbm"), "team_robot": os.path.join(ASSETS, "team_robot.hbm"),
         "equalities": os.path.join(MODELS_DIR, "equalities.xml")}
ARRAY_CODE = {"int": 0, "float": 1, "u64": 2}


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_tables_of_the_reference_models(name, tmp_path, hbmod):
    dump = tmp_path / "tables.bin"
    rc, out = run(PATHS[name], "--dump", dump)
    assert rc == 0
    f = fields(out)
    for k, v in EXPECT[name].items():
        assert f[k] == v, (k, f[k], v)
    m = hbmod.Model.load(PATHS[name])
    for k in ("nq", "nv", "nu", "nbody", "njnt", "ngeom", "ntendon", "nM", "npair"):
        assert f[k] == getattr(m, k), k
    assert f["nstate"] == 1 + f["nq"] + 2 * f["nv"] and f["nobs"] == m.nobs
    assert f["lds_floats"] > 0 and f["lds_floats"] % 4 == 0 and f["lds_floats"] * 4 <= 160 * 1024
    if name == "team_robot":  # the Newton layout on 256 rows, and the fast kernel's variant-1 layout
        assert (f["ncon_max"], f["nefc_max"], f["cstride"]) == (48, 256, 21) and 0 < f["fast_lds_floats"] < f["lds_floats"]
    else:
        assert (f["ncon_max"], f["nefc_max"], f["cstride"]) == (24, 63, 33)
    if name == "equalities":
        eq_type = np.asarray(m.array("eq_type")).astype(int)
        active = np.asarray(m.array("eq_active0")).astype(int)
        assert f["neq_rows"] == int(np.where(eq_type == 2, 1, 3)[active != 0].sum()) > 0
        assert f["nfric"] == int((np.asarray(m.array("dof_frictionloss")) > 0).sum())
    # every table lies inside its array, and the dump's fix-ups are the printed tables
    for t, (array, off, count, _) in f["table"].items():
        assert off + max(count, 1) <= f["array"][array], t
    iv, fix = read_dump(dump)
    printed = sorted((ARRAY_CODE[a], off) for t, (a, off, _, _) in f["table"].items() if t not in ("obs_jnt_act", "obs_src_act"))
    assert sorted((a, off) for _, a, off in fix) == printed and len(set(fo for fo, _, _ in fix)) == len(fix)
    for t in ("brec", "drec", "prec", "crec", "trec", "lrec", "arec", "frec", "erec", "mesh_vert", "mesh_nbr", "mesh_start"):
        assert f["table"][t][1] % 4 == 0, t  # (float4 records)
    # the dense view of the sparse mass matrix: symmetric, every entry once per triangle, nM the zero pad and nM + 1 the diagonal's pad
    array, off, count, _ = f["table"]["mdense"]
    assert (array, count) == ("int", 32 * 32) and len(iv) == f["array"]["int"]
    md = iv[off:off + count].reshape(32, 32)
    nv, nM = f["nv"], f["nM"]
    assert np.array_equal(md, md.T)
    assert (np.diag(md)[nv:] == nM + 1).all() and (np.diag(md)[:nv] < nM).all()
    off_diag = md[~np.eye(32, dtype=bool)]
    assert (off_diag[off_diag >= nM] == nM).all() and (md[nv:, :nv] == nM).all()
    assert sorted(md[np.tril_indices(32)][md[np.tril_indices(32)] < nM]) == list(range(nM))
