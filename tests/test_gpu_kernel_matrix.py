"""Every step kernel, named and held to the fp64 oracle at the sizes where the dispatch (hb_step.hip: select_step, launch_step) and
the dense, padded code change: nv 20 / 21 (the general Newton kernels' order 20, C stride 21), 28 / 29 (the classic kernels' order 28
and 32; a dense block with no padding row, then an odd order), 31 and 32, on capsule chains (tests/kernel_models.py) and on same-size
variants of the two assets the size-specialised kernels were written for.

TABLE has one row per (model, launch, knobs) and the kernel that launch must run (Batch.last_kernel).  For every model:
  - the full one-step kernel with the diagnostic outputs ("diag") against the oracle, teacher-forced from states every 10 steps along a
    300-step oracle rollout (rounded to fp32 first, then stepped by both): counts identical, PGS sweep counts identical, qacc and
    efc_force within 4e-4 * max(1, max|.|), qpos within 4e-5 relative, qvel within 4e-4 * max(1, max|qvel|), contact dist / pos
    within 1e-5 and frame within 1e-3, status zero (bounds.BOUNDS, the golden bounds of tests/test_gpu_parity.py);
  - every other launch of the row set bit for bit against it: one-step launches ("step") against the diag step, multi-step launches
    ("rollout", "steps": T single step calls) against the full kernel's T-step rollout ("rollout_qpos"), in state, counts and status;
  - rows whose knob selects another algorithm (staged=0, fastpass=0: the fused general step) are diag launches held to the oracle;
  - variants 2 and 3 run their diag step in the big kernel (BIG_KERNELS): there the one-group fast kernels' one-step reference is the
    full fast instantiation, its state, counts and sweep counts held to the oracle step.
Height-field rows use the rounding-fence allowance of tests/test_gpu_convex.py: a state whose contact set differs from the oracle's
must be PROVED to sit within fp32 rounding of one where the oracle gives the device's contacts (oracle_lib.prove_rounding_fence).
The worst deviation of every model is printed (pytest -s); profiles/kernel_matrix_parity.txt holds the numbers measured on MI355X.
"""
import os

import numpy as np
import pytest

from inverse_ref import force_scale, forward_at, inverse_terms
from kernel_models import CONFIG_COLUMNS, chain_xml, kernel_table, oracle_for, oracle_steps, perturbed_hbm, rollout_states, row_kinds
from oracle_lib import HFIELD_HBM, HUMANOID_HBM, MODELS_DIR, TEAM_HBM, Oracle
from step_lib import CHAINS, T, kernel_names_in_source, result, same, state_vs_oracle, vs_oracle

# ---- models: the generated chains (step_lib.CHAINS) and the assets / their same-size copies
# the assets: (path, solver override, keyframe, perturbed)
ASSET_MODELS = {
    "humanoid27_pgs": (HUMANOID_HBM, None, -1, False),
    "humanoid27_newton": (HUMANOID_HBM, 2, -1, False),
    "humanoid27_hfield": (HFIELD_HBM, None, -1, False),
    "team_robot": (TEAM_HBM, None, 0, False),
    "humanoid27_perturbed_pgs": (HUMANOID_HBM, None, -1, True),
    "humanoid27_perturbed_newton": (HUMANOID_HBM, 2, -1, True),
    "team_robot_perturbed": (TEAM_HBM, None, 0, True),
}

# ---- the expected-kernel table: model -> [(launch, knobs, kernel)]
V0_PGS = [("diag", {}, "hb_step_kernel"), ("step", {}, "hb_step_lean_kernel"), ("rollout_qpos", {}, "hb_step_kernel"),
          ("rollout", {}, "hb_step_lean_q_kernel"), ("steps", {}, "hb_step_lean_kernel"), ("step", {"lean": 0}, "hb_step_kernel"),
          ("rollout", {"lean": 0}, "hb_step_kernel")]
V0_PGS32 = [("diag", {}, "hb_step32_kernel"), ("step", {}, "hb_step32_kernel"), ("rollout_qpos", {}, "hb_step32_kernel"),
            ("rollout", {}, "hb_step32_kernel"), ("steps", {}, "hb_step32_kernel")]
V0_NEWTON = [("diag", {}, "hb_step_newton28_kernel"), ("step", {}, "hb_step_newton28_lean_kernel"), ("rollout_qpos", {}, "hb_step_newton28_kernel"),
             ("rollout", {}, "hb_step_newton28_lean_q_kernel"), ("steps", {}, "hb_step_newton28_lean_kernel"),
             ("step", {"lean": 0}, "hb_step_newton28_kernel"), ("rollout", {"lean": 0}, "hb_step_newton28_kernel")]
V0_NEWTON32 = [("diag", {}, "hb_step_newton32_kernel"), ("step", {}, "hb_step_newton32_kernel"), ("rollout_qpos", {}, "hb_step_newton32_kernel"),
               ("rollout", {}, "hb_step_newton32_kernel"), ("steps", {}, "hb_step_newton32_kernel")]
V1 = [("diag", {}, "hb_step_gen_fast_kernel"), ("step", {}, "hb_step_gen_fast_lean_kernel"), ("rollout_qpos", {}, "hb_step_gen_fast_kernel"),
      ("rollout", {}, "hb_step_gen_fast_lean_kernel"), ("steps", {}, "hb_step_gen_fast_lean_kernel"), ("step", {"lean": 0}, "hb_step_gen_fast_kernel"),
      ("diag", {"staged": 0}, "hb_step_gen_kernel"), ("diag", {"fastpass": 0}, "hb_step_gen_kernel")]
V2_20 = [("diag", {}, "hb_step_newton_big20_kernel"), ("step", {}, "hb_step_newton_gen20_lean_kernel"),
         ("rollout_qpos", {}, "hb_step_newton_gen20_kernel"), ("rollout", {}, "hb_step_newton_gen20_lean_kernel"),
         ("steps", {}, "hb_step_newton_gen20_lean_kernel"), ("step", {"lean": 0}, "hb_step_newton_gen20_kernel"),
         ("step", {"narrow_prim": 0}, "hb_step_newton_gen20_lean_kernel"),
         ("diag", {"staged": 0}, "hb_step_newton_big20_kernel"), ("diag", {"fastpass": 0}, "hb_step_newton_big20_kernel")]
V2_28 = [("diag", {}, "hb_step_newton_big28_kernel"), ("step", {}, "hb_step_newton_gen28_kernel"), ("step", {"lean": 0}, "hb_step_newton_gen28_kernel"),
         ("rollout_qpos", {}, "hb_step_newton_gen28_kernel"),
         ("rollout", {}, "hb_step_newton_gen28_kernel"), ("steps", {}, "hb_step_newton_gen28_kernel"),
         ("step", {"narrow_prim": 0}, "hb_step_newton_gen28_kernel"),
         ("diag", {"staged": 0}, "hb_step_newton_big28_kernel"), ("diag", {"fastpass": 0}, "hb_step_newton_big28_kernel")]
V3 = [("diag", {}, "hb_step_gen_big_kernel"), ("step", {}, "hb_step_gen_fast1_kernel"), ("step", {"lean": 0}, "hb_step_gen_fast1_kernel"),
      ("rollout_qpos", {}, "hb_step_gen_fast1_kernel"),
      ("rollout", {}, "hb_step_gen_fast1_kernel"), ("steps", {}, "hb_step_gen_fast1_kernel"), ("step", {"narrow_prim": 0}, "hb_step_gen_fast1_kernel"),
      ("diag", {"staged": 0}, "hb_step_gen_big_kernel"), ("diag", {"fastpass": 0}, "hb_step_gen_big_kernel")]
H27_PGS = [("diag", {}, "hb_step_kernel"), ("step", {}, "hb_step_h27_kernel"), ("rollout_qpos", {}, "hb_step_kernel"),
           ("rollout", {}, "hb_step_h27_q_kernel"), ("steps", {}, "hb_step_h27_kernel"), ("step", {"sized": 0}, "hb_step_lean_kernel"),
           ("rollout", {"sized": 0}, "hb_step_lean_q_kernel"), ("steps", {"sized": 0}, "hb_step_lean_kernel"),
           ("step", {"duo": 2}, "hb_step_duo_kernel"), ("rollout", {"duo": 2}, "hb_step_duo_q_kernel"), ("step", {"lean": 0}, "hb_step_kernel")]
H27_NEWTON = [("diag", {}, "hb_step_newton28_kernel"), ("step", {}, "hb_step_newton28_h27_kernel"), ("rollout_qpos", {}, "hb_step_newton28_kernel"),
              ("rollout", {}, "hb_step_newton28_lean_q_kernel"), ("steps", {}, "hb_step_newton28_h27_kernel"),
              ("step", {"sized": 0}, "hb_step_newton28_lean_kernel"), ("steps", {"sized": 0}, "hb_step_newton28_lean_kernel")]
H27_HFIELD = [("diag", {}, "hb_step_gen_fast_kernel"), ("step", {}, "hb_step_gen_fast_h27_kernel"), ("rollout_qpos", {}, "hb_step_gen_fast_kernel"),
              ("rollout", {}, "hb_step_gen_fast_h27_kernel"), ("steps", {}, "hb_step_gen_fast_h27_kernel"),
              ("step", {"sized": 0}, "hb_step_gen_fast_lean_kernel"), ("rollout", {"sized": 0}, "hb_step_gen_fast_lean_kernel")]
TEAM = [("diag", {}, "hb_step_newton_big20_kernel"), ("step", {}, "hb_step_newton_gen20_team_kernel"), ("step", {"lean": 0}, "hb_step_newton_gen20_kernel"),
        ("rollout_qpos", {}, "hb_step_newton_gen20_kernel"),
        ("rollout", {}, "hb_step_newton_gen20_team_kernel"), ("steps", {}, "hb_step_newton_gen20_team_kernel"),
        ("step", {"sized": 0}, "hb_step_newton_gen20_lean_kernel"), ("rollout", {"sized": 0}, "hb_step_newton_gen20_lean_kernel")]


def _chain_rows(spec):
    nv, _, floor, condim, solver = spec
    if floor == "hfield":
        return V1
    if condim in (4, 6):
        return (V2_20 if nv <= 20 else V2_28) if solver == "Newton" else V3
    if solver == "Newton":
        return V0_NEWTON if nv <= 28 else V0_NEWTON32
    return V0_PGS if nv <= 28 else V0_PGS32


TABLE = {name: _chain_rows(spec) for name, spec in CHAINS.items()}
TABLE.update(humanoid27_pgs=H27_PGS, humanoid27_newton=H27_NEWTON, humanoid27_hfield=H27_HFIELD, team_robot=TEAM,
             humanoid27_perturbed_pgs=H27_PGS, humanoid27_perturbed_newton=H27_NEWTON, team_robot_perturbed=TEAM)
# With the diagnostic outputs on, a variant-2 / -3 model steps in its own variant's kernel (the four- / two-group one: hb_batch.cpp, "the
# diagnostic buffers are laid out for the kernel of the model's own variant"), not in the one-group fast kernel of its staged step.  For
# those models the diag row is held to the oracle in full, and the fast kernels' one-step reference is the full fast instantiation
# (lean=0), whose state, counts and sweep counts are held to the oracle step.
BIG_KERNELS = {"hb_step_newton_big20_kernel", "hb_step_newton_big28_kernel", "hb_step_gen_big_kernel"}
DUO_KERNELS = {"hb_step_duo_kernel", "hb_step_duo_q_kernel"}  # (also held to the one-env kernel by tests/test_gpu_duo.py)
NOT_BIT_IDENTICAL = ("staged", "fastpass")  # knobs that select another algorithm: those rows are held to the oracle instead


def test_table_names_every_step_kernel():
    """(CPU) the table must name every step-kernel instantiation of hb_step.hip / hb_step_duo.hip: a new one fails here until it has a
    row, and a row cannot name a kernel that does not exist"""
    table = {k for rows in TABLE.values() for _, _, k in rows}
    src = kernel_names_in_source()
    assert len(src) >= 25
    assert src == table | DUO_KERNELS, (sorted(src - table - DUO_KERNELS), sorted(table - src))


def test_kernel_table_rows_are_unique():
    """(CPU) the dispatch takes the first row whose configuration matches (hb_step.hip: find_step_kernel), so a second row with the same
    eleven configuration columns would be shadowed silently, and a second row with the same name would not even be a second kernel"""
    rows = kernel_table()
    assert len(rows) >= 55
    names = [n for n, _ in rows]
    configs = [tuple(c[k] for k in CONFIG_COLUMNS) for _, c in rows]
    assert len(set(names)) == len(names), sorted(n for n in set(names) if names.count(n) > 1)
    assert len(set(configs)) == len(configs), sorted(n for (n, _), c in zip(rows, configs) if configs.count(c) > 1)


def test_generated_models_stay_inside_the_engine_and_reach_their_rows(hbmod, tmp_path):
    """(CPU) every generated model compiles to the sizes it was asked for inside the engine's limits, takes the variant its row expects
    (read off its row capacities) and, along its oracle rollout, has states with contact rows and states with joint-limit rows"""
    for name, spec in CHAINS.items():
        nv, _, floor, condim, solver = spec
        m, p, o = oracle_for(hbmod, chain_xml(*spec), tmp_path)
        assert m.nv == nv and m.nbody <= 64 and m.ngeom <= 64 and m.nM <= 1023, name
        general = floor == "hfield" or condim in (4, 6)
        caps = (48, 256) if general and solver == "Newton" else (48, 128) if condim in (4, 6) else (24, 63)  # (variants 2, 3; 0 and 1)
        assert (m.ncon_max, m.nefc_max) == caps, (name, m.ncon_max, m.nefc_max)
        st, ct = rollout_states(o)
        ref = oracle_steps(o, st, ct)
        con, lim = row_kinds(ref)
        assert con >= 10 and lim >= 10, (name, con, lim)
        assert max(ref["nefc"]) <= m.nefc_max and max(ref["ncon"]) <= m.ncon_max


# ---------------------------------------------------------------------------------------------------------------- GPU
def _setup(hbmod, name, tmp_path):
    """(model, .hbm path, oracle, states, controls, uses a height field or meshes)"""
    if name in CHAINS:
        spec = CHAINS[name]
        m, p, o = oracle_for(hbmod, chain_xml(*spec), tmp_path)
        st, ct = rollout_states(o)
        return m, p, o, st, ct, spec[2] == "hfield"
    path, solver, key, perturbed = ASSET_MODELS[name]
    if perturbed:
        path = perturbed_hbm(path, str(tmp_path / os.path.basename(path)), seed=3)
    m, o = hbmod.Model.load(path), Oracle(path)
    if solver is not None:
        m.set_opt(solver=solver, iterations=100)
        o.set_opt(solver=solver, iterations=100)
    st, ct = rollout_states(o, keyframe=key)
    return m, path, o, st, ct, path.endswith(("hfield.hbm", "team_robot.hbm"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_kernel_matrix(hbmod, gpu, tmp_path, name):
    m, path, o, st, ct, fences_ok = _setup(hbmod, name, tmp_path)
    rows = TABLE[name]
    n = len(st)
    ctrlT = np.random.default_rng(5).uniform(-1, 1, (T, n, m.nu)).astype(np.float32)
    ctrlT[0] = ct

    def batch(knobs):
        b = hbmod.Batch(m, n, gpu)
        b.tune(**knobs)
        return b
    print("\n%s (nv %d):" % (name, m.nv))
    # the references: the diag step (against the oracle) and the full kernel's T-step rollout
    b = batch({})
    vs_oracle(hbmod, b, o, st, ct, fences_ok, name + " diag")
    ref1 = result(hbmod, b)
    fast = rows[0][2] in BIG_KERNELS
    if fast:
        f = batch({"lean": 0})
        f.set_state(hbmod.STATE_INTEGRATION, st)
        f.step(ct)
        state_vs_oracle(hbmod, f, o, st, ct, fences_ok, "%s fast kernel [%s]" % (name, f.last_kernel()))
        ref1 = result(hbmod, f)
        f.close()
    b.set_state(hbmod.STATE_INTEGRATION, st)
    qT = b.rollout(ctrlT, want_qpos=True)
    refT = result(hbmod, b)
    assert np.array_equal(qT[-1], refT[0][:, 1:1 + m.nq])
    assert ref1[1][1].max() > 0 and not refT[2].any()
    b.close()
    for launch, knobs, kernel in rows:
        label = "%s %s %s" % (name, launch, knobs or "")
        b = batch(knobs)
        if launch == "diag" and knobs:
            assert set(knobs) <= set(NOT_BIT_IDENTICAL), label
            vs_oracle(hbmod, b, o, st, ct, fences_ok, label)
        elif launch == "diag":
            b.diag_enable(True); b.set_state(hbmod.STATE_INTEGRATION, st); b.step(ct)
            if not fast:
                same(result(hbmod, b), ref1, label)
        elif launch == "step":
            b.set_state(hbmod.STATE_INTEGRATION, st); b.step(ct)
            same(result(hbmod, b), ref1, label)
        elif launch == "steps":
            b.set_state(hbmod.STATE_INTEGRATION, st)
            for t in range(T):
                b.step(ctrlT[t])
            same(result(hbmod, b), refT, label)
        else:
            b.set_state(hbmod.STATE_INTEGRATION, st)
            q = b.rollout(ctrlT, want_qpos=launch == "rollout_qpos")
            same(result(hbmod, b), refT, label)
            if q is not None:
                assert np.array_equal(q, qT), label
        assert b.last_kernel() == kernel, (label, b.last_kernel(), kernel)
        b.close()


@pytest.mark.gpu
def test_general_model_past_28_dofs_is_refused(hbmod, gpu):
    for spec in ((29, True, "plane", 6, "Newton"), (29, True, "plane", 4, "PGS"), (29, True, "hfield", 3, "PGS")):
        m = hbmod.Model.from_xml_string(chain_xml(*spec))
        with pytest.raises(hbmod.HbError, match="at most 28 degrees of freedom"):
            hbmod.Batch(m, 4, gpu)


def test_perturbed_copies_keep_the_sizes(hbmod, tmp_path):
    """(CPU) the same-size copies differ from their assets where they should, and nowhere in their sizes"""
    for src in (HUMANOID_HBM, TEAM_HBM):
        p = perturbed_hbm(src, str(tmp_path / os.path.basename(src)), seed=3)
        a, b = hbmod.Model.load(src), hbmod.Model.load(p)
        for k in ("nq", "nv", "nu", "nbody", "njnt", "ngeom", "ntendon", "nM", "npair", "ncon_max", "nefc_max"):
            assert getattr(a, k) == getattr(b, k), k
        for field in ("body_mass", "jnt_axis", "jnt_range", "dof_damping", "geom_size", "actuator_gear"):
            x, y = a.array(field), b.array(field)
            assert x.shape == y.shape and not np.array_equal(x, y), field


@pytest.mark.gpu
def test_schedule_knob_is_bit_identical_on_a_pipelined_batch(hbmod, humanoid_model, gpu):
    """HB_TUNE_SCHEDULE: the heavy-first dispatch order changes which wave steps which env, never an env's result - 1024 envs, pipelined,
    ten step calls"""
    n = 1024
    ctrl = np.random.default_rng(2).uniform(-1, 1, (10, n, humanoid_model.nu)).astype(np.float32)
    res = []
    for sched in (1, 0):
        b = hbmod.Batch(humanoid_model, n, gpu)
        b.reset(perturb=True)
        b.rollout_halton(150)  # (onto the floor: envs with very different row counts)
        b.tune(schedule=sched)
        b.pipeline(True)
        for t in range(10):
            b.step(ctrl[t])
        b.join()
        res.append(result(hbmod, b))
        assert b.segments > 1
        b.close()
    same(res[0], res[1], "schedule=0")
    assert res[0][1][1].max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["ball_hfield", "chain28_cd6_newton"])
def test_narrow_prim_knob_is_bit_identical(hbmod, gpu, tmp_path, model):
    """HB_TUNE_NARROW_PRIM: the staged narrowphase's primitive-only collider against the general one - same contacts, same bits"""
    if model in CHAINS:
        m, p, o = oracle_for(hbmod, chain_xml(*CHAINS[model]), tmp_path)
        st, ct = rollout_states(o)
    else:
        m = hbmod.Model.load(os.path.join(MODELS_DIR, model + ".xml"))
        p = str(tmp_path / "m.hbm"); m.save(p)
        st, ct = rollout_states(Oracle(p))
    n = len(st)
    res = []
    for prim in (1, 0):
        b = hbmod.Batch(m, n, gpu)
        b.tune(narrow_prim=prim)
        b.set_state(hbmod.STATE_INTEGRATION, st)
        for _ in range(T):
            b.step(ct)
        res.append(result(hbmod, b))
        b.close()
    same(res[0], res[1], model + " narrow_prim=0")
    assert res[0][1][0].max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,kernel", [("chain21_cd3_pgs", "hb_inverse_kernel"), ("chain28_cd1_newton", "hb_inverse_kernel"),
                                         ("chain28_fixed_cd3_pgs", "hb_inverse_kernel"), ("chain29_cd1_newton", "hb_inverse32_kernel"),
                                         ("chain31_cd3_pgs", "hb_inverse32_kernel")])
def test_inverse_at_the_boundaries(hbmod, gpu, tmp_path, name, kernel):
    """hb_inverse at the dense orders' edges (28: no padding row; 29, 31: odd orders of the 32 instantiation) against the fp64
    restatement of tests/inverse_ref.py, on the oracle's states and random accelerations (the bounds of test_gpu_inverse.py)"""
    m, p, o, st, ct, _ = _setup(hbmod, name, tmp_path)
    nq, nv = m.nq, m.nv
    qpos, qvel = st[:, 1:1 + nq].astype(np.float32), st[:, 1 + nq:1 + nq + nv].astype(np.float32)
    qacc = np.random.default_rng(7).normal(size=qvel.shape).astype(np.float32) * 5.0
    b = hbmod.Batch(m, len(st), gpu)
    b.set_state(hbmod.STATE_INTEGRATION, np.concatenate([np.zeros((len(st), 1)), qpos, qvel, np.zeros_like(qvel)], axis=1))
    for discrete in (False, True):
        got = b.inverse(qacc, discrete=discrete)
        assert b.last_kernel() == kernel
        err, active = [], 0
        for e in range(len(st)):
            forward_at(o, qpos[e].astype(np.float64), qvel[e].astype(np.float64))
            t = inverse_terms(o, qacc[e].astype(np.float64), discrete)
            err.append(np.abs(got[e] - (t["Mqacc"] + t["bias"] - t["passive"] - t["constraint"])).max() / force_scale(t))
            active += t["active"]
        print("inverse %s discrete=%d: worst %.2e median %.2e, %d active rows" % (name, discrete, max(err), np.median(err), active))
        assert active > 0 and max(err) < 1e-3, (name, discrete, max(err))
    b.close()
