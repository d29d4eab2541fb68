"""Per-env model parameters (hb_env_domain_randomize: masses, armature, stiffness, limit margins and bounds, actuator gain / biasprm[1] /
force range, the floor-friction scale, the height map) in every kind of step kernel, against the fp64 oracle carrying the same parameters.

Every non-lean instantiation of the step template reads an env's block in place of the model tables.  ROWS names the smallest model
that reaches each instantiation and the kernels its launches must run (Batch.last_kernel).  A case is one row and one CONFIG: one
family of dr_ref.FAMILIES randomised alone (so that a kernel that ignores a small family cannot hide behind a large one), or "all".
A batch of N = 8 envs draws its blocks at once (env_domain_randomize on the plain Batch); the blocks are read back
(env_domain_params) and each env's diag step from teacher-forced states of the nominal rollout (kernel_models.rollout_states; ROUNDS
rounds, state (8 r + e) mod 30 on env e; row d "all": of the env's OWN rollout on its own block, so that it touches its own height
map - at least half of the cases must be in contact) is held to the oracle whose model arrays carry that env's block (dr_ref.apply): counts and PGS
sweep counts identical, status zero, qpos / qvel / qacc / efc_force / contact dist, pos, frame within bounds.BOUNDS.
The blocks are fp32 values handed to the oracle exactly: they add no error.  tests/test_dr_ref_cpu.py proves on the reference alone that
every (row, family) pair listed here is OBSERVABLE in every run mode the row has: the oracle's step with the env's block differs from its
step with the nominal block by at least 10 x the bound of a quantity THAT MODE COMPARES (a launch without diagnostic outputs: qpos, qvel
and the counts only) on at least half of the cases.  ROWS and the shared helpers live in tests/dr_rows.py.

  row                  kernels held                                              families (observable on the reference)
  a humanoid27_pgs     hb_step_kernel                                            mass arm_stiff limits actuator (the gain, kp 1 +- 0.3:
  b humanoid27_newton  hb_step_newton28_kernel                                   no motor of it is force-limited) friction
  c chain32_cd3_pgs    hb_step32_kernel                                          mass arm_stiff limits actuator friction
  c chain32_cd1_newton hb_step_newton32_kernel                                   mass arm_stiff limits actuator   (condim 1: no friction)
  d chain21_hfield_pgs hb_step_gen_fast_kernel; staged=0: hb_step_gen_kernel     mass arm_stiff limits actuator   (no plane floor: the scale
                       ("all": with every env's own height map)                                                   is ignored, pinned below)
  e chain21_cd6_pgs    hb_step_gen_big_kernel (diag), hb_step_gen_fast1_kernel   mass arm_stiff limits actuator friction
  e chain20_cd6_newton hb_step_newton_big20_kernel (diag), lean=0:               mass arm_stiff limits actuator friction
                       hb_step_newton_gen20_kernel (the narrow-phase kernels run too)
  f team_robot         hb_step_newton_big20_kernel (diag), lean=0:               mass arm_stiff limits actuator (kp 2 +- 0.5 and the force
                       hb_step_newton_gen20_kernel                               range)   (its floor is a height field: no friction scale)
  f chain21 position   hb_step_kernel                                            actuator (kp 2 +- 0.5 with bias1 = -gain: the team robot's
                       (chain21_cd3_pgs with <position kp="2"> servos)           motors have no affine bias, so this path needs servos)
  g fric28_cd1_newton  hb_fric_newton28_kernel   (reference: fric_ref.py)        mass arm_stiff limits actuator   (condim 1)
  g eq28_cd3_pgs       hb_eq_kernel              (reference: eq_ref.py)          mass arm_stiff limits actuator friction
  h humanoid27_rk4     hb_rk4_kernel             (reference: rk4_ref.py; the     mass arm_stiff limits actuator (the gain) friction
                       counts are the last stage's, sweep counts not compared)
The chains carry forcelimited motors here (chain_xml(forcerange=0.6)), so that the family "actuator" has a clamp to move.  On the
condim-6 rows the friction scale moves the sliding coefficient only: torsion and rolling stay the model's, in the device as in the
oracle (dr_ref.apply writes geom_friction[3 floor] alone).

Further: the launch forms under a block (rollout, step calls back to back, VecEnv substeps) bit for bit against single full-kernel steps;
switching the block off; the subtree sensors with per-env masses over the model's stale subtree mass; the draw itself against its numpy
restatement (dr_ref.draw) table by table; the masked redraw at an auto-reset; the friction scale on a model without a plane floor.
The worst deviations are printed (pytest -s); profiles/domain_params_parity.txt holds the numbers measured on MI355X.
"""
import numpy as np
import pytest

import dr_ref
from dr_rows import BOUNDS, CASES, N, ROUNDS, ROWS, T, config, deviation, ref_step, round_states, setup_row
from oracle_lib import load_state
from step_lib import report, result, same, state_vs_oracle, vs_oracle

# ---------------------------------------------------------------------------------------------------------------- GPU
def _vs_ref(hbmod, b, S, st, ct, label, before):
    """step_lib.vs_oracle for the rows whose reference is a restatement on top of the oracle (fric_ref, eq_ref, rk4_ref)"""
    b.diag_enable(True)
    b.set_state(hbmod.STATE_INTEGRATION, st)
    b.step(ct)
    dev = dict(qpos=b.qpos.astype(np.float64), qvel=b.qvel.astype(np.float64), qacc=b.qacc().astype(np.float64), force=b.efc_force().astype(np.float64))
    con = b.contacts().astype(np.float64)
    nc, ne, ni = b.counts()
    b.diag_enable(False)
    assert not b.status().any(), (label, b.status())
    worst = dict(qpos=0.0, qvel=0.0, qacc=0.0, force=0.0, dist=0.0, pos=0.0, frame=0.0)
    for k in range(len(st)):
        before(k)
        r = ref_step(S, st[k], ct[k])
        assert (nc[k], ne[k]) == (r["ncon"], r["nefc"]), (label, k, "counts differ", (nc[k], ne[k]), (r["ncon"], r["nefc"]))
        if r["niter"] is not None and ne[k]:
            assert ni[k] == r["niter"], (label, k, ni[k], r["niter"])
        for i, c in enumerate(r["con"]):
            assert (int(con[k, i, 14]), int(con[k, i, 15])) == (c["geom1"], c["geom2"]), (label, k, i)
            worst["dist"] = max(worst["dist"], abs(con[k, i, 0] - c["dist"]))
            worst["pos"] = max(worst["pos"], np.abs(con[k, i, 1:4] - c["pos"]).max())
            worst["frame"] = max(worst["frame"], np.abs(con[k, i, 4:13] - c["frame"].reshape(-1)).max())
        for key, x in deviation({q: v[k] for q, v in dev.items()}, r).items():
            worst[key] = max(worst[key], x)
        assert not dev["force"][k, r["nefc"]:].any()
    print("  %-48s worst %s" % (label, " ".join("%s %.2e" % kv for kv in worst.items())))
    for key, x in worst.items():
        assert x <= BOUNDS[key], (label, key, x, BOUNDS[key])
    return worst


def _profile(line):
    report(line, "HB_DR_PARITY_OUT", lead="  ")  # (set to collect the lines of profiles/domain_params_parity.txt)


def _batch(hbmod, gpu, S, D, knobs=None, n=N):
    b = hbmod.Batch(S["m"], n, gpu)
    b.tune(**(knobs or {}))
    b.env_domain_randomize(D)
    P = b.env_domain_params()
    return b, P, dr_ref.layout(S["m"], P.shape[1])


RUN_CASES = [(row, cfg, i) for row, cfg in CASES for i in range(len(ROWS[row]["runs"]))]  # (a case per run: a launch without diagnostic outputs fails on its own)


@pytest.mark.gpu
@pytest.mark.parametrize("row,cfg,run", RUN_CASES, ids=["%s-%s-%s" % (row, cfg, ROWS[row]["runs"][i][2]) for row, cfg, i in RUN_CASES])
def test_step_kernels_use_the_envs_parameters(hbmod, gpu, row, cfg, run):
    S = setup_row(row)
    o, base = S["o"], S["base"]
    knobs, mode, kernel = ROWS[row]["runs"][run]
    b, P, L = _batch(hbmod, gpu, S, config(S, cfg), knobs)
    assert np.abs(P[0] - P[1]).max() > 0  # (the envs differ)

    def before(k):
        dr_ref.apply(o, P[k], L, base)
    worst, touching = {}, 0
    try:
        for r in range(ROUNDS):
            st, ct = round_states(S, r, cfg)
            label = "%s %s %s %s round %d" % (row, cfg, mode, knobs or "", r)
            if S["kind"] != "plain":
                assert mode == "diag"
                w = _vs_ref(hbmod, b, S, st, ct, label, before)
            elif mode == "diag":
                w = vs_oracle(hbmod, b, o, st, ct, S["fences_ok"], label, before)
            else:
                b.set_state(hbmod.STATE_INTEGRATION, st)
                b.step(ct)
                w = state_vs_oracle(hbmod, b, o, st, ct, S["fences_ok"], label, before)
            assert b.last_kernel() == kernel, (label, b.last_kernel(), kernel)
            touching += int((b.counts()[0] > 0).sum())
            for key, x in w.items():
                worst[key] = max(worst.get(key, 0.0), x)
    finally:
        dr_ref.restore(o, base)
        b.close()
    _profile("%-22s %-10s %-28s %s, %d of %d cases in contact" % (row, cfg, kernel, " ".join("%s %.2e" % kv for kv in worst.items()), touching, N * ROUNDS))
    if cfg in ROWS[row].get("own_states", ()):  # (the envs stand on their own height maps: tests/test_dr_ref_cpu.py counts 25 of 32 on the oracle)
        assert touching >= N * ROUNDS // 2, (row, cfg, kernel, touching)


# ---- launch forms under a block
@pytest.mark.gpu
@pytest.mark.parametrize("row", ["a_humanoid27_pgs", "e_chain21_cd6_pgs"])
def test_launch_forms_under_a_block_are_bit_identical(hbmod, gpu, row):
    """a T-step rollout, T step calls enqueued back to back and VecEnv.step_arrays with n_substeps = T, each under a block, against T
    single steps of the full kernel - row a: T diag steps; row e: T steps with lean=0, because a variant-3 model's diag step runs the
    two-group kernel of its variant, which test_gpu_kernel_matrix holds to the oracle and not, bit for bit, to the one-group fast kernel
    (BIG_KERNELS there) - in state, counts and status; every launch names the full (non-lean) kernel"""
    S = setup_row(row)
    m = S["m"]
    D = config(S, "all")
    st, _ = round_states(S, 1)
    ctrl = np.random.default_rng(5).uniform(-1, 1, (N, m.nu)).astype(np.float32)
    ctrlT = np.repeat(ctrl[None], T, axis=0)  # (VecEnv holds one action over its substeps)
    full = "hb_step_kernel" if row.startswith("a_") else "hb_step_gen_fast1_kernel"
    big = not row.startswith("a_")
    b, P, _ = _batch(hbmod, gpu, S, D, {"lean": 0} if big else {})
    b.diag_enable(not big)
    b.set_state(hbmod.STATE_INTEGRATION, st)
    for t in range(T):
        b.step(ctrl)
        b.sync()
        assert b.last_kernel() == full, b.last_kernel()
    ref = result(hbmod, b)
    assert ref[1][1].max() > 0 and not ref[2].any()
    b.close()
    for form in ("rollout", "steps", "vecenv"):
        if form == "vecenv":
            env = hbmod.VecEnv(m, N, gpu, n_substeps=T, auto_reset=0, max_time=0.0, target_z=10.0)
            b = env.batch
            b.env_domain_randomize(D)
        else:
            b, _, _ = _batch(hbmod, gpu, S, D)
        assert np.array_equal(b.env_domain_params(), P), form
        b.set_state(hbmod.STATE_INTEGRATION, st)
        if form == "rollout":
            b.rollout(ctrlT)
        elif form == "steps":
            for t in range(T):
                b.step(ctrl)
        else:
            env.step_arrays(ctrl)
        same(result(hbmod, b), ref, "%s %s" % (row, form))
        assert b.last_kernel() == full, (row, form, b.last_kernel())
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("row,lean", [("a_humanoid27_pgs", ("hb_step_h27_kernel", "hb_step_h27_q_kernel")), ("e_chain21_cd6_pgs", ("hb_step_gen_fast1_kernel",))],
                         ids=["a_humanoid27_pgs", "e_chain21_cd6_pgs"])
def test_switching_the_block_off(hbmod, gpu, row, lean):
    """after env_domain_randomize(None) the batch steps bit-identically to one that never had a block, in the lean kernels such a batch
    runs: one step call, then T - 1 enqueued back to back.  (The humanoid's lean kernel has a twin that also writes the constraint
    forces out, hb_step_h27_q_kernel: a batch whose env buffers exist - env_domain_randomize allocates them - runs that one.)"""
    S = setup_row(row)
    st, ct = round_states(S, 1)
    res = []
    for had_block in (True, False):
        b = hbmod.Batch(S["m"], N, gpu)
        if had_block:
            b.env_domain_randomize(config(S, "all"))
            b.set_state(hbmod.STATE_INTEGRATION, st)
            b.step(ct)
            with_block = result(hbmod, b)
            b.env_domain_randomize(None)
            assert b.env_domain_params() is None
        b.set_state(hbmod.STATE_INTEGRATION, st)
        b.step(ct)
        b.sync()
        assert b.last_kernel() == (lean[-1] if had_block else lean[0]), (row, had_block, b.last_kernel())
        for t in range(T - 1):
            b.step(ct)
        res.append(result(hbmod, b))
        assert b.last_kernel() in lean, (row, had_block, b.last_kernel())
        if not had_block:
            b.set_state(hbmod.STATE_INTEGRATION, st)
            b.step(ct)
            assert not np.array_equal(result(hbmod, b)[0], with_block[0])  # (and the block did matter)
        b.close()
    same(res[0], res[1], row + " after env_domain_randomize(None)")


# ---- sensors: per-env masses over the model's (stale) subtree mass
@pytest.mark.gpu
def test_subtree_sensors_use_the_envs_masses(hbmod, gpu):
    """subtreecom and subtreelinvel of the whole tree and of a body's subtree, and framepos, with the mass family alone: the env's masses
    over the MODEL's subtree mass (body_subtreemass is a derived constant and stays stale, in MuJoCo as in the oracle's mj_comPos).
    Bounds: test_gpu_planner.py's (2e-4 of the largest entry for framepos | subtreecom | subtreelinvel of the tree, 2e-5 for the subtrees)."""
    from mjpc_ref import _ancestors, body_linvel
    S = setup_row("a_humanoid27_pgs")
    m, o, base = S["m"], S["o"], S["base"]
    nb = m.nbody
    head, foot, torso, waist = (m.name2id("body", n) for n in ("head", "foot_right", "torso", "waist_lower"))
    spec = hbmod.Batch.sensor_spec([head, foot], subtree_body=torso, subtreelinvel_bodies=[waist, foot])
    b, P, L = _batch(hbmod, gpu, S, config(S, "mass"))
    st, ct = round_states(S, 2)
    b.set_state(hbmod.STATE_INTEGRATION, st)
    s = b.sensors(spec, ct).astype(np.float64)
    b.close()
    assert s.shape == (N, 18)
    parent = o.info["body_parentid"]
    stale = base["body_mass"].copy()  # the model's subtree masses, restated from the model's masses
    sub = np.array([sum(stale[c] for c in range(1, nb) if r in _ancestors(c, parent)) for r in range(nb)])
    assert np.allclose(sub[1:], o.marr("body_subtreemass")[1:], rtol=1e-12)

    def reference():
        mass = o.marr("body_mass")
        xpos = o.xpos.reshape(nb, 3)
        lin = np.array([body_linvel(o, c, nb) if c else np.zeros(3) for c in range(nb)])
        out = [xpos[head], xpos[foot], o.subtree_com.reshape(nb, 3)[1], (mass[1:, None] * lin[1:]).sum(0) / sub[1]]
        for r in (waist, foot):
            members = [c for c in range(1, nb) if r in _ancestors(c, parent)]
            out.append(sum(mass[c] * lin[c] for c in members) / sub[r])
        return np.concatenate(out)
    worst, moved = np.zeros(2), 0
    try:
        for e in range(N):
            refs = []
            for block in (P[e], None):
                dr_ref.restore(o, base)
                if block is not None:
                    dr_ref.apply(o, block, L, base)
                load_state(o, st[e], ct[e].astype(np.float64))
                o.forward()
                refs.append(reference())
            ref, nominal = refs
            tol = np.concatenate([np.full(12, 2e-4), np.full(6, 2e-5)]) * max(1.0, np.abs(ref).max())
            err = np.abs(s[e] - ref)
            worst = np.maximum(worst, [(err[:12] / tol[:12]).max(), (err[12:] / tol[12:]).max()])
            assert (err <= tol).all(), (e, err / tol)
            moved += bool((np.abs(nominal - ref)[6:] >= 10 * tol[6:]).any())  # (the env's masses are visible in the subtree entries)
    finally:
        dr_ref.restore(o, base)
    _profile("sensors humanoid27 mass: worst / bound  framepos | subtreecom | subtreelinvel %.2f, subtreelinvel of two bodies %.2f; the masses move an entry by >= 10 x "
             "its bound in %d of %d envs" % (worst[0], worst[1], moved, N))
    assert moved >= N // 2


# ---- the draw
def _hold_draw(S, D, P, L, env_global, episodes, label):
    """P [n, stride] against dr_ref.draw table by table: equal but for contracted multiply-adds, within dr_ref.draw_bounds.  Returns
    table -> the worst distance in ulp of the largest term of the entry's expression (the unit of the bound, which is 2)"""
    worst = {t: 0.0 for t in dr_ref.TABLES}
    for e in range(len(P)):
        want, gain = dr_ref.draw(S["A"], D, env_global[e], episodes[e], want_gain=True)
        Bd = dr_ref.draw_bounds(S["A"], D, hfield_gain=gain)
        assert want.shape == P[e].shape
        for t in dr_ref.TABLES:
            g, w = dr_ref.table(P[e], L, t).astype(np.float64), dr_ref.table(want, L, t).astype(np.float64)
            if not len(w):
                continue
            err = np.abs(g - w)
            assert (err <= Bd[t]).all(), (label, t, e, err.max(), Bd[t].max(), int(np.argmax(err - Bd[t])))
            if (Bd[t] > 0).any():
                worst[t] = max(worst[t], (err[Bd[t] > 0] / (0.5 * Bd[t][Bd[t] > 0])).max())
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("row", ["a_humanoid27_pgs", "f_team_robot", "c_chain32_cd3_pgs", "d_chain21_hfield_pgs"])
def test_the_draw_matches_its_restatement(hbmod, gpu, row):
    """env_domain_params() against dr_ref.draw, every family drawn together (the team robot on its kp path, the height-field chain with
    its maps), at env offset 0 with factor 1 and, with factor 0.7, at the offset a Batch.reset(env_offset=...) leaves.  The bound per entry is 2 ulp of the largest
    term of its expression (dr_ref.draw_bounds): what a contracted multiply-add can move it by."""
    S = setup_row(row)
    bump = S["bump"] or 0.1  # (the team robot's height field: the reference's MAX_FLOOR_BUMP_HEIGHT)
    D = dr_ref.family("all", seed=21, kp=S["kp"], bump=bump)
    for off, rf in ((0, 1.0), (1000, 0.7)):  # (at factor 1 most products are exact; at 0.7 a contracted multiply-add shows)
        D.factor = rf
        b = hbmod.Batch(S["m"], 21, gpu)  # (21 envs at 16 per block of the draw kernel: two blocks, the second part full)
        if off:
            b.reset(env_offset=off)
        b.env_domain_randomize(D)
        P = b.env_domain_params()
        L = dr_ref.layout(S["m"], P.shape[1])
        b.close()
        worst = _hold_draw(S, D, P, L, [off + e for e in range(len(P))], [0] * len(P), "%s offset %d" % (row, off))
        _profile("draw %-22s offset %4d factor %.1f: worst distance in ulp of the largest term  %s" % (row, off, rf, " ".join("%s %.1f" % kv for kv in worst.items())))
        fr = dr_ref.table(P, L, "fric")[:, 0]
        assert fr.min() >= 1 - rf + dr_ref.FRICTION_RANGE[0] * rf - 1e-6 and fr.max() <= 1 - rf + dr_ref.FRICTION_RANGE[1] * rf + 1e-6 and fr.std() > 0
        if L["nhfielddata"]:
            h = dr_ref.table(P, L, "hfield")
            assert np.all(h.min(axis=1) == 0.0) and np.abs(h.max(axis=1) - rf * bump).max() <= 2e-7 * bump and np.abs(h[0] - h[1]).max() > 0.05


@pytest.mark.gpu
def test_masked_redraw_at_an_auto_reset(hbmod, humanoid_model, gpu):
    """only the envs whose episode ends draw again, with their own episode number + 1; every other env's block stays bit for bit"""
    m = humanoid_model
    env = hbmod.VecEnv(m, N, gpu, domain_randomization=True, seed=4, reward_kind=1, max_time=0.0)  # (a fall ends the episode; auto-reset on)
    assert env.cfg.auto_reset
    env.reset()
    b = env.batch
    A = dr_ref.model_arrays(m)
    S = dict(A=A)
    P0 = b.env_domain_params()
    L = dr_ref.layout(m, P0.shape[1])
    episodes = np.zeros(N, dtype=int)
    _hold_draw(S, env.domain, P0, L, list(range(N)), episodes, "episode 0")
    zeros = np.zeros((N, m.nu), np.float32)
    for fallen in ((1, 4, 6), (0, 4)):
        q = b.get_state(hbmod.STATE_QPOS)
        q[list(fallen), 3:7] = np.array([0.7071, 0.7071, 0.0, 0.0], np.float32)  # lying on the side: terminal
        b.set_state(hbmod.STATE_QPOS, q)
        before = b.env_domain_params()
        obs, rew, term, trunc, info = env.step_arrays(zeros)
        assert sorted(np.flatnonzero(term | trunc)) == sorted(fallen), (fallen, term, trunc)
        after = b.env_domain_params()
        episodes[list(fallen)] += 1
        kept = [e for e in range(N) if e not in fallen]
        assert np.array_equal(after[kept], before[kept])
        assert all(np.abs(after[e] - before[e]).max() > 1e-4 for e in fallen)
        _hold_draw(S, env.domain, after, L, list(range(N)), episodes, "after %s fell" % (fallen,))
    assert episodes.max() == 2
    env.close()


@pytest.mark.gpu
def test_friction_scale_without_a_plane_floor_is_ignored(hbmod, gpu):
    """include/hb.h: the scale applies to the first plane geom.  A model whose floor is a height field has none: two different
    friction multipliers step bit-identically (and identically to the multiplier 1)."""
    S = setup_row("d_chain21_hfield_pgs")
    st, ct = round_states(S, 1)
    res = []
    for lo, hi in ((1.0, 1.0), (0.3, 0.6), (1.5, 3.0)):
        D = config(S, "none")
        D.friction_min_mult, D.friction_max_mult = lo, hi
        b, P, L = _batch(hbmod, gpu, S, D)
        assert L["floor"] < 0
        fr = dr_ref.table(P, L, "fric")[:, 0]
        assert fr.min() >= lo - 1e-6 and fr.max() <= hi + 1e-6
        b.set_state(hbmod.STATE_INTEGRATION, st)
        for t in range(T):
            b.step(ct)
        assert b.last_kernel() == "hb_step_gen_fast_kernel"
        res.append(result(hbmod, b))
        b.close()
    assert res[0][1][0].max() > 0  # (there are contacts)
    same(res[1], res[0], "friction scale 0.3 .. 0.6")
    same(res[2], res[0], "friction scale 1.5 .. 3")
