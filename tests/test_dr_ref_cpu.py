"""(CPU) tests/dr_ref.py on the fp64 reference alone: writing an env's block into the oracle and taking it out again leaves no trace,
and every (row, family) pair that tests/test_gpu_domain_params.py holds the step kernels to is OBSERVABLE - with the GPU test's own
states, envs and blocks (dr_ref.draw), the reference's step with the env's block differs from its step with the nominal block by at
least 10 x the GPU bound of a compared quantity, on at least half of the (state, env) cases and on at least four.  Without that a kernel
that ignored the family would pass the GPU test."""
import functools

import numpy as np
import pytest

import dr_ref
from oracle_lib import Oracle, load_state
from dr_rows import BOUNDS, CASES, COMPARED, N, ROUNDS, ROWS, blocks, config, deviation, ref_step, round_states, setup_row
from step_lib import report

FACTOR = 10.0  # the reference's change over the GPU bound


def _record(o):
    return np.concatenate([[o.time], o.qpos, o.qvel, o.qacc_warmstart, o.qacc, o.efc_force[:o.nefc], [o.ncon, o.nefc]])


@pytest.mark.parametrize("row", ["a_humanoid27_pgs", "d_chain21_hfield_pgs", "f_team_robot"])
def test_apply_then_restore_leaves_the_oracle_as_it_was(hbmod, row):
    """one step from the same state: a fresh oracle, and the shared one after apply + restore, bit for bit; in between the block is in
    force (the step differs) and holds the values the layout says"""
    S = setup_row(row)
    o, base = S["o"], S["base"]
    fresh = Oracle(S["path"])
    fresh.set_opt(solver=o.opt("solver"), iterations=o.opt("iterations"))
    D = config(S, "all")
    L = dr_ref.layout(S["m"], dr_ref.stride_of(S["m"]))
    P = blocks(S, D)
    st, ct = round_states(S, 1)
    try:
        for e in (0, 5):
            dr_ref.apply(o, P[e], L, base)
            assert np.array_equal(o.marr("body_mass"), dr_ref.table(P[e], L, "mass").astype(np.float64))
            assert np.array_equal(o.marr("actuator_biasprm")[1::3], dr_ref.table(P[e], L, "bias1").astype(np.float64))
            assert np.array_equal(o.marr("body_subtreemass"), fresh.marr("body_subtreemass")) and np.array_equal(o.marr("dof_M0"), fresh.marr("dof_M0"))
            load_state(o, st[e], ct[e].astype(np.float64)); o.step()
            with_block = _record(o)
            dr_ref.restore(o, base)
            for k in dr_ref.ORACLE_ARRAYS:
                if k in base:
                    assert np.array_equal(o.marr(k), fresh.marr(k)), k
            recs = []
            for oo in (o, fresh):
                load_state(oo, st[e], ct[e].astype(np.float64)); oo.step()
                recs.append(_record(oo))
            assert np.array_equal(recs[0], recs[1]), (row, e)
            assert with_block.shape != recs[0].shape or not np.array_equal(with_block, recs[0])
    finally:
        dr_ref.restore(o, base)


def test_layout_is_the_device_layout(hbmod):
    """the offsets against DomainLayout's formula (hb_device.hpp) at the sizes of each model, and the candidates in constraint order"""
    for row, nlim, nhf in (("a_humanoid27_pgs", 2 * 21 + 2 * 2, 0), ("f_team_robot", 2 * 12, None), ("c_chain32_cd3_pgs", None, 0), ("d_chain21_hfield_pgs", None, 25)):
        S = setup_row(row)
        m = S["m"]
        L = dr_ref.layout(m, dr_ref.stride_of(m))
        if nlim is not None:
            assert L["nlimcand"] == nlim
        if nhf is not None:
            assert L["nhfielddata"] == nhf
        nb, nv, nu, nl = m.nbody, m.nv, m.nu, L["nlimcand"]
        assert [L[t] for t in dr_ref.TABLES] == [0, nb, nb + nv, nb + 2 * nv, nb + 2 * nv + nl, nb + 2 * nv + 2 * nl, nb + 2 * nv + 2 * nl + nu, nb + 2 * nv + 2 * nl + 2 * nu,
                                                 nb + 2 * nv + 2 * nl + 4 * nu, nb + 2 * nv + 2 * nl + 4 * nu + 1]
        assert L["stride"] == nb + 2 * nv + 2 * nl + 4 * nu + 1 + L["nhfielddata"] == sum(dr_ref.sizes(L).values())
        assert [c[2] for c in L["cand"]] == [-1, 1] * (nl // 2) and [c[0] for c in L["cand"]] == sorted(c[0] for c in L["cand"])
        with pytest.raises(AssertionError):
            dr_ref.layout(m, L["stride"] + 1)
    assert dr_ref.layout(setup_row("d_chain21_hfield_pgs")["m"], dr_ref.stride_of(setup_row("d_chain21_hfield_pgs")["m"]))["floor"] == -1


def test_the_nominal_draw_is_the_model(hbmod):
    """family "none": the block holds the model's own values rounded to fp32, so that applying it changes the oracle by rounding only"""
    for row in ("a_humanoid27_pgs", "f_team_robot", "d_chain21_hfield_pgs"):
        S = setup_row(row)
        m = S["m"]
        L = dr_ref.layout(m, dr_ref.stride_of(m))
        P = dr_ref.draw(S["A"], config(S, "none"), 3, 2)
        # (a drawn mass is never below 1e-5: a massless body of the model - the team robot has one - gets that much in every block)
        assert np.array_equal(dr_ref.table(P, L, "mass")[1:], np.maximum(np.float32(1e-5), m.array("body_mass").astype(np.float32)[1:])) and P[0] == 0
        assert np.array_equal(dr_ref.table(P, L, "arm"), m.array("dof_armature").astype(np.float32))
        assert np.array_equal(dr_ref.table(P, L, "gain"), m.array("actuator_gainprm").astype(np.float32))
        assert np.array_equal(dr_ref.table(P, L, "bias1"), m.array("actuator_biasprm").astype(np.float32)[1::3])
        assert np.array_equal(dr_ref.table(P, L, "frc"), m.array("actuator_forcerange").astype(np.float32))
        assert dr_ref.table(P, L, "fric")[0] == 1.0
        assert np.array_equal(dr_ref.table(P, L, "hfield"), m.array("hfield_data").astype(np.float32))


def test_chain_xml_forcerange_keeps_the_default_xml(hbmod):
    from kernel_models import chain_xml
    plain = chain_xml(21, True, "plane", 3, "PGS")
    assert chain_xml(21, True, "plane", 3, "PGS", forcerange=None) == plain and "forcelimited" not in plain
    m = hbmod.Model.from_xml_string(chain_xml(21, True, "plane", 3, "PGS", forcerange=0.6))
    assert np.array_equal(m.array("actuator_forcerange"), np.tile([-0.6, 0.6], m.nu)) and m.array("actuator_forcelimited").all()


@functools.lru_cache(maxsize=None)
def observability(row, family):
    """(computed once per (row, family) and shared) per run mode of the GPU test ("diag", "state") and per (state, env) case: the largest change, over its bound, of a quantity that
    a run of that mode compares (inf: the counts change - every mode compares those)"""
    S = setup_row(row)
    o, base = S["o"], S["base"]
    L = dr_ref.layout(S["m"], dr_ref.stride_of(S["m"]))
    P, P0 = blocks(S, config(S, family)), blocks(S, config(S, "none"))
    ratios = {mode: [] for mode in COMPARED}
    try:
        for r in range(ROUNDS):
            st, ct = round_states(S, r, family)
            for e in range(N):
                steps = []
                for block in (P0[e], P[e]):
                    dr_ref.apply(o, block, L, base)
                    steps.append(ref_step(S, st[e], ct[e]))
                a, b = steps
                same = (a["ncon"], a["nefc"]) == (b["ncon"], b["nefc"])
                dev = deviation(b, a) if same else {}
                for mode, keys in COMPARED.items():
                    ratios[mode].append(max(dev[k] / BOUNDS[k] for k in keys if k in dev) if same else np.inf)
    finally:
        dr_ref.restore(o, base)
    return {mode: np.array(v) for mode, v in ratios.items()}


@pytest.mark.parametrize("row", list(ROWS))
def test_every_tested_family_is_observable_on_the_reference(hbmod, row):
    """for every run mode the row has: a launch without diagnostic outputs is compared in qpos, qvel and the counts only, so its
    families must show in those"""
    S = setup_row(row)
    modes = sorted({mode for _, mode, _ in ROWS[row]["runs"]})
    print()
    for family in ROWS[row]["families"]:
        ratios = observability(row, family)
        for mode in modes:
            r = ratios[mode]
            seen = int((r >= FACTOR).sum())
            line = "observability %-22s %-10s %-5s (%s) change / bound >= %g in %2d of %d cases, median %.3g, counts change in %d" % (
                row, family, mode, ", ".join(COMPARED[mode]), FACTOR, seen, len(r), np.median(r), int(np.isinf(r).sum()))
            report(line, "HB_DR_PARITY_OUT", lead="  ")
            assert len(r) == N * ROUNDS and seen >= max(4, len(r) // 2), (row, family, mode, seen, np.sort(r)[:8])


def test_own_states_touch_their_own_height_maps(hbmod):
    """row d, config "all": every env's teacher-forced states come from its own rollout on its own drawn map, and with that map in the
    oracle at least half of the 32 cases are in contact (on the nominal rollout's states none of them is: they float above the drawn
    maps) - and the env's map matters there: with the NEXT env's map instead, the contacts differ"""
    row = "d_chain21_hfield_pgs"
    S = setup_row(row)
    assert ROWS[row]["own_states"] == ("all",)
    o, base = S["o"], S["base"]
    L = dr_ref.layout(S["m"], dr_ref.stride_of(S["m"]))
    P = blocks(S, config(S, "all"))
    touching = {"own": 0, "nominal": 0}
    differ = 0
    try:
        for r in range(ROUNDS):
            for which, (st, ct) in (("own", round_states(S, r, "all")), ("nominal", round_states(S, r))):
                for e in range(N):
                    dr_ref.apply(o, P[e], L, base)
                    mine = ref_step(S, st[e], ct[e])
                    touching[which] += mine["ncon"] > 0
                    if which == "own":
                        other = P[e].copy()
                        other[L["hfield"]:] = P[(e + 1) % N][L["hfield"]:]
                        dr_ref.apply(o, other, L, base)
                        x = ref_step(S, st[e], ct[e])
                        differ += (x["ncon"], x["nefc"]) != (mine["ncon"], mine["nefc"]) or deviation(x, mine)["qacc"] >= FACTOR * BOUNDS["qacc"]
    finally:
        dr_ref.restore(o, base)
    print("\n  row d all: in contact on the env's own map in %d of %d cases (nominal states: %d); another env's map changes the step in %d" % (
        touching["own"], N * ROUNDS, touching["nominal"], differ))
    assert touching["own"] >= N * ROUNDS // 2 and differ >= N * ROUNDS // 2, (touching, differ)


def test_families_left_out_of_a_row_are_left_out_for_a_reason(hbmod):
    """the table of the GPU test drops "friction" on the rows without a frictional plane floor: there the reference does not move at all
    (condim 1: no friction rows; a height-field floor: the scale has no geom to apply to)"""
    for row, spec in ROWS.items():
        if spec.get("focus"):
            continue
        for family in set(dr_ref.FAMILIES) - set(spec["families"]):
            assert family == "friction", (row, family)
            r = observability(row, family)["diag"]
            assert r.max() == 0.0, (row, family, r.max())
    assert len(CASES) == sum(len(s["families"]) + 1 for s in ROWS.values())
