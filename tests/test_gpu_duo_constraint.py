"""The stages of the two-envs-per-wave kernels (csrc/hb_step_duo.hip) between collision and the sweeps: mj_makeConstraint's table words are
requested ahead of their use (the limit candidates' records behind the narrowphase and kept for the limit-row pass, the pair words as
soon as a contact's pair is known, a tendon row's words in one go), and the operands of C = J W, of the jas / diag loop, of the AR tiles and
of the dual finish are read from LDS without a predicate and chosen by a select of values - so a row outside an env's range IS read (stale
rows of an earlier pass or step, non-finite rows of an env that takes the bad-qacc path) and must never reach a result.

Same arithmetic, so the same bits: hb_step_duo_kernel and hb_step_duo_q_kernel are held byte for byte (time, qpos, qvel, qacc_warmstart,
ncon / nefc / sweeps, status) to hb_step_h27_kernel, the one-env kernel.  Method and helpers: tests/duo_lib.py; the path a case takes is
asserted on the reference's own counts.  The pool is tests/test_gpu_duo_once.py's (duo_lib.once_pool: golden states, the collapsed regime,
bodies laid flat, fresh resets in the air) and behind it a few states built here from qpos: the standing
reset (8 contacts, 32 rows), bodies in the air with joints or a hamstring tendon beyond their range (limit rows without contacts; the
oracle says on the CPU which rows exist), the standing body with such joints (limits and contacts), and states whose step runs
mj_forward twice (a bad qacc).  A case the pool has no state for fails; only "exactly 32 rows" may take the nearest count above.
"""
import numpy as np
import pytest

import duo_lib
from duo_lib import BADQACC, NCON_HALF, ROWS_HALF, STEPS, both_kernels, fits_packed, light, roll_duo, step_duo
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu
LIMIT_JOINT, LIMIT_TENDON = 3, 4  # efc types of the oracle (mjCNSTR_LIMIT_JOINT, mjCNSTR_LIMIT_TENDON); contact rows are above
# qpos addresses: knee_right 13 (range up to 0.035), abdomen_y 8 (up to 0.52), knee_left 19, hip_y_right 12 and hip_y_left 18 (down to -2.62;
# the hamstring tendons 0.5 hip_y - 0.5 knee reach down to -0.3)
BUILT = (
    ("standing", 0.0, {}),
    ("air, one joint", 1.0, {13: 0.2}),
    ("air, joints", 1.0, {13: 0.2, 8: 0.7, 20: 1.0}),
    ("air, tendon", 1.0, {12: -1.5}),
    ("air, tendons and joint", 1.0, {12: -2.7, 18: -1.5}),
    ("standing, joints", 0.0, {13: 0.2, 19: 0.2}),
    ("standing, tendon", 0.0, {12: -1.5}),
)
NBAD = 3


@pytest.fixture(scope="module")
def made():
    """name -> (state record, oracle's ncon, nefc, efc types) of the states built from qpos"""
    o = Oracle()
    out = {}
    for name, lift, qset in BUILT:
        o.reset()
        o.qpos[2] += lift
        for k, v in qset.items():
            o.qpos[k] = v
        rec = np.concatenate([[0.0], o.qpos, np.zeros(2 * o.nv)]).astype(np.float32)
        o.qpos[:] = rec[1:1 + o.nq]  # (what the device gets)
        o.forward()
        out[name] = (rec, o.ncon, o.nefc, o.efc_types()[0].copy())
    return out


@pytest.fixture(scope="module")
def pool(hbmod, humanoid_model, gpu, made):
    """tests/test_gpu_duo_once.py's pool | the BUILT states | NBAD states with velocities that overflow the accelerations"""
    m = humanoid_model
    state, tape = duo_lib.once_pool(hbmod, m, gpu)
    extra = np.stack([made[name][0] for name, _, _ in BUILT])
    bad = np.stack([state[0], state[1], made["standing"][0]]).copy()
    bad[0, 1 + m.nq + 4] = 3e9              # an angular velocity of the root (tests/test_gpu_duo.py's recipe)
    bad[1, 1 + m.nq:1 + m.nq + m.nv] = 2e9  # every velocity
    bad[2, 1 + m.nq + 2] = 3e9              # a linear velocity, in contact
    add = np.concatenate([extra, bad]).astype(np.float32)
    state2 = np.ascontiguousarray(np.concatenate([state, add]), dtype=np.float32)
    tape2 = np.concatenate([tape, np.zeros((STEPS, len(add), m.nu), np.float32)], axis=1)
    return state2, np.ascontiguousarray(tape2)


@pytest.fixture(scope="module")
def ref(hbmod, humanoid_model, gpu, pool):
    """the one-env kernel's STEPS steps of the pool: per step (state, ncon, nefc, niter, status)"""
    out = duo_lib.reference(hbmod, humanoid_model, gpu, *pool, STEPS)
    nefc = out[0][2]
    print("\npool of %d envs, first step: envs per row count 0..40: %s" % (len(pool[0]), np.bincount(nefc, minlength=41)[:41].tolist()))
    return out


def at(pool, name):
    """pool index of a BUILT state"""
    return len(pool[0]) - NBAD - len(BUILT) + [b[0] for b in BUILT].index(name)


def pick(mask, k, what, taken=()):
    """the first k pool envs of `mask` that are not in `taken`; a pool without them is an error"""
    e = [i for i in np.flatnonzero(mask) if i not in set(taken)]
    assert len(e) >= k, "the pool has %d envs for '%s', the case needs %d" % (len(e), what, k)
    return e[:k]


def test_the_built_states_are_what_they_are_built_for(made, pool, ref):
    """the oracle on the CPU: which rows the built states have - and the one-env kernel counts the same"""
    ncon, nefc = ref[0][1], ref[0][2]
    for name, _, _ in BUILT:
        _, oc, oe, types = made[name]
        assert (ncon[at(pool, name)], nefc[at(pool, name)]) == (oc, oe), (name, ncon[at(pool, name)], nefc[at(pool, name)], oc, oe)
    assert made["standing"][1:3] == (8, 32)
    assert made["air, one joint"][1:3] == (0, 1) and list(made["air, one joint"][3]) == [LIMIT_JOINT]
    assert made["air, joints"][1] == 0 and list(made["air, joints"][3]) == [LIMIT_JOINT] * 3
    assert made["air, tendon"][1] == 0 and list(made["air, tendon"][3]) == [LIMIT_TENDON]
    assert made["air, tendons and joint"][1] == 0 and sorted(made["air, tendons and joint"][3]) == [LIMIT_JOINT, LIMIT_TENDON, LIMIT_TENDON]
    for name, kind in (("standing, joints", LIMIT_JOINT), ("standing, tendon", LIMIT_TENDON)):
        _, oc, oe, types = made[name]
        assert oc > 0 and (types == kind).sum() >= 1 and (types > LIMIT_TENDON).sum() >= 4 and oc <= NCON_HALF, (name, oc, oe, types)


def test_paired_tile_edges(hbmod, humanoid_model, gpu, pool, ref):
    """both envs at most 31 rows (split = 32, an env per row tile): an env without rows beside one with rows in both slots, both without
    rows, one row, and 31 rows - the y rows are then packed rows 31 and 63, the last of C - in either slot and in both"""
    ncon, nefc = ref[0][1], ref[0][2]
    ok = light(ref)
    empty = pick(ok & (nefc == 0) & (ncon == 0), 4, "no rows")
    rows = pick(ok & (nefc >= 8) & (nefc < ROWS_HALF), 6, "8..30 rows")
    one = at(pool, "air, one joint")
    full = pick(ok & (nefc == ROWS_HALF), 4, "31 rows")
    assert nefc[one] == 1 and all(nefc[e] == 31 for e in full)
    pairs = [(empty[0], rows[0]), (rows[1], empty[1]), (empty[2], empty[3]), (one, rows[2]), (rows[3], one),
             (full[0], rows[4]), (rows[5], full[1]), (full[2], full[3]), (full[0], one), (empty[0], full[1])]
    assert all(max(nefc[a], nefc[b]) <= ROWS_HALF and max(ncon[a], ncon[b]) <= NCON_HALF for a, b in pairs)
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=2, what="paired tile edges")


def test_packed_rows(hbmod, humanoid_model, gpu, pool, ref):
    """an env above 31 rows beside a light one (split > 32): the heavy env in either slot with rows of both envs in row tile 1, a low env of
    32 rows (the standing reset; the nearest count above if the pool's differs), and a split of 40 or more"""
    ncon, nefc, status = ref[0][1], ref[0][2], ref[0][4]
    lights = pick(light(ref) & (nefc >= 1) & (nefc <= 10), 8, "1..10 rows")
    heavy = pick((nefc >= 33) & (nefc <= 44) & (ncon <= NCON_HALF) & (status == 0), 4, "33..44 rows, at most 12 contacts")
    deep = pick((nefc >= 36) & (nefc <= 48) & (ncon <= NCON_HALF) & (status == 0), 2, "36..48 rows, at most 12 contacts", taken=heavy)
    n32 = min(n for n in set(nefc[(ncon <= NCON_HALF) & (status == 0)].tolist()) if n >= 32)
    low32 = [at(pool, "standing")] if nefc[at(pool, "standing")] == n32 else pick((nefc == n32) & (ncon <= NCON_HALF) & (status == 0), 1, "32 rows")
    print("\nthe low env of 32 rows has %d rows" % n32)
    pairs = [(heavy[0], lights[0]), (lights[1], heavy[1]), (heavy[2], lights[2]), (lights[3], heavy[3]),
             (low32[0], lights[4]), (lights[5], low32[0]), (deep[0], lights[6]), (lights[7], deep[1])]
    for a, b in pairs:
        nf, ns = max(nefc[a], nefc[b]), min(nefc[a], nefc[b])
        assert nf > ROWS_HALF and ns >= 1 and fits_packed(nf, ns) and max(ncon[a], ncon[b]) <= NCON_HALF, (nf, ns)
    split = [max((max(nefc[a], nefc[b]) + 4) & ~3, 32) for a, b in pairs]
    assert all(max(nefc[a], nefc[b]) >= 33 for a, b in pairs[:4]) and max(split) < 64  # row tile 1 holds rows of both envs
    assert split[4] == split[5] == ((n32 + 4) & ~3) and min(split[6:]) >= 40
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=2, what="packed rows")


@pytest.mark.parametrize("rows", ["at most 31", "32 or more"])
def test_one_env_alone_in_its_wave(hbmod, humanoid_model, gpu, pool, ref, rows):
    """three envs: the last wave holds one env (all 64 row lanes are its own: X1 / Y0 / Y1 from 32 rows on)"""
    ncon, nefc, status = ref[0][1], ref[0][2], ref[0][4]
    calm = pick(light(ref) & (nefc >= 4), 2, "a calm pair")
    if rows == "at most 31":
        single = pick(light(ref) & (nefc >= 12), 1, "12..31 rows", taken=calm)
    else:
        single = pick((nefc > 36) & (status == 0), 1, "above 36 rows") + [at(pool, "standing")]
        assert nefc[single[1]] >= 32
    for s in single:
        both_kernels(hbmod, humanoid_model, gpu, pool, ref, [tuple(calm)], [s], steps=2, what="one env alone, " + rows)


def test_a_serial_restart(hbmod, humanoid_model, gpu, pool, ref):
    """the pass restarts with one env at a time: an env above 12 contacts beside a light one in either slot, and two envs at most 12
    contacts each whose rows do not fit one wave"""
    ncon, nefc, status = ref[0][1], ref[0][2], ref[0][4]
    many = pick((ncon > NCON_HALF) & (status == 0), 2, "above 12 contacts")
    calm = pick(light(ref) & (nefc >= 4), 2, "a calm env")
    big = pick((nefc >= 32) & (ncon <= NCON_HALF) & (status == 0), 2, "32 rows or more, at most 12 contacts")
    pairs = [(many[0], calm[0]), (calm[1], many[1]), (big[0], big[1])]
    assert not fits_packed(max(nefc[big[0]], nefc[big[1]]), min(nefc[big[0]], nefc[big[1]]))
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=2, what="a serial restart")


def test_limit_rows(hbmod, humanoid_model, gpu, pool, ref):
    """rows of joints and of hamstring tendons beyond their range: in the air (no contact: the limit rows are all the rows there are), and
    beside contact rows; next to each other, next to an env without rows and next to one in contact, over three steps"""
    ncon, nefc = ref[0][1], ref[0][2]
    air = [at(pool, n) for n in ("air, one joint", "air, joints", "air, tendon", "air, tendons and joint")]
    ground = [at(pool, n) for n in ("standing, joints", "standing, tendon")]
    assert all(ncon[e] == 0 and nefc[e] > 0 for e in air) and all(ncon[e] > 0 and nefc[e] > 4 * ncon[e] for e in ground)
    empty = pick(light(ref) & (nefc == 0) & (ncon == 0), 2, "no rows")
    rows = pick(light(ref) & (nefc >= 8), 2, "8..31 rows")
    pairs = [(air[1], air[2]), (air[3], empty[0]), (empty[1], air[2]), (air[2], rows[0]), (rows[1], air[3]), (air[0], air[1]),
             (ground[0], air[2]), (air[3], ground[1]), (ground[1], ground[0])]
    for a, b in pairs:
        assert max(ncon[a], ncon[b]) <= NCON_HALF and (max(nefc[a], nefc[b]) <= ROWS_HALF or fits_packed(max(nefc[a], nefc[b]), min(nefc[a], nefc[b])))
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=3, what="limit rows")
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs[:1], [air[3]], steps=2, what="limit rows, an env alone")


def test_stale_rows_of_falling_counts(hbmod, humanoid_model, gpu, pool, ref):
    """three steps in one launch in which an env's row count falls from step to step: the rows beyond its count still hold the step
    before's C, and are read now (without a predicate) and chosen away"""
    n0, n1, n2 = ref[0][2], ref[1][2], ref[2][2]
    ok = light(ref, 0) & light(ref, 1) & light(ref, 2)
    falling = pick(ok & (n0 > n1) & (n1 > n2), 4, "rows falling over three steps")
    steady = pick(ok & (n0 >= 4) & (n0 == n1) & (n1 == n2), 2, "a steady env", taken=falling)
    pairs = [(falling[0], falling[1]), (falling[2], steady[0]), (steady[1], falling[3])]
    assert all(n0[e] > n1[e] > n2[e] for e in falling)
    roll_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=3, what="falling rows")
    step_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, what="falling rows")


def test_stale_rows_of_a_bad_qacc_partner(hbmod, humanoid_model, gpu, pool, ref):
    """an env whose velocities overflow its accelerations runs mj_forward a second time, alone: its rows of C are non-finite while the
    partner's bits are held - in either slot, beside envs in contact and beside one whose only row is a tendon's"""
    nefc, status = ref[0][2], ref[0][4]
    n = len(pool[0])
    bad = [e for e in range(n - NBAD, n) if (status[e] & BADQACC) and not (status[e] & 0x30)]  # (not reset by mj_checkPos / mj_checkVel before)
    assert len(bad) >= 2, status[n - NBAD:]
    calm = pick(light(ref) & (nefc >= 8), 3, "a calm env with rows")
    pairs = [(bad[0], calm[0]), (calm[1], bad[-1]), (bad[0], at(pool, "air, tendon")), (calm[2], bad[1])]
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=2, what="a bad-qacc partner")
