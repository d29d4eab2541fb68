"""The wide form of the two-envs-per-wave kernels' paired sweeps (csrc/hb_step_duo.hip): a pair in the paired layout (both envs at most 31 rows and
12 contacts) with an env of 17..31 rows holds every sweep quantity twice, once per DPP row of 16 lanes (U: rows 0..15, V: rows 16..31), and
its row step broadcasts lane k's proposal by v_fmac_f32_dpp row_newbcast inside each DPP row.  Once one env has stopped, the other sweeps on in
row layout: in the short broadcast form with at most 16 rows, in the one-env kernel's row step (v_readlane) above.  At most 16 rows in both
envs keeps the short form throughout, an env above 31 rows the packed layout.

Method and helpers are those of tests/test_gpu_duo_bcast.py: hb_step_duo_kernel (one step) and hb_step_duo_q_kernel (two and three steps) are
held byte for byte (time, qpos, qvel, warm start, ncon / nefc / sweeps, status) to hb_step_h27_kernel, whose result for an env does not depend
on the batch around it and is computed ONCE for a pool of states over three steps.  Every case is an index list into the pool, laid out so
that the pairing of dispatch slots puts the chosen envs into one wave; the path that wave takes (`path` below) is asserted on the reference's
own contact, row and sweep counts, and a pool that lacks the envs a case needs fails the case.  The pool is that file's recipe plus three
more collapsed regimes, for the rarer counts (31 rows, rows that cross 31 between two steps).  No env of the pool above 16 rows stops after
ONE sweep by its own test (none in 8 x 2048 fallen envs left alone for 100 to 3000 steps either): a paired loop of one sweep is held by a short
env with one sweep beside a tall one, and tall envs with one sweep by the iteration limit of 1.
"""
import os

import numpy as np
import pytest

from oracle_lib import GOLDEN, HUMANOID_HBM
from test_gpu_duo_bcast import CAP, DUO, NCON_HALF, ROWS_DPP, ROWS_HALF, STEPS, Picker, light, partners, place, reference, roll_duo, step_duo

pytestmark = pytest.mark.gpu


def path(ref, a, b, t=0):
    """(layout, form of the paired loop, form of the tail) of the wave that steps pool envs a (lanes 0..31) and b at step t, from the reference's counts:
    'paired' needs both envs at most 12 contacts and 31 rows; the paired loop runs while both sweep, in the short form when both have at most 16
    rows and in the wide form otherwise; the tail is the env with more sweeps alone, in the short form when IT has at most 16 rows and in the one-env
    kernel's row step ("tall") above"""
    ncon, nefc, niter = ref[t][1], ref[t][2], ref[t][3]
    if max(ncon[a], ncon[b]) > NCON_HALF or max(nefc[a], nefc[b]) > ROWS_HALF:
        return ("packed", None, None)
    loop = None if min(niter[a], niter[b]) == 0 else ("short" if max(nefc[a], nefc[b]) <= ROWS_DPP else "wide")
    last = a if niter[a] > niter[b] else b
    tail = None if niter[a] == niter[b] else ("short" if nefc[last] <= ROWS_DPP else "tall")
    return ("paired", loop, tail)


def collapsed(hbmod, m, gpu, n, steps, rng):
    """n envs fallen under the Halton control sequence, then `steps` steps with saturated actuators (limbs driven into the floor, joints into their limits)"""
    b = hbmod.Batch(m, n, gpu)
    b.reset(perturb=True)
    b.rollout_halton(150)
    ctrl = np.sign(rng.uniform(-1, 1, size=(n, m.nu))).astype(np.float32)
    for _ in range(steps):
        b.step(ctrl)
    state = b.get_state(hbmod.STATE_INTEGRATION)
    b.close()
    return state, ctrl


@pytest.fixture(scope="module")
def pool(hbmod, humanoid_model, gpu):
    """(state [N, 1 + nq + 2 nv] float32, control tape [STEPS, N, nu]): golden states | collapsed regimes after 60, 20, 40 and 90 steps | settled regime |
    fresh resets in the air"""
    m = humanoid_model
    g = np.load(os.path.join(GOLDEN, "humanoid27_steps.npz"))
    gstate = np.concatenate([g["time"][:, None], g["qpos"], g["qvel"], g["warm"]], axis=1).astype(np.float32)
    gctrl = g["ctrl"].astype(np.float32)
    rng = np.random.default_rng(11)
    n = 2048
    cstate, cctrl = collapsed(hbmod, m, gpu, n, 60, rng)
    b = hbmod.Batch(m, n, gpu)  # the benchmark's regime: fallen and settled under its control sequence
    b.reset(perturb=True)
    b.rollout_halton(600)
    sstate = b.get_state(hbmod.STATE_INTEGRATION)
    b.close()
    sctrl = rng.uniform(-1, 1, size=(n, m.nu)).astype(np.float32)
    more = [collapsed(hbmod, m, gpu, n, steps, rng) for steps in (20, 40, 90)]
    a = hbmod.Batch(m, 64, gpu)
    a.reset(perturb=True)
    astate = a.get_state(hbmod.STATE_INTEGRATION)
    a.close()
    astate[:, 1 + 2] += 1.0  # one metre up: no contact
    actrl = np.zeros((64, m.nu), np.float32)
    state = np.ascontiguousarray(np.concatenate([gstate, cstate, sstate] + [s for s, _ in more] + [astate]), dtype=np.float32)
    ctrl = np.concatenate([gctrl, cctrl, sctrl] + [c for _, c in more] + [actrl])
    tape = np.stack([np.roll(ctrl, 7 * t, axis=0) for t in range(STEPS)])
    tape[:, -64:] = 0.0  # (the envs in the air stay limp: no joint runs into its limit)
    return state, np.ascontiguousarray(tape)


@pytest.fixture(scope="module")
def ref(hbmod, humanoid_model, gpu, pool):
    state, tape = pool
    out = reference(hbmod, humanoid_model, gpu, state, tape, STEPS)
    nefc, niter = out[0][2], out[0][3]
    lt = light(out)
    print("\npool of %d envs, first step: rows 0..%d, %d envs that pair; of those with 17..31 rows: %s; with 32..63 rows and no warning: %d; "
          "tall and at the sweep cap %d, tall with one sweep %d" % (len(state), nefc.max(), lt.sum(), np.bincount(nefc[lt], minlength=32)[17:32].tolist(),
                                                                   ((nefc >= 32) & (nefc <= 63) & (out[0][4] == 0)).sum(),
                                                                   (lt & (nefc > 16) & (niter == CAP)).sum(), (lt & (nefc > 16) & (niter == 1)).sum()))
    return out


def both_kernels(hbmod, m, gpu, pool, ref, pairs, what, steps=(2,)):
    step_duo(hbmod, m, gpu, pool, ref, pairs, what=what)
    for k in steps:
        roll_duo(hbmod, m, gpu, pool, ref, pairs, steps=k, what=what)


def test_row_counts_at_the_edges_of_the_wide_form(hbmod, humanoid_model, gpu, pool, ref):
    """(17, 17) and (31, 31); 17 rows beside an env of one row, in both slots; 31 rows beside an env without rows, in both slots; 20 and 24 rows as
    the taller count (the last chunk of a sweep ends on a chunk of four, 24 on the chunk before the three-row one)"""
    ncon, nefc, niter = ref[0][1], ref[0][2], ref[0][3]
    ok = light(ref) & (nefc >= 1) & (niter >= 1)
    empty = (nefc == 0) & (ncon == 0) & (ref[0][4] == 0)
    pk = Picker(0)
    rows = lambda n: pk.take(ok & (nefc == n), "%d rows" % n)
    pairs = [(rows(17), rows(17)), (rows(31), rows(31)), (rows(17), rows(1)), (rows(1), rows(17)),
             (rows(31), pk.take(empty, "no rows")), (pk.take(empty, "no rows"), rows(31))]
    for n in (20, 24):
        pairs += [(rows(n), rows(n)), (rows(n), pk.take(ok & (nefc < n), "below %d rows" % n)), (pk.take(ok & (nefc < n), "below %d rows" % n), rows(n))]
    got = [(nefc[a], nefc[b]) for a, b in pairs]
    assert got[:6] == [(17, 17), (31, 31), (17, 1), (1, 17), (31, 0), (0, 31)] and [max(x) for x in got[6:]] == [20] * 3 + [24] * 3
    for a, b in pairs:
        p = path(ref, a, b)
        assert p[0] == "paired" and (p[1] == "wide" if min(nefc[a], nefc[b]) > 0 else (p[1] is None and p[2] == "tall")), (nefc[a], nefc[b], p)
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, "edges of the wide form", steps=(2, 3))


def test_every_residue_mod_4_of_both_row_counts(hbmod, humanoid_model, gpu, pool, ref):
    """both envs within 17..31 rows, every combination of the two counts mod 4: the chunks of four of the V rows, and the last chunk of three"""
    nefc, niter = ref[0][2], ref[0][3]
    ok = light(ref) & (nefc > ROWS_DPP) & (niter >= 1)
    pk = Picker(1)
    pairs = [(pk.take(ok & (nefc % 4 == ra), "17..31 rows, %d mod 4" % ra), pk.take(ok & (nefc % 4 == rb), "17..31 rows, %d mod 4" % rb)) for ra in range(4) for rb in range(4)]
    assert len({(nefc[a] % 4, nefc[b] % 4) for a, b in pairs}) == 16
    assert all(17 <= nefc[e] <= 31 for p in pairs for e in p) and all(path(ref, a, b)[:2] == ("paired", "wide") for a, b in pairs)
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, "17..31 rows mod 4")


def test_the_boundaries_of_the_wide_form(hbmod, humanoid_model, gpu, pool, ref):
    """(16, 17) and (17, 16) take the wide form, (16, 16) still the short one; an env of 31 rows beside one of 32 or more leaves the paired layout
    altogether, in both slots"""
    nefc, niter = ref[0][2], ref[0][3]
    ok = light(ref) & (niter >= 1)
    big = (nefc >= 32) & (nefc <= 63) & (ref[0][4] == 0)
    pk = Picker(2)
    rows = lambda n: pk.take(ok & (nefc == n), "%d rows" % n)
    pairs, want = [], []
    for na, nb, form in ((16, 17, "wide"), (17, 16, "wide"), (16, 16, "short")):
        for _ in range(2):
            pairs.append((rows(na), rows(nb)))
            want.append(("paired", form))
    pairs += [(rows(31), pk.take(big, "32..63 rows")), (pk.take(big, "32..63 rows"), rows(31))]
    want += [("packed", None)] * 2
    assert [(nefc[a], nefc[b]) for a, b in pairs[:6]] == [(16, 17)] * 2 + [(17, 16)] * 2 + [(16, 16)] * 2
    assert nefc[pairs[6][0]] == 31 and nefc[pairs[6][1]] >= 32 and nefc[pairs[7][0]] >= 32 and nefc[pairs[7][1]] == 31
    assert [path(ref, a, b)[:2] for a, b in pairs] == want
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, "16 | 17 and 31 | 32 rows")


def test_the_order_in_which_the_two_envs_stop(hbmod, humanoid_model, gpu, pool, ref):
    """a wide paired loop, then: the short tail (the env above 16 rows stops first, the one at or below 16 sweeps on), the tall tail (the reverse),
    the tall tail behind two envs above 16 rows - each in both slot orders -, no tail (equal sweep counts), the sweep cap of 50 beside a stop
    before 10, and a paired loop of ONE sweep (an env that stops after its first sweep beside a tall one that sweeps on)"""
    nefc, niter = ref[0][2], ref[0][3]
    ok = light(ref) & (nefc >= 1) & (niter >= 1)
    pk = Picker(3)
    lo, hi = (lambda e: nefc[e] <= ROWS_DPP), (lambda e: nefc[e] > ROWS_DPP)
    cases = []  # (pairs, the path all of them take)
    cases.append(([pk.pair(ok, lambda a, b: lo(a) and hi(b) and niter[b] < niter[a], "a short env that outlasts a tall one") for _ in range(2)]
                  + [pk.pair(ok, lambda a, b: hi(a) and lo(b) and niter[a] < niter[b], "a short env that outlasts a tall one") for _ in range(2)], ("paired", "wide", "short")))
    cases.append(([pk.pair(ok, lambda a, b: lo(a) and hi(b) and niter[a] < niter[b], "a tall env that outlasts a short one") for _ in range(2)]
                  + [pk.pair(ok, lambda a, b: hi(a) and lo(b) and niter[b] < niter[a], "a tall env that outlasts a short one") for _ in range(2)], ("paired", "wide", "tall")))
    cases.append(([pk.pair(ok, lambda a, b: hi(a) and hi(b) and niter[a] > niter[b] + 3, "two tall envs, the lower slot sweeps longer") for _ in range(2)]
                  + [pk.pair(ok, lambda a, b: hi(a) and hi(b) and niter[b] > niter[a] + 3, "two tall envs, the upper slot sweeps longer") for _ in range(2)], ("paired", "wide", "tall")))
    cases.append(([pk.pair(ok, lambda a, b: hi(a) and hi(b) and niter[a] == niter[b] < CAP, "two tall envs with equal sweep counts below the cap") for _ in range(2)]
                  + [pk.pair(ok, lambda a, b: hi(a) and hi(b) and niter[a] == niter[b] == CAP, "two tall envs at the cap")], ("paired", "wide", None)))
    cases.append(([pk.pair(ok, lambda a, b: hi(a) and hi(b) and niter[a] == CAP and niter[b] < 10, "a tall env at the cap beside a tall one that stops before 10"),
                   pk.pair(ok, lambda a, b: hi(a) and hi(b) and niter[b] == CAP and niter[a] < 10, "a tall env at the cap beside a tall one that stops before 10"),
                   pk.pair(ok, lambda a, b: hi(a) and niter[a] == CAP and niter[b] == 1, "a tall env at the cap beside one sweep"),
                   pk.pair(ok, lambda a, b: hi(b) and niter[b] == CAP and niter[a] == 1, "a tall env at the cap beside one sweep")], ("paired", "wide", "tall")))
    cases.append(([pk.pair(ok, lambda a, b: hi(a) and 4 < niter[a] < CAP and lo(b) and niter[b] == 1, "a short env with one sweep beside a tall one that sweeps on"),
                   pk.pair(ok, lambda a, b: hi(b) and 4 < niter[b] < CAP and lo(a) and niter[a] == 1, "a short env with one sweep beside a tall one that sweeps on")], ("paired", "wide", "tall")))
    pairs = []
    for ps, want in cases:
        assert all(path(ref, a, b) == want for a, b in ps), (want, [path(ref, a, b) for a, b in ps])
        pairs += ps
    assert len(pairs) == 21
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, "stopping order")


@pytest.mark.parametrize("limit", [0, 1, 2])
def test_iteration_limits(hbmod, gpu, pool, ref, limit):
    """opt.iterations 0, 1 and 2 against the one-env kernel with the same limit: two envs above 16 rows, one above beside one at or below in both
    slots, (16, 17) and (17, 16), 31 rows"""
    state, tape = pool
    nefc = ref[0][2]  # (the rows of a step do not depend on the sweeps of that step)
    ok = light(ref) & (nefc >= 1)
    pk = Picker(4)
    short, tall = ok & (nefc <= ROWS_DPP), ok & (nefc > ROWS_DPP)
    pairs = [(pk.take(tall, "above 16 rows"), pk.take(tall, "above 16 rows")) for _ in range(6)]
    pairs += [(pk.take(ok & (nefc == 16), "16 rows"), pk.take(ok & (nefc == 17), "17 rows")), (pk.take(ok & (nefc == 17), "17 rows"), pk.take(ok & (nefc == 16), "16 rows"))]
    pairs += [(pk.take(short, "at most 16 rows"), pk.take(tall, "above 16 rows")) for _ in range(3)] + [(pk.take(tall, "above 16 rows"), pk.take(short, "at most 16 rows")) for _ in range(3)]
    pairs += [(pk.take(ok & (nefc == 31), "31 rows"), pk.take(tall, "above 16 rows"))]
    m = hbmod.Model.load(HUMANOID_HBM)
    m.set_opt(iterations=limit)
    sel = np.array(sorted(e for p in pairs for e in p))
    where = {e: k for k, e in enumerate(sel)}
    sub = (np.ascontiguousarray(state[sel]), np.ascontiguousarray(tape[:, sel]))
    want = reference(hbmod, m, gpu, sub[0], sub[1], 2)
    assert np.array_equal(want[0][2], nefc[sel]) and want[0][3].max() == limit and want[1][3].max() == limit
    local = [(where[a], where[b]) for a, b in pairs]
    assert all(path(want, a, b)[0] == "paired" and max(want[0][2][a], want[0][2][b]) > ROWS_DPP for a, b in local)
    assert all(path(want, a, b)[1] == (None if limit == 0 else "wide") for a, b in local)
    step_duo(hbmod, m, gpu, sub, want, local, what="iterations=%d" % limit)
    roll_duo(hbmod, m, gpu, sub, want, local, steps=2, what="iterations=%d" % limit)


def test_row_counts_that_change_inside_one_launch(hbmod, humanoid_model, gpu, pool, ref):
    """three steps in the multi-step kernel: envs whose row count rises above 16 or falls to 16 or below from one step to the next, beside an env that
    stays at or below 16 (the wave's form follows the crossing env) and beside one that stays within 17..31; envs whose row count rises above 31
    or falls to 31 or below (the wave leaves the paired layout, or returns to it) beside an env that stays within 17..31: every step chooses anew"""
    n = [ref[t][2] for t in range(STEPS)]
    calm_status = (ref[0][4] == 0) & (ref[1][4] == 0) & (ref[2][4] == 0)
    ok = light(ref, 0) & light(ref, 1) & light(ref, 2) & (n[0] >= 1)
    up16 = ok & (((n[0] <= 16) & (n[1] > 16)) | ((n[1] <= 16) & (n[2] > 16)))
    down16 = ok & (((n[0] > 16) & (n[1] <= 16)) | ((n[1] > 16) & (n[2] <= 16)))
    small = calm_status & (np.maximum(np.maximum(n[0], n[1]), n[2]) <= 63)
    up31 = small & ((light(ref, 0) & (n[1] > 31)) | (light(ref, 1) & (n[2] > 31)))
    down31 = small & (((n[0] > 31) & light(ref, 1)) | ((n[1] > 31) & light(ref, 2)))
    calm = ok & (n[0] <= 16) & (n[1] <= 16) & (n[2] <= 16)
    tall = ok & (n[0] > 16) & (n[1] > 16) & (n[2] > 16)
    print("\nwithin three steps %d envs of the pool rise above 16 rows, %d fall to 16 or below, %d rise above 31, %d fall to 31 or below" % (up16.sum(), down16.sum(), up31.sum(), down31.sum()))
    pk = Picker(5)
    pairs = []
    for k in range(4):  # both slot orders
        for mask, what in ((up16, "rows rising above 16"), (down16, "rows falling to 16 or below")):
            for other, name in ((calm, "at most 16 rows in all three steps"), (tall, "17..31 rows in all three steps")):
                c, s = pk.take(mask, what), pk.take(other, name)
                pairs.append((c, s) if k % 2 == 0 else (s, c))
    for k in range(2):
        for mask, what in ((up31, "rows rising above 31"), (down31, "rows falling to 31 or below")):
            c, s = pk.take(mask, what), pk.take(tall, "17..31 rows in all three steps")
            pairs.append((c, s) if k % 2 == 0 else (s, c))
    assert len(pairs) == 20
    # (the partner's counts are those of its own three steps whatever the wave: the reference's result for an env does not depend on its batch)
    crossing = [sorted({path(ref, a, b, t)[0] for t in range(STEPS)}) for a, b in pairs[16:]]
    assert all(c == ["packed", "paired"] for c in crossing), crossing
    roll_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=3, what="rows crossing 16 and 31")


def test_the_torque_read_out_of_wide_pairs(hbmod, humanoid_model, gpu, pool, ref):
    """a launch that asks for the joint torques (which the dual finish feeds from the forces the sweeps leave) on waves of two envs above 16 rows and of
    one above beside one at or below: the torque array, and the observations, rewards and episode ends of the env step, equal the one-env kernel's
    byte for byte"""
    state, tape = pool
    nefc, niter = ref[0][2], ref[0][3]
    ok = light(ref) & (nefc >= 1) & (niter >= 1)
    pk = Picker(6)
    short, tall = ok & (nefc <= ROWS_DPP), ok & (nefc > ROWS_DPP)
    pairs = [(pk.take(tall, "above 16 rows"), pk.take(tall, "above 16 rows")) for _ in range(16)]
    pairs += [(pk.take(short, "at most 16 rows"), pk.take(tall, "above 16 rows")) for _ in range(8)] + [(pk.take(tall, "above 16 rows"), pk.take(short, "at most 16 rows")) for _ in range(8)]
    assert all(path(ref, a, b)[:2] == ("paired", "wide") for a, b in pairs)
    idx = place(pairs, partners)
    assert len(idx) == 64
    got, names = [], []
    for duo in (0, 2):
        env = hbmod.VecEnv(humanoid_model, len(idx), gpu)
        env.batch.tune(duo=duo, schedule=0)
        env.reset()
        env.batch.set_state(hbmod.STATE_INTEGRATION, state[idx])
        obs, rew, term, trunc, info = env.step_arrays(tape[0][idx])
        got.append([env.batch.env_joint_torques(), obs.copy(), rew.copy(), term.copy(), trunc.copy()])
        names.append(env.batch.last_kernel())
        if duo == 0:
            assert np.array_equal(env.batch.counts()[1], nefc[idx])  # the waves are the ones chosen
        env.close()
    assert names[0].startswith("hb_step_h27") and names[1] == DUO, names
    assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(got[0], got[1]))
    assert got[0][0].shape == (64, humanoid_model.nv) and (np.abs(got[0][0]).max(axis=1) > 0).all()  # every env has torques to compare
    assert np.abs(got[0][2]).max() > 0  # the rewards are not all zero
