"""The wide form of the two-envs-per-wave kernels' paired sweeps (csrc/hb_step_duo.hip): a pair in the paired layout (both envs at most 31 rows and
12 contacts) with an env of 17..31 rows holds every sweep quantity twice, once per DPP row of 16 lanes (U: rows 0..15, V: rows 16..31), and
its row step broadcasts lane k's proposal by v_fmac_f32_dpp row_newbcast inside each DPP row.  Once one env has stopped, the other sweeps on in
row layout: in the short broadcast form with at most 16 rows, in the one-env kernel's row step (v_readlane) above.  At most 16 rows in both
envs keeps the short form throughout, an env above 31 rows the packed layout.

Method and helpers: tests/duo_lib.py.  The path a wave takes (its `path`) is asserted on the reference's own contact, row and sweep counts.  The
pool is its wide_pool: bcast_pool's recipe plus three more collapsed regimes, for the rarer counts (31 rows, rows that cross 31 between two
steps).  No env of the pool above 16 rows stops after ONE sweep by its own test (none in 8 x 2048 fallen envs left alone for 100 to 3000 steps
either): a paired loop of one sweep is held by a short env with one sweep beside a tall one, and tall envs with one sweep by the iteration limit of 1.
"""
import functools

import numpy as np
import pytest

import duo_lib
from duo_lib import CAP, ROWS_DPP, STEPS, Picker, light, path

pytestmark = pytest.mark.gpu
roll_duo, both_kernels = (functools.partial(f, min_envs=16) for f in (duo_lib.roll_duo, duo_lib.both_kernels))  # every case is at least 8 waves


@pytest.fixture(scope="module")
def pool(hbmod, humanoid_model, gpu):
    """(state [N, 1 + nq + 2 nv] float32, control tape [STEPS, N, nu]): golden states | collapsed regime after 60 steps | settled regime | collapsed
    regimes after 20, 40 and 90 steps | fresh resets in the air"""
    return duo_lib.wide_pool(hbmod, humanoid_model, gpu)


@pytest.fixture(scope="module")
def ref(hbmod, humanoid_model, gpu, pool):
    out = duo_lib.wide_reference(hbmod, humanoid_model, gpu)
    nefc, niter = out[0][2], out[0][3]
    lt = light(out)
    print("\npool of %d envs, first step: rows 0..%d, %d envs that pair; of those with 17..31 rows: %s; with 32..63 rows and no warning: %d; "
          "tall and at the sweep cap %d, tall with one sweep %d" % (len(pool[0]), nefc.max(), lt.sum(), np.bincount(nefc[lt], minlength=32)[17:32].tolist(),
                                                                   ((nefc >= 32) & (nefc <= 63) & (out[0][4] == 0)).sum(),
                                                                   (lt & (nefc > 16) & (niter == CAP)).sum(), (lt & (nefc > 16) & (niter == 1)).sum()))
    return out


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
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, what="edges of the wide form", steps=(2, 3))


def test_every_residue_mod_4_of_both_row_counts(hbmod, humanoid_model, gpu, pool, ref):
    """both envs within 17..31 rows, every combination of the two counts mod 4: the chunks of four of the V rows, and the last chunk of three"""
    nefc, niter = ref[0][2], ref[0][3]
    ok = light(ref) & (nefc > ROWS_DPP) & (niter >= 1)
    pk = Picker(1)
    pairs = [(pk.take(ok & (nefc % 4 == ra), "17..31 rows, %d mod 4" % ra), pk.take(ok & (nefc % 4 == rb), "17..31 rows, %d mod 4" % rb)) for ra in range(4) for rb in range(4)]
    assert len({(nefc[a] % 4, nefc[b] % 4) for a, b in pairs}) == 16
    assert all(17 <= nefc[e] <= 31 for p in pairs for e in p) and all(path(ref, a, b)[:2] == ("paired", "wide") for a, b in pairs)
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, what="17..31 rows mod 4")


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
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, what="16 | 17 and 31 | 32 rows")


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
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, what="stopping order")


@pytest.mark.parametrize("limit", [0, 1, 2])
def test_iteration_limits(hbmod, gpu, pool, ref, limit):
    """opt.iterations 0, 1 and 2 against the one-env kernel with the same limit: two envs above 16 rows, one above beside one at or below in both
    slots, (16, 17) and (17, 16), 31 rows"""
    nefc = ref[0][2]  # (the rows of a step do not depend on the sweeps of that step)
    ok = light(ref) & (nefc >= 1)
    pk = Picker(4)
    short, tall = ok & (nefc <= ROWS_DPP), ok & (nefc > ROWS_DPP)
    pairs = [(pk.take(tall, "above 16 rows"), pk.take(tall, "above 16 rows")) for _ in range(6)]
    pairs += [(pk.take(ok & (nefc == 16), "16 rows"), pk.take(ok & (nefc == 17), "17 rows")), (pk.take(ok & (nefc == 17), "17 rows"), pk.take(ok & (nefc == 16), "16 rows"))]
    pairs += [(pk.take(short, "at most 16 rows"), pk.take(tall, "above 16 rows")) for _ in range(3)] + [(pk.take(tall, "above 16 rows"), pk.take(short, "at most 16 rows")) for _ in range(3)]
    pairs += [(pk.take(ok & (nefc == 31), "31 rows"), pk.take(tall, "above 16 rows"))]

    def check(want, local):
        assert all(path(want, a, b)[0] == "paired" and max(want[0][2][a], want[0][2][b]) > ROWS_DPP for a, b in local)
        assert all(path(want, a, b)[1] == (None if limit == 0 else "wide") for a, b in local)
    duo_lib.iteration_limit_case(hbmod, gpu, pool, ref, pairs, limit, min_envs=16, check=check)


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
    nefc, niter = ref[0][2], ref[0][3]
    ok = light(ref) & (nefc >= 1) & (niter >= 1)
    pk = Picker(6)
    short, tall = ok & (nefc <= ROWS_DPP), ok & (nefc > ROWS_DPP)
    pairs = [(pk.take(tall, "above 16 rows"), pk.take(tall, "above 16 rows")) for _ in range(16)]
    pairs += [(pk.take(short, "at most 16 rows"), pk.take(tall, "above 16 rows")) for _ in range(8)] + [(pk.take(tall, "above 16 rows"), pk.take(short, "at most 16 rows")) for _ in range(8)]
    assert all(path(ref, a, b)[:2] == ("paired", "wide") for a, b in pairs)
    duo_lib.torque_readout_case(hbmod, humanoid_model, gpu, pool, ref, pairs)
