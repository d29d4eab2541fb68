"""The sweep ends of the two-envs-per-wave kernels' PGS stage (csrc/hb_step_duo.hip): the paired loops (short: both envs at most 16 rows, wide: an
env of 17..31 rows) end a sweep with ONE convergence test for both envs - each env's sum on every lane of its half, one compare, env A's verdict
in the low word of the mask and env B's in the high word - and one branch back while both go on; row count, the zero of the steps and the test
for rows are set once per solve, in the paired loops and in the tails of the one env left (short: at most 16 rows, tall: above).  None of
it changes a bit.

Method and helpers: tests/duo_lib.py; the pool is its wide_pool, shared with tests/test_gpu_duo_wide.py.  The path a wave takes (its `path`) is
asserted on the reference's own counts.
"""
import functools

import numpy as np
import pytest

import duo_lib
from duo_lib import CAP, ROWS_DPP, ROWS_HALF, STEPS, Picker, light, path

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
    lt = light(out) & (niter >= 1)
    print("\npool of %d envs, first step, envs that pair and sweep: with 1..16 rows %s; of those with one sweep %s" %
          (len(pool[0]), np.bincount(nefc[lt], minlength=17)[1:17].tolist(), np.bincount(nefc[lt & (niter == 1)], minlength=17)[1:17].tolist()))
    return out


def test_every_row_count_of_the_short_paired_loop(hbmod, humanoid_model, gpu, pool, ref):
    """the paired sweeps run max(rows A, rows B) row steps: every such count 1..16, the taller env in the lower slot and in the upper one"""
    nefc, niter = ref[0][2], ref[0][3]
    ok = light(ref) & (nefc >= 1) & (niter >= 1)
    pk = Picker(0)
    pairs = []
    for n in range(1, ROWS_DPP + 1):
        pairs.append((pk.take(ok & (nefc == n), "%d rows" % n), pk.take(ok & (nefc <= n), "at most %d rows" % n)))
        pairs.append((pk.take(ok & (nefc <= n), "at most %d rows" % n), pk.take(ok & (nefc == n), "%d rows" % n)))
    assert [max(nefc[a], nefc[b]) for a, b in pairs] == [n for n in range(1, 17) for _ in range(2)]
    assert all(path(ref, a, b)[:2] == ("paired", "short") for a, b in pairs)
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, what="short paired loop of 1..16 rows", steps=(2, 3))


def test_every_row_count_of_the_short_tail(hbmod, humanoid_model, gpu, pool, ref):
    """the env that sweeps on alone with every row count 1..16, in the lower slot and in the upper one (the partner has stopped before it, or
    has nothing to sweep)"""
    nefc, niter = ref[0][2], ref[0][3]
    ok = light(ref)
    pk = Picker(1)
    pairs = []
    for n in range(1, ROWS_DPP + 1):
        for slot in range(2):
            e = pk.take(ok & (nefc == n) & (niter >= 1), "an env of %d rows that sweeps" % n)
            o = pk.take(ok & (niter < niter[e]), "a partner that stops before sweep %d" % niter[e])
            pairs.append((e, o) if slot == 0 else (o, e))
    last = [a if niter[a] > niter[b] else b for a, b in pairs]
    assert [nefc[e] for e in last] == [n for n in range(1, 17) for _ in range(2)]
    assert all(path(ref, a, b)[0] == "paired" and path(ref, a, b)[2] == "short" for a, b in pairs)
    assert sum(path(ref, a, b)[1] is not None for a, b in pairs) >= 16  # most tails follow a paired loop
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, what="short tail of 1..16 rows", steps=(2, 3))


@pytest.mark.parametrize("form", ["short", "wide"])
def test_the_order_in_which_the_two_envs_stop(hbmod, humanoid_model, gpu, pool, ref, form):
    """one test for both envs at the end of a paired sweep: both stop in the same sweep (below the cap, and at it), A first, B first; the 50-sweep
    cap beside a stop before 10, in both slots; a paired loop of ONE sweep; and (no paired loop at all) an env without rows beside one that sweeps"""
    ncon, nefc, niter = ref[0][1], ref[0][2], ref[0][3]
    ok = light(ref) & (nefc >= 1) & (niter >= 1)
    fits = (lambda a, b: max(nefc[a], nefc[b]) <= ROWS_DPP) if form == "short" else (lambda a, b: max(nefc[a], nefc[b]) > ROWS_DPP)
    pk = Picker(2)
    pairs = [pk.pair(ok, lambda a, b: fits(a, b) and niter[a] == niter[b] < CAP, "both envs stop in the same sweep") for _ in range(3)]
    pairs += [pk.pair(ok, lambda a, b: fits(a, b) and niter[a] == niter[b] == CAP, "both envs at the cap")]
    pairs += [pk.pair(ok, lambda a, b: fits(a, b) and niter[a] < niter[b] < CAP, "env A stops first") for _ in range(3)]
    pairs += [pk.pair(ok, lambda a, b: fits(a, b) and niter[b] < niter[a] < CAP, "env B stops first") for _ in range(3)]
    pairs += [pk.pair(ok, lambda a, b: fits(a, b) and niter[a] == CAP and niter[b] < 10, "the cap beside a stop before 10"),
              pk.pair(ok, lambda a, b: fits(a, b) and niter[b] == CAP and niter[a] < 10, "the cap beside a stop before 10")]
    pairs += [pk.pair(ok, lambda a, b: fits(a, b) and niter[a] == 1 and niter[b] > 4, "a paired loop of one sweep"),
              pk.pair(ok, lambda a, b: fits(a, b) and niter[b] == 1 and niter[a] > 4, "a paired loop of one sweep")]
    assert all(path(ref, a, b)[:2] == ("paired", form) for a, b in pairs)
    assert [path(ref, a, b)[2] is None for a, b in pairs] == [True] * 4 + [False] * 10
    empty = (nefc == 0) & (ncon == 0) & (ref[0][4] == 0)
    rows = ok & (niter > 4) & ((nefc <= ROWS_DPP) if form == "short" else (nefc > ROWS_DPP))
    pairs += [(pk.take(empty, "no rows"), pk.take(rows, "more than 4 sweeps")), (pk.take(rows, "more than 4 sweeps"), pk.take(empty, "no rows"))]
    assert all(path(ref, a, b) == ("paired", None, "short" if form == "short" else "tall") for a, b in pairs[-2:])
    assert len(pairs) == 16
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs, what="stopping order, %s form" % form)


@pytest.mark.parametrize("limit", [0, 1, 2])
def test_iteration_limits(hbmod, gpu, pool, ref, limit):
    """opt.iterations 0, 1 and 2 against the one-env kernel with the same limit: the cap ends the paired loop of both forms (limit 2: or the envs'
    own tests do), and no sweep runs at 0"""
    nefc = ref[0][2]  # (the rows of a step do not depend on the sweeps of that step)
    ok = light(ref) & (nefc >= 1)
    pk = Picker(3)
    short, tall = ok & (nefc <= ROWS_DPP), ok & (nefc > ROWS_DPP)
    pairs = [(pk.take(short, "at most 16 rows"), pk.take(short, "at most 16 rows")) for _ in range(6)]
    pairs += [(pk.take(tall, "above 16 rows"), pk.take(tall, "above 16 rows")) for _ in range(4)]
    pairs += [(pk.take(short, "at most 16 rows"), pk.take(tall, "above 16 rows")) for _ in range(3)] + [(pk.take(tall, "above 16 rows"), pk.take(short, "at most 16 rows")) for _ in range(3)]

    def check(want, local):
        forms = [path(want, a, b)[:2] for a, b in local]
        assert forms == ([("paired", None)] * 16 if limit == 0 else [("paired", "short")] * 6 + [("paired", "wide")] * 10)
    duo_lib.iteration_limit_case(hbmod, gpu, pool, ref, pairs, limit, min_envs=16, check=check)


def test_wide_pairs_tall_tails_and_a_packed_wave(hbmod, humanoid_model, gpu, pool, ref):
    """(17, 17), (31, 31), (17, 1), (1, 17) in the wide paired loop; the tall tail (the env that sweeps on has more than 16 rows), in both slots;
    an env above 31 rows: the packed layout, whose sweeps are unchanged"""
    nefc, niter = ref[0][2], ref[0][3]
    ok = light(ref) & (nefc >= 1) & (niter >= 1)
    big = (nefc > ROWS_HALF) & (nefc <= 63) & (ref[0][4] == 0)
    pk = Picker(4)
    rows = lambda n: pk.take(ok & (nefc == n), "%d rows" % n)
    pairs = [(rows(17), rows(17)), (rows(31), rows(31)), (rows(17), rows(1)), (rows(1), rows(17))]
    assert [(nefc[a], nefc[b]) for a, b in pairs] == [(17, 17), (31, 31), (17, 1), (1, 17)] and all(path(ref, a, b)[:2] == ("paired", "wide") for a, b in pairs)
    tails = [pk.pair(ok, lambda a, b: nefc[a] > ROWS_DPP and niter[a] > niter[b] + 3, "a tall env that outlasts its partner") for _ in range(2)]
    tails += [pk.pair(ok, lambda a, b: nefc[b] > ROWS_DPP and niter[b] > niter[a] + 3, "a tall env that outlasts its partner") for _ in range(2)]
    assert all(path(ref, a, b) == ("paired", "wide", "tall") for a, b in tails)
    packed = [(pk.take(big, "32..63 rows"), pk.take(ok, "an env that pairs")), (pk.take(ok, "an env that pairs"), pk.take(big, "32..63 rows"))]
    assert all(path(ref, a, b)[0] == "packed" for a, b in packed)
    both_kernels(hbmod, humanoid_model, gpu, pool, ref, pairs + tails + packed, what="wide pairs, tall tails, a packed wave", steps=(2, 3))


def test_row_counts_that_cross_16_inside_a_launch(hbmod, humanoid_model, gpu, pool, ref):
    """three steps in the multi-step kernel, envs whose row count rises above 16 or falls to 16 or below from one step to the next: every step sets
    its row count and chooses its form anew"""
    n = [ref[t][2] for t in range(STEPS)]
    ok = light(ref, 0) & light(ref, 1) & light(ref, 2) & (n[0] >= 1) & (n[1] >= 1) & (n[2] >= 1)  # (rows in every step: a paired loop in every step)
    up = ok & (((n[0] <= 16) & (n[1] > 16)) | ((n[1] <= 16) & (n[2] > 16)))
    down = ok & (((n[0] > 16) & (n[1] <= 16)) | ((n[1] > 16) & (n[2] <= 16)))
    calm = ok & (n[0] <= 16) & (n[1] <= 16) & (n[2] <= 16)
    pk = Picker(5)
    pairs = []
    for k in range(4):  # beside an env that stays at or below 16 rows, so that the wave's form follows the crossing env; both slot orders
        for mask, what in ((up, "rows rising above 16"), (down, "rows falling to 16 or below")):
            c, s = pk.take(mask, what), pk.take(calm, "at most 16 rows in all three steps")
            pairs.append((c, s) if k % 2 == 0 else (s, c))
    assert all(len({path(ref, a, b, t)[1] for t in range(STEPS)} & {"short", "wide"}) == 2 for a, b in pairs)
    roll_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=3, what="rows crossing 16")
