"""The DPP broadcast forms of the two-envs-per-wave kernels (csrc/hb_step_duo.hip): when both envs of a wave have at most 16 rows, the paired
Gauss-Seidel row step hands lane k's proposal to the row lanes of its env by v_fmac_f32_dpp row_newbcast:k; the one-env tail takes that form
whenever the env that sweeps on has at most 16 rows.  Above 16 rows the sweeps keep their earlier form.

Method and helpers: tests/duo_lib.py.  The pool is its bcast_pool (the 128 golden states of the fp64 oracle, a collapsed regime, the benchmark's
settled regime, fresh resets in the air) over three steps; which path a wave takes is asserted on the reference's own row and sweep counts.
"""
import functools

import pytest

import duo_lib
from duo_lib import CAP, ROWS_DPP, STEPS, Picker, light

pytestmark = pytest.mark.gpu
step_duo, roll_duo = (functools.partial(f, min_envs=16) for f in (duo_lib.step_duo, duo_lib.roll_duo))  # every case is at least 8 waves


@pytest.fixture(scope="module")
def pool(hbmod, humanoid_model, gpu):
    """(state [N, 1 + nq + 2 nv] float32, control tape [STEPS, N, nu]): golden states | collapsed regime | settled regime | fresh resets in the air"""
    return duo_lib.bcast_pool(hbmod, humanoid_model, gpu)


@pytest.fixture(scope="module")
def ref(hbmod, humanoid_model, gpu, pool):
    out = duo_lib.reference(hbmod, humanoid_model, gpu, *pool, STEPS, kernel=duo_lib.ONE_ANY)
    nefc, niter, lt = out[0][2], out[0][3], light(out)
    print("\npool of %d envs, first step: rows 0..%d, %d envs that pair; of those %d at most 16 rows, %d / %d / %d / %d with 1 / 15 / 16 / 17 rows, "
          "%d at the sweep cap, %d with one sweep" % (len(pool[0]), nefc.max(), lt.sum(), (lt & (nefc <= 16)).sum(), (lt & (nefc == 1)).sum(),
                                                     (lt & (nefc == 15)).sum(), (lt & (nefc == 16)).sum(), (lt & (nefc == 17)).sum(),
                                                     (lt & (niter == CAP)).sum(), (lt & (niter == 1)).sum()))
    return out


def test_both_envs_at_most_16_rows(hbmod, humanoid_model, gpu, pool, ref):
    """the short form of the paired sweeps and the tail: every combination of the two row counts mod 4, 16 rows in one env,
    16 rows in both, an env of one row"""
    nefc = ref[0][2]
    ok = light(ref) & (nefc >= 1) & (nefc <= ROWS_DPP)
    pk = Picker(0)
    pairs = [(pk.take(ok & (nefc % 4 == ra), "%d rows mod 4" % ra), pk.take(ok & (nefc % 4 == rb), "%d rows mod 4" % rb)) for ra in range(4) for rb in range(4)]
    pairs += [(pk.take(ok & (nefc == 16), "16 rows"), pk.take(ok & (nefc < 16), "below 16 rows")),
              (pk.take(ok & (nefc < 16), "below 16 rows"), pk.take(ok & (nefc == 16), "16 rows")),
              (pk.take(ok & (nefc == 16), "16 rows"), pk.take(ok & (nefc == 16), "16 rows")),
              (pk.take(ok & (nefc == 1), "1 row"), pk.take(ok & (nefc > 4), "above 4 rows")),
              (pk.take(ok & (nefc > 4), "above 4 rows"), pk.take(ok & (nefc == 1), "1 row"))]
    assert len({(nefc[a] % 4, nefc[b] % 4) for a, b in pairs}) == 16
    assert all(1 <= nefc[e] <= ROWS_DPP for p in pairs for e in p)
    assert any(nefc[a] == 16 and nefc[b] == 16 for a, b in pairs) and any(min(nefc[a], nefc[b]) == 1 for a, b in pairs)
    step_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, what="at most 16 rows")
    roll_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=2, what="at most 16 rows")


def test_the_boundary_between_16_and_17_rows(hbmod, humanoid_model, gpu, pool, ref):
    """(16, 17), (17, 16), (15, 16), (17, 17): the paired loop keeps its earlier form as soon as one env is above 16 rows"""
    nefc = ref[0][2]
    ok = light(ref)
    pk = Picker(1)
    pairs = []
    for na, nb in ((16, 17), (17, 16), (15, 16), (17, 17)):
        for _ in range(3):
            pairs.append((pk.take(ok & (nefc == na), "%d rows" % na), pk.take(ok & (nefc == nb), "%d rows" % nb)))
    assert [(nefc[a], nefc[b]) for a, b in pairs] == [x for x in ((16, 17), (17, 16), (15, 16), (17, 17)) for _ in range(3)]
    step_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, what="16 | 17 rows")
    roll_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=2, what="16 | 17 rows")


def test_the_tail_after_a_paired_loop_of_the_other_form(hbmod, humanoid_model, gpu, pool, ref):
    """one env above 16 rows: the paired loop in its earlier form, then the tail in the short form (the env above 16 stops first and the
    one at or below 16 sweeps on) or in the earlier form (the reverse), in both slot orders"""
    nefc, niter = ref[0][2], ref[0][3]
    ok = light(ref) & (nefc >= 1) & (niter >= 1)
    pk = Picker(2)
    lo, hi = (lambda e: nefc[e] <= ROWS_DPP), (lambda e: nefc[e] > ROWS_DPP)
    short_tail = [pk.pair(ok, lambda a, b: lo(a) and hi(b) and niter[b] < niter[a], "a short env that outlasts a tall one") for _ in range(4)]
    short_tail += [pk.pair(ok, lambda a, b: hi(a) and lo(b) and niter[a] < niter[b], "a short env that outlasts a tall one") for _ in range(4)]
    long_tail = [pk.pair(ok, lambda a, b: lo(a) and hi(b) and niter[a] < niter[b], "a tall env that outlasts a short one") for _ in range(4)]
    long_tail += [pk.pair(ok, lambda a, b: hi(a) and lo(b) and niter[b] < niter[a], "a tall env that outlasts a short one") for _ in range(4)]
    for pairs, what in ((short_tail, "short tail"), (long_tail, "tall tail")):
        assert len(pairs) == 8 and all(min(nefc[a], nefc[b]) <= ROWS_DPP < max(nefc[a], nefc[b]) and niter[a] != niter[b] for a, b in pairs)
        last = [a if niter[a] > niter[b] else b for a, b in pairs]  # the env of the tail
        assert all((nefc[e] <= ROWS_DPP) == (what == "short tail") for e in last)
        step_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, what=what)
        roll_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=2, what=what)


def test_sweep_counts_of_the_two_envs(hbmod, humanoid_model, gpu, pool, ref):
    """both envs at most 16 rows: the lower slot sweeping longer, shorter and as long as the upper; an env at the 50-sweep cap beside one
    that stops before 10; an env that stops after one sweep; an env without rows beside one that sweeps"""
    ncon, nefc, niter = ref[0][1], ref[0][2], ref[0][3]
    ok = light(ref) & (nefc >= 1) & (nefc <= ROWS_DPP)
    pk = Picker(3)
    pairs = [pk.pair(ok, lambda a, b: niter[a] > niter[b] + 3, "lower slot sweeps longer") for _ in range(2)]
    pairs += [pk.pair(ok, lambda a, b: niter[b] > niter[a] + 3, "upper slot sweeps longer") for _ in range(2)]
    pairs += [pk.pair(ok, lambda a, b: niter[a] == niter[b] and niter[a] < CAP, "equal sweep counts below the cap") for _ in range(2)]
    pairs += [pk.pair(ok, lambda a, b: niter[a] == CAP and 1 <= niter[b] < 10, "the cap beside fewer than 10 sweeps"),
              pk.pair(ok, lambda a, b: niter[b] == CAP and 1 <= niter[a] < 10, "the cap beside fewer than 10 sweeps"),
              pk.pair(ok, lambda a, b: niter[a] == CAP and niter[b] == CAP, "both at the cap")]
    pairs += [pk.pair(ok, lambda a, b: niter[a] == 1 and niter[b] > 4, "one sweep"), pk.pair(ok, lambda a, b: niter[b] == 1 and niter[a] > 4, "one sweep")]
    empty = (nefc == 0) & (ncon == 0) & (ref[0][4] == 0)
    pairs += [(pk.take(empty, "no rows"), pk.take(ok & (niter > 4), "more than 4 sweeps")), (pk.take(ok & (niter > 4), "more than 4 sweeps"), pk.take(empty, "no rows"))]
    assert len(pairs) == 13 and all(max(nefc[a], nefc[b]) <= ROWS_DPP for a, b in pairs)
    assert sum(min(nefc[a], nefc[b]) == 0 and max(niter[a], niter[b]) > 4 for a, b in pairs) == 2
    assert sum(max(niter[a], niter[b]) == CAP and 1 <= min(niter[a], niter[b]) < 10 for a, b in pairs) >= 2
    assert sum(min(niter[a], niter[b]) == 1 for a, b in pairs) >= 2
    step_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, what="sweep counts")
    roll_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=2, what="sweep counts")


@pytest.mark.parametrize("limit", [0, 1, 2])
def test_iteration_limits(hbmod, gpu, pool, ref, limit):
    """opt.iterations 0, 1 and 2 against the one-env kernel with the same limit: waves of at most 16 rows, of 16 | 17 rows and with one env above 16"""
    nefc = ref[0][2]  # (the rows of a step do not depend on the sweeps of that step)
    ok = light(ref) & (nefc >= 1)
    pk = Picker(4)
    short, tall = ok & (nefc <= ROWS_DPP), ok & (nefc > ROWS_DPP)
    pairs = [(pk.take(short, "at most 16 rows"), pk.take(short, "at most 16 rows")) for _ in range(8)]
    pairs += [(pk.take(ok & (nefc == 16), "16 rows"), pk.take(ok & (nefc == 17), "17 rows")), (pk.take(ok & (nefc == 17), "17 rows"), pk.take(ok & (nefc == 16), "16 rows"))]
    pairs += [(pk.take(short, "at most 16 rows"), pk.take(tall, "above 16 rows")) for _ in range(3)] + [(pk.take(tall, "above 16 rows"), pk.take(short, "at most 16 rows")) for _ in range(3)]
    duo_lib.iteration_limit_case(hbmod, gpu, pool, ref, pairs, limit, min_envs=16)


def test_row_counts_that_cross_16_between_steps(hbmod, humanoid_model, gpu, pool, ref):
    """three steps in the multi-step kernel, envs whose row count rises above 16 or falls to 16 or below from one step to the next: every
    step chooses its form anew"""
    n = [ref[t][2] for t in range(STEPS)]
    ok = light(ref, 0) & light(ref, 1) & light(ref, 2) & (n[0] >= 1)
    up = ok & (((n[0] <= 16) & (n[1] > 16)) | ((n[1] <= 16) & (n[2] > 16)))
    down = ok & (((n[0] > 16) & (n[1] <= 16)) | ((n[1] > 16) & (n[2] <= 16)))
    calm = ok & (n[0] <= 16) & (n[1] <= 16) & (n[2] <= 16)
    print("\n%d envs of the pool rise above 16 rows within three steps, %d fall to 16 or below" % (up.sum(), down.sum()))
    pk = Picker(5)
    pairs = []
    for k in range(6):  # beside an env that stays at or below 16 rows, so that the wave's form follows the crossing env; both slot orders
        for mask, what in ((up, "rows rising above 16"), (down, "rows falling to 16 or below")):
            c, s = pk.take(mask, what), pk.take(calm, "at most 16 rows in all three steps")
            pairs.append((c, s) if k % 2 == 0 else (s, c))
    pairs += [(pk.take(up, "rows rising above 16"), pk.take(down, "rows falling to 16 or below")) for _ in range(2)]
    assert len(pairs) == 14
    roll_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=3, what="rows crossing 16")


def test_the_torque_read_out(hbmod, humanoid_model, gpu, pool, ref):
    """a launch that asks for the joint torques (qfrc_smooth + qfrc_constraint = M qacc, which the dual finish feeds; the env adapter's reward
    reads them) on waves of at most 16 rows and of one env above 16: the torque array itself, and the observations, rewards and episode ends
    of the env step, equal the one-env kernel's byte for byte"""
    nefc = ref[0][2]
    ok = light(ref) & (nefc >= 1)
    pk = Picker(6)
    short, tall = ok & (nefc <= ROWS_DPP), ok & (nefc > ROWS_DPP)
    pairs = [(pk.take(short, "at most 16 rows"), pk.take(short, "at most 16 rows")) for _ in range(16)]
    pairs += [(pk.take(short, "at most 16 rows"), pk.take(tall, "above 16 rows")) for _ in range(8)] + [(pk.take(tall, "above 16 rows"), pk.take(short, "at most 16 rows")) for _ in range(8)]
    duo_lib.torque_readout_case(hbmod, humanoid_model, gpu, pool, ref, pairs)
