"""The stages of the two-envs-per-wave kernels (csrc/hb_step_duo.hip) that compute per-dof and per-tile work once: crb[body(i)] cdof_i once
per dof in the qM stage, the AR columns of a pair of envs at most 31 rows each handed over by one swap per register, and the tiles of
C = J W stored whole.

Method and helpers: tests/duo_lib.py.  Every case is at most 64 envs and one to three steps of its once_pool: the 128 golden states of the
fp64 oracle, the collapsed regime of tests/test_gpu_duo.py, bodies laid flat into the floor, fresh resets lifted off it.  Which path a wave
takes is asserted on the reference's own contact and row counts.
"""
import numpy as np
import pytest

import duo_lib
from duo_lib import DUO, NCON_HALF, ROWS_HALF, STEPS, env_steps_both_ways, fits_packed, light, partners, partners_q, roll_duo, step_duo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool(hbmod, humanoid_model, gpu):
    """(state [N, 1 + nq + 2 nv] float32, control tape [STEPS, N, nu]): golden states | collapsed regime | lying flat | fresh resets in the air"""
    return duo_lib.once_pool(hbmod, humanoid_model, gpu)


@pytest.fixture(scope="module")
def ref(hbmod, humanoid_model, gpu, pool):
    """the one-env kernel's STEPS steps of the pool: per step (state, ncon, nefc, niter, status)"""
    out = duo_lib.reference(hbmod, humanoid_model, gpu, *pool, STEPS)
    ncon, nefc = out[0][1], out[0][2]
    print("\npool of %d envs, first step: rows 0..%d (%d envs above 31, %d without rows), contacts 0..%d (%d envs above 12)"
          % (len(pool[0]), nefc.max(), (nefc > 31).sum(), (nefc == 0).sum(), ncon.max(), (ncon > 12).sum()))
    return out


def test_every_residue_of_the_two_row_counts(hbmod, humanoid_model, gpu, pool, ref):
    """both envs of a wave at most 31 rows (the paired sweeps: one swap per register hands both envs their AR columns), two waves for
    every combination of the row counts mod 4"""
    nefc = ref[0][2]
    ok = light(ref) & (nefc >= 1)
    rng = np.random.default_rng(0)
    used, pairs = set(), []
    for ra in range(4):
        for rb in range(4):
            for _ in range(2):
                a = [e for e in rng.permutation(np.flatnonzero(ok & (nefc % 4 == ra))) if e not in used][0]
                used.add(a)
                b = [e for e in rng.permutation(np.flatnonzero(ok & (nefc % 4 == rb))) if e not in used][0]
                used.add(b)
                pairs.append((a, b))
    combos = {(nefc[a] % 4, nefc[b] % 4) for a, b in pairs}
    assert len(pairs) == 32 and len(combos) == 16
    assert all(1 <= nefc[e] <= ROWS_HALF and ref[0][1][e] <= NCON_HALF for p in pairs for e in p)
    assert max(nefc[e] for p in pairs for e in p) >= 20  # (not only short columns)
    step_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, what="residues")
    roll_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=2, what="residues")


def test_an_env_above_31_rows_beside_a_light_one(hbmod, humanoid_model, gpu, pool, ref):
    """split > 32: the general AR layout (two swaps per register, the select-free sweep over the packed rows) and the second row tile of C"""
    ncon, nefc, status = ref[0][1], ref[0][2], ref[0][4]
    heavy = np.flatnonzero((nefc > ROWS_HALF) & (ncon <= NCON_HALF) & (status == 0))
    lights = [e for e in np.flatnonzero(light(ref) & (nefc >= 1)) if nefc[e] <= 12]
    pairs = []
    for k, hv in enumerate(heavy[:16]):
        lt = next((e for e in lights if fits_packed(nefc[hv], nefc[e])), None)
        if lt is None:
            continue
        lights.remove(lt)
        pairs.append((hv, lt) if k % 2 == 0 else (lt, hv))  # the heavy env in the lower and in the upper slot
    assert len(pairs) >= 4, (len(heavy), len(pairs))
    for a, b in pairs:
        nf, ns = max(nefc[a], nefc[b]), min(nefc[a], nefc[b])
        assert nf > 31 and fits_packed(nf, ns) and max(ncon[a], ncon[b]) <= NCON_HALF
    assert any(nefc[a] > 31 for a, _ in pairs) and any(nefc[b] > 31 for _, b in pairs)
    step_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, what="heavy beside light")
    roll_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=2, what="heavy beside light")


def test_an_env_above_12_contacts_is_stepped_alone(hbmod, humanoid_model, gpu, pool, ref):
    """more contacts than two envs to a wave hold: the wave steps its envs one at a time, at the one-env kernel's capacities"""
    ncon, nefc = ref[0][1], ref[0][2]
    many = np.flatnonzero(ncon > NCON_HALF)
    others = np.flatnonzero(light(ref) & (nefc >= 1))
    assert len(many) >= 2, len(many)
    many = many[:16]
    pairs = [(c, others[k]) if k % 2 == 0 else (others[k], c) for k, c in enumerate(many)]
    assert all(max(ncon[a], ncon[b]) > NCON_HALF for a, b in pairs)
    step_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, what="one env at a time")
    roll_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=2, what="one env at a time")


def test_an_odd_env_count(hbmod, humanoid_model, gpu, pool, ref):
    """the last wave holds one env"""
    nefc = ref[0][2]
    ok = np.flatnonzero(light(ref) & (nefc >= 4))
    rng = np.random.default_rng(1)
    pick = rng.permutation(ok)[:63]
    assert len(pick) == 63
    pairs, single = [(pick[2 * k], pick[2 * k + 1]) for k in range(31)], [pick[62]]
    assert (partners(63) < 0).sum() == 1 and (partners_q(63) < 0).sum() == 1 and nefc[single[0]] >= 4
    step_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, single, what="odd count")
    roll_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, single, steps=2, what="odd count")


def test_an_env_without_rows_beside_one_with_rows(hbmod, humanoid_model, gpu, pool, ref):
    """a fresh reset in the air: of its rows of C only the qfrc_smooth row exists (the whole-tile store of C = J W), beside an env in contact"""
    ncon, nefc = ref[0][1], ref[0][2]
    empty = np.flatnonzero((nefc == 0) & (ncon == 0) & (ref[0][4] == 0))
    rows = np.flatnonzero(light(ref) & (nefc >= 8))
    assert len(empty) >= 10 and len(rows) >= 8
    pairs = [(empty[k], rows[k]) if k % 2 == 0 else (rows[k], empty[k]) for k in range(8)] + [(empty[8], empty[9])]
    assert all(min(nefc[a], nefc[b]) == 0 for a, b in pairs) and sum(max(nefc[a], nefc[b]) >= 8 for a, b in pairs) == 8
    step_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, what="no rows beside rows")
    roll_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=3, what="no rows beside rows")


def test_row_counts_that_fall_from_step_to_step(hbmod, humanoid_model, gpu, pool, ref):
    """three steps in the multi-step kernel, both envs of a wave with fewer rows in every step than in the one before: rows a whole-tile
    store of C left behind lie beyond the env's count in the next step, and are never read as live"""
    n0, n1, n2 = ref[0][2], ref[1][2], ref[2][2]
    ok = light(ref, 0) & light(ref, 1) & light(ref, 2)
    falling = np.flatnonzero(ok & (n0 > n1) & (n1 > n2))
    print("\n%d envs of the pool with rows falling over three steps, e.g. %s" % (len(falling), [(n0[e], n1[e], n2[e]) for e in falling[:6]]))
    assert len(falling) >= 4, len(falling)
    falling = falling[:min(len(falling), 64) // 2 * 2]
    pairs = [(falling[2 * k], falling[2 * k + 1]) for k in range(len(falling) // 2)]
    assert all(n0[e] > n1[e] > n2[e] for p in pairs for e in p)
    # ... and from above 31 rows (the second row tile stored whole) to below, beside a light env, where the pool has such envs
    tall = [e for e in np.flatnonzero((n0 > ROWS_HALF) & (n2 <= ROWS_HALF) & (n1 <= n0) & (ref[0][1] <= NCON_HALF) & (ref[2][4] == 0))]
    small = [e for e in np.flatnonzero(ok & (n0 <= 10) & (n1 <= 10) & (n2 <= 10)) if e not in set(falling)]
    extra = [(t, s) for t, s in zip(tall[:4], small) if fits_packed(n0[t], n0[s])]
    pairs = pairs[:32 - len(extra)] + extra
    roll_duo(hbmod, humanoid_model, gpu, pool, ref, pairs, steps=3, what="falling rows")


def test_the_torque_read_out_is_the_one_env_kernels(hbmod, humanoid_model, gpu):
    """steps that ask for qfrc_smooth + qfrc_constraint = M qacc (the env adapter's reward reads it): the sum runs over all of the sparse M
    the qM stage left in LDS, so observations, rewards and episode ends equal the one-env kernel's"""
    n = 64
    acts = np.random.default_rng(9).uniform(-1, 1, (2, n, humanoid_model.nu)).astype(np.float32)
    got, names = env_steps_both_ways(hbmod, humanoid_model, gpu, acts)
    assert names[0].startswith("hb_step_h27") and names[1] == DUO, names
    assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(got[0], got[1]))
    assert all(np.abs(x).max() > 0 for x in got[0][2::4])  # the rewards are not all zero
