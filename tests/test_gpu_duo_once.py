"""The stages of the two-envs-per-wave kernels (csrc/hb_step_duo.hip) that compute per-dof and per-tile work once: crb[body(i)] cdof_i once
per dof in the qM stage, the AR columns of a pair of envs at most 31 rows each handed over by one swap per register, and the tiles of
C = J W stored whole.

hb_step_duo_kernel and hb_step_duo_q_kernel are held byte for byte (time, qpos, qvel, warm start, ncon / nefc / sweeps, status) to
hb_step_h27_kernel, the one-env kernel, on waves put together for the path they are to take.  Every case is at most 64 envs and one to three
steps.  The one-env kernel's result for an env does not depend on the batch around it, so it is computed ONCE, for a pool of states (the
128 golden states of the fp64 oracle, the collapsed regime of tests/test_gpu_duo.py, bodies laid flat into the floor, fresh resets lifted
off it) over three steps, and every case is an index list into that pool, laid out so that the duo kernels' pairing of dispatch slots puts the chosen envs into
one wave.  Which path a wave takes is asserted on the reference's own contact and row counts.
"""
import os

import numpy as np
import pytest

from oracle_lib import GOLDEN

pytestmark = pytest.mark.gpu
ONE, DUO, DUO_Q = "hb_step_h27_kernel", "hb_step_duo_kernel", "hb_step_duo_q_kernel"
STEPS = 3
NCON_HALF = 12   # contacts per env while two envs share a wave (kNCh)
ROWS_HALF = 31   # rows per env of the paired sweeps


def partners(n, anti=16):
    """env -> the env it shares its wave with (-1: none), as hb_step_duo_kernel pairs the dispatch slots of an n-env launch without a
    heavy-first order: the first `anti` slots with the last ones, the others with their neighbour (csrc/hb_step_duo.hip: kDuoAnti)"""
    k = min(anti, n >> 2)
    p = np.full(n, -1)
    for e in range(n):
        if e < k or e >= n - k:
            p[e] = n - 1 - e
        else:
            q = e + 1 if (e - k) % 2 == 0 else e - 1
            p[e] = q if q < n - k else -1
    return p


def partners_q(n):
    """the same for hb_step_duo_q_kernel: every slot with the one from the other end of the launch (the middle one of an odd count: none)"""
    p = n - 1 - np.arange(n)
    p[p == np.arange(n)] = -1
    return p


def place(pairs, singles, pairing):
    """pool indices per dispatch slot such that `pairing` puts every (a, b) of `pairs` into one wave, a in the lower slot (lanes 0..31)"""
    n = 2 * len(pairs) + len(singles)
    p = pairing(n)
    assert (p < 0).sum() == len(singles), (n, p)
    idx = np.full(n, -1)
    pairs, singles = list(pairs), list(singles)
    for e in range(n):
        if p[e] < 0:
            idx[e] = singles.pop(0)
        elif p[e] > e:
            assert p[p[e]] == e
            idx[e], idx[p[e]] = pairs.pop(0)
    assert (idx >= 0).all() and not pairs and not singles
    return idx


def fits_packed(nf, ns):
    """rows of two envs, the larger above 31, that one wave's 64 row lanes hold (csrc/hb_step_duo.hip: split)"""
    return max((nf + 1 + 3) & ~3, 32) + ns + 1 <= 64


@pytest.fixture(scope="module")
def pool(hbmod, humanoid_model, gpu):
    """(state [N, 1 + nq + 2 nv] float32, control tape [STEPS, N, nu]): golden states | collapsed regime | lying flat | fresh resets in the air"""
    m = humanoid_model
    g = np.load(os.path.join(GOLDEN, "humanoid27_steps.npz"))
    gstate = np.concatenate([g["time"][:, None], g["qpos"], g["qvel"], g["warm"]], axis=1).astype(np.float32)
    gctrl = g["ctrl"].astype(np.float32)
    n = 1792
    b = hbmod.Batch(m, n, gpu)
    b.reset(perturb=True)
    rng = np.random.default_rng(11)
    b.rollout_halton(150)
    cctrl = np.sign(rng.uniform(-1, 1, size=(n, m.nu))).astype(np.float32)  # saturated actuators: limbs driven into the floor
    for _ in range(60):
        b.step(cctrl)
    cstate = b.get_state(hbmod.STATE_INTEGRATION)
    b.close()
    a = hbmod.Batch(m, 64, gpu)
    a.reset(perturb=True)
    astate = a.get_state(hbmod.STATE_INTEGRATION)
    a.close()
    # lying flat, pressed into the floor: on the back, the front and either side at eight heights, limbs a little bent - every capsule of
    # the body against the plane, more contacts than the collapsed regime reaches
    lstate = astate.copy()
    lstate[:, 1 + m.nq:] = 0.0
    r = np.sqrt(0.5)
    for k in range(64):
        lstate[k, 1 + 2] = 0.03 + 0.012 * (k % 8)
        lstate[k, 1 + 3:1 + 7] = ((r, 0, -r, 0), (r, 0, r, 0), (0.5, 0.5, -0.5, 0.5), (0.5, -0.5, -0.5, -0.5))[(k // 8) % 4]
    lstate[:, 1 + 7:1 + m.nq] = np.random.default_rng(5).uniform(-0.1, 0.1, size=(64, m.nq - 7))
    astate[:, 1 + 2] += 1.0  # one metre up: no contact
    actrl = np.zeros((64, m.nu), np.float32)
    state = np.ascontiguousarray(np.concatenate([gstate, cstate, lstate, astate]), dtype=np.float32)
    ctrl = np.concatenate([gctrl, cctrl, actrl, actrl])
    tape = np.stack([np.roll(ctrl, 7 * t, axis=0) for t in range(STEPS)])
    tape[:, -64:] = 0.0  # (the envs in the air stay limp: no joint runs into its limit)
    return state, np.ascontiguousarray(tape)


@pytest.fixture(scope="module")
def ref(hbmod, humanoid_model, gpu, pool):
    """the one-env kernel's STEPS steps of the pool: per step (state, ncon, nefc, niter, status)"""
    state, tape = pool
    r = hbmod.Batch(humanoid_model, len(state), gpu)
    r.tune(duo=0)
    r.set_state(hbmod.STATE_INTEGRATION, state)
    out = []
    for t in range(STEPS):
        r.step(tape[t])
        assert r.last_kernel() == ONE
        ncon, nefc, niter = r.counts()
        out.append((r.get_state(hbmod.STATE_INTEGRATION), ncon, nefc, niter, r.status()))
    r.close()
    ncon, nefc = out[0][1], out[0][2]
    print("\npool of %d envs, first step: rows 0..%d (%d envs above 31, %d without rows), contacts 0..%d (%d envs above 12)"
          % (len(state), nefc.max(), (nefc > 31).sum(), (nefc == 0).sum(), ncon.max(), (ncon > 12).sum()))
    return out


def same_bytes(b, hbmod, want, idx, what):
    """state, counts [0..2] and status of batch b against the reference's of the pool envs idx, byte for byte"""
    ws, wncon, wnefc, wniter, wstatus = want
    got = b.get_state(hbmod.STATE_INTEGRATION)
    assert got.dtype == np.float32 and ws.dtype == np.float32
    bad = np.flatnonzero((got.view(np.uint32) != ws[idx].view(np.uint32)).any(axis=1))
    assert bad.size == 0, (what, "state of slots", bad[:8], "rows", wnefc[idx][bad[:8]], "contacts", wncon[idx][bad[:8]])
    for name, x, y in zip(("ncon", "nefc", "niter"), b.counts(), (wncon, wnefc, wniter)):
        assert np.array_equal(x, y[idx]), (what, name, np.flatnonzero(x != y[idx])[:8])
    assert np.array_equal(b.status(), wstatus[idx]), (what, "status")


def step_duo(hbmod, m, gpu, pool, ref, pairs, singles=(), what=""):
    """one step through hb_step_duo_kernel"""
    state, tape = pool
    idx = place(pairs, singles, partners)
    assert len(idx) <= 64
    b = hbmod.Batch(m, len(idx), gpu)
    b.tune(duo=2, schedule=0)  # (no heavy-first order: the pairing is that of the dispatch slots)
    b.set_state(hbmod.STATE_INTEGRATION, state[idx])
    b.step(tape[0][idx])
    assert b.last_kernel() == DUO
    same_bytes(b, hbmod, ref[0], idx, what + " [%s]" % DUO)
    b.close()


def roll_duo(hbmod, m, gpu, pool, ref, pairs, singles=(), steps=2, what=""):
    """`steps` steps through hb_step_duo_q_kernel (the state stays on chip in between)"""
    state, tape = pool
    idx = place(pairs, singles, partners_q)
    assert len(idx) <= 64 and 2 <= steps <= STEPS
    b = hbmod.Batch(m, len(idx), gpu)
    b.tune(duo=2, schedule=0)
    b.set_state(hbmod.STATE_INTEGRATION, state[idx])
    b.rollout(np.ascontiguousarray(tape[:steps, idx]))
    assert b.last_kernel() == DUO_Q
    same_bytes(b, hbmod, ref[steps - 1], idx, what + " [%s, %d steps]" % (DUO_Q, steps))
    b.close()


def light(ref, t=0):
    """envs that share a wave in the paired layout at step t: at most 12 contacts and 31 rows, no warning"""
    return (ref[t][1] <= NCON_HALF) & (ref[t][2] <= ROWS_HALF) & (ref[t][4] == 0)


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
    got, names = [], []
    for duo in (0, 2):
        env = hbmod.VecEnv(humanoid_model, n, gpu)
        env.batch.tune(duo=duo)
        out = [env.reset().copy()]
        for t in range(2):
            obs, rew, term, trunc, info = env.step_arrays(acts[t])
            out += [obs.copy(), rew.copy(), term.copy(), trunc.copy()]
        names.append(env.batch.last_kernel())
        got.append(out)
        env.close()
    assert names[0].startswith("hb_step_h27") and names[1] == DUO, names
    assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(got[0], got[1]))
    assert all(np.abs(x).max() > 0 for x in got[0][2::4])  # the rewards are not all zero
