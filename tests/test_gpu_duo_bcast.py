"""The DPP broadcast forms of the two-envs-per-wave kernels (csrc/hb_step_duo.hip): when both envs of a wave have at most 16 rows, the paired
Gauss-Seidel row step hands lane k's proposal to the row lanes of its env by v_fmac_f32_dpp row_newbcast:k; the one-env tail takes that form
whenever the env that sweeps on has at most 16 rows.  Above 16 rows the sweeps keep their earlier form.

hb_step_duo_kernel (one step) and hb_step_duo_q_kernel (two and three steps, the state on chip in between) are held byte for byte (time,
qpos, qvel, warm start, ncon / nefc / sweeps, status) to hb_step_h27_kernel, the one-env kernel, on waves put together for the path they are to
take.  The one-env kernel's result for an env does not depend on the batch around it, so it is computed ONCE for a pool of states (the 128
golden states of the fp64 oracle, a collapsed regime, the benchmark's settled regime, fresh resets in the air) over three steps; every case is
an index list into that pool, laid out so that the duo kernels' pairing of dispatch slots puts the chosen envs into one wave.  Which path a
wave takes is asserted on the reference's own row and sweep counts, and a pool that lacks the envs a case needs fails the case.
"""
import os

import numpy as np
import pytest

from oracle_lib import GOLDEN, HUMANOID_HBM

pytestmark = pytest.mark.gpu
ONE, DUO, DUO_Q = "hb_step_h27_kernel", "hb_step_duo_kernel", "hb_step_duo_q_kernel"
STEPS = 3
NCON_HALF = 12   # contacts per env while two envs share a wave (kNCh)
ROWS_HALF = 31   # rows per env of the paired sweeps
ROWS_DPP = 16    # rows per env of the broadcast forms: one DPP row of 16 lanes
CAP = 50         # the model's sweep limit (opt.iterations)


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


def place(pairs, pairing):
    """pool indices per dispatch slot such that `pairing` puts every (a, b) of `pairs` into one wave, a in the lower slot (lanes 0..31)"""
    n = 2 * len(pairs)
    p = pairing(n)
    assert (p >= 0).all(), (n, p)
    idx = np.full(n, -1)
    pairs = list(pairs)
    for e in range(n):
        if p[e] > e:
            assert p[p[e]] == e
            idx[e], idx[p[e]] = pairs.pop(0)
    assert (idx >= 0).all() and not pairs
    return idx


def reference(hbmod, m, gpu, state, tape, steps):
    """the one-env kernel's `steps` steps of the states: per step (state, ncon, nefc, niter, status)"""
    r = hbmod.Batch(m, len(state), gpu)
    r.tune(duo=0)
    r.set_state(hbmod.STATE_INTEGRATION, state)
    out = []
    for t in range(steps):
        r.step(tape[t])
        assert r.last_kernel().startswith(ONE[:-7])
        ncon, nefc, niter = r.counts()
        out.append((r.get_state(hbmod.STATE_INTEGRATION), ncon, nefc, niter, r.status()))
    r.close()
    return out


@pytest.fixture(scope="module")
def pool(hbmod, humanoid_model, gpu):
    """(state [N, 1 + nq + 2 nv] float32, control tape [STEPS, N, nu]): golden states | collapsed regime | settled regime | fresh resets in the air"""
    m = humanoid_model
    g = np.load(os.path.join(GOLDEN, "humanoid27_steps.npz"))
    gstate = np.concatenate([g["time"][:, None], g["qpos"], g["qvel"], g["warm"]], axis=1).astype(np.float32)
    gctrl = g["ctrl"].astype(np.float32)
    rng = np.random.default_rng(11)
    n = 2048
    b = hbmod.Batch(m, n, gpu)
    b.reset(perturb=True)
    b.rollout_halton(150)
    cctrl = np.sign(rng.uniform(-1, 1, size=(n, m.nu))).astype(np.float32)  # saturated actuators: limbs driven into the floor
    for _ in range(60):
        b.step(cctrl)
    cstate = b.get_state(hbmod.STATE_INTEGRATION)
    b.close()
    b = hbmod.Batch(m, n, gpu)  # the benchmark's regime: fallen and settled under its control sequence
    b.reset(perturb=True)
    b.rollout_halton(600)
    sstate = b.get_state(hbmod.STATE_INTEGRATION)
    b.close()
    sctrl = rng.uniform(-1, 1, size=(n, m.nu)).astype(np.float32)
    a = hbmod.Batch(m, 64, gpu)
    a.reset(perturb=True)
    astate = a.get_state(hbmod.STATE_INTEGRATION)
    a.close()
    astate[:, 1 + 2] += 1.0  # one metre up: no contact
    actrl = np.zeros((64, m.nu), np.float32)
    state = np.ascontiguousarray(np.concatenate([gstate, cstate, sstate, astate]), dtype=np.float32)
    ctrl = np.concatenate([gctrl, cctrl, sctrl, actrl])
    tape = np.stack([np.roll(ctrl, 7 * t, axis=0) for t in range(STEPS)])
    tape[:, -64:] = 0.0  # (the envs in the air stay limp: no joint runs into its limit)
    return state, np.ascontiguousarray(tape)


@pytest.fixture(scope="module")
def ref(hbmod, humanoid_model, gpu, pool):
    state, tape = pool
    out = reference(hbmod, humanoid_model, gpu, state, tape, STEPS)
    ncon, nefc, niter = out[0][1], out[0][2], out[0][3]
    lt = (ncon <= NCON_HALF) & (nefc <= ROWS_HALF) & (out[0][4] == 0)
    print("\npool of %d envs, first step: rows 0..%d, %d envs that pair; of those %d at most 16 rows, %d / %d / %d / %d with 1 / 15 / 16 / 17 rows, "
          "%d at the sweep cap, %d with one sweep" % (len(state), nefc.max(), lt.sum(), (lt & (nefc <= 16)).sum(), (lt & (nefc == 1)).sum(),
                                                     (lt & (nefc == 15)).sum(), (lt & (nefc == 16)).sum(), (lt & (nefc == 17)).sum(),
                                                     (lt & (niter == CAP)).sum(), (lt & (niter == 1)).sum()))
    return out


def same_bytes(b, hbmod, want, idx, what):
    """state, counts [0..2] and status of batch b against the reference's of the pool envs idx, byte for byte"""
    ws, wncon, wnefc, wniter, wstatus = want
    got = b.get_state(hbmod.STATE_INTEGRATION)
    assert got.dtype == np.float32 and ws.dtype == np.float32
    bad = np.flatnonzero((got.view(np.uint32) != ws[idx].view(np.uint32)).any(axis=1))
    assert bad.size == 0, (what, "state of slots", bad[:8], "rows", wnefc[idx][bad[:8]], "sweeps", wniter[idx][bad[:8]])
    for name, x, y in zip(("ncon", "nefc", "niter"), b.counts(), (wncon, wnefc, wniter)):
        assert np.array_equal(x, y[idx]), (what, name, np.flatnonzero(x != y[idx])[:8])
    assert np.array_equal(b.status(), wstatus[idx]), (what, "status")


def step_duo(hbmod, m, gpu, pool, ref, pairs, what=""):
    """one step through hb_step_duo_kernel"""
    state, tape = pool
    idx = place(pairs, partners)
    assert 16 <= len(idx) <= 64  # at least 8 waves
    b = hbmod.Batch(m, len(idx), gpu)
    b.tune(duo=2, schedule=0)  # (no heavy-first order: the pairing is that of the dispatch slots)
    b.set_state(hbmod.STATE_INTEGRATION, state[idx])
    b.step(tape[0][idx])
    assert b.last_kernel() == DUO
    same_bytes(b, hbmod, ref[0], idx, what + " [%s]" % DUO)
    b.close()


def roll_duo(hbmod, m, gpu, pool, ref, pairs, steps=2, what=""):
    """`steps` steps through hb_step_duo_q_kernel (the state stays on chip in between)"""
    state, tape = pool
    idx = place(pairs, partners_q)
    assert 16 <= len(idx) <= 64 and 2 <= steps <= STEPS
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


class Picker:
    """hands out pool envs that satisfy a mask, each at most once"""

    def __init__(self, seed=0):
        self.used = set()
        self.rng = np.random.default_rng(seed)

    def take(self, mask, what):
        cand = [e for e in self.rng.permutation(np.flatnonzero(mask)) if e not in self.used]
        assert cand, "the pool has no unused env for: " + what
        self.used.add(cand[0])
        return cand[0]

    def pair(self, mask, cond, what, tries=20000):
        """two unused envs (a, b) of the pool that satisfy the mask, with cond(a, b); a is for the lower slot"""
        ok = np.array([e for e in np.flatnonzero(mask) if e not in self.used])
        assert len(ok) >= 2, "the pool has no pair of envs for: " + what
        for ia, ib in self.rng.integers(len(ok), size=(tries, 2)):
            a, b = ok[ia], ok[ib]
            if a != b and cond(a, b):
                self.used.update((a, b))
                return a, b
        raise AssertionError("the pool has no pair of envs for: " + what)


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
    state, tape = pool
    nefc = ref[0][2]  # (the rows of a step do not depend on the sweeps of that step)
    ok = light(ref) & (nefc >= 1)
    pk = Picker(4)
    short, tall = ok & (nefc <= ROWS_DPP), ok & (nefc > ROWS_DPP)
    pairs = [(pk.take(short, "at most 16 rows"), pk.take(short, "at most 16 rows")) for _ in range(8)]
    pairs += [(pk.take(ok & (nefc == 16), "16 rows"), pk.take(ok & (nefc == 17), "17 rows")), (pk.take(ok & (nefc == 17), "17 rows"), pk.take(ok & (nefc == 16), "16 rows"))]
    pairs += [(pk.take(short, "at most 16 rows"), pk.take(tall, "above 16 rows")) for _ in range(3)] + [(pk.take(tall, "above 16 rows"), pk.take(short, "at most 16 rows")) for _ in range(3)]
    m = hbmod.Model.load(HUMANOID_HBM)
    m.set_opt(iterations=limit)
    sel = np.array(sorted(e for p in pairs for e in p))
    where = {e: k for k, e in enumerate(sel)}
    sub = (np.ascontiguousarray(state[sel]), np.ascontiguousarray(tape[:, sel]))
    want = reference(hbmod, m, gpu, sub[0], sub[1], 2)
    assert np.array_equal(want[0][2], nefc[sel]) and want[0][3].max() == limit and want[1][3].max() == limit
    local = [(where[a], where[b]) for a, b in pairs]
    step_duo(hbmod, m, gpu, sub, want, local, what="iterations=%d" % limit)
    roll_duo(hbmod, m, gpu, sub, want, local, steps=2, what="iterations=%d" % limit)


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
    state, tape = pool
    nefc = ref[0][2]
    ok = light(ref) & (nefc >= 1)
    pk = Picker(6)
    short, tall = ok & (nefc <= ROWS_DPP), ok & (nefc > ROWS_DPP)
    pairs = [(pk.take(short, "at most 16 rows"), pk.take(short, "at most 16 rows")) for _ in range(16)]
    pairs += [(pk.take(short, "at most 16 rows"), pk.take(tall, "above 16 rows")) for _ in range(8)] + [(pk.take(tall, "above 16 rows"), pk.take(short, "at most 16 rows")) for _ in range(8)]
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
