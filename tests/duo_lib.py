"""Helpers of tests/test_gpu_duo*.py, the tests of the two-envs-per-wave kernels (csrc/hb_step_duo.hip).  Not collected, no fixtures.

hb_step_duo_kernel (one step per launch) and hb_step_duo_q_kernel (several steps, the state on chip in between) are held byte for byte (time,
qpos, qvel, warm start, ncon / nefc / sweeps, status) to hb_step_h27_kernel, the one-env kernel, on waves put together for the path they are to
take.  The one-env kernel's result for an env does not depend on the batch around it, so it is computed ONCE for a pool of states over STEPS
steps (`reference`), and every case is an index list into that pool of at most 64 envs, laid out (`place`) so that the duo kernels' pairing of
dispatch slots (`partners`, `partners_q`) puts the chosen envs into one wave, and run by `step_duo` / `roll_duo`.  Which path a wave takes is
asserted by the test on the reference's own contact, row and sweep counts, and a pool that lacks the envs a case needs fails the case.

`reference` prints a digest of its pool and of every step's result, the drivers one of the index list they laid out (16 hex digits of the
SHA-256, shown under -s): a change to these helpers, or to a kernel, that leaves the listing as it was runs the same waves on the same bits.
"""
import fnmatch
import functools
import hashlib
import os

import numpy as np

from oracle_lib import GOLDEN, HUMANOID_HBM

ONE, DUO, DUO_Q = "hb_step_h27_kernel", "hb_step_duo_kernel", "hb_step_duo_q_kernel"
ONE_ANY = "hb_step_h27*"  # (for `reference`: any kernel of the one-env family)
STEPS = 3
NCON_HALF = 12   # contacts per env while two envs share a wave (kNCh)
ROWS_HALF = 31   # rows per env of the paired sweeps
ROWS_DPP = 16    # rows per env of the broadcast forms: one DPP row of 16 lanes
CAP = 50         # the model's sweep limit (opt.iterations)
BADQACC = 1 << 6


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


# ---- layout ----

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


def place(pairs, singles=(), pairing=partners):
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


# ---- the one-env kernels' results ----

def reference(hbmod, m, gpu, state, tape, steps, kernel=ONE):
    """the one-env kernel's `steps` steps of the states: per step (state, ncon, nefc, niter, status).  Every launch must be `kernel`'s: a name, or
    a pattern such as ONE_ANY"""
    r = hbmod.Batch(m, len(state), gpu)
    r.tune(duo=0)
    r.set_state(hbmod.STATE_INTEGRATION, state)
    out = []
    for t in range(steps):
        r.step(tape[t])
        assert fnmatch.fnmatchcase(r.last_kernel(), kernel), (r.last_kernel(), kernel)
        ncon, nefc, niter = r.counts()
        out.append((r.get_state(hbmod.STATE_INTEGRATION), ncon, nefc, niter, r.status()))
    r.close()
    print("\nreference: pool %s, steps %s" % (digest(state, tape), " ".join(digest(*s) for s in out)))
    return out


def reference_step(hbmod, m, gpu, state, ctrl):
    """one step through the full one-env kernel (a launch that asks for the diagnostics takes hb_step_kernel): (state, (ncon, nefc, niter), status)"""
    r = hbmod.Batch(m, len(state), gpu)
    r.diag_enable(True)
    r.set_state(hbmod.STATE_INTEGRATION, state)
    r.step(ctrl)
    assert r.last_kernel() == "hb_step_kernel"
    out = r.get_state(hbmod.STATE_INTEGRATION), r.counts(), r.status()
    r.close()
    return out


def light(ref, t=0):
    """envs that share a wave in the paired layout at step t: at most 12 contacts and 31 rows, no warning"""
    return (ref[t][1] <= NCON_HALF) & (ref[t][2] <= ROWS_HALF) & (ref[t][4] == 0)


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


# ---- comparison and drivers ----

def same_bytes(b, hbmod, want, idx, what):
    """state, counts [0..2] and status of batch b against the reference's of the pool envs idx, byte for byte"""
    ws, wncon, wnefc, wniter, wstatus = want
    got = b.get_state(hbmod.STATE_INTEGRATION)
    assert got.dtype == np.float32 and ws.dtype == np.float32
    bad = np.flatnonzero((got.view(np.uint32) != ws[idx].view(np.uint32)).any(axis=1))[:8]
    assert bad.size == 0, (what, "state of slots", bad, "rows", wnefc[idx][bad], "contacts", wncon[idx][bad], "sweeps", wniter[idx][bad])
    for name, x, y in zip(("ncon", "nefc", "niter"), b.counts(), (wncon, wnefc, wniter)):
        assert np.array_equal(x, y[idx]), (what, name, np.flatnonzero(x != y[idx])[:8])
    assert np.array_equal(b.status(), wstatus[idx]), (what, "status")


def _laid_out(hbmod, m, gpu, state, pairs, singles, pairing, min_envs, what):
    """(index list, batch holding those pool states) of a case; min_envs=16 asks for at least 8 waves"""
    idx = place(pairs, singles, pairing)
    assert min_envs <= len(idx) <= 64, len(idx)
    print("idx %s %s" % (digest(idx), what))
    b = hbmod.Batch(m, len(idx), gpu)
    b.tune(duo=2, schedule=0)  # (no heavy-first order: the pairing is that of the dispatch slots)
    b.set_state(hbmod.STATE_INTEGRATION, state[idx])
    return idx, b


def step_duo(hbmod, m, gpu, pool, ref, pairs, singles=(), steps=1, min_envs=0, what=""):
    """`steps` launches of hb_step_duo_kernel, held after every one"""
    assert 1 <= steps <= STEPS
    idx, b = _laid_out(hbmod, m, gpu, pool[0], pairs, singles, partners, min_envs, what + " [%s x %d]" % (DUO, steps))
    for t in range(steps):
        b.step(pool[1][t][idx])
        assert b.last_kernel() == DUO
        same_bytes(b, hbmod, ref[t], idx, what + " [%s, step %d]" % (DUO, t))
    b.close()


def roll_duo(hbmod, m, gpu, pool, ref, pairs, singles=(), steps=2, min_envs=0, what=""):
    """`steps` steps in one launch of hb_step_duo_q_kernel (the state stays on chip in between)"""
    assert 2 <= steps <= STEPS
    what += " [%s, %d steps]" % (DUO_Q, steps)
    idx, b = _laid_out(hbmod, m, gpu, pool[0], pairs, singles, partners_q, min_envs, what)
    b.rollout(np.ascontiguousarray(pool[1][:steps, idx]))
    assert b.last_kernel() == DUO_Q
    same_bytes(b, hbmod, ref[steps - 1], idx, what)
    b.close()


def both_kernels(hbmod, m, gpu, pool, ref, pairs, singles=(), steps=2, min_envs=0, what=""):
    """one step through hb_step_duo_kernel, and `steps` steps (a count, or several counts) through hb_step_duo_q_kernel"""
    step_duo(hbmod, m, gpu, pool, ref, pairs, singles, min_envs=min_envs, what=what)
    for k in np.atleast_1d(steps):
        roll_duo(hbmod, m, gpu, pool, ref, pairs, singles, steps=int(k), min_envs=min_envs, what=what)


# ---- pool segments: (states [n, 1 + nq + 2 nv], controls [n, nu]) ----

def golden_states():
    """the 128 golden states of the fp64 oracle and their controls"""
    g = np.load(os.path.join(GOLDEN, "humanoid27_steps.npz"))
    return np.concatenate([g["time"][:, None], g["qpos"], g["qvel"], g["warm"]], axis=1).astype(np.float32), g["ctrl"].astype(np.float32)


def collapsed(hbmod, m, gpu, n, steps, rng):
    """the collapsed regime of profiles/r01_soak_1e10.txt: n envs fallen under the Halton control sequence, then `steps` steps with saturated
    actuators (limbs driven into the floor, joints into their limits) - many contacts and limit rows at once"""
    b = hbmod.Batch(m, n, gpu)
    b.reset(perturb=True)
    b.rollout_halton(150)
    ctrl = np.sign(rng.uniform(-1, 1, size=(n, m.nu))).astype(np.float32)
    for _ in range(steps):
        b.step(ctrl)
    state = b.get_state(hbmod.STATE_INTEGRATION)
    b.close()
    return state, ctrl


def settled(hbmod, m, gpu, n, rng):
    """the benchmark's regime: fallen and settled under its control sequence"""
    b = hbmod.Batch(m, n, gpu)
    b.reset(perturb=True)
    b.rollout_halton(600)
    state = b.get_state(hbmod.STATE_INTEGRATION)
    b.close()
    return state, rng.uniform(-1, 1, size=(n, m.nu)).astype(np.float32)


def fresh(hbmod, m, gpu, n):
    b = hbmod.Batch(m, n, gpu)
    b.reset(perturb=True)
    state = b.get_state(hbmod.STATE_INTEGRATION)
    b.close()
    return state, np.zeros((n, m.nu), np.float32)


def flat(hbmod, m, gpu, n):
    """lying flat, pressed into the floor: on the back, the front and either side at eight heights, limbs a little bent - every capsule of
    the body against the plane, more contacts than the collapsed regime reaches"""
    state, ctrl = fresh(hbmod, m, gpu, n)
    state[:, 1 + m.nq:] = 0.0
    r = np.sqrt(0.5)
    for k in range(n):
        state[k, 1 + 2] = 0.03 + 0.012 * (k % 8)
        state[k, 1 + 3:1 + 7] = ((r, 0, -r, 0), (r, 0, r, 0), (0.5, 0.5, -0.5, 0.5), (0.5, -0.5, -0.5, -0.5))[(k // 8) % 4]
    state[:, 1 + 7:1 + m.nq] = np.random.default_rng(5).uniform(-0.1, 0.1, size=(n, m.nq - 7))
    return state, ctrl


def in_the_air(hbmod, m, gpu, n):
    """fresh resets one metre up: no contact"""
    state, ctrl = fresh(hbmod, m, gpu, n)
    state[:, 1 + 2] += 1.0
    return state, ctrl


def make_tape(ctrl, shift, limp_last=64):
    """control tape [STEPS, n, nu]: step t takes the controls of the env `shift` * t slots before; the last `limp_last` envs (those in the air)
    stay limp, so that no joint of theirs runs into its limit"""
    tape = np.stack([np.roll(ctrl, shift * t, axis=0) for t in range(STEPS)])
    if limp_last:
        tape[:, -limp_last:] = 0.0
    return np.ascontiguousarray(tape)


def _pool(segments):
    """(state, control tape) of the segments in their order, read-only: the pools are shared between test modules"""
    state = np.ascontiguousarray(np.concatenate([s for s, _ in segments]), dtype=np.float32)
    tape = make_tape(np.concatenate([c for _, c in segments]), 7)
    state.setflags(write=False)
    tape.setflags(write=False)
    return state, tape


@functools.lru_cache(maxsize=None)
def once_pool(hbmod, m, gpu):
    """golden states | collapsed regime | lying flat | fresh resets in the air"""
    return _pool([golden_states(), collapsed(hbmod, m, gpu, 1792, 60, np.random.default_rng(11)), flat(hbmod, m, gpu, 64), in_the_air(hbmod, m, gpu, 64)])


@functools.lru_cache(maxsize=None)
def bcast_pool(hbmod, m, gpu):
    """golden states | collapsed regime | settled regime | fresh resets in the air"""
    rng = np.random.default_rng(11)
    return _pool([golden_states(), collapsed(hbmod, m, gpu, 2048, 60, rng), settled(hbmod, m, gpu, 2048, rng), in_the_air(hbmod, m, gpu, 64)])


@functools.lru_cache(maxsize=None)
def wide_pool(hbmod, m, gpu):
    """bcast_pool's recipe with three more collapsed regimes (after 20, 40 and 90 steps) behind the settled one, for the rarer counts: 31 rows, rows
    that cross 31 between two steps"""
    rng = np.random.default_rng(11)
    return _pool([golden_states(), collapsed(hbmod, m, gpu, 2048, 60, rng), settled(hbmod, m, gpu, 2048, rng)]
                 + [collapsed(hbmod, m, gpu, 2048, steps, rng) for steps in (20, 40, 90)] + [in_the_air(hbmod, m, gpu, 64)])


@functools.lru_cache(maxsize=None)
def wide_reference(hbmod, m, gpu):
    """the reference of wide_pool, which two modules use; read-only"""
    out = reference(hbmod, m, gpu, *wide_pool(hbmod, m, gpu), STEPS, kernel=ONE_ANY)
    for a in (x for step in out for x in step):
        a.setflags(write=False)
    return out


# ---- cases that several modules have ----

def iteration_limit_case(hbmod, gpu, pool, ref, pairs, limit, min_envs=0, check=None):
    """the waves of `pairs` with opt.iterations = limit against the one-env kernel with the same limit.  check(want, local), if given, asserts the
    paths of these waves on that reference (want) of the selected envs, in which the pairs are `local`"""
    state, tape = pool
    m = hbmod.Model.load(HUMANOID_HBM)
    m.set_opt(iterations=limit)
    sel = np.array(sorted(e for p in pairs for e in p))
    where = {e: k for k, e in enumerate(sel)}
    sub = (np.ascontiguousarray(state[sel]), np.ascontiguousarray(tape[:, sel]))
    want = reference(hbmod, m, gpu, sub[0], sub[1], 2, kernel=ONE_ANY)
    assert np.array_equal(want[0][2], ref[0][2][sel]) and want[0][3].max() == limit and want[1][3].max() == limit
    local = [(where[a], where[b]) for a, b in pairs]
    if check:
        check(want, local)
    both_kernels(hbmod, m, gpu, sub, want, local, steps=2, min_envs=min_envs, what="iterations=%d" % limit)


def env_steps_both_ways(hbmod, m, gpu, acts, **kw):
    """the env adapter's steps of the actions [T, n, nu] with one env per wave (duo=0) and with two: (per run [first observation, then per step
    observation, reward, terminated, truncated], the two runs' last kernels)"""
    got, names = [], []
    for duo in (0, 2):
        env = hbmod.VecEnv(m, acts.shape[1], gpu, **kw)
        env.batch.tune(duo=duo)
        out = [env.reset().copy()]
        for a in acts:
            obs, rew, term, trunc, info = env.step_arrays(a)
            out += [obs.copy(), rew.copy(), term.copy(), trunc.copy()]
        names.append(env.batch.last_kernel())
        got.append(out)
        env.close()
    return got, names


def torque_readout_case(hbmod, m, gpu, pool, ref, pairs):
    """a launch that asks for the joint torques on the 32 waves of `pairs`: the torque array itself, and the observations, rewards and episode ends
    of the env step, equal the one-env kernel's byte for byte"""
    state, tape = pool
    idx = place(pairs)
    assert len(idx) == 64
    got, names = [], []
    for duo in (0, 2):
        env = hbmod.VecEnv(m, len(idx), gpu)
        env.batch.tune(duo=duo, schedule=0)
        env.reset()
        env.batch.set_state(hbmod.STATE_INTEGRATION, state[idx])
        obs, rew, term, trunc, info = env.step_arrays(tape[0][idx])
        got.append([env.batch.env_joint_torques(), obs.copy(), rew.copy(), term.copy(), trunc.copy()])
        names.append(env.batch.last_kernel())
        if duo == 0:
            assert np.array_equal(env.batch.counts()[1], ref[0][2][idx])  # the waves are the ones chosen
        env.close()
    assert names[0].startswith("hb_step_h27") and names[1] == DUO, names
    assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(got[0], got[1]))
    assert got[0][0].shape == (64, m.nv) and (np.abs(got[0][0]).max(axis=1) > 0).all()  # every env has torques to compare
    assert np.abs(got[0][2]).max() > 0  # the rewards are not all zero
