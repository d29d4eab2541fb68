"""The Gauss-Seidel sweeps of a wave's two envs (csrc/hb_step_duo.hip): the paired row step while both envs sweep, the one-env row step once
one of them has stopped, and the sums of the convergence test, on pairs whose sweep paths are known.

The 128 golden states of the fp64 oracle (0-24 rows, 0-50 sweeps, every residue mod 4) are stepped as four seeded permutations, i.e. four
different pairings, by hb_step_duo_kernel and hb_step_duo_q_kernel, and held bit-identical (state, counts, status) to the full one-env
kernel.  Which sweep paths the pairs took is asserted on the reference kernel's own row and sweep counts, so that the comparison cannot pass
without the loops it is about.  Rows above 31, too many contacts and a bad qacc are tests/test_gpu_duo.py's.
"""
import os

import numpy as np
import pytest

from duo_lib import DUO, DUO_Q, partners, reference_step
from oracle_lib import GOLDEN, HUMANOID_HBM

pytestmark = pytest.mark.gpu
SEEDS = (0, 1, 2, 3)


def _duo_step(hbmod, m, gpu, state, ctrl):
    b = hbmod.Batch(m, len(state), gpu)
    b.duo(2)
    b.set_state(hbmod.STATE_INTEGRATION, state)
    b.step(ctrl)
    assert b.last_kernel() == DUO
    out = b.get_state(hbmod.STATE_INTEGRATION), b.counts(), b.status()
    b.close()
    return out


def _same(got, want, what):
    (gs, gc, gst), (ws, wc, wst) = got, want
    bad = np.flatnonzero((gs != ws).any(axis=1))
    assert bad.size == 0, (what, "state", bad[:8], wc[1][bad[:8]], wc[2][bad[:8]])
    for name, x, y in zip(("ncon", "nefc", "niter"), gc, wc):
        assert np.array_equal(x, y), (what, name, np.flatnonzero(x != y)[:8])
    assert np.array_equal(gst, wst), (what, "status")


@pytest.fixture(scope="module")
def batches():
    """the golden states in four seeded orders: (state, ctrl) per seed"""
    g = np.load(os.path.join(GOLDEN, "humanoid27_steps.npz"))
    state = np.concatenate([g["time"][:, None], g["qpos"], g["qvel"], g["warm"]], axis=1)
    ctrl = g["ctrl"].astype(np.float32)
    assert len(state) == 128
    out = []
    for s in SEEDS:
        p = np.random.default_rng(s).permutation(128)
        out.append((state[p], ctrl[p]))
    return out


@pytest.fixture(scope="module")
def references(hbmod, humanoid_model, gpu, batches):
    """the one-env kernel's step of every batch, computed once: (state, (ncon, nefc, niter), status) per seed"""
    return [reference_step(hbmod, humanoid_model, gpu, st, ct) for st, ct in batches]


def test_pairs_cover_every_sweep_path(references):
    """the four pairings hold enough waves of every kind (counted on the reference kernel's rows and sweeps; a case is a wave)"""
    p = partners(128)
    assert (p >= 0).all() and (p[p] == np.arange(128)).all()
    lower = np.flatnonzero(np.arange(128) < p)  # one entry per wave: its lower-slot env
    cases = {}

    def add(name, mask):
        cases[name] = cases.get(name, 0) + int(mask.sum())
    for _, (_, nefc, niter), _ in references:
        rA, rB, sA, sB = nefc[lower], nefc[p[lower]], niter[lower], niter[p[lower]]
        add("lower-slot env sweeps longer, partner sweeps at least once", (sA > sB) & (sB >= 1))
        add("upper-slot env sweeps longer, partner sweeps at least once", (sB > sA) & (sA >= 1))
        add("both sweep equally often, more than 0", (sA == sB) & (sA > 0))
        add("an env without rows beside one that sweeps", ((rA == 0) & (sB > 0)) | ((rB == 0) & (sA > 0)))
        add("an env at the iteration cap beside one that stops before 10", ((sA == 50) & (sB < 10)) | ((sB == 50) & (sA < 10)))
        add("an env stopping after a single sweep", (sA == 1) | (sB == 1))
        longer = np.where(sA >= sB, rA, rB)  # rows of the longer-sweeping env (equal sweeps: the lower slot's)
        for r in range(4):
            add("max(nA, nB) %% 4 == %d in a wave that sweeps" % r, ((sA > 0) | (sB > 0)) & (np.maximum(rA, rB) % 4 == r))
            add("rows of the longer-sweeping env %% 4 == %d" % r, (sA != sB) & (longer % 4 == r))
    print()
    for name, k in cases.items():
        print("%4d waves: %s" % (k, name))
    short = {name: k for name, k in cases.items() if k < 8}
    assert not short, short


def test_one_step_of_every_pairing_is_bit_identical(hbmod, humanoid_model, gpu, batches, references):
    for s, (st, ct), want in zip(SEEDS, batches, references):
        _same(_duo_step(hbmod, humanoid_model, gpu, st, ct), want, "seed %d" % s)


def test_two_steps_in_the_multi_step_kernel_are_bit_identical(hbmod, humanoid_model, gpu, batches, references):
    """a rollout of a recorded two-step control tape (hb_step_duo_q_kernel: the state stays on chip between the steps) against two single
    steps of the one-env kernel"""
    m = humanoid_model
    for s, (st, ct), (mid, _, _) in zip(SEEDS, batches, references):
        ct2 = np.ascontiguousarray(ct[::-1])  # the second step's controls: another env's
        want = reference_step(hbmod, m, gpu, mid, ct2)
        b = hbmod.Batch(m, len(st), gpu)
        b.duo(2)
        b.set_state(hbmod.STATE_INTEGRATION, st)
        b.rollout(np.stack([ct, ct2]))
        assert b.last_kernel() == DUO_Q
        got = b.get_state(hbmod.STATE_INTEGRATION), b.counts(), b.status()
        b.close()
        _same(got, want, "seed %d, second step" % s)


@pytest.mark.parametrize("iterations", [1, 2, 0])
def test_iteration_limits(hbmod, gpu, batches, iterations):
    """sweeps cut short by the model's limit: every env stops in the paired loop (1, 2), or never enters it and keeps its warm start (0)"""
    m = hbmod.Model.load(HUMANOID_HBM)
    m.set_opt(iterations=iterations)
    st, ct = batches[0]
    want = reference_step(hbmod, m, gpu, st, ct)
    nefc, niter = want[1][1], want[1][2]
    assert (niter <= iterations).all() and (niter[nefc > 0] == iterations).sum() >= (8 if iterations else 0)
    if iterations == 0:
        assert (niter == 0).all()
    _same(_duo_step(hbmod, m, gpu, st, ct), want, "iterations=%d" % iterations)
