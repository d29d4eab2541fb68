"""The qM stage of the two-envs-per-wave kernels (csrc/hb_step_duo.hip): its eight rounds over the 243 entries of the sparse M are unrolled,
their table words are requested ahead of the crb sweep and the LDS rows of round r + 1 are read before the sum of round r.  Same arithmetic,
so the same bits: hb_step_duo_kernel and hb_step_duo_q_kernel are held byte for byte (time, qpos, qvel, qacc_warmstart, ncon / nefc /
sweeps, status) to hb_step_h27_kernel, the one-env kernel, on the waves whose qM rounds run differently: a full pair, a lone env (the
partial last round with one half idle), a pass restarted with one env at a time, a model without damping (H = M: no timestep term), and
a step that runs mj_forward twice (a bad qacc).

hb_get_qacc is a read-out of the FULL kernels (a launch that asks for it takes hb_step_kernel: tests/test_gpu_duo.py), so the lean kernels
held here cannot report it.  What they keep of the solver's qacc is the warm start of the state record (mj_step: qacc_warmstart = qacc), and
that is held twice: to the one-env lean kernel's, and to what hb_get_qacc reports for the same step through hb_step_kernel.

Every case is at most eight envs and three steps; the one-env kernel's result for an env does not depend on the batch around it, so it is
computed once per model for a small pool of states and every case is an index list into that pool (tests/test_gpu_duo_once.py's layout
helpers put the chosen envs into one wave).
"""
import os

import numpy as np
import pytest

from oracle_lib import GOLDEN, HUMANOID_HBM
from test_gpu_duo_once import DUO, DUO_Q, NCON_HALF, ONE, ROWS_HALF, partners, partners_q, place, same_bytes

pytestmark = pytest.mark.gpu
STEPS = 3
NGOLD, NFLAT, NBAD = 32, 16, 3
BADQACC = 1 << 6


def zero_damping_hbm(dst):
    """a copy of the humanoid's .hbm with every dof_damping at 0 (tests/kernel_models.py: perturbed_hbm's way into the text records)"""
    lines = open(HUMANOID_HBM).read().splitlines()
    at = [i for i, ln in enumerate(lines) if ln[:2] in ("D ", "d ") and ln.split()[1] == "dof_damping"]
    assert len(at) == 1, at
    tok = lines[at[0]].split()
    assert len(tok) == 3 + 27 and any(float(x) > 0 for x in tok[3:])
    lines[at[0]] = " ".join(tok[:3] + ["0"] * 27)
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")
    return dst


@pytest.fixture(scope="module")
def models(hbmod, humanoid_model, tmp_path_factory):
    undamped = hbmod.Model.load(zero_damping_hbm(str(tmp_path_factory.mktemp("qm") / "humanoid27_undamped.hbm")))
    assert not undamped.array("dof_damping").any() and humanoid_model.array("dof_damping").any()
    return {"humanoid": humanoid_model, "undamped": undamped}


@pytest.fixture(scope="module")
def pool(hbmod, humanoid_model, gpu):
    """(state [N, 1 + nq + 2 nv] float32, control tape [STEPS, N, nu]): NGOLD golden states of the fp64 oracle | NFLAT bodies laid flat into
    the floor (tests/test_gpu_duo_once.py: more than 12 contacts) | NBAD of these states with velocities that overflow the accelerations
    (tests/test_gpu_duo.py: BADQACC)"""
    m = humanoid_model
    g = np.load(os.path.join(GOLDEN, "humanoid27_steps.npz"))
    gstate = np.concatenate([g["time"][:, None], g["qpos"], g["qvel"], g["warm"]], axis=1).astype(np.float32)[:NGOLD]
    gctrl = g["ctrl"].astype(np.float32)[:NGOLD]
    a = hbmod.Batch(m, NFLAT, gpu)
    a.reset(perturb=True)
    lstate = a.get_state(hbmod.STATE_INTEGRATION)
    a.close()
    lstate[:, 1 + m.nq:] = 0.0
    r = np.sqrt(0.5)
    for k in range(NFLAT):
        lstate[k, 1 + 2] = 0.03 + 0.012 * (k % 8)
        lstate[k, 1 + 3:1 + 7] = ((r, 0, -r, 0), (r, 0, r, 0), (0.5, 0.5, -0.5, 0.5), (0.5, -0.5, -0.5, -0.5))[(k // 8) % 4]
    lstate[:, 1 + 7:1 + m.nq] = np.random.default_rng(5).uniform(-0.1, 0.1, size=(NFLAT, m.nq - 7))
    bad = np.concatenate([gstate[:2], lstate[:1]])  # NBAD candidates
    bad[0, 1 + m.nq + 4] = 3e9              # an angular velocity of the root
    bad[1, 1 + m.nq:1 + m.nq + m.nv] = 2e9  # every velocity
    bad[2, 1 + m.nq + 2] = 3e9              # a linear velocity, in contact
    state = np.ascontiguousarray(np.concatenate([gstate, lstate, bad]), dtype=np.float32)
    ctrl = np.concatenate([gctrl, np.zeros((NFLAT, m.nu), np.float32), gctrl[:2], np.zeros((1, m.nu), np.float32)])
    tape = np.stack([np.roll(ctrl, 5 * t, axis=0) for t in range(STEPS)])
    return state, np.ascontiguousarray(tape)


@pytest.fixture(scope="module")
def ref(hbmod, models, gpu, pool):
    """per model, the one-env kernel's STEPS steps of the pool: per step (state, ncon, nefc, niter, status)"""
    state, tape = pool
    out = {}
    for name, m in models.items():
        r = hbmod.Batch(m, len(state), gpu)
        r.tune(duo=0)
        r.set_state(hbmod.STATE_INTEGRATION, state)
        steps = []
        for t in range(STEPS):
            r.step(tape[t])
            assert r.last_kernel() == ONE
            ncon, nefc, niter = r.counts()
            steps.append((r.get_state(hbmod.STATE_INTEGRATION), ncon, nefc, niter, r.status()))
        r.close()
        out[name] = steps
    a, b = out["humanoid"][0][0], out["undamped"][0][0]
    assert (a[:NGOLD] != b[:NGOLD]).any(axis=1).all()  # the damping is in every env's step: the two references differ
    return out


def run_steps(hbmod, m, gpu, pool, want, pairs, singles=(), steps=1, what=""):
    """`steps` launches of hb_step_duo_kernel, held after every one"""
    state, tape = pool
    idx = place(pairs, singles, partners)
    b = hbmod.Batch(m, len(idx), gpu)
    b.tune(duo=2, schedule=0)  # (no heavy-first order: the pairing is that of the dispatch slots)
    b.set_state(hbmod.STATE_INTEGRATION, state[idx])
    for t in range(steps):
        b.step(tape[t][idx])
        assert b.last_kernel() == DUO
        same_bytes(b, hbmod, want[t], idx, what + " [%s, step %d]" % (DUO, t))
    b.close()


def run_roll(hbmod, m, gpu, pool, want, pairs, singles=(), steps=STEPS, what=""):
    """`steps` steps in one launch of hb_step_duo_q_kernel (the state stays on chip in between: the rounds run again on it)"""
    state, tape = pool
    idx = place(pairs, singles, partners_q)
    b = hbmod.Batch(m, len(idx), gpu)
    b.tune(duo=2, schedule=0)
    b.set_state(hbmod.STATE_INTEGRATION, state[idx])
    b.rollout(np.ascontiguousarray(tape[:steps, idx]))
    assert b.last_kernel() == DUO_Q
    same_bytes(b, hbmod, want[steps - 1], idx, what + " [%s, %d steps]" % (DUO_Q, steps))
    b.close()


def calm(want):
    """golden envs that share a wave in the paired layout in every step, with rows, without a warning"""
    ok = np.ones(NGOLD, bool)
    for s in want:
        ok &= (s[1][:NGOLD] <= NCON_HALF) & (s[2][:NGOLD] <= ROWS_HALF) & (s[2][:NGOLD] >= 1) & (s[4][:NGOLD] == 0)
    return np.flatnonzero(ok)


@pytest.mark.parametrize("model", ["humanoid", "undamped"])
def test_a_pair(hbmod, models, gpu, pool, ref, model):
    """two golden envs in one wave: one step and three (hb_step_duo_kernel launch by launch, hb_step_duo_q_kernel in one launch).  On the
    model without damping eulerdamp is false: diag(H) is the diagonal of M, held through everything the solve makes of it"""
    want = ref[model]
    e = calm(want)
    assert len(e) >= 2, len(e)
    pairs = [(e[0], e[1])]
    run_steps(hbmod, models[model], gpu, pool, want, pairs, steps=1, what="a pair, " + model)
    run_steps(hbmod, models[model], gpu, pool, want, pairs, steps=3, what="a pair, " + model)
    run_roll(hbmod, models[model], gpu, pool, want, pairs, steps=2, what="a pair, " + model)
    run_roll(hbmod, models[model], gpu, pool, want, pairs, steps=3, what="a pair, " + model)


@pytest.mark.parametrize("model", ["humanoid", "undamped"])
def test_a_lone_env(hbmod, models, gpu, pool, ref, model):
    """three envs: the last wave holds one env, so its pass runs with the upper half idle (the partial last round included)"""
    want = ref[model]
    e = calm(want)
    assert len(e) >= 3 and (partners(3) < 0).sum() == 1 and (partners_q(3) < 0).sum() == 1
    run_steps(hbmod, models[model], gpu, pool, want, [(e[0], e[1])], [e[2]], steps=3, what="a lone env, " + model)
    run_roll(hbmod, models[model], gpu, pool, want, [(e[0], e[1])], [e[2]], steps=3, what="a lone env, " + model)


@pytest.mark.parametrize("model", ["humanoid", "undamped"])
def test_a_serial_restart(hbmod, models, gpu, pool, ref, model):
    """an env above 12 contacts beside a light one, in the lower and in the upper half: the pass restarts one env at a time, and qM runs
    once per env with the other half masked"""
    want = ref[model]
    ncon = want[0][1]
    many = NGOLD + np.flatnonzero(ncon[NGOLD:NGOLD + NFLAT] > NCON_HALF)
    e = calm(want)
    assert len(many) >= 2 and len(e) >= 2, (len(many), len(e), ncon[NGOLD:NGOLD + NFLAT])
    pairs = [(many[0], e[0]), (e[1], many[1])]
    assert all(max(ncon[a], ncon[b]) > NCON_HALF and min(ncon[a], ncon[b]) <= NCON_HALF for a, b in pairs)
    run_steps(hbmod, models[model], gpu, pool, want, pairs, steps=1, what="a serial restart, " + model)
    run_roll(hbmod, models[model], gpu, pool, want, pairs, steps=2, what="a serial restart, " + model)


def test_a_bad_qacc(hbmod, models, gpu, pool, ref):
    """an env whose step runs mj_forward a second time (tests/test_gpu_duo.py's recipe: a velocity that overflows the accelerations), in
    either half beside a calm env: the qM rounds run again on the reset state"""
    want = ref["humanoid"]
    status = want[0][4][NGOLD + NFLAT:NGOLD + NFLAT + NBAD]
    bad = NGOLD + NFLAT + np.flatnonzero(((status & BADQACC) != 0) & ((status & 0x30) == 0))  # (not reset by mj_checkPos / mj_checkVel before)
    assert len(bad) >= 1, status
    e = calm(want)
    pairs = [(bad[0], e[0]), (e[1], bad[-1])]
    run_steps(hbmod, models["humanoid"], gpu, pool, want, pairs, steps=1, what="a bad qacc")
    run_roll(hbmod, models["humanoid"], gpu, pool, want, pairs, steps=2, what="a bad qacc")


def test_the_warm_start_is_the_full_kernels_qacc(hbmod, humanoid_model, gpu, pool, ref):
    """hb_get_qacc of the same step through hb_step_kernel (the read-out takes the full kernel) against the warm start the duo kernel leaves"""
    state, tape = pool
    m = humanoid_model
    e = calm(ref["humanoid"])
    idx = place([(e[0], e[1])], [e[2]], partners)
    f = hbmod.Batch(m, len(idx), gpu)
    f.diag_enable(True)
    f.set_state(hbmod.STATE_INTEGRATION, state[idx])
    f.step(tape[0][idx])
    assert f.last_kernel() == "hb_step_kernel"
    qacc = f.qacc()
    f.close()
    b = hbmod.Batch(m, len(idx), gpu)
    b.tune(duo=2, schedule=0)
    b.set_state(hbmod.STATE_INTEGRATION, state[idx])
    b.step(tape[0][idx])
    assert b.last_kernel() == DUO
    warm = b.get_state(hbmod.STATE_INTEGRATION)[:, 1 + m.nq + m.nv:]
    b.close()
    assert qacc.dtype == warm.dtype == np.float32 and np.abs(qacc).max() > 0
    assert np.array_equal(qacc.view(np.uint32), warm.view(np.uint32))
