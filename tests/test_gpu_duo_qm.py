"""The qM stage of the two-envs-per-wave kernels (csrc/hb_step_duo.hip): its eight rounds over the 243 entries of the sparse M are unrolled,
their table words are requested ahead of the crb sweep and the LDS rows of round r + 1 are read before the sum of round r.  Same arithmetic,
so the same bits: hb_step_duo_kernel and hb_step_duo_q_kernel are held byte for byte (time, qpos, qvel, qacc_warmstart, ncon / nefc /
sweeps, status) to hb_step_h27_kernel, the one-env kernel, on the waves whose qM rounds run differently: a full pair, a lone env (the
partial last round with one half idle), a pass restarted with one env at a time, a model without damping (H = M: no timestep term), and
a step that runs mj_forward twice (a bad qacc).

hb_get_qacc is a read-out of the FULL kernels (a launch that asks for it takes hb_step_kernel: tests/test_gpu_duo.py), so the lean kernels
held here cannot report it.  What they keep of the solver's qacc is the warm start of the state record (mj_step: qacc_warmstart = qacc), and
that is held twice: to the one-env lean kernel's, and to what hb_get_qacc reports for the same step through hb_step_kernel.

Method and helpers: tests/duo_lib.py.  Every case is at most eight envs and three steps of a small pool of its own, whose reference is computed
once per model.
"""
import numpy as np
import pytest

import duo_lib
from duo_lib import BADQACC, DUO, NCON_HALF, ROWS_HALF, STEPS, partners, partners_q, place, roll_duo, step_duo
from oracle_lib import HUMANOID_HBM

pytestmark = pytest.mark.gpu
NGOLD, NFLAT, NBAD = 32, 16, 3


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
    gstate, gctrl = (x[:NGOLD] for x in duo_lib.golden_states())
    lstate, lctrl = duo_lib.flat(hbmod, m, gpu, NFLAT)
    bad = np.concatenate([gstate[:2], lstate[:1]])  # NBAD candidates
    bad[0, 1 + m.nq + 4] = 3e9              # an angular velocity of the root
    bad[1, 1 + m.nq:1 + m.nq + m.nv] = 2e9  # every velocity
    bad[2, 1 + m.nq + 2] = 3e9              # a linear velocity, in contact
    state = np.ascontiguousarray(np.concatenate([gstate, lstate, bad]), dtype=np.float32)
    return state, duo_lib.make_tape(np.concatenate([gctrl, lctrl, gctrl[:2], lctrl[:1]]), 5, limp_last=0)


@pytest.fixture(scope="module")
def ref(hbmod, models, gpu, pool):
    """per model, the one-env kernel's STEPS steps of the pool: per step (state, ncon, nefc, niter, status)"""
    out = {name: duo_lib.reference(hbmod, m, gpu, *pool, STEPS) for name, m in models.items()}
    a, b = out["humanoid"][0][0], out["undamped"][0][0]
    assert (a[:NGOLD] != b[:NGOLD]).any(axis=1).all()  # the damping is in every env's step: the two references differ
    return out


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
    step_duo(hbmod, models[model], gpu, pool, want, pairs, steps=1, what="a pair, " + model)
    step_duo(hbmod, models[model], gpu, pool, want, pairs, steps=3, what="a pair, " + model)
    roll_duo(hbmod, models[model], gpu, pool, want, pairs, steps=2, what="a pair, " + model)
    roll_duo(hbmod, models[model], gpu, pool, want, pairs, steps=3, what="a pair, " + model)


@pytest.mark.parametrize("model", ["humanoid", "undamped"])
def test_a_lone_env(hbmod, models, gpu, pool, ref, model):
    """three envs: the last wave holds one env, so its pass runs with the upper half idle (the partial last round included)"""
    want = ref[model]
    e = calm(want)
    assert len(e) >= 3 and (partners(3) < 0).sum() == 1 and (partners_q(3) < 0).sum() == 1
    step_duo(hbmod, models[model], gpu, pool, want, [(e[0], e[1])], [e[2]], steps=3, what="a lone env, " + model)
    roll_duo(hbmod, models[model], gpu, pool, want, [(e[0], e[1])], [e[2]], steps=3, what="a lone env, " + model)


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
    step_duo(hbmod, models[model], gpu, pool, want, pairs, steps=1, what="a serial restart, " + model)
    roll_duo(hbmod, models[model], gpu, pool, want, pairs, steps=2, what="a serial restart, " + model)


def test_a_bad_qacc(hbmod, models, gpu, pool, ref):
    """an env whose step runs mj_forward a second time (tests/test_gpu_duo.py's recipe: a velocity that overflows the accelerations), in
    either half beside a calm env: the qM rounds run again on the reset state"""
    want = ref["humanoid"]
    status = want[0][4][NGOLD + NFLAT:NGOLD + NFLAT + NBAD]
    bad = NGOLD + NFLAT + np.flatnonzero(((status & BADQACC) != 0) & ((status & 0x30) == 0))  # (not reset by mj_checkPos / mj_checkVel before)
    assert len(bad) >= 1, status
    e = calm(want)
    pairs = [(bad[0], e[0]), (e[1], bad[-1])]
    step_duo(hbmod, models["humanoid"], gpu, pool, want, pairs, steps=1, what="a bad qacc")
    roll_duo(hbmod, models["humanoid"], gpu, pool, want, pairs, steps=2, what="a bad qacc")


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
