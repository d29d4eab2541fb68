"""GPU parity tests: the HIP path (through the C-ABI of libhb.so) against the fp64 oracle.

Tolerances (fp32 device arithmetic vs fp64 oracle, stated per SURVEY.md §8(c)/(d)):
  one step, teacher-forced from identical states
      qpos   : |d| <= 4e-5 * max(1, |qpos|)            (measured: median 7e-8, max 1.2e-5 on one stiff 6-limit-row impact state)
      qvel   : |d| <= 4e-4 * max(1, max|qvel|)         (measured: median 8e-7, max 1.35e-4; qvel' = qvel + h*qacc, |qacc| up to 4e3)
      qacc   : |d| <= 4e-4 * max(1, max|qacc|)         (measured: median 2e-6, max 1.30e-4)
      contact: dist/pos 1e-5; frame 1e-3 (a capsule-capsule normal is (p2-p1)/|p2-p1| of two nearly coincident
               closest points under deep penetration: ill-conditioned in fp32, measured max 2.3e-4, median 1e-7);
               counts (ncon, nefc) identical
      forces : |d| <= 4e-4 * max(1, max|efc_force|)   (measured: median 3e-6, max 1.26e-4; PGS sweep counts identical)
  (measurements: tools/gpu_parity_report.py on the 128 golden states, profiles/r01_parity_report.txt; every bound is at
  most 3x the measured maximum, so a 3x numerical regression fails.  History: the bounds were 1e-4 / 1e-3 / 2e-3 / 2e-3 in
  round 1, loosened from 1e-5 for qpos when the first hardware runs measured 1.1e-5 and 2.6e-5 on the impact state.)
  free-running, contact-free segment (through joint-limit rows as well): relative qpos drift <= 1e-4 (the north-star bar);
  free-running through contacts: chaotic, reported not asserted beyond sanity.
"""
import os

import numpy as np
import pytest

from bounds import FREE_RUNNING_BOUND
from oracle_lib import GOLDEN, HFIELD_HBM, HUMANOID_HBM, Oracle, halton, MODELS_DIR as MODELS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "humanoid27_steps.npz"))


def pack_state(g, idx):
    return np.concatenate([g["time"][idx, None], g["qpos"][idx], g["qvel"][idx], g["warm"][idx]], axis=1)


def test_one_step_parity_on_golden_states(hbmod, humanoid_model, gpu, golden):
    g = golden
    n = len(g["env"])
    b = hbmod.Batch(humanoid_model, n, gpu)
    b.diag_enable(True)
    b.set_state(hbmod.STATE_INTEGRATION, pack_state(g, np.arange(n)))
    b.step(g["ctrl"].astype(np.float32))
    q, v, a = b.qpos.astype(np.float64), b.qvel.astype(np.float64), b.qacc().astype(np.float64)
    ncon, nefc, niter = b.counts()
    assert not b.status().any()
    assert np.array_equal(ncon, g["ncon"]) and np.array_equal(nefc, g["nefc"])
    dq = np.abs(q - g["qpos1"]) / np.maximum(1.0, np.abs(g["qpos1"]))
    assert dq.max() <= 4e-5, dq.max()
    assert np.median(dq.max(axis=1)) <= 1e-6
    vs = np.maximum(1.0, np.abs(g["qvel1"]).max(axis=1, keepdims=True))
    assert (np.abs(v - g["qvel1"]) / vs).max() <= 4e-4
    as_ = np.maximum(1.0, np.abs(g["qacc"]).max(axis=1, keepdims=True))
    assert (np.abs(a - g["qacc"]) / as_).max() <= 4e-4
    # time advanced by one timestep
    assert np.allclose(b.time, g["time"] + 0.005, atol=1e-5)
    # contact geometry
    con = b.contacts().astype(np.float64)
    for k in range(n):
        nc = int(g["ncon"][k])
        assert np.abs(con[k, :nc, 0] - g["con_dist"][k, :nc]).max(initial=0) <= 1e-5
        assert np.abs(con[k, :nc, 1:4] - g["con_pos"][k, :nc]).max(initial=0) <= 1e-5
        assert np.abs(con[k, :nc, 4:13] - g["con_frame"][k, :nc]).max(initial=0) <= 1e-3
        assert np.array_equal(con[k, :nc, 14:16], g["con_geom"][k, :nc])
    # constraint forces
    f = b.efc_force().astype(np.float64)
    fs = np.maximum(1.0, np.abs(g["efc_force"]).max(axis=1, keepdims=True))
    assert (np.abs(f - g["efc_force"]) / fs).max() <= 4e-4


def test_forward_matches_oracle_and_leaves_state(hbmod, humanoid_model, gpu, golden):
    g = golden
    idx = np.arange(0, len(g["env"]), 4)
    b = hbmod.Batch(humanoid_model, len(idx), gpu)
    b.diag_enable(True)
    st = pack_state(g, idx)
    b.set_state(hbmod.STATE_INTEGRATION, st)
    b.forward(g["ctrl"][idx].astype(np.float32))
    assert np.allclose(b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64), st.astype(np.float32), atol=0)
    a = b.qacc()
    as_ = np.maximum(1.0, np.abs(g["qacc"][idx]).max(axis=1, keepdims=True))
    assert (np.abs(a - g["qacc"][idx]) / as_).max() <= 4e-4


def test_contact_free_drift_within_north_star_bar(hbmod, humanoid_model, gpu):
    """Free-running GPU vs oracle over the contact-free opening of the benchmark workload: every env is compared up to
    its first constraint row (contact or joint limit) on either side.  (Once an env has been through a contact its
    later contact-free stretches carry that history: those are covered, teacher-forced, by the one-step tests.)"""
    envs = list(range(64))
    n = len(envs)
    b = hbmod.Batch(humanoid_model, n, gpu)
    b.reset(perturb=True)
    oracles = []
    for e in envs:
        o = Oracle()
        o.init_env(e)
        oracles.append(o)
    # initial state identical (fp32 rounding of the Halton perturbation aside)
    q0 = b.qpos
    for i, o in enumerate(oracles):
        assert np.abs(q0[i] - o.qpos).max() < 1e-6
    T = 50
    worst = 0.0
    free = [True] * n  # still in its contact-free opening: no constraint row on either side so far
    compared = 0
    # the wider window: contact-free, but THROUGH joint-limit rows.  Round 1 measured 1.25e-4 here (an env passing through a limit
    # row, the mass matrix eliminated on the matrix cores; DESIGN.md §2 records the history) and only reported it; since round 3
    # it measures 6e-6, and is held to the same bar
    nocontact = [True] * n
    worst_wide, compared_wide = 0.0, 0
    for t in range(T):
        ctrl = np.stack([o.ctrl_env(t, e) for o, e in zip(oracles, envs)]).astype(np.float32)
        b.step(ctrl)
        for o, c in zip(oracles, ctrl):
            o.ctrl[:] = c
            o.step()
        q = b.qpos
        ncon, nefc, _ = b.counts()
        for i, o in enumerate(oracles):
            free[i] = free[i] and o.nefc == 0 and int(nefc[i]) == 0
            nocontact[i] = nocontact[i] and o.ncon == 0 and int(ncon[i]) == 0
            d = float((np.abs(q[i] - o.qpos) / np.maximum(1.0, np.abs(o.qpos))).max())
            if free[i]:
                compared += 1
                worst = max(worst, d)
            if nocontact[i]:
                compared_wide += 1
                worst_wide = max(worst_wide, d)
    print("\ncontact-free drift: up to the first constraint row %.3e (%d env-steps, asserted <= 1e-4); "
          "through joint-limit rows %.3e (%d env-steps, asserted <= 1e-4)" % (worst, compared, worst_wide, compared_wide))
    assert compared >= 100 and compared_wide >= 500, (compared, compared_wide)
    assert worst <= FREE_RUNNING_BOUND, worst
    assert worst_wide <= FREE_RUNNING_BOUND, worst_wide


def test_long_rollout_statistics_match_oracle(hbmod, humanoid_model, gpu):
    """1000 free-running steps: trajectories decorrelate (chaos), so compare ensemble statistics and
    check physical sanity instead of per-env drift."""
    n, T = 256, 1000
    b = hbmod.Batch(humanoid_model, n, gpu)
    b.reset(perturb=True)
    b.rollout_halton(T)
    b.sync()
    q = b.qpos
    assert np.isfinite(q).all() and np.isfinite(b.qvel).all()
    assert not b.status().any()
    assert np.allclose(np.linalg.norm(q[:, 3:7], axis=1), 1.0, atol=1e-4)
    assert q[:, 2].min() > -0.02 and q[:, 2].max() < 1.0  # everybody is lying on the floor, nobody below it
    o = Oracle()
    _, qo, st = o.rollout_threads(n, T, os.cpu_count() or 4, 0, True)
    assert abs(q[:, 2].mean() - qo[:, 2].mean()) < 0.02
    nc, ne, ni = b.counts()
    assert abs(ne.mean() - st["mean_nefc"]) < 4.0
    assert abs(np.abs(q[:, 7:]).mean() - np.abs(qo[:, 7:]).mean()) < 0.05
    assert np.allclose(b.time, T * 0.005, rtol=1e-4)


def test_rollout_equals_repeated_steps_bitwise(hbmod, humanoid_model, gpu):
    n, T = 64, 40
    rng = np.random.default_rng(3)
    ctrl = rng.uniform(-1, 1, size=(T, n, humanoid_model.nu)).astype(np.float32)
    a = hbmod.Batch(humanoid_model, n, gpu)
    c = hbmod.Batch(humanoid_model, n, gpu)
    a.reset(perturb=True)
    c.reset(perturb=True)
    qs = a.rollout(ctrl, want_qpos=True)
    for t in range(T):
        c.step(ctrl[t])
        if t in (0, 17, T - 1):
            assert np.array_equal(qs[t], c.qpos)
    assert np.array_equal(a.get_state(hbmod.STATE_INTEGRATION), c.get_state(hbmod.STATE_INTEGRATION))
    # n_substeps: same control held
    d = hbmod.Batch(humanoid_model, n, gpu)
    e = hbmod.Batch(humanoid_model, n, gpu)
    d.reset(perturb=True); e.reset(perturb=True)
    d.step(ctrl[0], n_substeps=5)
    for _ in range(5):
        e.step(ctrl[0])
    assert np.array_equal(d.get_state(hbmod.STATE_INTEGRATION), e.get_state(hbmod.STATE_INTEGRATION))


def test_device_halton_controls_and_determinism(hbmod, humanoid_model, gpu):
    n, T, off = 32, 12, 4096
    b = hbmod.Batch(humanoid_model, n, gpu)
    nu = humanoid_model.nu
    buf = b.dev_alloc(T * n * nu * 4)
    b.halton_ctrl_dev(T, 3, off, buf)
    got = b.from_dev(buf, (T, n, nu))
    want = np.array([[[2 * halton(1 + 3 + t + 1000 * (off + e), i + 2) - 1 for i in range(nu)] for e in range(n)] for t in range(T)])
    assert np.abs(got - want).max() < 2e-6
    # rollout with the control tensor in HBM == rollout generating the same controls on chip
    b.reset(perturb=True, env_offset=off)
    b.rollout_dev(buf, T)
    s1 = b.get_state(hbmod.STATE_INTEGRATION)
    b.reset(perturb=True, env_offset=off)
    b.rollout_halton(T, t0=3, env_offset=off)
    s2 = b.get_state(hbmod.STATE_INTEGRATION)
    assert np.array_equal(s1, s2)
    # and again: bitwise reproducible
    b.reset(perturb=True, env_offset=off)
    b.rollout_halton(T, t0=3, env_offset=off)
    assert np.array_equal(s2, b.get_state(hbmod.STATE_INTEGRATION))
    b.dev_free(buf)


def test_sharding_by_env_offset_is_exact(hbmod, humanoid_model, gpu):
    """Envs are independent: one batch of 2N envs == two batches of N with env_offset (multi-GPU split)."""
    n, T = 128, 30
    whole = hbmod.Batch(humanoid_model, 2 * n, gpu)
    whole.reset(perturb=True)
    whole.rollout_halton(T)
    sw = whole.get_state(hbmod.STATE_INTEGRATION)
    for r in range(2):
        part = hbmod.Batch(humanoid_model, n, gpu)
        part.reset(perturb=True, env_offset=r * n)
        part.rollout_halton(T, env_offset=r * n)
        assert np.array_equal(part.get_state(hbmod.STATE_INTEGRATION), sw[r * n:(r + 1) * n])


def test_pipelined_stepping_is_bit_identical(hbmod, humanoid_model, gpu):
    """hb_batch_pipeline: env segments on their own streams, each step following only its own
    segment's previous step.  Same states, bit for bit, as the single launch per step — including
    across a mid-run reset of some envs, a host state read and a switch back to unpipelined stepping."""
    n, T = 1000, 40  # not a multiple of the segment count's natural sizes
    ref = hbmod.Batch(humanoid_model, n, gpu)
    pip = hbmod.Batch(humanoid_model, n, gpu)
    pip.pipeline(3)  # three uneven segments
    mask = (np.arange(n) % 7 == 0).astype(np.uint8)
    for b in (ref, pip):
        b.reset(perturb=True)
        for t in range(T):
            b.rollout_halton(1, t0=t)
        mid = b.get_state(hbmod.STATE_INTEGRATION)     # joins the pipes
        b.reset(mask=mask, perturb=True)
        for t in range(T, 2 * T):
            b.rollout_halton(1, t0=t)
        if b is pip:
            b.pipeline(False)
        b.rollout_halton(5, t0=2 * T)
        b.final = b.get_state(hbmod.STATE_INTEGRATION)
        b.mid = mid
    assert np.array_equal(ref.mid, pip.mid)
    assert np.array_equal(ref.final, pip.final)
    assert np.array_equal(ref.status(), pip.status())
    for a, c in zip(ref.counts(), pip.counts()):
        assert np.array_equal(a, c)


def test_default_pipeline_picks_its_segment_count_by_probe(hbmod, humanoid_model, gpu):
    """hb_batch_pipeline(1): three segments when their streams run kernels side by side, two otherwise - also with other batches
    (and their streams) alive in the process - and up to eight on request; the states stay those of the single launch."""
    n, T = 1000, 12
    ref = hbmod.Batch(humanoid_model, n, gpu)
    ref.reset(perturb=True)
    for t in range(T):
        ref.rollout_halton(1, t0=t)
    want = ref.get_state(hbmod.STATE_INTEGRATION)
    others = [hbmod.Batch(humanoid_model, 64, gpu) for _ in range(3)]
    for o in others:
        o.pipeline(2)
        o.reset(perturb=True)
        o.rollout_halton(1)
    for on in (True, 8, True):
        b = hbmod.Batch(humanoid_model, n, gpu)
        b.pipeline(on)
        assert b.segments in ((2, 3) if on is True else (8,))
        b.reset(perturb=True)
        for t in range(T):
            b.rollout_halton(1, t0=t)
        assert np.array_equal(b.get_state(hbmod.STATE_INTEGRATION), want)
        b.close()
    for o in others:
        o.close()


@pytest.mark.parametrize("solver", [0, 2])
def test_lean_kernels_are_bit_identical_to_the_full_ones(hbmod, humanoid_model, gpu, solver):
    """A launch without optional inputs / outputs runs step_body's LEAN instantiation (hb_step_lean_kernel, hb_step_newton28_lean_kernel);
    asking for any of them - here the recorded qpos trajectory - runs the full one.  Same arithmetic: same bits, same counts."""
    m = hbmod.Model.load(HUMANOID_HBM)  # (a model of its own: the solver is set on it)
    m.set_opt(solver=solver, iterations=50 if solver == 0 else 100)
    if True:
        n, T = 512, 60
        rng = np.random.default_rng(4)
        ctrl = rng.uniform(-1, 1, size=(T, n, m.nu)).astype(np.float32)
        a = hbmod.Batch(m, n, gpu); b = hbmod.Batch(m, n, gpu)
        a.reset(perturb=True); b.reset(perturb=True)
        a.rollout_halton(200); b.rollout_halton(200)          # lean in both: onto the floor
        c = hbmod.Batch(m, n, gpu)
        c.reset(perturb=True); c.rollout_halton(200)
        a.rollout(ctrl)                                         # lean, multi-step (LEAN = 2)
        q = b.rollout(ctrl, want_qpos=True)                     # full kernel (qpos_out)
        for t in range(T):
            c.step(ctrl[t])                                     # single steps: the leanest kernel - for this model's PGS the size-specialised hb_step_h27_kernel
        sa, sb, sc = a.get_state(hbmod.STATE_INTEGRATION), b.get_state(hbmod.STATE_INTEGRATION), c.get_state(hbmod.STATE_INTEGRATION)
        assert np.array_equal(sa, sb) and np.array_equal(sc, sb)
        assert np.array_equal(c.status(), b.status())
        c.close()
        assert np.array_equal(q[-1], sb[:, 1:1 + m.nq])
        for x, y in zip(a.counts(), b.counts()):
            assert np.array_equal(x, y)
        assert np.array_equal(a.status(), b.status()) and a.counts()[1].max() > 0
        a.close(); b.close()


def test_state_io_reset_and_keyframes(hbmod, humanoid_model, gpu):
    m = humanoid_model
    n = 16
    b = hbmod.Batch(m, n, gpu)
    assert b.state_size(hbmod.STATE_INTEGRATION) == 1 + m.nq + 2 * m.nv
    assert b.state_size(hbmod.STATE_QPOS | hbmod.STATE_QVEL) == m.nq + m.nv
    qpos0 = m.array("qpos0")
    assert np.allclose(b.qpos, qpos0.astype(np.float32)[None])
    assert not b.qvel.any() and not b.time.any()
    # set / get round trip in mjtState bit order
    rng = np.random.default_rng(1)
    st = rng.normal(size=(n, b.state_size(hbmod.STATE_INTEGRATION))).astype(np.float32)
    b.set_state(hbmod.STATE_INTEGRATION, st)
    assert np.array_equal(b.get_state(hbmod.STATE_INTEGRATION), st)
    assert np.array_equal(b.get_state(hbmod.STATE_QVEL), st[:, 1 + m.nq:1 + m.nq + m.nv])
    part = rng.normal(size=(n, m.nv)).astype(np.float32)
    b.set_state(hbmod.STATE_QVEL, part)
    st[:, 1 + m.nq:1 + m.nq + m.nv] = part
    assert np.array_equal(b.get_state(hbmod.STATE_INTEGRATION), st)
    # masked reset to a keyframe
    key = m.array("key_qpos").reshape(m.nkey, m.nq)
    mask = np.zeros(n, np.uint8)
    mask[::2] = 1
    b.reset(mask=mask, keyframe=m.name2id("key", "squat"))
    q = b.qpos
    assert np.allclose(q[::2], key[0].astype(np.float32)[None])
    assert np.array_equal(q[1::2], st[1::2, 1:1 + m.nq])
    with pytest.raises(hbmod.HbError):
        b.reset(keyframe=7)


def test_bad_state_is_flagged_and_reset(hbmod, humanoid_model, gpu):
    """mj_checkPos / mj_checkVel / mj_checkAcc semantics (mujoco.h:301-307) against the oracle: NaN or |x| > 1e10 raises the
    warning and resets the data — qpos0, zero velocity, warm start, ctrl and xfrc_applied, time 0 — and the step carries on
    from there (a bad qacc runs mj_forward a second time on the reset data, then integrates); other envs are untouched."""
    m = humanoid_model
    n = 8
    b = hbmod.Batch(m, n, gpu)
    b.reset(perturb=True)
    b.rollout_halton(30)
    spec = hbmod.STATE_INTEGRATION | hbmod.STATE_XFRC_APPLIED
    st = b.get_state(spec, dtype=np.float64)
    st0 = st.copy()
    nint = 1 + m.nq + 2 * m.nv
    st[2, 5] = np.nan                      # qpos      -> mjWARN_BADQPOS
    st[5, 1 + m.nq + 3] = 1e12             # qvel      -> mjWARN_BADQVEL
    st[6, nint + 6 * 1 + 2] = 1e14         # xfrc_applied on the torso: |qacc| > 1e10 -> mjWARN_BADQACC
    b.set_state(spec, st)
    ctrl = np.full((n, m.nu), 0.7, np.float32)
    b.step(ctrl)
    s = b.status()
    assert s[2] == hbmod.WARN_BADQPOS and s[5] == hbmod.WARN_BADQVEL and s[6] == hbmod.WARN_BADQACC
    assert not s[[0, 1, 3, 4, 7]].any()
    q, v, t = b.qpos.astype(np.float64), b.qvel.astype(np.float64), b.time
    assert np.isfinite(q).all() and np.isfinite(v).all()
    # the oracle on the same inputs: flagged envs end up at "qpos0 stepped once with zero controls", time = h
    for e in range(n):
        o = Oracle()
        o.reset()
        o.L.om_data_set_time(o.d, st[e, 0])
        o.qpos[:] = st[e, 1:1 + m.nq]; o.qvel[:] = st[e, 1 + m.nq:1 + m.nq + m.nv]; o.qacc_warmstart[:] = st[e, 1 + m.nq + m.nv:nint]
        o.xfrc_applied[:] = st[e, nint:]
        o.ctrl[:] = ctrl[e]
        o.step()
        want_bad = e in (2, 5, 6)
        assert (o.dint("warn_badqpos"), o.dint("warn_badqvel"), o.dint("warn_badqacc")) == (int(e == 2), int(e == 5), int(e == 6))
        assert abs(t[e] - o.time) < 1e-6 and (abs(o.time - 0.005) < 1e-12) == want_bad
        assert (np.abs(q[e] - o.qpos) / np.maximum(1, np.abs(o.qpos))).max() <= 4e-5
        assert np.abs(v[e] - o.qvel).max() <= 4e-4 * max(1.0, np.abs(o.qvel).max())
    # the three reset envs are the same state (nothing of their old data survives), and it is not simply qpos0: gravity acted
    assert np.array_equal(q[2], q[5]) and np.array_equal(q[2], q[6]) and np.array_equal(v[2], v[6])
    assert np.abs(v[2]).max() > 1e-3
    # mj_resetData also cleared xfrc_applied of the flagged env, and only that one's
    after = b.get_state(spec, dtype=np.float64)
    assert not after[6, nint:].any() and np.array_equal(after[0, nint:], st0[0, nint:])
    b.reset()
    assert not b.status().any()


def test_config3_last_rank_shard_at_env_offset_28672(hbmod, humanoid_model, gpu):
    """BASELINE configs[2]: 32768 envs over 8 GPUs, env e on GPU floor(e / 4096).  Rank 7's shard: env_offset = 28672,
    Halton indices 1 + t + 1000 e up to 3.3e7 (beyond 2^24: the device generator divides in integers), initial
    perturbation indexed by the global env; two half shards at that offset equal the whole one bit for bit."""
    n, off, T = 4096, 28672, 200
    nu = humanoid_model.nu
    b = hbmod.Batch(humanoid_model, n, gpu)
    # device Halton controls vs the fp64 Python generator, sampled over the shard (first, last and strided envs; late steps)
    buf = b.dev_alloc(4 * n * nu * 4)
    b.halton_ctrl_dev(4, T - 4, off, buf)
    got = b.from_dev(buf, (4, n, nu))
    envs = [0, 1, 2047, 2048, 4094, 4095] + list(range(5, n, 611))
    for t in (0, 3):
        for e in envs:
            want = np.array([2 * halton(1 + (T - 4) + t + 1000 * (off + e), i + 2) - 1 for i in range(nu)])
            assert np.abs(got[t, e] - want).max() < 2e-6, (t, e)
    b.dev_free(buf)
    # initial state and a free-running start against the oracle at the global indices
    b.reset(perturb=True, env_offset=off)
    q0 = b.qpos
    for e in (0, 4095):
        o = Oracle()
        o.init_env(off + e)
        assert np.abs(q0[e] - o.qpos).max() < 1e-6
    b.rollout_halton(T, 0, off)
    whole = b.get_state(hbmod.STATE_INTEGRATION)
    assert np.isfinite(whole).all() and not b.status().any()
    o = Oracle()
    o.init_env(off + 4095)
    for t in range(20):  # contact-free opening: the device follows the oracle
        o.ctrl[:] = o.ctrl_env(t, off + 4095)
        o.step()
    c = hbmod.Batch(humanoid_model, 1, gpu)
    c.reset(perturb=True, env_offset=off + 4095)
    c.rollout_halton(20, 0, off + 4095)
    assert (np.abs(c.qpos[0] - o.qpos) / np.maximum(1, np.abs(o.qpos))).max() <= 1e-4
    # sharded == whole, bitwise, on a 2 x 2048 split of this shard
    for r in range(2):
        part = hbmod.Batch(humanoid_model, n // 2, gpu)
        part.reset(perturb=True, env_offset=off + r * (n // 2))
        part.rollout_halton(T, 0, off + r * (n // 2))
        assert np.array_equal(part.get_state(hbmod.STATE_INTEGRATION), whole[r * (n // 2):(r + 1) * (n // 2)])
    # and the shard differs from rank 0's (the offset really selects other envs)
    b.reset(perturb=True, env_offset=0)
    assert not np.array_equal(b.qpos, q0)


def test_config3_all_32768_envs_on_one_gpu(hbmod, humanoid_model, gpu):
    """The whole of configs[2] as one batch: size-independent properties after 300 steps, and its rank-3 block equal to a
    4096-env batch at env_offset 3 * 4096 (what the 8-GPU run computes on GPU 3)."""
    n, T = 32768, 300
    b = hbmod.Batch(humanoid_model, n, gpu)
    b.reset(perturb=True)
    b.rollout_halton(T)
    st = b.get_state(hbmod.STATE_INTEGRATION)
    q = st[:, 1:1 + humanoid_model.nq]
    assert np.isfinite(st).all() and not b.status().any()
    assert np.abs(np.linalg.norm(q[:, 3:7], axis=1) - 1).max() < 1e-4
    assert q[:, 2].min() > -0.02 and q[:, 2].max() < 1.6
    assert np.allclose(st[:, 0], T * 0.005, rtol=1e-4)
    nc, ne, ni = b.counts()
    assert nc.max() <= humanoid_model.ncon_max and ne.max() <= humanoid_model.nefc_max
    assert len(np.unique(q[:, 2])) > n // 2
    part = hbmod.Batch(humanoid_model, 4096, gpu)
    part.reset(perturb=True, env_offset=3 * 4096)
    part.rollout_halton(T, 0, 3 * 4096)
    assert np.array_equal(part.get_state(hbmod.STATE_INTEGRATION), st[3 * 4096:4 * 4096])


def test_benchmark_workload_stays_inside_the_row_capacity(hbmod, humanoid_model, gpu):
    """Row capacity (24 contacts / 63 rows per env) against the benchmark workload: 4096 envs x 3000 steps = 1.2e7 env-steps
    (fall, impact, flailing on the floor) without a single dropped contact or row — status bits are sticky, so a clean status
    word at the end means no env-step overflowed; the distribution's tail is printed.  (The collapsed zero-control regime
    sits at the edge: profiles/r01_soak_1e10.txt saw one CNSTRFULL in 1e10 env-steps; VecEnv reports the bits, see
    test_gpu_env.py.)"""
    n, T = 4096, 3000
    b = hbmod.Batch(humanoid_model, n, gpu)
    b.reset(perturb=True)
    mx_c = mx_e = 0
    for k in range(T // 100):
        b.rollout_halton(100, 100 * k)
        nc, ne, _ = b.counts()
        mx_c, mx_e = max(mx_c, int(nc.max())), max(mx_e, int(ne.max()))
    s = b.status()
    print("\nmax ncon %d / %d, max nefc %d / %d sampled every 100 steps over %.1e env-steps; envs flagged %d"
          % (mx_c, humanoid_model.ncon_max, mx_e, humanoid_model.nefc_max, n * T, int((s != 0).sum())))
    assert not (s & (hbmod.WARN_CONTACTFULL | hbmod.WARN_CNSTRFULL)).any()
    assert not s.any()


def test_disable_flags_and_options(hbmod, gpu):
    from humanoid_mujoco_amd import engine
    m = hbmod.Model.load(HUMANOID_HBM)
    m.set_opt(disableflags=engine.DSBL_CONTACT | engine.DSBL_LIMIT)
    b = hbmod.Batch(m, 8, gpu)
    b.reset(keyframe=0)
    for _ in range(20):
        b.step(np.ones((8, m.nu), np.float32))
    nc, ne, _ = b.counts()
    assert not nc.any() and not ne.any()
    # gravity off + everything passive off: free body keeps its velocity exactly
    m2 = hbmod.Model.load(HUMANOID_HBM)
    m2.set_opt(disableflags=engine.DSBL_CONTACT | engine.DSBL_LIMIT | engine.DSBL_GRAVITY | engine.DSBL_PASSIVE | engine.DSBL_ACTUATION)
    b2 = hbmod.Batch(m2, 2, gpu)
    st = b2.get_state(hbmod.STATE_INTEGRATION)
    st[:, 1 + m2.nq + 0] = 1.5  # root x velocity
    b2.set_state(hbmod.STATE_INTEGRATION, st)
    b2.step(np.zeros((2, m2.nu), np.float32), n_substeps=10)
    assert np.allclose(b2.qvel[:, 0], 1.5, atol=1e-5)
    assert np.allclose(b2.qpos[:, 0], 1.5 * 10 * 0.005, atol=1e-5)


@pytest.mark.parametrize("name,steps", [("ball_plane", 400), ("capsules", 300), ("chain", 300), ("pendulum_limit", 500),
                                        ("maxsize", 600)])
def test_other_models_one_step_parity_along_oracle_trajectory(hbmod, gpu, tmp_path, name, steps):
    """Multi-tree models, slide joints, tendon limits, affine actuators, condim-1 pairs, and the engine's capacity
    limits all at once (maxsize: nv = 32, a 17-dof chain, three joints on a body, six children under one):
    teacher-forced one-step parity at states sampled along an oracle rollout."""
    xml = os.path.join(MODELS, name + ".xml")
    m = hbmod.Model.load(xml)
    p = str(tmp_path / (name + ".hbm"))
    m.save(p)
    o = Oracle(p)
    o.reset(0 if name == "chain" else -1)
    rng = np.random.default_rng(11)
    states, ctrls, outs = [], [], []
    for t in range(steps):
        c = rng.uniform(-1, 1, size=max(o.nu, 1))[:o.nu]
        o.ctrl[:] = c
        if t % 10 == 0:
            states.append(np.concatenate([[o.time], o.qpos, o.qvel, o.qacc_warmstart]))
            ctrls.append(c.copy())
        o.step()
        if t % 10 == 0:
            outs.append((o.qpos.copy(), o.qvel.copy(), o.ncon, o.nefc))
    n = len(states)
    b = hbmod.Batch(m, n, gpu)
    b.set_state(hbmod.STATE_INTEGRATION, np.array(states))
    b.step(np.array(ctrls, dtype=np.float32).reshape(n, m.nu))
    q, v = b.qpos.astype(np.float64), b.qvel.astype(np.float64)
    nc, ne, _ = b.counts()
    assert not b.status().any()
    for k, (qo, vo, nco, neo) in enumerate(outs):
        assert (nc[k], ne[k]) == (nco, neo), (k, nc[k], ne[k], nco, neo)
        assert (np.abs(q[k] - qo) / np.maximum(1, np.abs(qo))).max() <= 1e-4
        assert np.abs(v[k] - vo).max() <= 1e-3 * max(1.0, np.abs(vo).max())


def test_xfrc_applied(hbmod, humanoid_model, gpu):
    """Cartesian push on a body (CPUEnv._apply_external_forces, cpu_env.py:618-654) vs the oracle."""
    m = humanoid_model
    n = 4
    b = hbmod.Batch(m, n, gpu)
    b.reset(perturb=True)
    st = b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
    xf = np.zeros((n, m.nbody, 6))
    xf[:, 1, 0] = [10, -5, 0, 3]
    xf[:, 7, 1] = [0, 8, -8, 1]
    xf[2, 12, 3:6] = [0.5, -0.25, 1.0]
    b.set_state(hbmod.STATE_XFRC_APPLIED, xf.reshape(n, -1))
    b.step(np.zeros((n, m.nu), np.float32))
    v = b.qvel
    for e in range(n):
        o = Oracle()
        o.reset()
        o.qpos[:] = st[e, 1:1 + m.nq]
        o.xfrc_applied[:] = xf[e].ravel()
        o.step()
        assert np.abs(v[e] - o.qvel).max() <= 1e-3 * max(1.0, np.abs(o.qvel).max())
    assert np.array_equal(b.get_state(hbmod.STATE_XFRC_APPLIED).reshape(n, m.nbody, 6), xf.astype(np.float32))


def test_observation_layout(hbmod, humanoid_model, gpu):
    """obs[48] = hinge qpos (21), hinge qvel (21), root angular velocity (3), gravity in torso frame (3):
    the 27-DoF analogue of CPUEnv._get_obs (cpu_env.py:554-571), SURVEY.md §8(a) a18."""
    m = humanoid_model
    n = 8
    b = hbmod.Batch(m, n, gpu)
    b.reset(perturb=True)
    b.rollout_halton(80)
    obs, rew, term, trunc = b.obs()
    q, v = b.qpos, b.qvel
    assert obs.shape == (n, 48)
    assert np.array_equal(obs[:, :21], q[:, 7:]) and np.array_equal(obs[:, 21:42], v[:, 6:])
    assert np.array_equal(obs[:, 42:45], v[:, 3:6])
    for e in range(n):
        w, x, y, z = q[e, 3:7] / np.linalg.norm(q[e, 3:7])
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        assert np.allclose(obs[e, 45:48], R.T @ np.array([0, 0, -1.0]), atol=1e-5)
    assert np.isfinite(rew).all() and not term.any() and not trunc.any()


def test_full_size_batch_properties(hbmod, humanoid_model, gpu):
    """BASELINE config 2 size (4096 envs): size-independent properties after 300 steps."""
    n, T = 4096, 300
    b = hbmod.Batch(humanoid_model, n, gpu)
    b.reset(perturb=True)
    b.rollout_halton(T)
    q, v = b.qpos, b.qvel
    assert np.isfinite(q).all() and np.isfinite(v).all()
    assert not b.status().any()
    assert np.abs(np.linalg.norm(q[:, 3:7], axis=1) - 1).max() < 1e-4
    assert q[:, 2].min() > -0.02
    nc, ne, ni = b.counts()
    assert nc.max() <= humanoid_model.ncon_max and ne.max() <= humanoid_model.nefc_max and ni.max() <= 50
    # joint limits are soft but hold to within a few degrees
    rng_ = humanoid_model.array("jnt_range").reshape(-1, 2)[1:]
    viol = np.maximum(q[:, 7:] - rng_[None, :, 1], rng_[None, :, 0] - q[:, 7:]).max()
    assert viol < 0.35
    # distinct environments really are distinct, identical ones identical
    assert len(np.unique(q[:, 2])) > n // 2


def test_heightfield_terrain_humanoid_config5(hbmod, gpu):
    """BASELINE config 5 (terrain humanoid, PGS exactly 50 sweeps): teacher-forced one-step parity along an
    oracle trajectory on the height-field model, then an 8192-env sanity rollout.  The terrain collider is MuJoCo's scheme
    (mjc_ConvexHField: prisms under the geom, MPR per prism; oracle convex_hfield, device collide_general), restated, not pinned."""
    path = HFIELD_HBM
    m = hbmod.Model.load(path)
    assert m.opt.tolerance == 0.0 and m.opt.iterations == 50
    o = Oracle(path)
    states, ctrls, outs = [], [], []
    for e in (0, 3):
        o.init_env(e)
        for t in range(420):
            c = o.ctrl_env(t, e)
            o.ctrl[:] = c
            take = t % 20 == 0
            if take:
                states.append(np.concatenate([[o.time], o.qpos, o.qvel, o.qacc_warmstart]))
                ctrls.append(c.copy())
            o.step()
            if take:
                outs.append((o.qpos.copy(), o.qvel.copy(), o.ncon, o.nefc, o.dint("solver_niter")))
    n = len(states)
    b = hbmod.Batch(m, n, gpu)
    b.set_state(hbmod.STATE_INTEGRATION, np.array(states))
    b.step(np.array(ctrls, dtype=np.float32))
    assert b.last_kernel() == "hb_step_gen_fast_h27_kernel"  # the staged step's sized fast kernel: what the configs[4] measurement times
    q, v = b.qpos.astype(np.float64), b.qvel.astype(np.float64)
    nc, ne, ni = b.counts()
    assert not b.status().any()
    seen_contacts = 0
    for k, (qo, vo, nco, neo, nio) in enumerate(outs):
        assert (nc[k], ne[k]) == (nco, neo)
        assert ni[k] == nio  # exactly 50 sweeps whenever there are constraints
        seen_contacts += nco
        assert (np.abs(q[k] - qo) / np.maximum(1, np.abs(qo))).max() <= 1e-4
        assert np.abs(v[k] - vo).max() <= 1e-3 * max(1.0, np.abs(vo).max())
    assert seen_contacts > 20
    big = hbmod.Batch(m, 8192, gpu)
    big.reset(perturb=True)
    big.rollout_halton(300)
    qq = big.qpos
    assert np.isfinite(qq).all() and not big.status().any()
    assert qq[:, 2].min() > -0.15 and qq[:, 2].max() < 1.5
    _, _, it = big.counts()
    assert set(np.unique(it)) <= {0, 50}


def test_capacity_overflow_is_flagged_not_fatal(hbmod, gpu):
    """More contacts / constraint rows than the device buffers hold: the extras are dropped and the env is
    flagged (mjWARN_CONTACTFULL / mjWARN_CNSTRFULL semantics, mjdata.h:54-65), nothing crashes or goes NaN,
    and other batches are unaffected."""
    m = hbmod.Model.load(os.path.join(MODELS, "overflow.xml"))
    assert m.nv == 30 and m.ngeom == 31
    b = hbmod.Batch(m, 4, gpu)
    b.step(np.zeros((4, 0), np.float32), n_substeps=3)
    s = b.status()
    assert (s & hbmod.WARN_CONTACTFULL).all() and (s & hbmod.WARN_CNSTRFULL).all()
    nc, ne, _ = b.counts()
    assert (nc == m.ncon_max).all() and (ne <= m.nefc_max).all() and (ne >= 60).all()
    assert np.isfinite(b.qpos).all() and np.isfinite(b.qvel).all()
    b.reset()
    assert not b.status().any()
