"""The contact-force read-out (include/hb.h: hb_contact_readout; hb_step.hip: the epilogue behind the solver) on the GPU.

Two tiers, so that a solver difference cannot pass for a wrong decode and a wrong decode cannot hide behind the solver's tolerance:
  DECODE  the read-out against the fp64 decode (tests/contact_ref.py) of the DEVICE's own efc_force and contacts.  What is left is the
          fp32 arithmetic of the decode itself: sums of at most ~100 terms.  Anything above 1e-5 would be a wrong decode.
  PARITY  the read-out against the decode of the ORACLE's rows at the same state: carries the solver's fp32 error (rows are held to 4e-4
          of max |efc_force|, tests/test_gpu_parity.py; a contact force sums up to 10 of them, a body's wrench a few contacts).
Both relative to max(1, max |efc_force|) of the state.  Measured on MI355X (tools/gpu_contact_force_report.py,
profiles/contact_force_parity_report.txt), maxima over every model and kernel below; each bound is at most 3 x its maximum:
  decode: contact forces 3.94e-7 (team robot, condim 6), body wrenches 5.91e-7 (RK4 Newton)             -> DECODE_BOUND 1.5e-6
  parity: contact forces and body wrenches 1.69e-4 (team robot, Newton on 256 rows; humanoid 5.6e-5 PGS, 6.4e-5 Newton,
          9.6e-5 RK4 Newton; chains <= 1.4e-5)                                                           -> PARITY_BOUND 5e-4
"""
import os

import numpy as np
import pytest

import contact_ref
import rk4_ref
from bounds import CONTACT_DECODE_BOUND as DECODE_BOUND, CONTACT_PARITY_BOUND as PARITY_BOUND
from oracle_lib import HUMANOID_HBM, MODELS_DIR, Oracle, load_state

pytestmark = pytest.mark.gpu
# which kernels may write a model's read-out (Batch.last_kernel after the step; a staged step is named after its fast pass)
KERNELS = {"humanoid27_pgs": ("hb_step_kernel",), "humanoid27_newton": ("hb_step_newton28_kernel",), "humanoid27_pgs_unsized": ("hb_step_kernel",),
           "chain12_cd4": ("hb_step_gen_big_kernel", "hb_step_gen_fast1_kernel"), "chain12_cd6": ("hb_step_gen_big_kernel", "hb_step_gen_fast1_kernel"),
           "chain12_hfield": ("hb_step_gen_kernel", "hb_step_gen_fast_kernel"), "team_robot": ("hb_step_newton_big20_kernel", "hb_step_newton_gen20_kernel")}
# the staged steps whose fast pass runs on a one-group layout: (kernel with the diagnostics, which switch that pass off; kernel without)
FAST_PASS = {"chain12_cd4": ["hb_step_gen_big_kernel", "hb_step_gen_fast1_kernel"], "chain12_cd6": ["hb_step_gen_big_kernel", "hb_step_gen_fast1_kernel"],
             "team_robot": ["hb_step_newton_big20_kernel", "hb_step_newton_gen20_kernel"]}
TORSO, FOOT_R, FOOT_L = 1, 7, 10  # bodies of humanoid27.hbm


def _show(label, kernel, err, differ):
    print("\n  %-24s %-30s differ %d | " % (label, kernel, differ) + "  ".join("%s %.2e" % (k, v.max()) for k, v in sorted(err.items()) if len(v)))


@pytest.fixture(scope="module")
def golden_runs(hbmod, gpu, tmp_path_factory):
    """the golden states under PGS/50 and Newton/100, stepped once with the read-out on, and held against the reference once"""
    out = {}
    for name in ("humanoid27_pgs", "humanoid27_newton"):
        m, o, st, ct, tune = contact_ref.make_case(hbmod, name, tmp_path_factory.mktemp(name))
        dev = contact_ref.device_readout(hbmod, m, st, ct, gpu, tune)
        err, differ = contact_ref.compare(o, st, ct, dev)
        _show(name, dev["kernel"], err, differ)
        out[name] = (dev, err, differ, len(st))
    return out


@pytest.mark.parametrize("name", ["humanoid27_pgs", "humanoid27_newton"])
def test_decode_is_the_linear_map_of_the_devices_own_rows(golden_runs, name):
    dev, err, differ, n = golden_runs[name]
    assert dev["kernel"] in KERNELS[name] and not dev["status"].any()
    assert differ == 0 and len(err["decode_f"]) == n  # (ncon, nefc) and every contact's geoms and dimension are the oracle's
    assert (dev["ncon"] > 0).sum() == 102 and dev["ncon"].max() == 6
    assert err["beyond"].max() == 0.0
    assert err["decode_f"].max() <= DECODE_BOUND and err["decode_w"].max() <= DECODE_BOUND, (err["decode_f"].max(), err["decode_w"].max())


@pytest.mark.parametrize("name", ["humanoid27_pgs", "humanoid27_newton"])
def test_parity_with_the_oracle_on_the_same_states(golden_runs, name):
    dev, err, differ, n = golden_runs[name]
    assert differ == 0
    assert err["parity_f"].max() <= PARITY_BOUND and err["parity_w"].max() <= PARITY_BOUND, (err["parity_f"].max(), err["parity_w"].max())


@pytest.mark.parametrize("name", ["humanoid27_pgs_unsized", "chain12_cd4", "chain12_cd6", "chain12_hfield", "team_robot"])
def test_the_other_kernels(hbmod, gpu, tmp_path, name):
    """The kernels of the other variants, by name: the classic kernel with the size-specialised instantiations switched off, PGS on two
    row groups (condim 4 / 6 chains), the height-field chain (variant 1) and the team robot (Newton on four row groups; without the
    diagnostics its staged step runs the one-group fast pass first).  A state whose row set differs from the oracle's (a pair on its
    margin boundary, another MPR portal: the rounding fences of tests/oracle_lib.py; smoke() allows two in 16) has no oracle row
    addresses to decode with: at most two per model, every other state is held to both bounds."""
    m, o, st, ct, tune = contact_ref.make_case(hbmod, name, tmp_path)
    runs = [("", contact_ref.device_readout(hbmod, m, st, ct, gpu, tune))]
    if name in FAST_PASS:
        runs.append((" (fast pass)", contact_ref.device_readout(hbmod, m, st, ct, gpu, tune, diag=False)))
    names = []
    for label, dev in runs:
        err, differ = contact_ref.compare(o, st, ct, dev)
        _show(name + label, dev["kernel"], err, differ)
        names.append(dev["kernel"])
        assert dev["kernel"] in KERNELS[name], dev["kernel"]
        assert not dev["status"].any()
        assert differ <= 2 and (dev["ncon"] > 0).sum() >= 8
        assert err["beyond"].max() == 0.0
        for key in ("decode_f", "decode_w"):
            if key in err:
                assert err[key].max() <= DECODE_BOUND, (name, key, err[key].max())
        assert err["parity_f"].max() <= PARITY_BOUND and err["parity_w"].max() <= PARITY_BOUND, (name, err["parity_f"].max(), err["parity_w"].max())
    if name in FAST_PASS:
        assert names == FAST_PASS[name], names
    if name == "team_robot":
        assert names == ["hb_step_newton_big20_kernel", "hb_step_newton_gen20_kernel"], names
        assert np.abs(runs[0][1]["cf"][:, :, 3:6]).max() > 0  # torsional / rolling entries are there


def _sensor_case(hbmod, gpu):
    m, _, st, _, _ = contact_ref.make_case(hbmod, "humanoid27_pgs", None)
    st = st.copy()
    st[5] = 0.0  # env 5: the reset pose five metres up, at rest: in free flight (and clear of itself) for all eight steps
    st[5, 1:1 + m.nq] = Oracle().marr("qpos0")
    st[5, 3] += 5.0
    return m, st


def test_sensor_rows_are_the_single_steps_getters(hbmod, gpu):
    """T = 8 steps of hb_rollout_sensors in one launch with touch and contact-force entries on both feet and the torso, against eight
    single steps each followed by the getters: the contact-force entries are body_contact's force rows, the touch entries the fp32 sum in
    contact order of contact_force's normal forces over the body's contacts - bit for bit."""
    m, st = _sensor_case(hbmod, gpu)
    n, T = len(st), 8
    bodies = (FOOT_R, FOOT_L, TORSO)
    spec = hbmod.Batch.sensor_spec(framepos_bodies=(TORSO,), touch_bodies=bodies, contactforce_bodies=bodies)
    ctrl = np.random.default_rng(2).uniform(-1, 1, (T, n, m.nu)).astype(np.float32)
    b = hbmod.Batch(m, n, gpu)
    b.set_state(hbmod.STATE_INTEGRATION, st)
    rows, _ = b.rollout_sensors(ctrl, spec)
    with pytest.raises(hbmod.HbError):
        b.contact_force()  # a sensor spec does not switch the getters on
    end = b.get_state(hbmod.STATE_INTEGRATION)
    b.close()
    assert rows.shape == (T, n, 3 + 3 + 9)
    gb = Oracle().info["geom_bodyid"]
    s = hbmod.Batch(m, n, gpu)
    s.diag_enable(True)
    s.contact_readout(True)
    s.set_state(hbmod.STATE_INTEGRATION, st)
    loaded = 0
    for t in range(T):
        s.step(ctrl[t])
        cf, bc, con, (nc, _, _) = s.contact_force(), s.body_contact(), s.contacts(), s.counts()
        touch = np.zeros((n, 3), np.float32)
        for e in range(n):
            for k in range(nc[e]):
                for i, body in enumerate(bodies):
                    if body in (gb[int(con[e, k, 14])], gb[int(con[e, k, 15])]):
                        touch[e, i] = np.float32(touch[e, i] + cf[e, k, 0])
        assert np.array_equal(rows[t, :, 3:6], touch), t
        assert np.array_equal(rows[t, :, 6:15], bc[:, bodies, 0:3].reshape(n, 9)), t
        assert not rows[t, 5, 3:].any() and nc[5] == 0  # free flight reads zeros
        loaded += int((touch[:, :2] > 0).any(axis=1).sum())
    assert np.array_equal(s.get_state(hbmod.STATE_INTEGRATION), end)
    assert loaded >= T * 8  # feet in contact in many env-steps
    # hb_sensors (a forward pass) and hb_transition_fd_sensors take the entries as well
    r = s.sensors(spec, ctrl[0])
    assert np.array_equal(r[:, 6:15], s.body_contact()[:, bodies, 0:3].reshape(n, 9))
    x = np.concatenate([s.qpos[:1], s.qvel[:1]], axis=1).astype(np.float64)
    C = s.transition_fd(x, ctrl[0, :1].astype(np.float64), centered=False, sensor_spec=spec)[2]  # (1 + 2 nv + nu = 76 envs of the 128)
    assert C.shape == (1, 15, 2 * m.nv) and np.isfinite(C).all()
    s.close()


def _rk4_model(hbmod):
    m = hbmod.Model.load(HUMANOID_HBM)
    m.set_opt(integrator=hbmod.INT_RK4)
    return m


def test_rk4_sensors_hold_the_first_stage_and_getters_the_last(hbmod, gpu):
    m, _, st, ct, _ = contact_ref.make_case(hbmod, "humanoid27_pgs", None)
    m = _rk4_model(hbmod)
    o = Oracle()
    n = len(st)
    bodies = (FOOT_R, FOOT_L, TORSO)
    first, last = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    scale = np.ones(n)
    for k in range(n):
        load_state(o, st[k], ct[k].astype(np.float64))
        o.forward()
        _, w0, _ = contact_ref.oracle_readout(o)
        scale[k] = max(1.0, float(np.abs(o.efc_force[:o.nefc]).max(initial=0.0)))
        rk4_ref.rk4_step(o, st[k], ct[k])  # leaves the oracle at the last stage
        _, w3, _ = contact_ref.oracle_readout(o)
        scale[k] = max(scale[k], 1.0, float(np.abs(o.efc_force[:o.nefc]).max(initial=0.0)))
        first[k], last[k] = w0[list(bodies), 0:3], w3[list(bodies), 0:3]
    apart = np.abs(first - last).max(axis=(1, 2)) / scale
    pick = np.flatnonzero(apart > 10 * PARITY_BOUND)  # chosen on the reference alone: the two stages' forces differ by far more than the bound
    print("\n  rk4: %d of %d states whose first and last stage differ by more than 10 x the bound" % (len(pick), n))
    assert len(pick) >= 20, len(pick)
    b = hbmod.Batch(m, n, gpu)
    b.contact_readout(True)
    b.set_state(hbmod.STATE_INTEGRATION, st)
    spec = hbmod.Batch.sensor_spec(contactforce_bodies=bodies)
    rows, _ = b.rollout_sensors(ct[None], spec)
    got_first = rows[0].astype(np.float64).reshape(n, 3, 3)
    got_last = b.body_contact().astype(np.float64)[:, bodies, 0:3]
    assert b.last_kernel() == "hb_rk4_kernel" and not b.status().any()
    b.close()
    e_first = np.abs(got_first - first).max(axis=(1, 2)) / scale
    e_last = np.abs(got_last - last).max(axis=(1, 2)) / scale
    print("\n  rk4: sensor row vs first stage %.2e, getters vs last stage %.2e; stages apart by >= %.2e on %d states" % (e_first[pick].max(), e_last[pick].max(), apart[pick].min(), len(pick)))
    assert e_first[pick].max() <= PARITY_BOUND and e_last[pick].max() <= PARITY_BOUND


def _run_steps(hbmod, gpu, m, st, ctrl, readout, pipelined=False, duo=None):
    b = hbmod.Batch(m, len(st), gpu)
    if duo is not None:
        b.tune(duo=duo)
    if readout:
        b.contact_readout(True)
    b.set_state(hbmod.STATE_INTEGRATION, st)
    if pipelined:
        b.pipeline(True)
        nb = ctrl[0].nbytes
        d = b.dev_alloc(len(ctrl) * nb)
        for t in range(len(ctrl)):
            b.to_dev(d + t * nb, ctrl[t])
        for t in range(len(ctrl)):
            b.step_dev(d + t * nb)
        b.sync()
    else:
        for t in range(len(ctrl)):
            b.step(ctrl[t])
    out = (b.get_state(hbmod.STATE_INTEGRATION), b.status(), b.last_kernel(), (b.contact_force(), b.body_contact()) if readout else None)
    if pipelined:
        b.dev_free(d)
    b.close()
    return out


def test_nothing_else_moves(hbmod, gpu):
    """50 steps with the read-out on and off: the same states bit for bit, step by step and as folded step calls on a pipelined batch;
    and the two-envs-per-wave knob changes no read-out (such a launch takes the full kernel)"""
    m, _, st, _, _ = contact_ref.make_case(hbmod, "humanoid27_pgs", None)
    ctrl = np.random.default_rng(7).uniform(-1, 1, (50, len(st), m.nu)).astype(np.float32)
    off = _run_steps(hbmod, gpu, m, st, ctrl, False)
    on = _run_steps(hbmod, gpu, m, st, ctrl, True)
    assert off[2] != on[2] and on[2] == "hb_step_kernel", (off[2], on[2])
    assert np.array_equal(off[0], on[0]) and np.array_equal(off[1], on[1])
    poff = _run_steps(hbmod, gpu, m, st, ctrl, False, pipelined=True)
    pon = _run_steps(hbmod, gpu, m, st, ctrl, True, pipelined=True)
    assert np.array_equal(poff[0], off[0]) and np.array_equal(pon[0], off[0])
    assert np.array_equal(pon[3][0], on[3][0]) and np.array_equal(pon[3][1], on[3][1])
    duo = _run_steps(hbmod, gpu, m, st, ctrl, True, duo=2)
    assert duo[2] == "hb_step_kernel"
    assert np.array_equal(duo[0], off[0]) and np.array_equal(duo[3][0], on[3][0]) and np.array_equal(duo[3][1], on[3][1])
    assert np.abs(on[3][1]).max() > 0


def test_edges(hbmod, gpu, humanoid_model):
    m = humanoid_model
    b = hbmod.Batch(m, 8, gpu)
    for getter in (b.contact_force, b.body_contact, b.contact_readout_dev):
        with pytest.raises(hbmod.HbError):
            getter()  # before contact_readout
    b.contact_readout(True)
    b.reset()
    q = b.get_state(hbmod.STATE_QPOS)
    q[:, 2] += 5.0  # zero contacts: free flight
    b.set_state(hbmod.STATE_QPOS, q)
    b.step(np.zeros((8, m.nu), np.float32))
    assert not b.counts()[0].any() and not b.contact_force().any() and not b.body_contact().any()
    assert b.contact_force().shape == (8, m.ncon_max, 6) and b.body_contact().shape == (8, m.nbody, 6)
    pc, pb = b.contact_readout_dev()
    assert pc and pb and np.array_equal(b.from_dev(pb, (8, m.nbody, 6)), b.body_contact())
    b.contact_readout(False)
    with pytest.raises(hbmod.HbError):
        b.body_contact()
    b.close()


def test_dropped_rows_read_zero(hbmod, gpu):
    """tests/models/overflow.xml: 30 resting spheres, 24 contacts kept, 15 of them get their four rows (60 of 63), the other nine are
    dropped with HB_WARN_CNSTRFULL and read zero; the warning bits and the states are those of a batch without the read-out"""
    m = hbmod.Model.load(os.path.join(MODELS_DIR, "overflow.xml"))
    got = []
    for readout in (False, True):
        b = hbmod.Batch(m, 4, gpu)
        if readout:
            b.contact_readout(True)
        b.step(np.zeros((4, 0), np.float32), n_substeps=3)
        got.append((b.status(), b.counts()[:2], b.get_state(hbmod.STATE_INTEGRATION)))
        if readout:
            cf, bc = b.contact_force(), b.body_contact()
        b.close()
    assert np.array_equal(got[0][0], got[1][0]) and (got[1][0] & hbmod.WARN_CNSTRFULL).all() and (got[1][0] & hbmod.WARN_CONTACTFULL).all()
    assert np.array_equal(got[0][2], got[1][2])
    assert (got[1][1][0] == 24).all() and (got[1][1][1] == 60).all()
    assert (cf[:, :15, 0] > 0).all() and not cf[:, 15:].any()
    # what the world carries is what the 15 contacts push with
    assert np.allclose(bc[:, 0, 2], -cf[:, :15, 0].sum(axis=1), rtol=1e-5)


def test_vecenv_body_contact_forces(hbmod, gpu, humanoid_model):
    m = humanoid_model
    env = hbmod.VecEnv(m, 32, gpu, randomization_factor=0.0, auto_reset=0, max_time=0.0, contact_forces=True)
    env.reset()
    for _ in range(10):  # the unperturbed reset pose stands on its feet
        env.step_arrays(np.zeros((32, m.nu), np.float32))
    w = env.body_contact_forces()
    assert np.array_equal(w, env.batch.body_contact()) and w.shape == (32, m.nbody, 6)
    print("\n  standing humanoid: foot loads %.1f / %.1f N" % (w[0, FOOT_R, 2], w[0, FOOT_L, 2]))
    assert (w[:, FOOT_R, 2] > 0).all() and (w[:, FOOT_L, 2] > 0).all()
    plain = hbmod.VecEnv(m, 4, gpu)
    with pytest.raises(RuntimeError):
        plain.body_contact_forces()
    env.close()
    plain.close()


def test_a_masked_env_keeps_its_rows(hbmod, gpu, humanoid_model):
    """hb_env_reset with reset_collision_mode = 2 steps every env once and then re-draws and steps, under an env mask, only the envs that
    ended in a self-collision.  An env whose first draw stood is skipped by those later launches; its state is then the plain reset's
    advanced by one zero-control step, bit for bit (tests/test_gpu_env_realism.py) - and so must its read-out rows be, which the
    masked launches around it may not have touched."""
    m, n = humanoid_model, 128
    kw = dict(randomization_factor=1.0, auto_reset=0, max_time=0.0, target_z=10.0, contact_forces=True)
    a = hbmod.VecEnv(m, n, gpu, reset_collision_mode=2, **kw)
    a.reset()
    b = hbmod.VecEnv(m, n, gpu, **kw)
    b.reset()
    b.step_arrays(np.zeros((n, m.nu), np.float32))
    first_draw = (a.batch.get_state(hbmod.STATE_INTEGRATION) == b.batch.get_state(hbmod.STATE_INTEGRATION)).all(axis=1)
    wa, wb = a.body_contact_forces(), b.body_contact_forces()
    fa, fb = a.batch.contact_force(), b.batch.contact_force()
    loaded = (wa != 0).any(axis=(1, 2))
    print("\n  %d envs kept their first draw (%d of them with contact forces), %d were re-drawn under a mask" % (first_draw.sum(), (loaded & first_draw).sum(), (~first_draw).sum()))
    assert (~first_draw).sum() >= 8 and (loaded & first_draw).sum() >= 8
    assert np.array_equal(wa[first_draw], wb[first_draw]) and np.array_equal(fa[first_draw], fb[first_draw])
    a.close()
    b.close()
