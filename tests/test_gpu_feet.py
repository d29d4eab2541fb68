"""Foot-contact terms of the env kernel on the GPU (include/hb.h: hb_env_feet): air time, impacts, stumbles, collisions and contact
resets against tests/feet_ref.py, on the device's own contact read-out.

Model: humanoid27.hbm (48 observations, 21 actuators, timestep 5 ms; torso 1, right foot 7, left foot 10).  64 envs unless a test says
otherwise.  tests/feet_lib.py describes the scenario and what was chosen for it: lifts, the flat envs, weights, step counts, the seed.

Bounds:
  bits     contact flags, masks, t_last, terminated, truncated, the flag columns of every row, the zero-weight configuration against
           a batch with the read-out alone, replays of recorded actions: equality;
  reward   PARITY_WORST is the worst |reward - reference| tools/gpu_feet_parity.py measured over feet_lib.CASES (profiles/feet_parity.txt,
           next to the figure of a feet-less twin on the same states); every reward check asserts 4 times that, rounded up to one
           digit.  The margin covers the lane-order summation on other states.  The bound must stay below 1e-4 of the run's largest
           |reward|: every real mistake (a wrong time base, a term paid twice, a flag off by a step) moves the reward by 1e-2 or more.
"""
import numpy as np
import pytest

import cmd_lib
import feet_lib
import feet_ref
from feet_lib import FOOT_L, FOOT_R, bits

pytestmark = pytest.mark.gpu

NOBS, NU = 48, 21
PARITY_WORST = 1.464e-05  # profiles/feet_parity.txt
BOUND = 6e-05             # 4 x PARITY_WORST, rounded up to one digit


def _check_run(out, n_feet):
    """the reward bound and the non-vacuity counts of one run of the scenario"""
    assert BOUND <= 1e-4 * out["scale"], (BOUND, out["scale"])
    assert out["feet"] <= BOUND, out
    real = min(n_feet, 2)
    assert out["touchdowns"].sum() >= 16 and (out["touchdowns"][:real] > 0).all(), out["touchdowns"]
    assert out["impact"] >= 8 and out["stumble"] >= 8 and out["collision"] >= 8 and out["terminated"] >= 4, out


@pytest.mark.parametrize("case", feet_lib.CASES, ids=lambda c: "sub%d-feet%d-gate%d-%s-kind%d" % c)
def test_step_by_step(hbmod, gpu, case):
    """the landing scenario: records and flags bit for bit after every step, the reward within the bound, and enough of every event;
    the first two cases carry the feet-less twin, whose states stay equal bit for bit (the terms do not touch the physics)"""
    out = feet_lib.run_scenario(hbmod, gpu, 64, *case, twin=case in feet_lib.CASES[:2], log=lambda s: print("\n  " + s, end=""))
    _check_run(out, case[1])


def test_gate_closed_by_the_target_velocity(hbmod, gpu):
    """the gate on with no commands installed and hb_env_config.target_velocity below air_cmd_min: no touchdown is paid, the records
    move all the same, and the reward stays within the bound (case gate 2 of feet_lib.CASES is the same with the gate open)"""
    out = feet_lib.run_scenario(hbmod, gpu, 64, 4, 2, 3, "torso", 0, twin=False, log=lambda s: print("\n  " + s, end=""))
    assert BOUND <= 1e-4 * out["scale"] and out["feet"] <= BOUND, out
    assert out["touchdowns"].sum() == 0 and out["gated"] >= 16, out


def test_part_filled_block(hbmod, gpu):
    """37 envs: two full blocks of the env kernel (16 envs each) and a part-filled one"""
    out = feet_lib.run_scenario(hbmod, gpu, 37, 1, 2, 0, "torso", 0, twin=False, log=lambda s: print("\n  " + s, end=""))
    assert BOUND <= 1e-4 * out["scale"] and out["feet"] <= BOUND, out
    assert out["touchdowns"].sum() >= 16 and out["terminated"] >= 4, out


def test_zero_weights_move_nothing(hbmod, gpu):
    """all weights zero, no terminal bodies, not observed: obs, reward, flags and states of 20 steps equal bit for bit those of a batch
    with the contact read-out and no feet, from the same kernel in the same number of launches"""
    n = 64
    mdl = feet_lib.model(hbmod)
    opts = feet_lib.feet_options(hbmod, mdl, 2, 0, "torso", **feet_lib.ZERO_WEIGHTS)
    opts["terminal"] = ()
    kw = dict(auto_reset=1, max_time=0.0499, realism=True, domain_randomization=True)
    a = feet_lib.env(hbmod, gpu, n, opts, None, mdl, **kw)
    c = feet_lib.env(hbmod, gpu, n, None, None, mdl, contact_forces=True, **kw)
    assert a.nobs == c.nobs == NOBS and a.batch.env_nobs == NOBS
    assert np.array_equal(bits(a.reset()), bits(c.reset()))
    rng = np.random.default_rng(3)
    ended = 0
    for t in range(20):
        act = cmd_lib.actions(rng, n, NU, 0.6)
        la, lc = a.batch.step_launches(), c.batch.step_launches()
        ra, rc = a.step_arrays(act), c.step_arrays(act)
        assert a.batch.step_launches() - la == c.batch.step_launches() - lc and a.batch.last_kernel() == c.batch.last_kernel(), t
        for x, y in zip(ra[:4], rc[:4]):
            assert np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y), t
        assert np.array_equal(bits(a.batch.get_state(hbmod.STATE_INTEGRATION)), bits(c.batch.get_state(hbmod.STATE_INTEGRATION))), t
        ended += int((ra[2] | ra[3]).sum())
    assert ended >= n, "no episode ended"
    assert a.foot_contacts().shape == (n, 2) and a.foot_air_time().shape == (n, 2)
    a.close(); c.close()


def _obs_env(hbmod, gpu, n, **kw):
    import ray_cases
    mdl = hbmod.Model.load(ray_cases.HFIELD_HBM)
    xs, ys = [-0.3, 0.0, 0.3], [-0.2, 0.0, 0.2]
    return feet_lib.env(hbmod, gpu, n, feet_lib.feet_options(hbmod, mdl, 2, 1, "torso", observe=1), cmd_lib.CMD, mdl,
                        height_scan=dict(body=1, xs=xs, ys=ys, z0=1.0, cutoff=4.0), obs_extend=dict(prev_action=True, height_scan=dict(offset=1.0, scale=1.0, clip=(-4.0, 4.0))), **kw)


def test_observation_layout_and_flags(hbmod, gpu):
    """observed flags with the last action, a 3 x 3 scan and observed commands in the row: the width, the slices, the flag columns against
    feet() after reset, after every step and from hb_get_obs - which, called twice, returns the same bits and leaves the record alone"""
    n = 64
    a = _obs_env(hbmod, gpu, n)
    L = a.obs_layout()
    want_L, width = feet_ref.layout(NOBS, NU, 9, True, True, 2, True)
    assert L == want_L and a.nobs == a.batch.env_nobs == width == NOBS + NU + 9 + 2 + 3
    o = a.reset()
    assert (o[:, L["foot_contact"]] == 1.0).all() and a.foot_contacts().all()  # after reset every flag is one
    assert np.array_equal(bits(o[:, L["command"]]), bits(a.commands()))
    feet_lib.lift(hbmod, [a])
    rng = np.random.default_rng(4)
    seen = set()
    for t in range(30):
        o = a.step_arrays(cmd_lib.actions(rng, n, NU, 0.6))[0]
        t_last, contact = a.batch.feet()
        assert np.array_equal(o[:, L["foot_contact"]], contact.astype(np.float32)), t
        assert np.array_equal(bits(o[:, -3:]), bits(a.commands())) and L["command"] == slice(width - 3, width), t
        assert np.array_equal(contact.astype(bool), a.foot_contacts())
        seen |= {tuple(r) for r in contact.tolist()}
        if t % 10 == 4:
            g1, g2 = a.batch.obs(want_reward=True), a.batch.obs(want_reward=True)
            assert all(np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y) for x, y in zip(g1, g2))
            assert np.array_equal(g1[0][:, L["foot_contact"]], contact.astype(np.float32))
            t2, c2 = a.batch.feet()
            assert np.array_equal(bits(t2), bits(t_last)) and np.array_equal(c2, contact)
            air = a.foot_air_time()
            assert np.array_equal(bits(air), bits(a.batch.get_state(hbmod.STATE_TIME).reshape(-1, 1) - t_last)) and (air[contact == 1] == 0).all()
    assert {(0, 0), (1, 1)} <= seen and len(seen) >= 3, seen
    a.close()


def test_auto_reset_rows_and_records(hbmod, gpu):
    """auto_reset with the left foot terminal: an episode ends at the touchdown; the terminal-observation row carries the ending state's
    flags, the env's next row ones, and its record the new state's time and a full mask"""
    n = 64
    mdl = feet_lib.model(hbmod)
    a = feet_lib.env(hbmod, gpu, n, feet_lib.feet_options(hbmod, mdl, 2, 0, "foot", observe=1), None, mdl, auto_reset=1)
    col = a.obs_layout()["foot_contact"]
    assert col == slice(NOBS, NOBS + 2) and a.nobs == NOBS + 2
    a.reset()
    feet_lib.lift(hbmod, [a])
    rng = np.random.default_rng(5)
    ends, airborne_ends = 0, 0
    for t in range(40):
        o, r, te, tr, _ = a.step_arrays(cmd_lib.actions(rng, n, NU, 0.6))
        w = a.batch.body_contact()
        c = np.array([[feet_ref.in_contact(a.feet_cfg, w[e, b]) for b in (FOOT_R, FOOT_L)] for e in range(n)])
        assert np.array_equal(te.astype(bool), c[:, 1]) and not tr.any(), t  # (nothing but the left foot ends an episode here)
        done = te.astype(bool)
        t_last, contact = a.batch.feet()
        time = a.batch.get_state(hbmod.STATE_TIME).reshape(-1)
        assert np.array_equal(o[~done][:, col], c[~done].astype(np.float32)) and np.array_equal(contact[~done], c[~done].astype(np.uint8)), t
        if done.any():
            tobs = a.batch.env_terminal_obs()
            assert np.array_equal(tobs[done][:, col], c[done].astype(np.float32)), t
            assert (o[done][:, col] == 1.0).all() and (contact[done] == 1).all(), t
            assert (time[done] == 0.0).all() and np.array_equal(bits(t_last[done]), bits(np.repeat(time[done, None], 2, axis=1))), t
            assert (r[done] == a.cfg.terminal_reward).all()
            ends += int(done.sum())
            airborne_ends += int((~c[done][:, 0]).sum())
    print("\n  %d episodes ended by the left foot's contact, %d of them with the right foot in the air" % (ends, airborne_ends), end="")
    assert ends >= n // 2, ends
    a.close()


def test_collection_replays(hbmod, gpu):
    """collect_torch(T = 8) with a Gaussian actor on the widened row replays bit for bit as step_torch fed the recorded actions: obs
    tapes, rewards, terminated, and the records at the end"""
    import torch
    n, T = 64, 8
    a, c = (_obs_env(hbmod, gpu, n, auto_reset=1, max_time=0.0249) for _ in range(2))
    L = a.obs_layout()
    rng = np.random.default_rng(6)
    net = ([a.nobs, 16, NU], [rng.normal(0.0, 0.3, (a.nobs, 16)).astype(np.float32), rng.normal(0.0, 0.3, (16, NU)).astype(np.float32)],
           [np.zeros(16, np.float32), np.zeros(NU, np.float32)])
    a.actor_set(*net, head="gaussian", log_std=np.full(NU, -1.0, np.float32))
    assert np.array_equal(bits(a.reset()), bits(c.reset()))
    feet_lib.lift(hbmod, [a, c])
    buf = a.collect_torch(T, terminal_obs=True)
    out = {k: v.cpu().numpy() for k, v in buf.items()}
    assert out["obs"].shape == (T + 1, n, a.nobs)
    flags = set()
    for k in range(T):
        o, r, te, tr = c.step_torch(torch.from_numpy(out["action"][k]).to(buf["obs"].device))
        o = o.cpu().numpy()
        assert np.array_equal(bits(o), bits(out["obs"][k + 1])), k
        assert np.array_equal(bits(r.cpu().numpy()), bits(out["reward"][k])), k
        assert np.array_equal(te.cpu().numpy(), out["terminated"][k]) and np.array_equal(tr.cpu().numpy(), out["truncated"][k]), k
        assert np.array_equal(o[:, L["foot_contact"]], c.batch.feet()[1].astype(np.float32)), k
        flags |= {tuple(x) for x in o[:, L["foot_contact"]].tolist()}
    assert (out["terminated"] | out["truncated"]).any() and len(flags) >= 2, flags
    (ta, ca), (tc, cc) = a.batch.feet(), c.batch.feet()
    assert np.array_equal(bits(ta), bits(tc)) and np.array_equal(ca, cc)
    a.close(); c.close()


def test_refusals_on_a_batch(hbmod, gpu):
    """the read-out cannot be switched off under the feet, the width cannot change under an actor, feet() needs a configuration - and a
    refused call changes nothing: the next step gives the bits of an untouched twin"""
    n = 16
    mdl = feet_lib.model(hbmod)
    opts = feet_lib.feet_options(hbmod, mdl, 2, 0, "torso", observe=1)
    a, c = (feet_lib.env(hbmod, gpu, n, opts, None, mdl) for _ in range(2))
    plain = feet_lib.env(hbmod, gpu, n, None, None, mdl)
    with pytest.raises(hbmod.HbError, match="no feet configuration"):
        plain.batch.feet()
    with pytest.raises(RuntimeError, match="feet="):
        plain.foot_contacts()
    rng = np.random.default_rng(7)
    W = lambda i, o: rng.normal(0.0, 0.3, (i, o)).astype(np.float32)
    z = lambda k: np.zeros(k, np.float32)
    plain.actor_set([NOBS, 16, NU], [W(NOBS, 16), W(16, NU)], [z(16), z(NU)], head="gaussian", log_std=z(NU))
    with pytest.raises(hbmod.HbError, match="observation width would change"):
        plain.batch.feet_configure(None, **opts)
    assert plain.batch.env_nobs == NOBS
    plain.batch.feet_configure(None, **dict(opts, observe=0))  # (the width stays: allowed)
    assert plain.batch.env_nobs == NOBS and plain.batch.feet()[1].shape == (n, 2)
    plain.close()
    assert np.array_equal(bits(a.reset()), bits(c.reset()))
    feet_lib.lift(hbmod, [a, c])
    a.actor_set([a.nobs, 16, NU], [W(a.nobs, 16), W(16, NU)], [z(16), z(NU)], head="gaussian", log_std=z(NU))
    before = a.batch.feet()
    with pytest.raises(hbmod.HbError, match="foot-contact terms"):
        a.batch.contact_readout(False)
    for kw in (dict(opts, observe=0), dict(opts, bodies=(FOOT_R,)), None):
        with pytest.raises(hbmod.HbError, match="observation width would change"):
            a.batch.feet_configure(None, **kw) if kw else a.batch.feet_configure(None)
    with pytest.raises(hbmod.HbError, match="contact_threshold"):
        a.batch.feet_configure(None, **dict(opts, contact_threshold=0.0))
    with pytest.raises(hbmod.HbError, match="named twice"):
        a.batch.feet_configure(None, **dict(opts, bodies=(FOOT_R, FOOT_R)))
    assert a.batch.env_nobs == NOBS + 2 and all(np.array_equal(x, y) for x, y in zip(before, a.batch.feet()))
    for t in range(6):
        act = cmd_lib.actions(rng, n, NU, 0.6)
        ra, rc = a.step_arrays(act), c.step_arrays(act)
        for x, y in zip(ra[:4], rc[:4]):
            assert np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y), t
    (ta, ca), (tc, cc) = a.batch.feet(), c.batch.feet()
    assert np.array_equal(bits(ta), bits(tc)) and np.array_equal(ca, cc)
    a.close(); c.close()
