"""The layout of an observation row of the env adapter on the GPU (include/hb.h: hb_env_row): for every combination of
the four optional parts, hb_env_row, hb_env_nobs and VecEnv.obs_layout() against the order written out here, and every part of the rows
the env kernel writes against its own source.

Model: humanoid27_hfield.hbm (48 observations, 21 actuators).  17 envs: the env kernel serves 16 envs per block, so one full block and one
part-filled one.  A 2 x 2 height scan, no realism layer, no reset perturbation: every env starts in the reset pose, whose feet hang 4 mm
above the floor; the even envs are lowered 1 cm (their feet press into the floor) and the odd ones lifted 5 cm, so that contact flags of
both values occur.  Commands and feet are installed in every combination; `observe` is what varies.

Bounds - none of them new:
  bits   the last action against the action, the command against commands(), the flags against hb_env_get_feet, the scan against the
         float32 transform (tests/obs_ext_ref.py) of Batch.rays() at the same state: equality;
  base   tests/env_ref.py's observation of the device's own state: tests/test_gpu_env.py's atol = 1e-5 for that comparison after a step.
"""
import itertools

import numpy as np
import pytest

import cmd_lib
import obs_ext_ref
from cmd_lib import bits
from env_ref import obs_from_state
from oracle_lib import HFIELD_HBM

pytestmark = pytest.mark.gpu

NOBS, NU, N = 48, 21, 17
XS, YS, Z0, CUTOFF = [-0.2, 0.2], [-0.15, 0.15], 1.0, 4.0
HS = dict(offset=1.0, scale=2.0, clip=(-4.0, 5.0))
BASE_ATOL = 1e-5  # tests/test_gpu_env.py
COMBOS = list(itertools.product((False, True), repeat=4))


def _env(hbmod, gpu, act, scan, feet, cmd, **kw):
    mdl = hbmod.Model.load(HFIELD_HBM)
    ext = dict(prev_action=act)
    if scan:
        ext["height_scan"] = HS
    kw.setdefault("target_z", 10.0)  # (out of reach: standing ends no episode)
    kw.setdefault("max_time", 0.0)
    return hbmod.VecEnv(mdl, N, gpu, seed=7, randomization_factor=0.0, height_scan=dict(body=1, xs=XS, ys=YS, z0=Z0, cutoff=CUTOFF),
                        obs_extend=ext if act or scan else None, commands=dict(cmd_lib.CMD, observe=int(cmd)),
                        feet=dict(bodies=("foot_right", "foot_left"), observe=int(feet)), **kw)


def _want_layout(act, scan, feet, cmd):
    """the order base | last action | scan | foot flags | command, written out: {part: (offset, count)} and the width"""
    parts, at = {"base": (0, NOBS)}, NOBS
    for name, count in (("prev_action", NU if act else 0), ("scan", len(XS) * len(YS) if scan else 0), ("foot_contact", 2 if feet else 0), ("command", 3 if cmd else 0)):
        parts[name] = (at, count)
        at += count
    return parts, at


def _check_layout(env, combo):
    parts, width = _want_layout(*combo)
    row = env.batch.env_row()
    assert row.base == NOBS and row.width == width == env.batch.env_nobs == env.nobs
    for name in ("prev_action", "scan", "foot_contact", "command"):
        assert (getattr(row, name), getattr(row, "n_" + name)) == parts[name], (name, combo)
    key = {"scan": "height_scan"}
    want = {key.get(name, name): slice(at, at + count) for name, (at, count) in parts.items() if count}
    assert env.obs_layout() == want, combo
    return want


def _check_row(hbmod, env, L, o, act, combo, what):
    """one table of rows against the state, the records and the rays the env has now"""
    st = env.batch.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
    nq, nv = env.model.nq, env.model.nv
    for e in range(N):
        ref, _ = obs_from_state(st[e, 1:1 + nq], st[e, 1 + nq:1 + nq + nv])
        assert np.allclose(o[e, L["base"]], ref, atol=BASE_ATOL), (what, combo, e)
    if "prev_action" in L:
        assert np.array_equal(bits(o[:, L["prev_action"]]), bits(act)), (what, combo)
    if "height_scan" in L:
        dist, gid = env.batch.rays()
        assert np.array_equal(bits(o[:, L["height_scan"]]), bits(obs_ext_ref.scan_entries(dist, gid, CUTOFF, **HS))), (what, combo)
    if "foot_contact" in L:
        assert np.array_equal(bits(o[:, L["foot_contact"]]), bits(env.batch.feet()[1].astype(np.float32))), (what, combo)
    if "command" in L:
        assert np.array_equal(bits(o[:, L["command"]]), bits(env.commands())), (what, combo)


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "act%d-scan%d-feet%d-cmd%d" % tuple(map(int, c)))
def test_layout_and_parts(hbmod, gpu, combo):
    """hb_env_row, hb_env_nobs and obs_layout() agree with the order written out here; after each of two steps with random actions every
    part of every row holds what its source holds"""
    env = _env(hbmod, gpu, *combo)
    L = _check_layout(env, combo)
    o = env.reset()
    assert o.shape == (N, env.nobs)
    _check_row(hbmod, env, L, o, np.zeros((N, NU), np.float32), combo, "reset")
    st = env.batch.get_state(hbmod.STATE_INTEGRATION)
    st[0::2, 1 + 2] -= np.float32(0.01)
    st[1::2, 1 + 2] += np.float32(0.05)
    env.batch.set_state(hbmod.STATE_INTEGRATION, st)
    rng = np.random.default_rng(11)
    flags = set()
    for t in range(2):
        act = cmd_lib.actions(rng, N, NU, 0.6)
        o, _, term, trunc, _ = env.step_arrays(act)
        assert not (term | trunc).any()
        _check_row(hbmod, env, L, o, act, combo, "step %d" % t)
        flags |= set(env.batch.feet()[1].ravel().tolist())
    assert flags == {0, 1}, flags  # (the lowered envs touch the floor, the lifted ones do not)
    env.close()


def test_terminal_rows(hbmod, gpu):
    """every part on and max_time below one control step: every env ends at its first step.  The terminal rows follow the same layout with
    the action just applied and the old command; the new rows hold a zero last action, the new command, every flag set, and the scan and
    the base observation of the new state"""
    combo = (True, True, True, True)
    env = _env(hbmod, gpu, *combo, max_time=0.001)
    L = _check_layout(env, combo)
    env.reset()
    old_cmd = env.commands()
    act = cmd_lib.actions(np.random.default_rng(12), N, NU, 0.6)
    o, _, term, trunc, _ = env.step_arrays(act)
    assert term.all()
    tobs = env.batch.env_terminal_obs()
    assert tobs.shape == o.shape == (N, env.nobs)
    assert np.array_equal(bits(tobs[:, L["prev_action"]]), bits(act))
    assert np.array_equal(bits(tobs[:, L["command"]]), bits(old_cmd))
    assert np.isin(tobs[:, L["foot_contact"]], (0.0, 1.0)).all()
    new_cmd = env.commands()
    assert (bits(new_cmd) != bits(old_cmd)).any(axis=1).sum() >= N // 2  # (draw 0 of episode 1 against draw 0 of episode 0)
    assert (env.batch.feet()[1] == 1).all()
    _check_row(hbmod, env, L, o, np.zeros((N, NU), np.float32), combo, "new episode")
    env.close()
