"""The normaliser without a GPU: the fp64 reference of tests/norm_ref.py against closed forms (what the GPU tests compare the device
with), the host merge of two ranks' records, and the C structs and symbols of include/hb.h against their ctypes mirrors."""
import ctypes
import os
import subprocess

import numpy as np

import norm_ref as nr
from conftest import ROOT

NOBS = 7
SYMBOLS = ("hb_norm_default_config", "hb_norm_configure", "hb_norm_get_stats", "hb_norm_set_stats", "hb_norm_get_env", "hb_norm_episode_totals",
           "hb_norm_step_dev", "hb_norm_reset_dev", "hb_norm_obs_dev", "hb_env_collect_norm_dev")


def _with_prior(x):
    """np.mean / np.var of the rows x with the prior folded in: a pseudo-batch of weight 1e-4 with mean 0 and variance 1"""
    w, n = 1e-4, x.shape[0]
    mean = x.sum(axis=0) / (w + n)
    var = (w * (1.0 + mean ** 2) + ((x - mean) ** 2).sum(axis=0)) / (w + n)
    return mean, var


def test_updates_equal_the_moments_of_the_concatenation():
    rng = np.random.default_rng(0)
    rms = nr.RunningMeanStd((NOBS,))
    batches = [rng.normal(loc=rng.uniform(-3, 3, NOBS), scale=rng.uniform(0.1, 4, NOBS), size=(n, NOBS)) for n in (1, 37, 64, 5, 200, 13)]
    for x in batches:
        rms.update(x)
    allx = np.concatenate(batches)
    mean, var = _with_prior(allx)
    assert rms.count == 1e-4 + len(allx)
    np.testing.assert_allclose(rms.mean, mean, rtol=0, atol=1e-12)
    np.testing.assert_allclose(rms.var, var, rtol=1e-12, atol=1e-12)
    # (and without the prior's weight the plain moments, to the prior's weight)
    np.testing.assert_allclose(rms.mean, allx.mean(axis=0), atol=1e-4 * np.abs(allx.mean(axis=0)).max())


def test_host_merge_of_two_ranks_equals_the_single_batch():
    rng = np.random.default_rng(1)
    nobs, K = 5, 4
    obs = rng.normal(2.0, 3.0, size=(K, 64, nobs)).astype(np.float32)
    rew = rng.normal(size=(K, 64)).astype(np.float32)
    done = rng.random((K, 64)) < 0.2
    one, a, b = nr.NormRef(64, nobs), nr.NormRef(37, nobs), nr.NormRef(27, nobs)
    for t in range(K):
        one.step(obs[t], rew[t], done[t], np.zeros(64, bool))
        a.step(obs[t, :37], rew[t, :37], done[t, :37], np.zeros(37, bool))
        b.step(obs[t, 37:], rew[t, 37:], done[t, 37:], np.zeros(27, bool))
    merged = nr.merge_records(a.record(), b.record(), nobs)
    # both ranks started from the prior (count 1e-4, mean 0, var 1), the single batch holds it once: the merged record carries it twice,
    # a pseudo-row of weight w = 1e-4 among N = 64 K rows moves a mean by at most w / N (|mean| + 0) and a variance by at most
    # w / N (1 + mean^2 + var) (its own variance 1 and its distance from the mean), to first order in w / N: twice that as the bound
    ref = one.record()
    assert abs(merged[2 * nobs] - ref[2 * nobs] - 1e-4) < 1e-9
    w_n = 1e-4 / (64 * K)
    for m, v in ((slice(0, nobs), slice(nobs, 2 * nobs)), (slice(2 * nobs + 1, 2 * nobs + 2), slice(2 * nobs + 2, 2 * nobs + 3))):
        assert np.all(np.abs(merged[m] - ref[m]) <= 2 * w_n * np.abs(ref[m]))
        assert np.all(np.abs(merged[v] - ref[v]) <= 2 * w_n * (1 + ref[m] ** 2 + ref[v]))
    # with the prior removed from one rank (a rank that starts from count 0 is exact): the update formula is associative to rounding
    x, y = rng.normal(size=(37, nobs)), rng.normal(1.0, 2.0, size=(27, nobs))
    r1 = nr.RunningMeanStd((nobs,)); r1.update(x)
    r2 = nr.RunningMeanStd((nobs,)); r2.count = 0.0; r2.update(y)
    r1.update_from_moments(r2.mean, r2.var, r2.count)
    r3 = nr.RunningMeanStd((nobs,)); r3.update(np.concatenate([x, y]))
    np.testing.assert_allclose(r1.mean, r3.mean, atol=1e-13)
    np.testing.assert_allclose(r1.var, r3.var, rtol=1e-13)


def test_discounted_return_and_monitor_follow_the_episodes():
    rng = np.random.default_rng(2)
    n, K, gamma = 6, 40, 0.9
    ref = nr.NormRef(n, 3, gamma=gamma)
    g = float(np.float32(gamma))
    rew = rng.normal(size=(K, n)).astype(np.float32)
    done = rng.random((K, n)) < 0.15
    done[:, 0] = False          # env 0 never ends
    done[:, 1] = True           # env 1 ends every step
    start = np.zeros(n, int)
    n_ep, sum_r, sum_r2, sum_l = 0, 0.0, 0.0, 0
    for t in range(K):
        ret_before_reset = ref.ret * g + rew[t].astype(np.float64)
        out = ref.step(np.zeros((n, 3), np.float32), rew[t], done[t], np.zeros(n, bool))
        for e in range(n):
            seg = rew[start[e]:t + 1, e].astype(np.float64)
            disc = sum(r * g ** (len(seg) - 1 - i) for i, r in enumerate(seg))  # the episode's discounted sum so far
            assert abs(ret_before_reset[e] - disc) < 1e-12
            if done[t, e]:
                assert out["ep_length"][e] == len(seg) and out["ep_return"][e] == np.float32(seg.sum())
                n_ep += 1; sum_r += seg.sum(); sum_r2 += seg.sum() ** 2; sum_l += len(seg)
                start[e] = t + 1
                assert ref.ret[e] == 0.0 and ref.ep_ret[e] == 0.0 and ref.ep_len[e] == 0
            else:
                assert out["ep_length"][e] == 0 and out["ep_return"][e] == 0.0
    np.testing.assert_allclose(ref.totals, [n_ep, sum_r, sum_r2, sum_l], rtol=1e-12, atol=1e-12)


def test_clipping_returns_the_clip_and_a_constant_column_gives_zero():
    rng = np.random.default_rng(3)
    ref = nr.NormRef(32, 4, clip_obs=2.5, clip_reward=1.5)
    obs = rng.normal(size=(32, 4)).astype(np.float32)
    obs[:, 1] = 0.75                 # constant: its variance decays to the prior's share and (x - mean) is 0 to the prior's weight
    obs[0, 0], obs[1, 0] = 1e4, -1e4
    rew = rng.normal(size=32).astype(np.float32)
    rew[0], rew[1] = 1e6, -1e6
    out = ref.step(obs, rew, np.zeros(32, bool), np.zeros(32, bool))
    assert out["obs"][0, 0] == np.float32(2.5) and out["obs"][1, 0] == np.float32(-2.5)
    assert out["reward"][0] == np.float32(1.5) and out["reward"][1] == np.float32(-1.5)
    assert np.abs(out["obs"]).max() <= 2.5 and np.abs(out["reward"]).max() <= 1.5
    # without the prior the constant column is exactly 0; with it, 0.75 (1e-4 / 32) / sqrt(var) - of the order of 1e-4
    assert np.abs(out["obs"][:, 1]).max() < 2e-3
    rms = nr.RunningMeanStd((4,)); rms.count = 0.0; rms.update(obs)
    assert rms.var[1] == 0.0 and rms.mean[1] == 0.75
    ref2 = nr.NormRef(32, 4, training=False)
    ref2.obs_rms = rms
    assert np.all(ref2.normalize_obs(obs)[:, 1] == 0.0)


def test_frozen_statistics_and_switches():
    rng = np.random.default_rng(4)
    ref = nr.NormRef(8, 3)
    obs, rew = rng.normal(size=(8, 3)).astype(np.float32), rng.normal(size=8).astype(np.float32)
    ref.step(obs, rew, np.zeros(8, bool), np.zeros(8, bool))
    rec = ref.record()
    ref.training = False
    out = ref.step(obs * 3, rew, np.ones(8, bool), np.zeros(8, bool))
    assert np.array_equal(ref.record(), rec) and ref.totals[0] == 8 and np.all(out["ep_length"] == 2)
    off = nr.NormRef(8, 3, norm_obs=False, norm_reward=False)
    out = off.step(obs, rew, np.zeros(8, bool), np.zeros(8, bool))
    assert np.array_equal(out["obs"], obs) and np.array_equal(out["reward"], rew)
    assert off.ret_rms.count == 8 + 1e-4 and off.obs_rms.count == 1e-4  # (ret_rms is updated whether or not norm_reward is set)


def test_ctypes_structs_match_the_header(hbmod, tmp_path):
    """hb_norm_config, hb_norm_io and hb_norm_tapes have the size and the field offsets include/hb.h gives them (the pattern of
    tests/test_actor_cpu.py; the header compiles as C99)"""
    import humanoid_mujoco_amd.engine as eng
    pairs = [("hb_norm_config", eng.HbNormConfig), ("hb_norm_io", eng.HbNormIo), ("hb_norm_tapes", eng.HbNormTapes)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hb.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = {r[0]: r[1:] for r in (l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())}
    for cname, cls in pairs:
        assert int(out[cname][0]) == ctypes.sizeof(cls), (cname, out[cname], ctypes.sizeof(cls))
        for fname, _ in cls._fields_:
            assert int(out["%s.%s" % (cname, fname)][0]) == getattr(cls, fname).offset, (cname, fname)


def test_library_exports_the_symbols_and_the_defaults(hbmod):
    import humanoid_mujoco_amd.engine as eng
    L = ctypes.CDLL(eng.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(L, s), s
    cfg = eng.HbNormConfig()
    assert hbmod.lib().hb_norm_default_config(ctypes.byref(cfg)) == 0
    d = nr.DEFAULTS
    assert (cfg.norm_obs, cfg.norm_reward, cfg.training) == (1, 1, 1)
    assert (cfg.clip_obs, cfg.clip_reward) == (d["clip_obs"], d["clip_reward"])
    assert cfg.gamma == np.float32(d["gamma"]) and cfg.epsilon == np.float32(d["epsilon"])
    assert hbmod.lib().hb_norm_default_config(None) == -1
    header = open(os.path.join(ROOT, "include", "hb.h")).read()
    for s in SYMBOLS:
        assert s + "(" in header, s
