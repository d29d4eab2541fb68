"""The PPO buffer without a GPU: the fp64 reference of tests/gae_ref.py against the definition and closed forms, the layout of the two C
structs against their ctypes mirrors, and the NULL-batch refusals of the two entry points."""
import ctypes
import math
import os
import subprocess

import numpy as np

import actor_ref as ar
import gae_ref as gr
from conftest import ROOT


def _tapes(T, n, seed, p_term=0.09, p_trunc=0.09):
    """random tapes with 15 - 20 % ends per step (terminated, truncated and both); terminal values NaN where the env is not bootstrapped"""
    rng = np.random.default_rng(seed)
    reward = rng.normal(size=(T, n))
    value = rng.normal(size=(T + 1, n)) * 3.0
    te = rng.random((T, n)) < p_term
    tr = rng.random((T, n)) < p_trunc
    tv = np.where(tr & ~te, rng.normal(size=(T, n)) * 3.0, np.nan)
    return reward, value, tv, te, tr


def test_recurrence_equals_the_per_episode_sums():
    for T, n, seed in ((8, 37, 0), (1, 5, 1), (13, 64, 2)):
        reward, value, tv, te, tr = _tapes(T, n, seed)
        frac = (te | tr).mean()
        if T * n > 100:
            assert 0.15 <= frac <= 0.20, frac
        for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0), (0.0, 0.7)):
            for boot in (True, False):
                a, r = gr.gae(reward, value, tv, te, tr, gamma, lam, boot)
                a2, r2 = gr.gae_by_episode(reward, value, tv, te, tr, gamma, lam, boot)
                assert np.isfinite(a).all() and np.isfinite(r).all()
                err = max(np.abs(a - a2).max(), np.abs(r - r2).max())
                print("gae vs per-episode sums: T %d, %d envs, gamma %.2f lam %.2f boot %d: %.2e (bound 1e-12)" % (T, n, gamma, lam, boot, err))
                assert err <= 1e-12


def test_lambda_zero_is_the_td_residual_and_lambda_one_the_discounted_return():
    T, n, gamma = 9, 21, 0.97
    reward, value, tv, te, tr = _tapes(T, n, 3)
    done = te | tr
    rp = gr.shaped_reward(reward, tv, te, tr, gamma)
    a0, _ = gr.gae(reward, value, tv, te, tr, gamma, 0.0)
    assert np.array_equal(a0, rp + gamma * np.where(done, 0.0, value[1:]) - value[:-1])
    # lam = 1: the discounted return of the rest of the episode, bootstrapped with V at the end of the tape, minus value[t]
    a1, r1 = gr.gae(reward, value, tv, te, tr, gamma, 1.0)
    for e in range(n):
        for t in range(T):
            ret, w, k = 0.0, 1.0, t
            while True:
                ret += w * rp[k, e]
                if done[k, e]:
                    break
                w *= gamma
                k += 1
                if k == T:
                    ret += w * value[T, e]
                    break
            assert abs(r1[t, e] - ret) <= 1e-12 and abs(a1[t, e] - (ret - value[t, e])) <= 1e-12


def test_bootstrap_term_appears_exactly_where_truncated_alone():
    T, n, gamma, lam = 6, 40, 0.99, 0.95
    reward, value, tv, te, tr = _tapes(T, n, 4, p_term=0.15, p_trunc=0.3)
    boot = gr.boot_mask(te, tr)
    assert boot.any() and (te & tr).any() and (te & ~tr).any() and np.array_equal(boot, tr & ~te)
    assert not gr.boot_mask(te, tr, False).any()
    rp = gr.shaped_reward(reward, tv, te, tr, gamma)
    assert np.array_equal(rp[~boot], reward[~boot])
    assert np.array_equal(rp[boot], reward[boot] + gamma * tv[boot])
    assert np.array_equal(gr.shaped_reward(reward, tv, te, tr, gamma, False), reward)
    # the TD residual differs by gamma V(terminal_obs) there and nowhere else
    d_on = gr.deltas(reward, value, tv, te, tr, gamma, True)
    d_off = gr.deltas(reward, value, tv, te, tr, gamma, False)
    assert np.array_equal(d_on[~boot], d_off[~boot]) and np.allclose(d_on[boot] - d_off[boot], gamma * tv[boot], rtol=0, atol=1e-14)
    # and the advantage of the steps before a bootstrapped end moves by (gamma lam)^k times that
    a_on, _ = gr.gae(reward, value, tv, te, tr, gamma, lam, True)
    a_off, _ = gr.gae(reward, value, tv, te, tr, gamma, lam, False)
    done = te | tr
    for e in range(n):
        for t in range(T):
            k = t
            while k < T and not done[k, e]:
                k += 1
            want = (gamma * lam) ** (k - t) * gamma * tv[k, e] if k < T and boot[k, e] else 0.0
            assert abs((a_on[t, e] - a_off[t, e]) - want) <= 1e-13


def test_gaussian_log_prob_is_the_normal_log_density_of_the_action():
    rng = np.random.default_rng(5)
    nu = 21
    mean = rng.normal(size=(7, nu)) * 2.0
    ls = np.linspace(-1.5, 0.3, nu)
    eps = rng.normal(size=(7, nu))
    action = ar.head_action(ar.GAUSSIAN, mean, ls, eps)
    sigma = np.exp(ls)
    z = (action - mean) / sigma
    want = (-0.5 * z * z - np.log(sigma) - 0.5 * math.log(2.0 * math.pi)).sum(axis=-1)
    got = gr.log_prob(ar.GAUSSIAN, eps, ls)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_squash_correction():
    x = np.linspace(-8.0, 8.0, 1601)
    want = np.log1p(-np.tanh(x) ** 2)
    got = gr.squash_correction(x)
    # (log1p(-tanh^2) itself loses digits as tanh^2 -> 1: at |x| = 8, 1 - tanh^2 = 4.5e-7 carries 2.5e-10 relative)
    assert np.abs(got - want).max() <= 1e-9
    assert np.abs(got[np.abs(x) <= 2] - want[np.abs(x) <= 2]).max() <= 1e-14
    big = gr.squash_correction(np.array([-25.0, 25.0]))
    assert np.isfinite(big).all() and np.allclose(big, 2.0 * (math.log(2.0) - 25.0), rtol=0, atol=1e-12)
    # the squashed head's log_prob is the Gaussian one minus the correction at x = mean + sigma eps
    rng = np.random.default_rng(6)
    mean, ls, eps = rng.normal(size=(4, 5)), rng.uniform(-2, 1, size=(4, 5)), rng.normal(size=(4, 5))
    xx = mean + np.exp(ls) * eps
    assert np.allclose(gr.log_prob(ar.SQUASHED, eps, ls, mean), gr.log_prob(ar.GAUSSIAN, eps, ls) - gr.squash_correction(xx).sum(axis=-1), rtol=0, atol=1e-13)


def test_values_are_the_linear_top_of_the_network():
    rng = np.random.default_rng(7)
    obs = rng.normal(size=(3, 5, 48))
    ws, bs = ar.make_actor([48, 40, 24, 1], seed=2)
    v = gr.values(obs, ws, bs)
    assert v.shape == (3, 5)
    h = np.tanh(np.tanh(obs @ ws[0].astype(np.float64) + bs[0]) @ ws[1].astype(np.float64) + bs[1])
    assert np.allclose(v, (h @ ws[2].astype(np.float64) + bs[2])[..., 0], rtol=0, atol=1e-14)


def test_ctypes_structs_match_the_header(hbmod, tmp_path):
    """hb_gae_config and hb_gae_out have the size and the field offsets include/hb.h gives them"""
    import humanoid_mujoco_amd.engine as eng
    pairs = [("hb_gae_config", eng.HbGaeConfig), ("hb_gae_out", eng.HbGaeOut)]
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
    rows = [l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines()]
    out = {r[0]: r[1:] for r in rows}
    for cname, cls in pairs:
        assert int(out[cname][0]) == ctypes.sizeof(cls), (cname, out[cname], ctypes.sizeof(cls))
        for fname, _ in cls._fields_:
            assert int(out["%s.%s" % (cname, fname)][0]) == getattr(cls, fname).offset, (cname, fname)
    assert [f for f, _ in eng.HbGaeOut._fields_] == ["value", "terminal_value", "log_prob", "advantage", "returns"]


def test_null_batch_is_refused(hbmod):
    L = hbmod.lib()
    sizes = (ctypes.c_int * 2)(48, 1)
    w, b = np.zeros((48, 1), np.float32), np.zeros(1, np.float32)
    wp, bp = (ctypes.c_void_p * 1)(w.ctypes.data), (ctypes.c_void_p * 1)(b.ctypes.data)
    assert L.hb_critic_set_mlp(None, 1, sizes, wp, bp) == -1
    dummy = ctypes.c_float(0.0)
    out = hbmod.HbGaeOut(value=ctypes.addressof(dummy))
    assert L.hb_collect_gae_dev(None, 1, ctypes.byref(hbmod.HbCollectOut()), ctypes.byref(hbmod.HbGaeConfig(0.99, 0.95, 1)), ctypes.byref(out)) == -1
