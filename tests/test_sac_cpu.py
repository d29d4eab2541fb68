"""The SAC learner without a GPU: the fp64 reference (sac_ref.py) against torch autograd and torch.optim.Adam in float64, its Polyak step and
interval gating, the conditions random_problem has to produce, the replay buffer on the CPU device, the flat record, the ctypes structs
against the header, and the refusals that need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mlp_ref as ml
import sac_ref as sr
from conftest import ROOT
from sac_lib import NETS, problem as _problem

NOBS, NU = 48, 21


@pytest.mark.parametrize("net", sorted(NETS))
def test_reference_losses_and_gradients_equal_autograd(net):
    torch = pytest.importorskip("torch")
    asz, qsz = NETS[net]
    pb = _problem(net, 200)
    cfg = sr.config()
    sel = np.random.default_rng(1).permutation(200)[:120]
    ep, en = pb["eps_pi"][sel], pb["eps_next"][sel]
    st_c, g_c, ex = sr.critic_phase(pb["flat"], pb["targets"], asz, qsz, pb["rows"], sel, ep, en, cfg)
    st_a, g_a, exa = sr.actor_phase(pb["flat"], asz, qsz, pb["rows"], sel, ep, ex["alpha"])
    # no branch can hide: rows with done, raw log_std beyond both clamp bounds, both Q networks the smaller one somewhere
    raw = ex["pi"]["raw"]
    assert pb["rows"]["done"][sel].any() and not pb["rows"]["done"][sel].all()
    assert (raw < -20).mean() > 0.05 and (raw > 2).mean() > 0.03
    assert (exa["q1"] < exa["q2"]).any() and (exa["q2"] < exa["q1"]).any()
    ent, crit, act, leaves = sr.torch_losses(torch, torch.float64, pb["flat"], pb["targets"], asz, qsz, pb["rows"], sel, ep, en, cfg)
    for got, want in ((ent, st_c["ent_coef_loss"]), (crit, st_c["critic_loss"]), (act, st_a["actor_loss"])):
        assert abs(float(got.detach()) - want) <= 1e-12 * max(1.0, abs(want)), (float(got.detach()), want)
    ref = {**g_c, **g_a}
    # SB3 takes each loss's gradient for its own group only
    for loss, group in ((ent, ("log_ent_coef",)), (crit, ("q1", "q2")), (act, ("actor",))):
        names = [k for k in leaves if k.startswith(group)]
        grads = torch.autograd.grad(loss, [leaves[k] for k in names], retain_graph=True)
        for k, g in zip(names, grads):
            g = g.numpy()
            assert np.abs(g - ref[k]).max() <= 1e-10 * np.abs(g).max(), (k, np.abs(g - ref[k]).max(), np.abs(g).max())


def test_tie_of_the_two_q_values_splits_the_gradient():
    """Q1 == Q2 exactly (the same network twice): torch.min's backward sends half to each, and so does the reference"""
    torch = pytest.importorskip("torch")
    asz, qsz = NETS["mixed"]
    pb = _problem("mixed", 200)
    t = sr.split(pb["flat"], asz, qsz)
    for k in list(t):
        if k.startswith("q2"):
            t[k] = t["q1" + k[2:]]
    flat = sr.join(t, asz, qsz)
    sel = np.arange(30)
    ep, en = pb["eps_pi"][sel], pb["eps_next"][sel]
    alpha = float(np.float32(np.exp(t["log_ent_coef"][0])))
    _, g_a, ex = sr.actor_phase(flat, asz, qsz, pb["rows"], sel, ep, alpha)
    assert np.array_equal(ex["q1"], ex["q2"])
    _, _, act, leaves = sr.torch_losses(torch, torch.float64, flat, pb["targets"], asz, qsz, pb["rows"], sel, ep, en, sr.config())
    names = [k for k in leaves if k.startswith("actor")]
    for k, g in zip(names, torch.autograd.grad(act, [leaves[k] for k in names])):
        assert np.abs(g.numpy() - g_a[k]).max() <= 1e-10 * np.abs(g.numpy()).max(), k


def test_reference_adam_equals_torch_adam_per_group():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(11)
    cfg = sr.config(lr_actor=1e-2, lr_critic=3e-3, lr_ent=2e-2)
    for lr in (cfg["lr_actor"], cfg["lr_critic"], cfg["lr_ent"]):
        p0 = rng.normal(size=200)
        leaf = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
        opt = torch.optim.Adam([leaf], lr=lr, betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"])
        p, m, v = p0.copy(), np.zeros(200), np.zeros(200)
        for t in range(1, 4):
            g = rng.normal(size=200)
            leaf.grad = torch.tensor(g.copy())
            opt.step()
            p, m, v = ml.adam(p, m, v, t, g, lr, cfg)
            assert np.abs(leaf.detach().numpy() - p).max() <= 1e-12 * np.abs(p).max()


def test_polyak_and_the_update_interval():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    q, tg = rng.normal(size=50), rng.normal(size=50)
    tq, tt = torch.tensor(q), torch.tensor(tg.copy())
    tt.mul_(1 - 0.005)
    torch.add(tt, tq, alpha=0.005, out=tt)  # (stable-baselines3's polyak_update)
    assert np.abs(tt.numpy() - sr.polyak(q, tg, 0.005)).max() <= 1e-15
    assert [sr.polyak_due(t, sr.config(target_update_interval=3)) for t in range(1, 8)] == [False, False, True, False, False, True, False]
    assert all(sr.polyak_due(t, sr.config()) for t in range(1, 5))
    # a whole step: the targets move on the due steps only, log_ent_coef only with auto_ent
    asz, qsz = NETS["one_layer"]
    pb = _problem("one_layer", 200)
    lo, hi = sr.q_range(asz, qsz)
    n = pb["flat"].size
    sel = np.arange(40)
    for interval, auto in ((2, 1), (1, 0)):
        cfg = sr.config(target_update_interval=interval, auto_ent=auto, lr_critic=1e-2)
        st = dict(params=pb["flat"], m=np.zeros(n), v=np.zeros(n), targets=pb["targets"], t=0)
        s1, stats, g = sr.step(st, asz, qsz, pb["rows"], sel, pb["eps_pi"][sel], pb["eps_next"][sel], cfg)
        assert s1["t"] == 1 and np.array_equal(s1["targets"], pb["targets"]) == (interval == 2)
        assert (s1["params"][-1] == pb["flat"][-1]) == (auto == 0) and g[-1] != 0.0
        if interval == 1:
            assert np.allclose(s1["targets"], 0.005 * s1["params"][lo:hi] + 0.995 * pb["targets"], rtol=0, atol=1e-15)
        s2, _, _ = sr.step(s1, asz, qsz, pb["rows"], sel, pb["eps_pi"][sel], pb["eps_next"][sel], cfg)
        assert s2["t"] == 2 and not np.array_equal(s2["targets"], s1["targets"])
        assert np.abs(s1["params"][lo:hi] - pb["flat"][lo:hi]).max() > 1e-3 and np.abs(s1["params"][:lo] - pb["flat"][:lo]).max() > 1e-5
        assert set(stats) == set(sr.STATS)


@pytest.mark.parametrize("net", sorted(NETS))
def test_random_problem_meets_its_conditions(net):
    """what the GPU tests rely on: rows with done = 1, raw log_std beyond both clamp bounds, at most 1 % of the rows rejected, and both
    margins kept by every row that stays"""
    asz, qsz = NETS[net]
    La, Lq = len(asz) - 1, len(qsz) - 1
    for n_rows in (200, 4112) if net == "small" else (200,):
        pb = _problem(net, n_rows)
        assert pb["rejected"] <= 0.01 * n_rows, pb["rejected"]
        t = sr.split(pb["flat"], asz, qsz)
        rows = pb["rows"]
        assert rows["done"].any() and not rows["done"].all() and rows["done"].dtype == np.uint8
        pi = sr.head(t, La, rows["obs"], pb["eps_pi"])
        raw = pi["raw"]
        # both clamp branches carry a good share of the entries: about 9 % below -20; 5 to 15 % above 2 behind a tanh layer, and up to a
        # quarter for the one-layer net, whose raw log_std sees the observations themselves
        lo_share, hi_share = (raw < -20).mean(), (raw > 2).mean()
        print("\n  %s, %d rows: raw log_std below -20 %.3f, above 2 %.3f, rejected rows %d" % (net, n_rows, lo_share, hi_share, pb["rejected"]))
        assert 0.07 <= lo_share <= 0.12 and 0.05 <= hi_share <= (0.25 if net == "one_layer" else 0.15), (lo_share, hi_share)
        assert np.minimum(np.abs(raw + 20), np.abs(raw - 2)).min() >= 1e-3
        xin = np.concatenate([rows["obs"].astype(np.float64), pi["a"]], axis=1)
        q1, q2 = ml.forward(t, "q1", Lq, xin)[1], ml.forward(t, "q2", Lq, xin)[1]
        assert np.abs(q1 - q2).min() >= 1e-4 * max(np.abs(q1).max(), np.abs(q2).max())


@pytest.mark.parametrize("net", sorted(NETS))
def test_forward_error_bounds_leave_a_quarter_of_the_margins(net):
    """Each net's derived float32 forward-error bound (the layer recurrence of mlp_ref.fwd_err on exact input rows)
    is below a quarter of the margin random_problem keeps on its output: 1e-3 on the actor's raw log_std, 1e-4 max|Q| on Q1 and on Q2 at
    (obs, a_pi).  The recurrence is a worst-case sum; what the kernels lose is 0.001 to 0.01 of it (profiles/sac_parity.txt)."""
    asz, qsz = NETS[net]
    La, Lq = len(asz) - 1, len(qsz) - 1
    for n_rows in (200, 4112) if net == "small" else (200,):
        pb = _problem(net, n_rows)
        t = sr.split(pb["flat"], asz, qsz)
        rows = pb["rows"]
        pi = sr.head(t, La, rows["obs"], pb["eps_pi"])
        xin = np.concatenate([rows["obs"].astype(np.float64), pi["a"]], axis=1)
        acts1, q1, _ = ml.forward(t, "q1", Lq, xin)
        acts2, q2, _ = ml.forward(t, "q2", Lq, xin)
        qmax = max(np.abs(q1).max(), np.abs(q2).max())
        e_ls = ml.fwd_err(t, "actor", La, pi["acts"])[0][:, NU:].max()
        e_q = max(ml.fwd_err(t, "q1", Lq, acts1)[0].max(), ml.fwd_err(t, "q2", Lq, acts2)[0].max())
        print("\n  %s, %d rows: log_std bound %.2e of 2.5e-4, Q bound %.2e of %.2e" % (net, n_rows, e_ls, e_q, 0.25e-4 * qmax))
        assert e_ls < 0.25 * 1e-3, e_ls
        assert e_q < 0.25 * 1e-4 * qmax, (e_q, qmax)


def test_flat_layout_round_trips_through_the_split(hbmod):
    import humanoid_mujoco_amd.engine as eng
    for asz, qsz in NETS.values():
        n = sum(int(np.prod(sh)) for _, sh in sr.flat_shapes(asz, qsz))
        flat = np.arange(n, dtype=np.float32)
        assert eng.sac_flat_shapes(asz, qsz) == sr.flat_shapes(asz, qsz)
        t = eng.sac_split(flat, asz, qsz)
        assert list(t) == [k for k, _ in sr.flat_shapes(asz, qsz)]
        assert t["actor.w0"].shape == (48, asz[1]) and t["actor.w0"][1, 0] == asz[1] and t["log_ent_coef"][0] == n - 1
        lo, hi = sr.q_range(asz, qsz)
        assert t["q1.w0"][0, 0] == lo and hi == n - 1 and t["q1.w0"].shape == (69, qsz[1])
        assert np.array_equal(eng.sac_join(t, asz, qsz), flat)
        with pytest.raises(ValueError):
            eng.sac_split(flat[:-1], asz, qsz)


def test_replay_buffer_on_the_cpu_device(hbmod):
    torch = pytest.importorskip("torch")
    nobs, nu, T, n = 5, 2, 3, 4
    rng = np.random.default_rng(0)

    def tapes(base):
        obs = torch.tensor(base + rng.normal(size=(T + 1, n, nobs)).astype(np.float32))
        te = torch.zeros((T, n), dtype=torch.bool)
        tr = torch.zeros((T, n), dtype=torch.bool)
        te[0, 1] = True                 # terminated: done, next_obs = terminal_obs
        tr[1, 2] = True                 # truncated alone: NOT done, next_obs = terminal_obs
        te[2, 3] = tr[2, 3] = True      # both: done
        return dict(obs=obs, action=torch.tensor(rng.normal(size=(T, n, nu)).astype(np.float32)), reward=torch.tensor(rng.normal(size=(T, n)).astype(np.float32)),
                    terminated=te, truncated=tr, terminal_obs=torch.tensor(100.0 + rng.normal(size=(T, n, nobs)).astype(np.float32)))
    rb = hbmod.ReplayBuffer(30, nobs, nu, "cpu")
    with pytest.raises(RuntimeError):
        rb.sample_index(4)
    a = tapes(0.0)
    rb.add(a)
    assert rb.size == 12 and rb.pos == 12
    for t in range(T):
        for e in range(n):
            r = t * n + e  # the (t, e) order
            assert torch.equal(rb.obs[r], a["obs"][t, e]) and torch.equal(rb.action[r], a["action"][t, e]) and rb.reward[r] == a["reward"][t, e]
            ended = bool(a["terminated"][t, e] | a["truncated"][t, e])
            assert torch.equal(rb.next_obs[r], a["terminal_obs"][t, e] if ended else a["obs"][t + 1, e])
            assert int(rb.done[r]) == int(a["terminated"][t, e])
    assert rb.done.dtype == torch.uint8 and int(rb.done[:12].sum()) == 2 and int(rb.done[1 * n + 2]) == 0
    g = torch.Generator().manual_seed(1)
    idx = rb.sample_index(500, g)
    assert idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) == 11 and len(torch.unique(idx)) == 12
    assert torch.equal(idx, rb.sample_index(500, torch.Generator().manual_seed(1)))
    # wrap-around: 12 + 12 + 12 rows into 30 slots
    b, c = tapes(10.0), tapes(20.0)
    rb.add(b)
    rb.add(c)
    assert rb.size == 30 and rb.pos == 6
    assert torch.equal(rb.obs[:6], c["obs"][:T].reshape(12, nobs)[6:]) and torch.equal(rb.obs[24:], c["obs"][:T].reshape(12, nobs)[:6])
    assert torch.equal(rb.obs[12:24], b["obs"][:T].reshape(12, nobs)) and torch.equal(rb.obs[6:12], a["obs"][:T].reshape(12, nobs)[6:])
    assert int(rb.sample_index(2000, g).max()) == 29
    # more rows than the capacity in one call: the last `capacity` stay
    small = hbmod.ReplayBuffer(5, nobs, nu, "cpu")
    small.add(a)
    assert small.size == 5 and small.pos == 12 % 5
    flat = a["obs"][:T].reshape(12, nobs)
    for r in range(7, 12):
        assert torch.equal(small.obs[r % 5], flat[r])
    with pytest.raises(ValueError):
        rb.add({k: v for k, v in a.items() if k != "terminal_obs"})


def test_ctypes_structs_match_the_header(hbmod, tmp_path):
    """hb_sac_config and hb_sac_rows have the size and the field offsets include/hb.h gives them"""
    import humanoid_mujoco_amd.engine as eng
    pairs = [("hb_sac_config", eng.HbSacConfig), ("hb_sac_rows", eng.HbSacRows)]
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


def test_defaults_and_null_batch_refusals(hbmod):
    import humanoid_mujoco_amd.engine as eng
    L = hbmod.lib()
    c = eng.HbSacConfig()
    assert L.hb_sac_default_config(ctypes.byref(c)) == 0 and L.hb_sac_default_config(None) == -1
    got = {k: getattr(c, k) for k, _ in eng.HbSacConfig._fields_}
    ints = ("auto_ent", "target_entropy_auto", "target_update_interval", "seed")
    assert got == {k: (v if k in ints else np.float32(v)) for k, v in sr.DEFAULTS.items()}, got
    assert eng.SAC_STATS == sr.STATS
    rows = eng.HbSacRows()
    buf = np.zeros(4, np.float32)
    t = ctypes.c_longlong()
    sizes = (ctypes.c_int * 2)(69, 1)
    wp, bp = (ctypes.c_void_p * 1)(buf.ctypes.data), (ctypes.c_void_p * 1)(buf.ctypes.data)
    assert L.hb_q_set_mlp(None, 0, 1, sizes, wp, bp) == -1
    assert L.hb_q_values_dev(None, buf.ctypes.data, buf.ctypes.data, 1, buf.ctypes.data, None) == -1
    assert L.hb_sac_create(None, ctypes.byref(c)) == -1 and L.hb_sac_configure(None, ctypes.byref(c)) == -1 and L.hb_sac_destroy(None) == -1
    assert L.hb_sac_param_count(None) == -1 and L.hb_sac_target_count(None) == -1
    assert L.hb_sac_get_params(None, buf.ctypes.data, 4) == -1 and L.hb_sac_set_params(None, buf.ctypes.data, 4) == -1
    assert L.hb_sac_get_grads(None, buf.ctypes.data, 4) == -1
    assert L.hb_sac_get_state(None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 4, buf.ctypes.data, 4, ctypes.byref(t)) == -1
    assert L.hb_sac_set_state(None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 4, buf.ctypes.data, 4, 0) == -1
    assert L.hb_sac_step_dev(None, ctypes.byref(rows), None) == -1
