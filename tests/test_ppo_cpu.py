"""The PPO learner without a GPU: the fp64 reference (ppo_ref.py) against torch autograd and torch.optim.Adam in float64, the tie rule of
the clipped surrogate, the flat record, the ctypes structs against the header, and the refusals that need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ppo_ref as pr
from conftest import ROOT

NETS = {"three_layers": ([48, 20, 33, 21], [48, 20, 33, 1]), "one_layer": ([48, 21], [48, 1])}


def _torch_loss(torch, flat, asz, csz, rows, cfg, sel):
    return pr.torch_loss(torch, torch.float64, flat, asz, csz, rows, cfg, sel)


@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("net", sorted(NETS))
def test_reference_gradients_equal_autograd(net, normalize):
    torch = pytest.importorskip("torch")
    asz, csz = NETS[net]
    flat, rows = pr.random_problem(asz, csz, 70, seed=3)
    cfg = pr.config(normalize_advantage=normalize, ent_coef=0.01)
    sel = np.random.default_rng(1).permutation(70)[:50]
    stats, g, _ = pr.loss_and_grads(flat, asz, csz, rows, cfg, index=sel)
    # the clip branch cannot hide: a good share of the rows on either side of it
    assert 0.2 <= stats["clip_fraction"] <= 0.8, stats["clip_fraction"]
    loss, leaves, parts = _torch_loss(torch, flat, asz, csz, rows, cfg, sel)
    loss.backward()
    for k, v in parts.items():
        v = v.detach()
        assert abs(float(v) - stats[k]) <= 1e-12 * max(1.0, abs(stats[k])), (k, float(v), stats[k])
    ref = pr.split(g, asz, csz, asz[-1])
    for k, leaf in leaves.items():
        got = leaf.grad.numpy()
        assert np.abs(got - ref[k]).max() <= 1e-12 * np.abs(got).max(), (k, np.abs(got - ref[k]).max(), np.abs(got).max())


def test_tie_rule_at_the_clip_boundary_and_at_zero_advantage():
    """ratio == 1 + c exactly carries the gradient (the bounds are inside); adv == 0 carries none - as autograd's min over clamp"""
    torch = pytest.importorskip("torch")
    asz, csz = NETS["one_layer"]
    flat, rows = pr.random_problem(asz, csz, 6, seed=5)
    sel = np.arange(6)
    _, _, ex = pr.loss_and_grads(flat, asz, csz, rows, pr.config(normalize_advantage=0), index=sel)
    rows = dict(rows)
    old = ex["lp"].copy()
    # row 0 stands exactly on the upper bound: c is taken from the ratio, c = exp(d) - 1, which is exact for a ratio in [1, 2), and so
    # is 1 + c.  d is one where numpy's and torch's exp agree to the last bit, so that both see the tie.
    for shift in np.arange(0.2, 0.3, 0.001):
        d0 = ex["lp"][0] - (ex["lp"][0] - shift)
        if np.exp(d0) == float(torch.exp(torch.tensor(d0, dtype=torch.float64))):
            break
    else:
        raise AssertionError("no common value of exp")
    old[0] = ex["lp"][0] - shift
    c = float(np.exp(d0) - 1.0)
    assert 1.0 + c == np.exp(d0)
    old[2] = ex["lp"][2] - np.log(1.5)
    old[3] = ex["lp"][3] - np.log(1.5)
    rows["old_log_prob"] = old
    adv = np.array([1.0, -1.0, 2.0, -2.0, 0.0, 0.0])
    rows["advantage"] = adv
    cfg = pr.config(normalize_advantage=0, clip_range=c)
    stats, g, ex = pr.loss_and_grads(flat, asz, csz, rows, cfg, index=sel)
    assert ex["ratio"][0] == 1.0 + c and ex["ratio"][1] == 1.0
    assert ex["glp"][0] == -adv[0] * (1.0 + c) / 6 and ex["glp"][1] == -adv[1] / 6      # on the bound: inside
    assert ex["glp"][2] == 0.0 and ex["glp"][3] != 0.0                                   # ratio 1.5: clipped for A > 0, not for A < 0
    assert ex["glp"][4] == 0.0 and ex["glp"][5] == 0.0                                   # A == 0
    loss, leaves, _ = _torch_loss(torch, flat, asz, csz, rows, cfg, sel)
    loss.backward()
    ref = pr.split(g, asz, csz, asz[-1])
    for k, leaf in leaves.items():
        got = leaf.grad.numpy()
        assert np.abs(got - ref[k]).max() <= 1e-12 * max(np.abs(got).max(), 1e-300), k


def test_single_row_skips_advantage_normalisation():
    asz, csz = NETS["one_layer"]
    flat, rows = pr.random_problem(asz, csz, 4, seed=7)
    a, ga, exa = pr.loss_and_grads(flat, asz, csz, rows, pr.config(normalize_advantage=1), first=2, mb=1)
    b, gb, exb = pr.loss_and_grads(flat, asz, csz, rows, pr.config(normalize_advantage=0), first=2, mb=1)
    assert np.array_equal(ga, gb) and np.isfinite(ga).all() and exa["A"][0] == rows["advantage"][2] and a["adv_std"] == 0.0


def test_reference_adam_equals_torch_adam_after_clip_grad_norm():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(11)
    cfg = pr.config(max_grad_norm=0.5, lr=1e-2)
    p0 = rng.normal(size=300)
    leaf = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([leaf], lr=cfg["lr"], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"])
    p, m, v, t = p0.copy(), np.zeros(300), np.zeros(300), 0
    clipped = []
    for step in range(3):
        g = rng.normal(size=300) * (0.01 if step == 1 else 1.0)  # (step 1: the norm is below max_grad_norm)
        leaf.grad = torch.tensor(g.copy())
        torch.nn.utils.clip_grad_norm_([leaf], cfg["max_grad_norm"])
        opt.step()
        p, m, v, t, gn, skipped = pr.adam_step(p, m, v, t, g, cfg)
        clipped.append(gn > cfg["max_grad_norm"])
        assert not skipped and np.abs(leaf.detach().numpy() - p).max() <= 1e-12 * np.abs(p).max()
    assert clipped == [True, False, True] and t == 3
    q = pr.adam_step(p, m, v, t, np.where(np.arange(300) == 5, np.inf, 0.0), cfg)
    assert q[5] and q[3] == 3 and np.array_equal(q[0], p) and np.array_equal(q[1], m) and np.array_equal(q[2], v)
    assert pr.clip_scale(10.0, 0.0) == 1.0


def test_flat_layout_round_trips_through_the_split(hbmod):
    import humanoid_mujoco_amd.engine as eng
    for asz, csz in NETS.values():
        nu = asz[-1]
        n = sum(int(np.prod(sh)) for _, sh in pr.flat_shapes(asz, csz, nu))
        flat = np.arange(n, dtype=np.float32)
        assert eng.ppo_flat_shapes(asz, csz, nu) == pr.flat_shapes(asz, csz, nu)
        t = eng.ppo_split(flat, asz, csz, nu)
        assert list(t) == [k for k, _ in pr.flat_shapes(asz, csz, nu)]
        assert t["actor.w0"].shape == (48, asz[1]) and t["actor.w0"][1, 0] == asz[1]  # row-major [K][N]
        assert t["log_std"][0] == n - sum(int(np.prod(sh)) for k, sh in pr.flat_shapes(asz, csz, nu) if k.startswith("critic")) - nu
        assert np.array_equal(eng.ppo_join(t, asz, csz, nu), flat)
        assert all(np.array_equal(pr.split(flat, asz, csz, nu)[k], t[k]) for k in t)
        with pytest.raises(ValueError):
            eng.ppo_split(flat[:-1], asz, csz, nu)


def test_ctypes_structs_match_the_header(hbmod, tmp_path):
    """hb_ppo_config and hb_ppo_rows have the size and the field offsets include/hb.h gives them"""
    import humanoid_mujoco_amd.engine as eng
    pairs = [("hb_ppo_config", eng.HbPpoConfig), ("hb_ppo_rows", eng.HbPpoRows)]
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
    assert [f for f, _ in eng.HbPpoConfig._fields_] == ["clip_range", "ent_coef", "vf_coef", "max_grad_norm", "normalize_advantage", "lr", "beta1", "beta2", "eps"]


def test_defaults_and_null_batch_refusals(hbmod):
    import humanoid_mujoco_amd.engine as eng
    L = hbmod.lib()
    c = eng.HbPpoConfig()
    assert L.hb_ppo_default_config(ctypes.byref(c)) == 0 and L.hb_ppo_default_config(None) == -1
    got = {k: getattr(c, k) for k, _ in eng.HbPpoConfig._fields_}
    assert got == {k: (np.float32(v) if k != "normalize_advantage" else v) for k, v in pr.DEFAULTS.items()}, got
    rows = eng.HbPpoRows()
    buf = np.zeros(4, np.float32)
    t = ctypes.c_longlong()
    p, n = ctypes.c_void_p(), ctypes.c_longlong()
    assert L.hb_learner_create(None, ctypes.byref(c)) == -1
    assert L.hb_learner_configure(None, ctypes.byref(c)) == -1
    assert L.hb_learner_destroy(None) == -1
    assert L.hb_learner_param_count(None) == -1
    assert L.hb_learner_get_params(None, buf.ctypes.data, 4) == -1 and L.hb_learner_set_params(None, buf.ctypes.data, 4) == -1
    assert L.hb_learner_get_grads(None, buf.ctypes.data, 4) == -1
    assert L.hb_learner_get_state(None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 4, ctypes.byref(t)) == -1
    assert L.hb_learner_set_state(None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 4, 0) == -1
    assert L.hb_learner_grad_dev(None, ctypes.byref(p), ctypes.byref(n)) == -1
    assert L.hb_ppo_grad_dev(None, ctypes.byref(rows), None) == -1
    assert L.hb_ppo_adam_dev(None, None) == -1
    assert L.hb_ppo_minibatch_dev(None, ctypes.byref(rows), None) == -1
    # the chunk rule of the row reductions: 64 rows up to 4096, then at most 64 chunks of whole 16-row tiles
    assert [eng.ppo_row_chunk(m) for m in (0, 1, 64, 4096, 4097, 131072)] == [0, 64, 64, 64, 80, 2048]
    for m in (4097, 5000, 32768, 100000):
        ch = eng.ppo_row_chunk(m)
        assert ch % 16 == 0 and (m + ch - 1) // ch <= 64
