"""tests/mlp_ref.py and act_ref.py without a device: the fp64 MLP with a chosen hidden activation against torch autograd in float64 (nn.Tanh /
nn.ReLU / nn.ELU), tanh as the default the learner references run; the margin conditions of exactly the problems tests/test_gpu_act.py runs; and the refusals of
hb_mlp_set_activation / hb_mlp_get_activation that need no device."""
import numpy as np
import pytest

import act_ref as ac
import mlp_ref as ml


def _net(sizes, seed, tag="n"):
    rng = np.random.default_rng(seed)
    t = {}
    for l in range(len(sizes) - 1):
        t["%s.w%d" % (tag, l)] = rng.normal(0.0, 1.0 / np.sqrt(sizes[l]), (sizes[l], sizes[l + 1]))
        t["%s.b%d" % (tag, l)] = rng.normal(0.0, 0.1, sizes[l + 1])
    return t


@pytest.mark.parametrize("activation", ml.ACTIVATIONS)
@pytest.mark.parametrize("sizes", [[48, 20, 72, 21], [69, 256, 1], [48, 21]])
def test_forward_and_backward_equal_autograd(activation, sizes):
    torch = pytest.importorskip("torch")
    n = len(sizes) - 1
    t = _net(sizes, 3)
    rng = np.random.default_rng(4)
    x, top = rng.normal(size=(40, sizes[0])), rng.normal(size=(40, sizes[-1]))
    acts, out, zs = ml.forward(t, "n", n, x, activation)
    grads = {}
    dx = ml.backward(t, "n", n, acts, top, activation, grads)
    leaves = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in t.items()}
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    o = ml.torch_mlp(torch, leaves, "n", n, xt, activation)
    assert np.abs(o.detach().numpy() - out).max() <= 1e-13 * max(1.0, np.abs(out).max())
    (o * torch.tensor(top)).sum().backward()
    assert np.abs(xt.grad.numpy() - dx).max() <= 1e-12 * max(1.0, np.abs(dx).max())
    for k in t:
        assert np.abs(leaves[k].grad.numpy() - grads[k]).max() <= 1e-12 * max(1.0, np.abs(grads[k]).max()), k
    assert len(zs) == n - 1 and all(np.array_equal(ml.act(activation, z), a) for z, a in zip(zs, acts[1:]))


def test_tanh_is_the_existing_references():
    """ppo_ref and sac_ref run mlp_ref with the activation left out where their caller names none: that default is tanh, bit for bit,
    and tanh is what those references stated themselves before - np.tanh behind a hidden layer, the derivative 1 - a^2 from its output"""
    t = _net([48, 20, 72, 21], 5, "actor")
    rng = np.random.default_rng(6)
    x, top = rng.normal(size=(40, 48)), rng.normal(size=(40, 21))
    acts, out, zs = ml.forward(t, "actor", 3, x, "tanh")
    racts, rout, _ = ml.forward(t, "actor", 3, x)
    assert np.array_equal(rout, out) and all(np.array_equal(a, b) for a, b in zip(racts, acts))
    assert all(np.array_equal(np.tanh(z), a) for z, a in zip(zs, acts[1:]))
    assert all(np.array_equal(ml.slope("tanh", a), 1.0 - a ** 2) for a in acts[1:])
    g, gd = {}, {}
    dx = ml.backward(t, "actor", 3, acts, top, "tanh", g)
    assert np.array_equal(ml.backward(t, "actor", 3, acts, top, grads=gd), dx)
    for k in g:
        assert np.array_equal(g[k], gd[k]), k
    e, _ = ml.fwd_err(t, "actor", 3, acts, "tanh")
    assert np.array_equal(e, ml.fwd_err(t, "actor", 3, acts)[0])


def test_activations_at_their_edges():
    z = np.array([-np.inf, -30.0, -1.0, -0.0, 0.0, 2.0, np.inf, np.nan])
    with np.errstate(invalid="ignore"):
        r, e = ml.act("relu", z), ml.act("elu", z)
    assert np.array_equal(r[:7], [0.0, 0.0, 0.0, 0.0, 0.0, 2.0, np.inf]) and np.isnan(r[7])   # (NaN stays NaN: a select, not a maximum)
    assert np.array_equal(e[[0, 3, 4, 5, 6]], [-1.0, 0.0, 0.0, 2.0, np.inf]) and e[2] == np.expm1(-1.0) and np.isnan(e[7])
    assert np.array_equal(ml.slope("relu", r[:6]), [0, 0, 0, 0, 0, 1])                            # (0 at v <= 0, as torch)
    assert np.allclose(ml.slope("elu", e[:6]), np.exp(np.minimum(z[:6], 0.0)), rtol=0, atol=1e-15)


@pytest.mark.parametrize("key", sorted(ac.PPO_SEEDS))
def test_ppo_problems_meet_the_margin(key):
    net, activation = key
    flat, rows = ac.ppo_problem(net, activation, activation, ac.PPO_SEEDS[key])
    rows = {k: v[ac.SEL] for k, v in rows.items()}
    m = ac.ppo_margin(net, flat, rows, activation, activation)
    print("\n  ppo %s %s seed %d: smallest |z| / bound %.1f" % (net, activation, ac.PPO_SEEDS[key], m))
    assert m >= ac.MARGIN


@pytest.mark.parametrize("key", sorted(ac.SAC_SEEDS))
def test_sac_problems_meet_their_conditions(key):
    """at the problem's parameters, and for the actor phase at the reference's own critic update (the device's differs from it by
    roundings of the parameters, and test_gpu_act.py asserts the same conditions at what it downloads)"""
    torch = pytest.importorskip("torch")
    net, activation = key
    asz, qsz = ac.sac_sizes(net)
    pb = ac.sac_problem(torch, net, activation, activation, ac.SAC_SEEDS[key])
    ep, en = pb["eps_pi"][ac.SEL], pb["eps_next"][ac.SEL]
    c0 = ac.sac_conditions(net, pb["flat"], pb["rows"], ac.SEL, ep, activation, activation)
    mid = ac.sac_mid(torch, net, pb["flat"], pb["targets"], pb["rows"], ac.SEL, ep, en, ac.sac_cfg(), activation, activation)
    c1 = ac.sac_conditions(net, mid, pb["rows"], ac.SEL, ep, activation, activation)
    print("\n  sac %s %s seed %d: %s | after the critic step %s" % (net, activation, ac.SAC_SEEDS[key], {k: round(v, 1) for k, v in c0.items()},
                                                                   {k: round(v, 1) for k, v in c1.items()}))
    for k in ("actor", "q1", "q2", "log_std"):
        assert c0[k] >= ac.MARGIN, (k, c0[k])
    for k in ("q1_pi", "q2_pi", "q1_q2"):
        assert c1[k] >= 2 * ac.MARGIN, (k, c1[k])   # (twice: the device's own critic step stands in for the reference's on the GPU)


def test_seeds_cover_every_case():
    cases = {(net, a) for net in ac.HIDDEN for a in ("relu", "elu")}
    assert set(ac.PPO_SEEDS) == cases and set(ac.SAC_SEEDS) == cases


def test_null_batch_and_constants(hbmod):
    L = hbmod.lib()
    assert L.hb_mlp_set_activation(None, hbmod.NET_ACTOR, hbmod.ACT_RELU) == -1
    assert L.hb_mlp_get_activation(None, hbmod.NET_ACTOR) == -1
    assert (hbmod.ACT_TANH, hbmod.ACT_RELU, hbmod.ACT_ELU) == (0, 1, 2)
    assert (hbmod.NET_POLICY, hbmod.NET_ACTOR, hbmod.NET_CRITIC, hbmod.NET_Q1, hbmod.NET_Q2) == (0, 1, 2, 3, 4)
    import humanoid_mujoco_amd.engine as eng
    with pytest.raises(ValueError):
        eng._activation("gelu")
    with pytest.raises(ValueError):
        eng._net("value")
    assert eng._activation("elu") == 2 and eng._net("q2") == 4
