"""The one fp64 numpy MLP of the learner references (ppo_ref.py, sac_ref.py, act_ref.py): tanh, ReLU or ELU behind every hidden layer
(include/hb.h: hb_mlp_set_activation), the last layer linear, over a dict of tensors tag.w0 [K, N], tag.b0 [N], ...  The forward pass with
kept activations, the backward pass that forms the derivative from the kept OUTPUT a as the kernels do (1 - a^2; a > 0 ? 1 : 0;
a > 0 ? 1 : a + 1), the derived float32 forward bound, the flat record's split and join, Adam, and the same network in torch.

The forward bound by row and column: a K-term f32 MFMA chain and the bias per layer, then the error carried in,
e' = (K + 2) u (|a| |W| + |b|) + e |W| + c u, with the activation's own term c: 4 ulp behind tanhf, 0 behind ReLU (a select), EXPM1_ULP
behind ELU (|expm1(v)| < 1 for v <= 0, so an ulp of the result is at most u; v > 0 is passed through).  All three have slopes of at most
1, so the error carried in is not amplified.

Pure numpy, and independent of the package: humanoid_mujoco_amd/engine.py states the record's layout a second time on purpose, and
test_ppo_cpu.py and test_sac_cpu.py hold the two statements against each other."""
import numpy as np

U = 2.0 ** -24
ACTIVATIONS = ("tanh", "relu", "elu")
# expm1f on the device over every float32 in [-20, -0] against fp64: worst error 0.8905 ulp (profiles/act_parity.txt); twice that, rounded up
EXPM1_ULP = 2
ACT_ULP = {"tanh": 4, "relu": 0, "elu": EXPM1_ULP}


def act(name, z):
    if name == "tanh":
        return np.tanh(z)
    if name == "relu":
        return np.where(z < 0.0, 0.0, z)
    assert name == "elu", name
    return np.where(z > 0.0, z, np.expm1(np.minimum(z, 0.0)))


def slope(name, a):
    """the activation's derivative from its OUTPUT a"""
    if name == "tanh":
        return 1.0 - a * a
    if name == "relu":
        return np.where(a > 0.0, 1.0, 0.0)
    assert name == "elu", name
    return np.where(a > 0.0, 1.0, a + 1.0)


def forward(tensors, tag, n_layers, x, activation="tanh"):
    """acts[l]: the input of layer l (acts[0] = x); the last layer's (linear) output; zs[l]: the pre-activation of hidden layer l"""
    acts, zs, a = [], [], np.asarray(x, dtype=np.float64)
    for l in range(n_layers):
        acts.append(a)
        z = a @ np.asarray(tensors["%s.w%d" % (tag, l)], dtype=np.float64) + np.asarray(tensors["%s.b%d" % (tag, l)], dtype=np.float64)
        if l < n_layers - 1:
            zs.append(z)
            a = act(activation, z)
        else:
            a = z
    return acts, a, zs


def backward(tensors, tag, n_layers, acts, dz, activation="tanh", grads=None):
    """dz: dloss / d(the last layer's output); fills grads[tag.w*], grads[tag.b*] where grads is given; returns dloss / d(input rows)"""
    for l in range(n_layers - 1, -1, -1):
        if grads is not None:
            grads["%s.w%d" % (tag, l)] = acts[l].T @ dz
            grads["%s.b%d" % (tag, l)] = dz.sum(axis=0)
        dz = dz @ np.asarray(tensors["%s.w%d" % (tag, l)], dtype=np.float64).T
        if l > 0:
            dz = dz * slope(activation, acts[l])
    return dz


def fwd_err(tensors, tag, n_layers, acts, activation="tanh", e0=None):
    """the derived forward error of a network on the device; e0: the error carried in by the input rows.  Returns (the bound of the last
    layer's output by row and column, [the bound of every hidden layer's PRE-activation])"""
    e = np.zeros_like(acts[0]) if e0 is None else e0
    pre = []
    for l in range(n_layers):
        W, bias = np.abs(tensors["%s.w%d" % (tag, l)]), np.abs(tensors["%s.b%d" % (tag, l)])
        e = (W.shape[0] + 2) * U * (np.abs(acts[l]) @ W + bias) + e @ W
        if l < n_layers - 1:
            pre.append(e)
            e = e + ACT_ULP[activation] * U
    return e, pre


# ---- the flat record: tensors one behind the other, each row-major

def net_shapes(tag, sizes):
    """(name, shape) of a network's tensors in the record's order: W [K, N] | b [N] layer by layer"""
    out = []
    for l in range(len(sizes) - 1):
        out += [("%s.w%d" % (tag, l), (sizes[l], sizes[l + 1])), ("%s.b%d" % (tag, l), (sizes[l + 1],))]
    return out


def split(flat, shapes):
    flat = np.asarray(flat)
    out, o = {}, 0
    for name, sh in shapes:
        n = int(np.prod(sh))
        out[name] = flat[o:o + n].reshape(sh).copy()
        o += n
    assert o == flat.size, (o, flat.size)
    return out


def join(tensors, shapes):
    return np.concatenate([np.asarray(tensors[name], dtype=np.float64).reshape(sh).ravel() for name, sh in shapes])


def adam(p, m, v, t, g, lr, cfg):
    """torch.optim.Adam on fp64 arrays, t being the step count this step included: (p, m, v)"""
    p, m, v, g = (np.asarray(x, dtype=np.float64) for x in (p, m, v, g))
    b1, b2 = float(cfg["beta1"]), float(cfg["beta2"])
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - float(lr) / (1.0 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + float(cfg["eps"]))
    return p, m, v


# ---- the same network in torch (float64: what the references are held to; float32: the noise floor)

def torch_act(torch, activation):
    return {"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU, "elu": torch.nn.ELU}[activation]()


def torch_mlp(torch, par, tag, n, x, activation="tanh"):
    f = torch_act(torch, activation)
    for l in range(n):
        x = x @ par["%s.w%d" % (tag, l)] + par["%s.b%d" % (tag, l)]
        if l < n - 1:
            x = f(x)
    return x
