"""fp64 reference of the sampling actor (hb_actor_kernel, include/hb.h: hb_actor_set_mlp / hb_env_collect_dev): the MLP with its three
heads in numpy, and the N(0, 1) draws through env_ref.rng_normal.  Test infrastructure: the package never imports it."""
import numpy as np

from env_ref import rng_normal

DETERMINISTIC, GAUSSIAN, SQUASHED = 0, 1, 2
RS_ACTOR = 32  # the random-number stream of the actor's draws (include/hb.h)
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0


def make_actor(sizes, seed=0, scale=None):
    """weights [in, out] and biases of an MLP with the given sizes: U(-k, k), k = 1 / sqrt(fan_in) (nn.Linear's default) or `scale`"""
    rng = np.random.default_rng(seed)
    ws, bs = [], []
    for a, c in zip(sizes[:-1], sizes[1:]):
        k = 1.0 / np.sqrt(a) if scale is None else scale
        ws.append(rng.uniform(-k, k, size=(a, c)).astype(np.float32))
        bs.append(rng.uniform(-k, k, size=c).astype(np.float32))
    return ws, bs


def draws(seed, env_offset, n_env, nu, draw0, T=1):
    """eps[t][e][i] = rng_normal(seed, env_offset + e, 0, draw0 + t, RS_ACTOR, i), float64 [T, n_env, nu]"""
    out = np.empty((T, n_env, nu))
    for t in range(T):
        for e in range(n_env):
            for i in range(nu):
                out[t, e, i] = rng_normal(seed, env_offset + e, 0, draw0 + t, RS_ACTOR, i)
    return out


def network(obs, ws, bs, head):
    """the last layer's output in fp64: tanh after every hidden layer; the last layer has tanh for head 0 and is linear otherwise"""
    x = np.asarray(obs, dtype=np.float64)
    for l, (w, b) in enumerate(zip(ws, bs)):
        x = x @ w.astype(np.float64) + b.astype(np.float64)
        if l + 1 < len(ws) or head == DETERMINISTIC:
            x = np.tanh(x)
    return x


def head_action(head, mean, log_std, eps):
    """the head's arithmetic on given mean / log_std / eps (fp64)"""
    mean, eps = np.asarray(mean, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    if head == DETERMINISTIC:
        return mean
    pre = mean + np.exp(np.asarray(log_std, dtype=np.float64)) * eps
    return np.tanh(pre) if head == SQUASHED else pre


def actor(obs, ws, bs, head, log_std=None, eps=None, deterministic=False):
    """dict(mean, log_std, eps, action) [n, nu] in fp64 for observations [n, nobs]; eps: the draws [n, nu] (ignored when deterministic)"""
    y = network(obs, ws, bs, head)
    if head == SQUASHED:
        nu = y.shape[-1] // 2
        mean, ls = y[..., :nu], np.clip(y[..., nu:], LOG_STD_MIN, LOG_STD_MAX)
    else:
        nu = y.shape[-1]
        mean = y
        ls = np.zeros_like(y) if head == DETERMINISTIC else np.broadcast_to(np.asarray(log_std, dtype=np.float64), y.shape)
    e = np.zeros_like(mean) if deterministic or head == DETERMINISTIC or eps is None else np.asarray(eps, dtype=np.float64)
    return {"mean": mean, "log_std": ls, "eps": e, "action": head_action(head, mean, ls, e)}
