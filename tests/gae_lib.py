"""The harness of the PPO buffer's tests (tests/test_gpu_gae.py) that the normaliser's end-to-end test (tests/test_gpu_norm.py) runs
too: the sizes, the critics, the upload-and-call of hb_collect_gae_dev and the scan's derived bound.  The derivation of the bound is
in tests/test_gpu_gae.py's docstring, tier (a).

TEST INFRASTRUCTURE: the product package never imports this module.
"""
import ctypes

import numpy as np

import actor_ref as ar
import gae_ref as gr
from bounds import VALUE_TOL  # noqa: F401  (the critic's values against the fp64 critic: taken from here by both test files)

NOBS, NU = 48, 21
U = 2.0 ** -24
C_SCAN = 5
GAMMA, LAM = float(np.float32(0.99)), float(np.float32(0.95))  # (what the C struct holds: the reference gets the same numbers)
CRITICS = {"linear": [NOBS, 1], "small": [NOBS, 40, 24, 1], "wide": [NOBS, 256, 256, 1]}
TAPES = ("obs", "action", "mean", "log_std", "eps", "reward", "terminated", "truncated", "terminal_obs")
OUTS = ("value", "terminal_value", "log_prob", "advantage", "returns")


def critic(kind):
    sizes = CRITICS[kind]
    ws, bs = ar.make_actor(sizes, seed=21, scale=0.35 if len(sizes) > 2 else 0.5)
    return sizes, ws, bs


def log_std():
    return np.linspace(-1.5, 0.3, NU).astype(np.float32)


def run(b, T, tp, gamma=GAMMA, lam=LAM, boot=True, outs=OUTS, tapes=TAPES, raw=False):
    """uploads the tapes, calls hb_collect_gae_dev with the outputs in `outs` (prefilled with NaN), returns them as numpy (raw: the return
    code and the outputs, no exception)"""
    n = b.n_env
    tptr = {k: b.dev_alloc(max(4, tp[k].nbytes)) for k in tapes}
    for k in tapes:
        b.to_dev(tptr[k], tp[k])
    shape = {k: (T + 1, n) if k == "value" else (T, n) for k in outs}
    optr = {k: b.dev_alloc(max(4, int(np.prod(s)) * 4)) for k, s in shape.items()}
    for k, s in shape.items():
        if np.prod(s):
            b.to_dev(optr[k], np.full(s, np.nan, np.float32))
    try:
        if raw:
            import humanoid_mujoco_amd as hbm
            rc = hbm.lib().hb_collect_gae_dev(b._h, T, ctypes.byref(hbm.HbCollectOut(**tptr)), ctypes.byref(hbm.HbGaeConfig(gamma, lam, int(boot))),
                                              ctypes.byref(hbm.HbGaeOut(**optr)))
        else:
            b.collect_gae_dev(T, gamma, lam, boot, **tptr, **optr)
        got = {k: b.from_dev(optr[k], s) for k, s in shape.items()}
    finally:
        for p in list(tptr.values()) + list(optr.values()):
            b.dev_free(p)
    return (rc, got) if raw else got


def scan_bounds(tp, value, tv, gamma, lam, boot=True):
    """(reference advantage, returns, tier (a) bound of advantage, of returns) for the given value tapes"""
    adv, ret = gr.gae(tp["reward"], value, tv, tp["terminated"], tp["truncated"], gamma, lam, boot)
    rp = gr.shaped_reward(tp["reward"], tv, tp["terminated"], tp["truncated"], gamma, boot)
    v = np.asarray(value, dtype=np.float64)
    S = float((np.abs(rp) + 2.0 * np.maximum(np.abs(v[:-1]), np.abs(v[1:])) + np.abs(adv)).max())
    b_adv = C_SCAN * U * S / (1.0 - gamma * lam)
    return adv, ret, b_adv, b_adv + U * S
