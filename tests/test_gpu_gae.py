"""The on-device PPO buffer (include/hb.h: hb_critic_set_mlp, hb_collect_gae_dev) against the fp64 reference of tests/gae_ref.py.  The tapes
are made in numpy and uploaded, so every edge is placed by hand (_make_tapes): an env that is truncated at t = 0 and terminated at T - 1, one
that never ends, one that ends every step (truncated, terminated, both in turn), ends in consecutive steps, both flags at once; a 16-row
block of the terminal-observation rows with no bootstrapped row and one with exactly one; terminal_obs is NaN wherever the env is not
bootstrapped.  Shapes: 1, 37 (three blocks, 5 live rows in the last) and 64 envs, T in {1, 8}; critics 48 -> 1, 48 -> 40 -> 24 -> 1
(every layer on the split-K path, widths that are no multiples of 16 or 4), and once 48 -> 256 -> 256 -> 1.

Two tiers, u = 2^-24:
 (a) the scan and log_prob against the reference fed the device's OWN value / terminal_value tapes and the same input tapes.
     advantage: the kernel as written (csrc/hb_gae.hip) rounds c = 5 times per step - r' = fma(gamma, tv, reward), q = fma(gamma nt, V', r'),
     delta = q - V, A = fma(gl nt, A', delta), and gl = gamma lam itself rounded once - each by at most u times a quantity below
     S = max (|r'| + 2 |V| + |A|) over the tape, so the error obeys e_t <= gamma lam e_{t+1} + c u S and stays below c u S / (1 - gamma lam).
     returns = A + V: one rounding more, + u S.
     log_prob: the sum of nu terms in index order, (nu + c') u sum_i M_i, where M_i is term i's magnitude taken piece by piece (so that
     cancellation inside a term is covered): eps^2 / 2 + |ls| + log(2 pi) / 2, and for head 2 also 2 (log 2 + |mean| + sigma |eps| +
     log1p(exp(-2 |x|))).  nu: the running sum's roundings.  c' = 3 for head 1 (the fma, the subtraction, the constant); c' = 12 for
     head 2: those 3, expf(ls) at 1 ulp = 2 u on sigma |eps|, which the correction's slope 2 |tanh x| <= 2 doubles and M_i holds twice (2),
     the fma of x (1), expf(-2 |x|) at 1 ulp, 2 u e <= 2.9 u log1p(e) since log1p(e) >= e log 2 on [0, 1] (1.5), log1pf at 1 ulp (1), the
     constant log 2 (0.5), log 2 - |x| (1), minus the log1p (1), term - corr (1).
 (b) value and terminal_value against the fp64 critic on the same observations: 5e-5 max(1, |ref|), the bound tests/test_gpu_collect.py and
     tests/test_gpu_policy.py hold this arithmetic to (f32 MFMA chains, tanhf).  End-to-end advantage / returns against the reference fed
     the fp64 critic: with eps_V = 5e-5 max(1, max |V|, max |V_terminal|), delta moves by at most (1 + 2 gamma) eps_V (V[t], gamma V[t+1],
     gamma V_terminal), so advantage by (1 + 2 gamma) eps_V / (1 - gamma lam) plus tier (a)'s bound, and returns by eps_V more.
HB_GAE_PARITY_OUT=<file> collects the worst values (profiles/gae_parity.txt)."""
import ctypes

import numpy as np
import pytest

import actor_ref as ar
import gae_ref as gr
from gae_lib import C_SCAN, CRITICS, GAMMA, LAM, NOBS, NU, OUTS, TAPES, VALUE_TOL, U, critic as _critic, log_std as _log_std  # noqa: F401
from gae_lib import run as _run, scan_bounds as _scan_bounds
from oracle_lib import HUMANOID_HBM  # noqa: F401  (the model of the humanoid_model fixture)
from step_lib import report

pytestmark = pytest.mark.gpu

SEED = 2024
C_LOGP = {ar.GAUSSIAN: 3, ar.SQUASHED: 12}


def _report(line):
    report(line, "HB_GAE_PARITY_OUT")


def _blocks(T, n):
    """the two 16-row blocks of the [T n] terminal-observation rows that are shaped by hand: (none bootstrapped, exactly one), or None"""
    if T * n >= 64:
        return 1, 3
    if T * n > 32:
        return 1, 2
    return None


_tape_cache = {}


def _make_tapes(T, n):
    """numpy tapes [T, n, ...] with the end patterns of the module docstring; computed once per shape and shared (read only)"""
    if (T, n) in _tape_cache:
        return _tape_cache[(T, n)]
    rng = np.random.default_rng(100 * T + n)
    te = rng.random((T, n)) < 0.08
    tr = rng.random((T, n)) < 0.12
    kinds = [(0, 1), (1, 0), (1, 1)]  # (terminated, truncated): truncated alone, terminated alone, both
    for e in range(min(n, 6)):
        te[:, e] = tr[:, e] = False
    te[T - 1, 0] = T > 1          # env 0: truncated alone at t = 0 (bootstrapped), terminated at t = T - 1
    tr[0, 0] = True
    if n > 2:                     # env 1 never ends; env 2 ends every step
        for t in range(T):
            te[t, 2], tr[t, 2] = kinds[t % 3]
    if n > 3 and T >= 4:          # env 3: ends in consecutive steps, both bootstrapped
        tr[2, 3] = tr[3, 3] = True
    if n > 4 and T >= 2:          # env 4: both flags at once (not bootstrapped)
        te[1, 4] = tr[1, 4] = True
    if n > 5:                     # env 5: terminated alone at t = T - 1
        te[T - 1, 5] = True
    blk = _blocks(T, n)
    if blk and n >= 37:
        fte, ftr = te.reshape(-1), tr.reshape(-1)  # (views: rows t n + e)
        rows = np.arange(16 * blk[0], min(16 * blk[0] + 16, T * n))
        ftr[rows] = False                          # no bootstrapped row in this block (terminated ones stay)
        rows = np.arange(16 * blk[1], min(16 * blk[1] + 16, T * n))
        ftr[rows] = False
        ftr[rows[2]], fte[rows[2]] = True, False   # exactly one in this one
    boot = tr & ~te
    f32 = np.float32
    tp = {"obs": rng.normal(size=(T + 1, n, NOBS)).astype(f32), "action": np.zeros((T, n, NU), f32),
          "mean": (1.5 * rng.normal(size=(T, n, NU))).astype(f32), "log_std": rng.uniform(-3.0, 1.5, size=(T, n, NU)).astype(f32),
          "eps": rng.normal(size=(T, n, NU)).astype(f32), "reward": rng.normal(size=(T, n)).astype(f32),
          "terminated": te.astype(np.uint8), "truncated": tr.astype(np.uint8)}
    tp["mean"][0, 0, 0], tp["mean"][0, 0, 1] = 30.0, -30.0  # (|x| far in tanh's saturation: the squashed head's correction stays finite)
    tobs = np.full((T, n, NOBS), np.nan, f32)
    tobs[boot] = rng.normal(size=(int(boot.sum()), NOBS)).astype(f32)
    tp["terminal_obs"] = tobs
    _tape_cache[(T, n)] = tp
    return tp


def _cut(tp, lo, hi):
    return {k: np.ascontiguousarray(v[:, lo:hi]) for k, v in tp.items()}


def _batch(hbmod, m, n, gpu, critic="small", head=ar.GAUSSIAN):
    b = hbmod.Batch(m, n, gpu)
    sizes, ws, bs = _critic(critic)
    b.critic_set(sizes, ws, bs)
    if head is not None:
        asz = [NOBS, 32, 2 * NU if head == ar.SQUASHED else NU]
        aw, ab = ar.make_actor(asz, seed=5)
        b.actor_set(asz, aw, ab, head=head, log_std=_log_std() if head == ar.GAUSSIAN else None, seed=SEED)
    return b, ws, bs


def _logp_bound(head, tp, ls):
    eps, ls = tp["eps"].astype(np.float64), np.broadcast_to(np.asarray(ls, dtype=np.float64), tp["eps"].shape)
    M = 0.5 * eps * eps + np.abs(ls) + 0.5 * gr.LOG_2PI
    if head == ar.SQUASHED:
        mean = tp["mean"].astype(np.float64)
        x = mean + np.exp(ls) * eps
        M = M + 2.0 * (np.log(2.0) + np.abs(mean) + np.exp(ls) * np.abs(eps) + np.log1p(np.exp(-2.0 * np.abs(x))))
    return (NU + C_LOGP[head]) * U * M.sum(axis=-1)


def _check(hbmod, m, gpu, n, T, critic, head):
    tp = _make_tapes(T, n)
    te, tr = tp["terminated"].astype(bool), tp["truncated"].astype(bool)
    boot = tr & ~te
    assert boot[0, 0] and np.isnan(tp["terminal_obs"][~boot]).all() and np.isfinite(tp["terminal_obs"][boot]).all()
    blk = _blocks(T, n)
    if blk and n >= 37:
        fb = boot.reshape(-1)
        assert fb[16 * blk[0]:16 * blk[0] + 16].sum() == 0 and fb[16 * blk[1]:16 * blk[1] + 16].sum() == 1
    if n >= 6 and T == 8:
        done = te | tr
        assert not done[:, 1].any() and done[:, 2].all() and done[2:4, 3].all() and (te & tr)[1, 4] and done[0, 0] and done[T - 1, 0]
    b, ws, bs = _batch(hbmod, m, n, gpu, critic, head)
    got = _run(b, T, tp)
    b.close()
    for k in OUTS:
        assert np.isfinite(got[k]).all(), k
    assert not got["terminal_value"][~boot].any()  # exactly 0 where the env is not bootstrapped
    # tier (a): the scan and log_prob on the device's own value tapes
    adv, ret, b_adv, b_ret = _scan_bounds(tp, got["value"], got["terminal_value"], GAMMA, LAM)
    e_adv, e_ret = float(np.abs(got["advantage"] - adv).max()), float(np.abs(got["returns"] - ret).max())
    ls = tp["log_std"] if head == ar.SQUASHED else _log_std()
    lp = gr.log_prob(head, tp["eps"], ls, tp["mean"])
    lp_ratio = float((np.abs(got["log_prob"] - lp) / _logp_bound(head, tp, ls)).max())
    # tier (b): the critic against fp64, and the whole chain
    v64 = gr.values(tp["obs"], ws, bs)
    tv64 = np.zeros((T, n))
    tv64[boot] = gr.values(tp["terminal_obs"][boot], ws, bs)
    e_v = float((np.abs(got["value"] - v64) / np.maximum(1.0, np.abs(v64))).max())
    e_tv = float((np.abs(got["terminal_value"] - tv64) / np.maximum(1.0, np.abs(tv64))).max())
    adv64, ret64, _, _ = _scan_bounds(tp, v64, tv64, GAMMA, LAM)
    eps_v = VALUE_TOL * max(1.0, float(np.abs(v64).max()), float(np.abs(tv64).max()))
    b_adv64 = (1.0 + 2.0 * GAMMA) * eps_v / (1.0 - GAMMA * LAM) + b_adv
    b_ret64 = b_adv64 + eps_v + (b_ret - b_adv)
    e_adv64, e_ret64 = float(np.abs(got["advantage"] - adv64).max()), float(np.abs(got["returns"] - ret64).max())
    _report("gae %d envs, T %d, critic %s, head %d: (a) advantage %.3g (bound %.3g), returns %.3g (%.3g), log_prob / bound %.3g; (b) value %.3g, "
            "terminal_value %.3g (bound %.0e), advantage %.3g (%.3g), returns %.3g (%.3g); %d bootstrapped rows, |V| max %.2f, |A| max %.2f, |log_prob| max %.1f"
            % (n, T, "-".join(map(str, CRITICS[critic])), head, e_adv, b_adv, e_ret, b_ret, lp_ratio, e_v, e_tv, VALUE_TOL, e_adv64, b_adv64, e_ret64, b_ret64,
               int(boot.sum()), np.abs(v64).max(), np.abs(adv64).max(), np.abs(lp).max()))
    assert e_adv <= b_adv and e_ret <= b_ret
    assert lp_ratio <= 1.0
    assert e_v <= VALUE_TOL and e_tv <= VALUE_TOL
    assert e_adv64 <= b_adv64 and e_ret64 <= b_ret64


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("n", [1, 37, 64])
@pytest.mark.parametrize("critic", ["linear", "small"])
def test_matches_reference(hbmod, humanoid_model, gpu, n, T, critic):
    _check(hbmod, humanoid_model, gpu, n, T, critic, ar.GAUSSIAN if critic == "small" else ar.SQUASHED)


def test_reference_sizes(hbmod, humanoid_model, gpu):
    """48 -> 256 -> 256 -> 1, the critic beside the reference's actor (sixteen output tiles in the hidden layers: no split), squashed head"""
    _check(hbmod, humanoid_model, gpu, 37, 8, "wide", ar.SQUASHED)


def test_options_and_partial_outputs(hbmod, humanoid_model, gpu):
    """lam 0 / gamma 1 / no bootstrap, and every output alone (the value tapes then live in the batch's scratch): the same bits as together"""
    m, n, T = humanoid_model, 37, 8
    tp = _make_tapes(T, n)
    b, ws, bs = _batch(hbmod, m, n, gpu)
    full = _run(b, T, tp)
    for k in OUTS:
        need = {"value": ("obs",), "terminal_value": ("terminal_obs", "terminated", "truncated"), "log_prob": ("eps",),
                "advantage": ("obs", "reward", "terminated", "truncated", "terminal_obs"), "returns": ("obs", "reward", "terminated", "truncated", "terminal_obs")}[k]
        one = _run(b, T, tp, outs=(k,), tapes=need)  # (and only the tapes the header lists for it)
        assert np.array_equal(one[k], full[k]), k
    for gamma, lam, boot in ((GAMMA, 0.0, True), (1.0, float(np.float32(0.9)), True), (GAMMA, LAM, False), (0.0, 0.0, True)):
        got = _run(b, T, tp, gamma, lam, boot)
        assert np.array_equal(got["value"], full["value"])
        assert np.array_equal(got["terminal_value"], full["terminal_value"]) if boot else not got["terminal_value"].any()
        adv, ret, b_adv, b_ret = _scan_bounds(tp, got["value"], got["terminal_value"], gamma, lam, boot)
        assert np.abs(got["advantage"] - adv).max() <= b_adv and np.abs(got["returns"] - ret).max() <= b_ret, (gamma, lam, boot)
    b.close()


def test_same_bits_on_any_split(hbmod, humanoid_model, gpu):
    m, T = humanoid_model, 8
    tp = _make_tapes(T, 64)
    res = {}
    for name, lo, hi in (("whole", 0, 64), ("head", 0, 37), ("tail", 37, 64)):
        b, _, _ = _batch(hbmod, m, hi - lo, gpu, "small", ar.SQUASHED)
        res[name] = _run(b, T, _cut(tp, lo, hi))
        b.close()
    for k in OUTS:
        assert np.array_equal(res["whole"][k][:, :37], res["head"][k]), k
        assert np.array_equal(res["whole"][k][:, 37:], res["tail"][k]), k


def _env(hbmod, m, n, gpu):
    env = hbmod.VecEnv(m, n, gpu, realism=True, domain_randomization=True, seed=7, reward_kind=1, max_time=0.02)
    asz = [NOBS, 40, 24, NU]
    aw, ab = ar.make_actor(asz, seed=11, scale=0.35)
    env.actor_set(asz, aw, ab, head="gaussian", log_std=_log_std(), seed=SEED)
    sizes, ws, bs = _critic("small")
    env.critic_set(sizes, ws, bs)
    return env, ws, bs


def test_purity(hbmod, humanoid_model, gpu):
    """the call writes nothing of the batch: state, status words, counts, launch counter and kernel name, and the actor's draw counter"""
    m, n, T = humanoid_model, 37, 8
    env, _, _ = _env(hbmod, m, n, gpu)
    b = env.batch
    env.reset()
    first = env.collect(T, terminal_obs=True)
    before = (b.get_state(hbmod.STATE_INTEGRATION), b.status(), np.asarray(b.counts()), b.step_launches(), b.last_kernel())
    tp = {k: np.ascontiguousarray(v.astype(np.uint8) if v.dtype == bool else v) for k, v in first.items()}
    got = _run(b, T, tp, tapes=tuple(tp))
    assert all(np.isfinite(got[k]).all() for k in OUTS)
    after = (b.get_state(hbmod.STATE_INTEGRATION), b.status(), np.asarray(b.counts()), b.step_launches(), b.last_kernel())
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    second = env.collect(T)
    assert np.abs(second["eps"] - ar.draws(SEED, 0, n, NU, T, T)).max() < 2e-5  # the draw counter went on at T
    assert np.array_equal(second["obs"][0], first["obs"][T])
    env.close()


def test_integration_with_a_real_collection(hbmod, humanoid_model, gpu):
    """27-dof humanoid, 37 envs, T = 8, reward_kind 1 with a 20 ms time limit: every env is truncated inside T.  collect_torch(T, gae=...)
    equals the tapes fed to Batch.collect_gae_dev by hand bit for bit, and passes tier (b)."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    m, n, T = humanoid_model, 37, 8
    env, ws, bs = _env(hbmod, m, n, gpu)
    env.reset()
    out = {k: v.cpu().numpy() for k, v in env.collect_torch(T, gae=dict(gamma=GAMMA, lam=LAM)).items()}
    assert sorted(out) == sorted(["obs", "action", "mean", "eps", "reward", "terminated", "truncated", "terminal_obs", "value", "log_prob", "advantage", "returns"])
    assert out["value"].shape == (T + 1, n) and out["advantage"].shape == out["returns"].shape == out["log_prob"].shape == (T, n)
    te, tr = out["terminated"], out["truncated"]
    boot = tr & ~te
    assert boot.any(), "no env was bootstrapped inside the window"
    tp = {k: np.ascontiguousarray(out[k].astype(np.uint8) if out[k].dtype == bool else out[k]) for k in TAPES if k in out}
    hand = _run(env.batch, T, tp, tapes=tuple(tp))
    for k in ("value", "log_prob", "advantage", "returns"):
        assert np.array_equal(hand[k], out[k]), k
    # tier (b)
    v64 = gr.values(out["obs"], ws, bs)
    tv64 = np.zeros((T, n))
    tv64[boot] = gr.values(out["terminal_obs"][boot], ws, bs)
    e_v = float((np.abs(out["value"] - v64) / np.maximum(1.0, np.abs(v64))).max())
    e_tv = float((np.abs(hand["terminal_value"] - tv64) / np.maximum(1.0, np.abs(tv64))).max())
    _, _, b_adv, b_ret = _scan_bounds(tp, hand["value"], hand["terminal_value"], GAMMA, LAM)
    adv64, ret64, _, _ = _scan_bounds(tp, v64, tv64, GAMMA, LAM)
    eps_v = VALUE_TOL * max(1.0, float(np.abs(v64).max()), float(np.abs(tv64).max()))
    b_adv64 = (1.0 + 2.0 * GAMMA) * eps_v / (1.0 - GAMMA * LAM) + b_adv
    e_adv64, e_ret64 = float(np.abs(out["advantage"] - adv64).max()), float(np.abs(out["returns"] - ret64).max())
    lp = gr.log_prob(ar.GAUSSIAN, out["eps"], _log_std())
    lp_ratio = float((np.abs(out["log_prob"] - lp) / _logp_bound(ar.GAUSSIAN, tp, _log_std())).max())
    _report("gae on a collection (humanoid, %d envs, T %d, %d bootstrapped rows): value %.3g, terminal_value %.3g (bound %.0e), advantage %.3g (%.3g), "
            "returns %.3g (%.3g), log_prob / bound %.3g" % (n, T, int(boot.sum()), e_v, e_tv, VALUE_TOL, e_adv64, b_adv64, e_ret64, b_adv64 + eps_v + (b_ret - b_adv), lp_ratio))
    assert e_v <= VALUE_TOL and e_tv <= VALUE_TOL
    assert e_adv64 <= b_adv64 and e_ret64 <= b_adv64 + eps_v + (b_ret - b_adv)
    assert lp_ratio <= 1.0
    # gae=None: exactly the call as it was
    plain = env.collect_torch(T)
    assert sorted(plain) == sorted(["obs", "action", "mean", "eps", "reward", "terminated", "truncated"])
    env.close()


def test_argument_checks(hbmod, humanoid_model, gpu):
    m, n, T = humanoid_model, 8, 2
    L = hbmod.lib()
    EINVAL, EUNSUPPORTED = -1, -4
    tp = _cut(_make_tapes(8, 37), 0, n)
    tp = {k: np.ascontiguousarray(v[:T + 1] if k == "obs" else v[:T]) for k, v in tp.items()}
    env = hbmod.VecEnv(m, n, gpu)
    b = env.batch
    obs0 = env.reset()

    def install(sizes, batch=b, null=None):
        ws = [np.zeros((a, c), np.float32) for a, c in zip(sizes[:-1], sizes[1:])]
        bs = [np.full(c, 0.5, np.float32) for c in sizes[1:]]
        csz = (ctypes.c_int * len(sizes))(*sizes)
        wp = (ctypes.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
        bp = (ctypes.c_void_p * len(bs))(*[x.ctypes.data for x in bs])
        if null == "w0":
            wp[0] = None
        if null == "b0":
            bp[0] = None
        return L.hb_critic_set_mlp(batch._h if batch is not None else None, len(ws), None if null == "sizes" else csz, None if null == "weights" else wp,
                                   None if null == "biases" else bp)

    def call(**kw):
        rc, got = _run(b, T, tp, raw=True, **kw)
        if rc != 0:  # a refused call leaves the outputs untouched (the NaN they were filled with)
            assert all(np.isnan(v).all() for v in got.values())
        return rc

    value_outs = ("value", "terminal_value", "advantage", "returns")
    # no critic, no actor yet
    assert call(outs=("value",)) == EINVAL and call(outs=("advantage",)) == EINVAL and call(outs=("terminal_value",)) == EINVAL
    assert call(outs=("log_prob",)) == EINVAL
    # hb_critic_set_mlp
    assert install([NOBS, 32, 1], batch=None) == EINVAL
    for null in ("sizes", "weights", "biases", "w0", "b0"):
        assert install([NOBS, 32, 1], null=null) == EINVAL
    assert L.hb_critic_set_mlp(b._h, 0, None, None, None) == EINVAL
    assert install([NOBS, 8, 8, 8, 8, 1]) == EINVAL      # five layers
    assert install([NOBS + 1, 32, 1]) == EINVAL          # input width
    assert install([NOBS, 32, 2]) == EINVAL              # output width
    assert install([NOBS, 0, 1]) == EINVAL
    assert install([NOBS, 257, 1]) == EUNSUPPORTED       # wider than the fused kernel's tiles: no fallback
    assert call(outs=("value",)) == EINVAL               # refused calls installed nothing
    assert install([NOBS, 256, 1]) == 0
    assert install([NOBS, 300, 1]) == EUNSUPPORTED and install([NOBS, 32, 3]) == EINVAL
    rc, got = _run(b, T, tp, raw=True, outs=("value",))  # a refused call leaves the installed critic as it was: zero weights, bias 0.5
    assert rc == 0 and np.array_equal(got["value"], np.full((T + 1, n), 0.5, np.float32))
    with pytest.raises(hbmod.HbError):
        b.critic_set([NOBS, 300, 1], [np.zeros((NOBS, 300)), np.zeros((300, 1))], [np.zeros(300), np.zeros(1)])
    # hb_collect_gae_dev
    assert call(outs=("log_prob",)) == EINVAL            # still no actor
    asz = [NOBS, 32, NU]
    aw, ab = ar.make_actor(asz, seed=5)
    b.actor_set(asz, aw, ab, head="deterministic")
    assert call(outs=("log_prob",)) == EINVAL            # head 0 has no density
    assert call(outs=value_outs) == 0
    b.actor_set([NOBS, 32, 2 * NU], *ar.make_actor([NOBS, 32, 2 * NU], seed=5), head="squashed")
    assert call(outs=("log_prob",)) == 0
    assert call(outs=("log_prob",), tapes=("eps", "mean")) == EINVAL and call(outs=("log_prob",), tapes=("eps", "log_std")) == EINVAL
    assert call(outs=("log_prob",), tapes=("mean", "log_std")) == EINVAL
    b.actor_set(asz, aw, ab, head="gaussian", log_std=_log_std())
    assert call(outs=("log_prob",), tapes=("eps",)) == 0 and call(outs=("log_prob",), tapes=("mean",)) == EINVAL
    cfg, tapes, out = hbmod.HbGaeConfig(GAMMA, LAM, 1), hbmod.HbCollectOut(), hbmod.HbGaeOut()
    assert L.hb_collect_gae_dev(None, T, ctypes.byref(tapes), ctypes.byref(cfg), ctypes.byref(out)) == EINVAL
    assert L.hb_collect_gae_dev(b._h, T, None, ctypes.byref(cfg), ctypes.byref(out)) == EINVAL
    assert L.hb_collect_gae_dev(b._h, T, ctypes.byref(tapes), None, ctypes.byref(out)) == EINVAL
    assert L.hb_collect_gae_dev(b._h, T, ctypes.byref(tapes), ctypes.byref(cfg), None) == EINVAL
    assert call(outs=()) == EINVAL                       # all outputs NULL
    rc, _ = _run(b, 0, tp, raw=True)
    assert rc == EINVAL                                  # T < 1
    for gamma, lam in ((float("nan"), LAM), (GAMMA, float("inf")), (-0.1, LAM), (1.5, LAM), (GAMMA, -0.1), (GAMMA, 1.01)):
        assert call(gamma=gamma, lam=lam) == EINVAL
    assert call(gamma=0.0, lam=1.0) == 0 and call(gamma=1.0, lam=0.0) == 0
    # a missing tape for a requested output
    every = set(TAPES)
    assert call(outs=("value",), tapes=tuple(every - {"obs"})) == EINVAL
    for miss in ("obs", "reward", "terminated", "truncated", "terminal_obs"):
        assert call(outs=("advantage",), tapes=tuple(every - {miss})) == EINVAL and call(outs=("returns",), tapes=tuple(every - {miss})) == EINVAL
    assert call(outs=("advantage", "returns"), tapes=tuple(every - {"terminal_obs"}), boot=False) == 0
    for miss in ("terminal_obs", "terminated", "truncated"):
        assert call(outs=("terminal_value",), tapes=tuple(every - {miss})) == EINVAL
    assert call(outs=("log_prob",), tapes=tuple(every - {"eps"})) == EINVAL
    with pytest.raises(hbmod.HbError):
        b.collect_gae_dev(T, GAMMA, LAM)
    # the batch collects and steps afterwards
    r = env.collect(2, obs0=obs0, gae=dict(gamma=GAMMA, lam=LAM))
    assert all(np.isfinite(r[k]).all() for k in ("obs", "action", "value", "log_prob", "advantage", "returns"))
    o, rew, *_ = env.step_arrays(np.zeros((n, NU), np.float32))
    assert np.isfinite(o).all() and np.isfinite(rew).all()
    env.close()
