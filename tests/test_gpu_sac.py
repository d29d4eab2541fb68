"""The SAC learner on the device (include/hb.h: hb_q_*, hb_sac_*) against the fp64 reference of tests/sac_ref.py, from the GPU's own
downloaded state.  Batches of 16 envs, synthetic rows (no physics), the draws given (eps_given = 1).

Bounds, u = 2^-24:
 (a) derived from the arithmetic, by row and summed (sac_lib.derived_*): the statistics, the top-layer bias gradients of Q1 and Q2 and the
     log_ent_coef gradient.  The forward error of a network follows its layers (mlp_ref.fwd_err), the error of a sampled action carried
     into the Q networks' input rows (sac_ref.action_err); from there the log-probabilities (sac_ref.lp_err), the target (sac_ref.target),
     the residuals Qk - y, each a handful of f32 roundings; means are formed in fp64 from the f32 terms.
 (b) the back-propagated gradients - every W and hidden bias of Q1, Q2, and EVERY tensor of the actor, whose top dZ already holds
     dQ / da, a back-propagated quantity -, per tensor: max|g_gpu - g_64| <= k max|g_64|, k = 8 x the float32 noise floor, the floor
     being max|g_32 - g_64| / max|g_64| of torch's CPU float32 autograd on the same inputs; one k per group (critics, actor) and
     minibatch: the largest floor over the group's tensors that are held to it.  The actor's reference runs at the device's POST-step
     critic parameters and the alpha of the start of the step.
 (c) Adam and Polyak against the fp64 step fed the downloaded gradient, moments, parameters and targets: |m - m_ref| <= u |m_ref|,
     |v - v_ref| <= u |v_ref|, |p - p_ref| <= ulp(p) / 2 + 2^-36 |delta p|, |target - target_ref| <= ulp / 2.
HB_SAC_PARITY_OUT=<file> collects the measured values (profiles/sac_parity.txt)."""
import ctypes

import numpy as np
import pytest

import mlp_ref as ml
import sac_ref as sr
from oracle_lib import HUMANOID_HBM  # noqa: F401  (the model of the humanoid_model fixture)
from sac_lib import NETS, NOBS, NU, TAPES, Dev, U  # noqa: F401
from sac_lib import cfg as _cfg, check_step as _check_step, install as _install, layers as _layers, line as _line, new_worst as _new_worst
from sac_lib import problem as _problem, worst_ratio as _worst_ratio
from step_lib import report

pytestmark = pytest.mark.gpu

WIDE_Q = [69, 256, 256, 256, 1]


def _report(line):
    report(line, "HB_SAC_PARITY_OUT")


def _learner(hbmod, m, gpu, net, pb, **cfg):
    """a batch with the problem's networks, a SAC learner, the problem's targets and log_ent_coef"""
    b = hbmod.Batch(m, 16, gpu)
    _install(b, net, pb["flat"])
    b.sac_create(**cfg)
    st = b.sac_state()
    assert np.array_equal(st["params"][:-1], pb["flat"][:-1].astype(np.float32)) and st["t"] == 0 and not st["m"].any() and not st["v"].any()
    lo, hi = sr.q_range(*NETS[net])
    assert np.array_equal(st["targets"], st["params"][lo:hi])                    # the targets are made as copies
    assert st["params"][-1] == np.float32(np.log(np.float64(np.float32(cfg.get("ent_coef_init", 1.0)))))
    st["params"], st["targets"] = pb["flat"].astype(np.float32), pb["targets"].astype(np.float32)
    b.sac_set_state(st)
    return b


def _q_tensors(qsz, seed):
    rng = np.random.default_rng(seed)
    t = {}
    for k in (1, 2):
        for l in range(len(qsz) - 1):
            t["q%d.w%d" % (k, l)] = rng.normal(0.0, 1.0 / np.sqrt(qsz[l]), (qsz[l], qsz[l + 1])).astype(np.float32)
            t["q%d.b%d" % (k, l)] = rng.normal(0.0, 0.1, qsz[l + 1]).astype(np.float32)
    return t


@pytest.mark.parametrize("net", ["mixed", "one_layer", "small", "wide"])
def test_q_values_against_fp64(hbmod, humanoid_model, gpu, net):
    """hb_q_values_dev: the obs | action input tile, at the derived forward bound; 1, 16 and 40 rows"""
    qsz = WIDE_Q if net == "wide" else NETS[net][1]
    Lq = len(qsz) - 1
    t = _q_tensors(qsz, 5)
    b = hbmod.Batch(humanoid_model, 16, gpu)
    b.q_set(0, qsz, *_layers(t, "q1", qsz))
    b.q_set(1, qsz, *_layers(t, "q2", qsz))
    rng = np.random.default_rng(8)
    worst = 0.0
    for n in (1, 16, 40):
        obs, act = rng.normal(size=(n, NOBS)).astype(np.float32), np.tanh(rng.normal(size=(n, NU))).astype(np.float32)
        po, pa, p1, p2 = b.dev_alloc(obs.nbytes), b.dev_alloc(act.nbytes), b.dev_alloc(4 * n), b.dev_alloc(4 * n)
        b.to_dev(po, obs); b.to_dev(pa, act)
        b.to_dev(p1, np.full(n, np.nan, np.float32)); b.to_dev(p2, np.full(n, np.nan, np.float32))
        b.q_values_dev(po, pa, n, q1=p1, q2=p2)
        got = [b.from_dev(p1, (n,)), b.from_dev(p2, (n,))]
        b.to_dev(p1, np.full(n, np.nan, np.float32))
        b.q_values_dev(po, pa, n, q2=p1)                      # one output alone
        assert np.array_equal(b.from_dev(p1, (n,)), got[1])
        xin = np.concatenate([obs, act], axis=1).astype(np.float64)
        for k, tag in enumerate(("q1", "q2")):
            acts, q, _ = ml.forward(t, tag, Lq, xin)
            bound = ml.fwd_err(t, tag, Lq, acts)[0][:, 0]
            r = _worst_ratio(np.abs(got[k] - q[:, 0]), bound)
            worst = max(worst, r)
            assert r <= 1.0, (net, n, tag, r)
        for p in (po, pa, p1, p2):
            b.dev_free(p)
    b.close()
    _report("sac q_values %-9s: worst |Q - Q_64| / derived forward bound over 1, 16, 40 rows %.3f" % (net, worst))


@pytest.mark.parametrize("net", sorted(NETS))
def test_one_step_from_the_downloaded_state(hbmod, humanoid_model, gpu, net):
    pytest.importorskip("torch")
    pb = _problem(net, 200)
    cfg = _cfg(lr_actor=1e-3, lr_critic=1e-3, lr_ent=1e-3, ent_coef_init=0.3)
    b = _learner(hbmod, humanoid_model, gpu, net, pb, **cfg)
    worst = _new_worst()
    rng = np.random.default_rng(9)
    _check_step(b, net, pb, np.array([7]), cfg, worst, "mb1", contiguous=True)
    _check_step(b, net, pb, rng.permutation(200)[:40], cfg, worst, "mb40_index")
    _check_step(b, net, pb, np.arange(100, 164), cfg, worst, "mb64_first", contiguous=True)
    _check_step(b, net, pb, rng.permutation(200), cfg, worst, "mb200_index")
    b.close()
    _report(_line("sac step %-9s" % net, worst))


def test_one_step_of_4112_rows(hbmod, humanoid_model, gpu):
    """more than 64 rows per chunk (80) and a short last chunk (32 rows)"""
    pytest.importorskip("torch")
    import humanoid_mujoco_amd.engine as eng
    assert eng.ppo_row_chunk(4112) == 80 and 4112 % 80 == 32
    pb = _problem("small", 4112)
    cfg = _cfg(lr_actor=1e-3, lr_critic=1e-3, lr_ent=1e-3, ent_coef_init=0.3)
    b = _learner(hbmod, humanoid_model, gpu, "small", pb, **cfg)
    worst = _new_worst()
    _check_step(b, "small", pb, np.arange(4112), cfg, worst, "mb4112", contiguous=True)
    b.close()
    _report(_line("sac step small, 4112 rows", worst))


def test_three_consecutive_steps_interval_and_fixed_ent_coef(hbmod, humanoid_model, gpu):
    """each step held to a reference restarted from the state downloaded before it: a forward operand, a packed transpose or a target
    operand left stale behind Adam or Polyak shows in the next step.  target_update_interval 2: the targets stay on steps 1 and 3;
    then auto_ent = 0: log_ent_coef stays"""
    pytest.importorskip("torch")
    net = "small"
    pb = _problem(net, 200)
    cfg = _cfg(lr_actor=3e-3, lr_critic=3e-3, lr_ent=3e-3, ent_coef_init=0.3, target_update_interval=2, tau=0.05)
    b = _learner(hbmod, humanoid_model, gpu, net, pb, **cfg)
    worst = _new_worst()
    rng = np.random.default_rng(4)
    p0 = b.sac_params()
    for i in range(3):
        _check_step(b, net, pb, rng.permutation(200)[:70], cfg, worst, "step%d" % i)
    assert b.sac_state()["t"] == 3 and np.abs(b.sac_params() - p0).max() > 1e-3
    cfg = _cfg(lr_actor=3e-3, lr_critic=3e-3, lr_ent=3e-3, ent_coef_init=0.3, target_update_interval=1, tau=0.05, auto_ent=0)
    b.sac_configure(**cfg)
    _check_step(b, net, pb, rng.permutation(200)[:70], cfg, worst, "fixed_ent")
    b.close()
    _report(_line("sac four steps small   ", worst))


def test_determinism_draws_and_checkpoint(hbmod, humanoid_model, gpu):
    net = "mixed"
    pb = _problem(net, 200)
    cfg = _cfg(lr_actor=1e-3, lr_critic=1e-3, lr_ent=1e-3, seed=5)
    b = _learner(hbmod, humanoid_model, gpu, net, pb, **cfg)
    sel = np.random.default_rng(2).permutation(200)[:65]
    s0 = b.sac_state()

    def run(dev, given, t=None):
        st = dict(s0)
        if t is not None:
            st["t"] = t
        b.sac_set_state(st)
        stats = dev.step(eps_given=given)
        return stats, b.sac_state(), b.sac_grads()
    # the same state, rows and t: the same bits
    d = Dev(b, pb["rows"], 65, pb["eps_pi"][sel], pb["eps_next"][sel], sel)
    a1, a2 = run(d, True), run(d, True)
    assert np.array_equal(a1[0], a2[0]) and np.array_equal(a1[2], a2[2]) and all(np.array_equal(a1[1][k], a2[1][k]) for k in ("params", "m", "v", "targets"))
    d.free()
    # draws made on the device: recorded, the same at equal t, others at another t; fed back they reproduce the step bit for bit
    d = Dev(b, pb["rows"], 65, None, None, sel)
    r1 = run(d, False)
    e1 = d.draws()
    r2 = run(d, False)
    e2 = d.draws()
    r3 = run(d, False, t=1)
    e3 = d.draws()
    assert all(np.isfinite(e).all() for e in e1) and np.array_equal(e1[0], e2[0]) and np.array_equal(e1[1], e2[1])
    assert not np.array_equal(e1[0], e3[0]) and not np.array_equal(e1[1], e3[1]) and not np.array_equal(e1[0], e1[1])
    assert abs(float(e1[0].mean())) < 0.1 and abs(float(e1[0].std()) - 1.0) < 0.1
    assert np.array_equal(r1[2], r2[2]) and not np.array_equal(r1[2], r3[2])
    d.free()
    d = Dev(b, pb["rows"], 65, e1[0], e1[1], sel)
    r4 = run(d, True)
    assert np.array_equal(r1[0], r4[0]) and np.array_equal(r1[2], r4[2]) and all(np.array_equal(r1[1][k], r4[1][k]) for k in ("params", "m", "v", "targets"))
    # get_state -> two steps equals set_state of that record -> two steps
    ck = b.sac_state()
    assert ck["t"] == 1

    def two():
        d.step(eps_given=False)
        d.step(eps_given=False)
        return b.sac_state()
    x = two()
    b.sac_set_state(ck)
    y = two()
    assert x["t"] == y["t"] == 3 and all(np.array_equal(x[k], y[k]) for k in ("params", "m", "v", "targets")) and not np.array_equal(x["params"], ck["params"])
    # the packed operands re-made from the flat record (zero padded by construction): the same bits
    g3 = (d.step(eps_given=False), b.sac_grads())
    b.sac_set_state(y)
    b.sac_set_params(y["params"])
    g4 = (d.step(eps_given=False), b.sac_grads())
    assert np.array_equal(g3[0], g4[0]) and np.array_equal(g3[1], g4[1])
    d.free()
    b.close()


def test_purity(hbmod, humanoid_model, gpu):
    """sac_step_dev leaves the batch's state, status words, hb_last_kernel and the step-launch count; the collection's draw counter is
    covered by test_the_loop (two collections around an update differ from each other as the counter says)"""
    net = "small"
    pb = _problem(net, 200)
    b = _learner(hbmod, humanoid_model, gpu, net, pb, **_cfg())
    b.reset(perturb=True)
    b.step(np.zeros((16, humanoid_model.nu), np.float32))
    d = Dev(b, pb["rows"], 50, None, None, None)
    before = (b.get_state(hbmod.STATE_INTEGRATION), b.last_kernel(), b.step_launches(), b.status().copy())
    d.step(first=3, eps_given=False)
    after = (b.get_state(hbmod.STATE_INTEGRATION), b.last_kernel(), b.step_launches(), b.status().copy())
    assert np.array_equal(before[0], after[0]) and before[1:3] == after[1:3] and np.array_equal(before[3], after[3])
    assert b.sac_state()["t"] == 1
    d.free()
    b.close()


def test_the_loop(hbmod, humanoid_model, gpu):
    """VecEnv: collect_torch -> ReplayBuffer.add -> sac_update, no actor_set: the next collection runs the trained actor, and its draws
    are those of an identically seeded env that made no update (the draw counter is untouched)"""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    net = "mixed"
    asz, qsz = NETS[net]
    pb = _problem(net, 200)
    t0 = sr.split(pb["flat"].astype(np.float32), asz, qsz)
    envs = []
    for _ in range(2):
        env = hbmod.VecEnv(humanoid_model, 16, gpu, seed=7)
        env.actor_set(asz, *_layers(t0, "actor", asz), head="squashed")
        env.q_set(0, qsz, *_layers(t0, "q1", qsz))
        env.q_set(1, qsz, *_layers(t0, "q2", qsz))
        env.reset()
        envs.append(env)
    env, twin = envs
    env.sac_learner(lr_actor=1e-2, lr_critic=1e-2, lr_ent=1e-2)
    rb = hbmod.ReplayBuffer(256, NOBS, NU, torch.device("cuda", gpu))
    buf = env.collect_torch(4, terminal_obs=True)
    twin.collect_torch(4, terminal_obs=True)
    rb.add(buf)
    assert rb.size == 64
    log = env.sac_update(rb, gradient_steps=3, batch_size=32)
    assert log["n_updates"] == 3 and np.isfinite(list(log.values())).all() and log["ent_coef"] > 0.9
    st = env.batch.sac_state()
    assert st["t"] == 3
    flat = st["params"]
    t = sr.split(flat.astype(np.float64), asz, qsz)
    assert np.abs(flat[:-1] - pb["flat"][:-1]).max() > 1e-3
    out = {k: v.cpu().numpy() for k, v in env.collect_torch(4, terminal_obs=True).items()}
    ref = {k: v.cpu().numpy() for k, v in twin.collect_torch(4, terminal_obs=True).items()}
    assert np.array_equal(out["eps"], ref["eps"]) and np.abs(out["eps"]).max() > 0       # the draw counter stayed
    La = len(asz) - 1
    for tt, differs in ((t, False), (sr.split(pb["flat"], asz, qsz), True)):
        acts, o64, _ = ml.forward(tt, "actor", La, out["obs"][:4].reshape(64, NOBS).astype(np.float64))
        e = ml.fwd_err(tt, "actor", La, acts)[0]
        mean64, ls64 = o64[:, :NU].reshape(4, 16, NU), np.clip(o64[:, NU:], -20, 2).reshape(4, 16, NU)
        ok = (np.abs(out["mean"] - mean64) <= e[:, :NU].reshape(4, 16, NU)).all() and (np.abs(out["log_std"] - ls64) <= e[:, NU:].reshape(4, 16, NU)).all()
        assert ok != differs
    env.close()
    twin.close()


def test_refusals(hbmod, humanoid_model, gpu):
    import humanoid_mujoco_amd.engine as eng
    L = hbmod.lib()
    net = "mixed"
    asz, qsz = NETS[net]
    pb = _problem(net, 200)
    t = sr.split(pb["flat"].astype(np.float32), asz, qsz)
    b = hbmod.Batch(humanoid_model, 16, gpu)
    cfg = eng.HbSacConfig()
    L.hb_sac_default_config(ctypes.byref(cfg))

    def create():
        return L.hb_sac_create(b._h, ctypes.byref(cfg))
    d0 = Dev(b, pb["rows"], 40, pb["eps_pi"][:40], pb["eps_next"][:40])
    pp = [d0.ptr[k] for k in TAPES]

    def step(**kw):
        a = dict(obs=pp[0], action=pp[1], reward=pp[2], next_obs=pp[3], done=pp[4], index=None, n_rows=200, first=0, mb=40, eps_pi=d0.eps[0],
                 eps_next=d0.eps[1], eps_given=1)
        a.update(kw)
        return L.hb_sac_step_dev(b._h, ctypes.byref(eng.HbSacRows(**a)), None)
    buf = np.zeros(8, np.float32)
    tt = ctypes.c_longlong()
    # calls without a learner
    assert step() == -1 and L.hb_sac_destroy(b._h) == -1 and L.hb_sac_configure(b._h, ctypes.byref(cfg)) == -1
    assert L.hb_sac_param_count(b._h) == -1 and L.hb_sac_target_count(b._h) == -1 and L.hb_sac_get_params(b._h, buf.ctypes.data, 8) == -1
    assert L.hb_sac_get_state(b._h, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 8, buf.ctypes.data, 8, ctypes.byref(tt)) == -1
    # missing networks
    assert create() == -1                                                   # nothing installed
    _install(b, net, pb["flat"], actor=False)
    assert create() == -1                                                   # no actor
    gz = [NOBS, 64, NU]
    b.actor_set(gz, [t["actor.w0"], np.zeros((64, NU), np.float32)], [t["actor.b0"], np.zeros(NU, np.float32)], head="gaussian", log_std=np.zeros(NU))
    assert create() == -4
    with pytest.raises(hbmod.HbError, match="squashed"):
        b.sac_create()
    b.actor_set(gz, [t["actor.w0"], np.zeros((64, NU), np.float32)], [t["actor.b0"], np.zeros(NU, np.float32)], head="deterministic")
    assert create() == -4
    b2 = hbmod.Batch(humanoid_model, 16, gpu)
    b2.actor_set(asz, *_layers(t, "actor", asz), head="squashed")
    b2.q_set(1, qsz, *_layers(t, "q2", qsz))
    assert L.hb_sac_create(b2._h, ctypes.byref(cfg)) == -1                  # Q1 missing
    b2.q_set(0, [69, 1], [np.zeros((69, 1), np.float32)], [np.zeros(1, np.float32)])
    assert L.hb_sac_create(b2._h, ctypes.byref(cfg)) == -1                  # unequal Q sizes
    b2.close()
    # hb_q_set_mlp's own checks: a refused call leaves the installed network
    z = lambda *sh: np.zeros(sh, np.float32)  # noqa: E731
    po, pa, pq = b.dev_alloc(4 * NOBS), b.dev_alloc(4 * NU), b.dev_alloc(4)
    b.to_dev(po, z(NOBS)); b.to_dev(pa, z(NU))
    b.q_values_dev(po, pa, 1, q1=pq)
    q_before = b.from_dev(pq, (1,))
    for k, sizes, code in ((0, [68, 1], -1), (0, [69, 2], -1), (0, [69, 257, 1], -4), (2, [69, 1], -1), (-1, [69, 1], -1)):
        ws, bs = [z(sizes[l], sizes[l + 1]) for l in range(len(sizes) - 1)], [z(sizes[l + 1]) for l in range(len(sizes) - 1)]
        w_, b_, csz, wp, bp = eng._mlp_args("q_set", ws, bs, sizes)
        assert L.hb_q_set_mlp(b._h, k, len(ws), csz, wp, bp) == code, (k, sizes)
    assert L.hb_q_set_mlp(b._h, 0, 0, None, None, None) == -1
    b.q_values_dev(po, pa, 1, q1=pq)
    assert np.array_equal(b.from_dev(pq, (1,)), q_before)
    assert L.hb_q_values_dev(b._h, po, pa, 0, pq, None) == -1 and L.hb_q_values_dev(b._h, po, pa, 1, None, None) == -1
    assert L.hb_q_values_dev(b._h, None, pa, 1, pq, None) == -1
    for p in (po, pa, pq):
        b.dev_free(p)
    # the hyper-parameters
    b.actor_set(asz, *_layers(t, "actor", asz), head="squashed")
    assert L.hb_sac_create(b._h, None) == -1
    bad = (("gamma", -0.1), ("gamma", 1.5), ("tau", -0.1), ("tau", 1.1), ("lr_actor", -1e-3), ("lr_critic", -1e-3), ("lr_ent", -1e-3), ("beta1", 1.0),
           ("beta2", -0.1), ("eps", 0.0), ("ent_coef_init", 0.0), ("target_update_interval", 0), ("gamma", float("nan")), ("tau", float("inf")),
           ("lr_actor", float("nan")), ("target_entropy", float("nan")), ("ent_coef_init", float("inf")), ("eps", float("nan")))
    for k, v in bad:
        with pytest.raises(hbmod.HbError):
            b.sac_create(**{k: v})
        assert L.hb_sac_param_count(b._h) == -1
    b.sac_create(lr_critic=1e-3)
    P, PT = b.sac_param_count(), b.sac_target_count()
    lo, hi = sr.q_range(asz, qsz)
    assert P == pb["flat"].size and PT == hi - lo
    for k, v in bad:
        with pytest.raises(hbmod.HbError):
            b.sac_configure(**{k: v})
    big = np.zeros(P + 1, np.float32)
    assert L.hb_sac_get_params(b._h, big.ctypes.data, P + 1) == -1 and L.hb_sac_set_params(b._h, big.ctypes.data, P - 1) == -1
    assert L.hb_sac_get_grads(b._h, big.ctypes.data, P + 1) == -1 and L.hb_sac_get_params(b._h, None, P) == -1
    assert L.hb_sac_get_state(b._h, big.ctypes.data, big.ctypes.data, big.ctypes.data, P, big.ctypes.data, PT + 1, ctypes.byref(tt)) == -1
    assert L.hb_sac_set_state(b._h, big.ctypes.data, big.ctypes.data, big.ctypes.data, P, big.ctypes.data, PT, -1) == -1
    assert L.hb_sac_set_state(b._h, big.ctypes.data, big.ctypes.data, big.ctypes.data, P + 1, big.ctypes.data, PT, 0) == -1
    # the rows
    s0 = b.sac_state()
    assert step(mb=0) == -1 and step(n_rows=0) == -1 and step(first=161) == -1 and step(first=-1) == -1
    for k in TAPES:
        assert step(**{k: None}) == -1
    assert step(eps_pi=None) == -1 and step(eps_next=None) == -1
    assert L.hb_sac_step_dev(b._h, None, None) == -1
    s1 = b.sac_state()
    assert s1["t"] == 0 and all(np.array_equal(s0[k], s1[k]) for k in ("params", "m", "v", "targets"))   # the refused calls changed nothing
    assert step(first=160) == 0 and step(eps_pi=None, eps_next=None, eps_given=0) == 0 and b.sac_state()["t"] == 2
    # hb_actor_set_mlp and hb_q_set_mlp destroy the learner
    b.actor_set(asz, *_layers(t, "actor", asz), head="squashed")
    assert L.hb_sac_param_count(b._h) == -1 and step() == -1
    b.sac_create()
    b.q_set(1, qsz, *_layers(t, "q2", qsz))
    assert L.hb_sac_param_count(b._h) == -1
    b.sac_create()
    b.sac_destroy()
    assert L.hb_sac_param_count(b._h) == -1
    d0.free()
    b.close()
