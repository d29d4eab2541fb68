"""On-device rollout collection (include/hb.h: hb_actor_set_mlp, hb_env_collect_dev): the actor kernel against the fp64 reference of
tests/actor_ref.py, and the loop against hb_env_step_dev driven from Python with the recorded actions.

Shapes: 37 envs (three blocks of 16, the last with 5 live rows) and 64 (full blocks); networks 48 -> 40 -> 24 -> 21 (-> 42 for the squashed
head): widths that are neither multiples of 16 nor all multiples of 4, every layer on the split-K path, and once the reference's
48 -> 256 -> 256 -> 21 (sixteen output tiles: no split).  T = 8.

Bounds:
  mean, log_std  5e-5 - tests/test_gpu_policy.py's bound for the same arithmetic (f32 MFMA chains, tanhf) - times max(1, |ref|) for the
                 linear last layers, whose outputs are not confined to (-1, 1);
  eps            2e-5 absolute - the stricter of the two tolerances (2e-5, 5e-5) tests/test_gpu_env_realism.py holds observations that carry
                 the device's normal draws to.  (Box-Muller in fp32: the angle 2 pi u2 carries <= 6e-7 of rounding, the radius is below 5.9
                 and carries 2e-7 relative: <= 5e-6.)
  action         the head formula in fp64 on the device's OWN mean / log_std / eps tapes: 2e-6 max(1, |action|, sigma |eps|) for the Gaussian
                 head (one expf, one product, one sum in fp32; |eps| <= 5.9 for a 24-bit uniform), 2e-6 absolute for the squashed head (tanhf
                 on top, slope <= 1), and equality with mean for the deterministic one.
HB_COLLECT_PARITY_OUT=<file> collects the worst values (profiles/collect_parity.txt)."""
import numpy as np
import pytest

import actor_ref as ar
from bounds import MEAN_TOL
from oracle_lib import HUMANOID_HBM, TEAM_HBM  # noqa: F401  (the model of the humanoid_model fixture)
from step_lib import report

pytestmark = pytest.mark.gpu

SEED, T, NOBS, NU = 2024, 8, 48, 21  # (tests/test_actor_cpu.py checks the draws of this seed)
EPS_TOL, ACT_TOL = 2e-5, 2e-6


def _report(line):
    report(line, "HB_COLLECT_PARITY_OUT")


class Tapes:
    """device buffers of one collection, through the library's own allocation helpers (no torch in this file)"""
    FIELDS = ("obs", "action", "mean", "log_std", "eps", "reward", "terminated", "truncated", "terminal_obs")

    def __init__(self, batch, T, nobs, nu, log_std=False, terminal_obs=False, only=None):
        n = batch.n_env
        self.b, self.T = batch, T
        self.shape = {"obs": (T + 1, n, nobs), "action": (T, n, nu), "mean": (T, n, nu), "eps": (T, n, nu), "reward": (T, n),
                      "terminated": (T, n), "truncated": (T, n)}
        if log_std:
            self.shape["log_std"] = (T, n, nu)
        if terminal_obs:
            self.shape["terminal_obs"] = (T, n, nobs)
        if only is not None:
            self.shape = {k: v for k, v in self.shape.items() if k in only}
        self.dtype = {k: np.uint8 if k in ("terminated", "truncated") else np.float32 for k in self.shape}
        self.ptr = {k: batch.dev_alloc(int(np.prod(s)) * np.dtype(self.dtype[k]).itemsize) for k, s in self.shape.items()}
        for k, s in self.shape.items():  # (a tape the call should have written and did not must not pass as plausible numbers)
            batch.to_dev(self.ptr[k], np.full(s, 0xEE if self.dtype[k] == np.uint8 else np.nan, dtype=self.dtype[k]))

    def collect(self, obs0, n_substeps=1):
        self.b.to_dev(self.ptr["obs"], np.ascontiguousarray(obs0, dtype=np.float32))
        self.b.env_collect_dev(self.T, n_substeps, **self.ptr)
        return self.read()

    def read(self):
        return {k: self.b.from_dev(self.ptr[k], s, self.dtype[k]) for k, s in self.shape.items()}

    def free(self):
        for p in self.ptr.values():
            self.b.dev_free(p)
        self.ptr = {}


def _sizes(head, hidden=(40, 24), nobs=NOBS, nu=NU):
    return [nobs, *hidden, 2 * nu if head == ar.SQUASHED else nu]


def _log_std(nu=NU):
    return np.linspace(-1.5, 0.3, nu).astype(np.float32)


def _make_env(hbmod, model, n, gpu, **kw):
    kw.setdefault("max_time", 0.02)  # four control steps of 5 ms: every env ends an episode inside T = 8 and is reset in place
    kw.setdefault("target_z", 10.0)  # (out of reach: standupReward's success - standing, which the reset pose is - ends no episode)
    return hbmod.VecEnv(model, n, gpu, realism=True, domain_randomization=True, seed=7, **kw)


@pytest.mark.parametrize("head", [ar.DETERMINISTIC, ar.GAUSSIAN, ar.SQUASHED])
@pytest.mark.parametrize("n", [37, 64])
def test_actor_matches_fp64_reference(hbmod, humanoid_model, gpu, head, n):
    _check_actor(hbmod, humanoid_model, gpu, head, n, (40, 24))


def test_actor_reference_sizes(hbmod, humanoid_model, gpu):
    """48 -> 256 -> 256 -> 21, the sizes the reference trains (simulation/hyperparam_config.py:21-27), Gaussian head"""
    _check_actor(hbmod, humanoid_model, gpu, ar.GAUSSIAN, 37, (256, 256))


def _check_actor(hbmod, m, gpu, head, n, hidden):
    assert (m.nobs, m.nu) == (NOBS, NU)
    env = _make_env(hbmod, m, n, gpu)
    b = env.batch
    sizes = _sizes(head, hidden)
    # (weights wide enough that the means leave (-1, 1) and the squashed head's log_std varies over several units, past the upper clamp)
    ws, bs = ar.make_actor(sizes, seed=11, scale=0.35)
    ls = _log_std()
    b.actor_set(sizes, ws, bs, head=head, log_std=ls if head == ar.GAUSSIAN else None, seed=SEED)
    tp = Tapes(b, T, NOBS, NU, log_std=head == ar.SQUASHED)
    out = tp.collect(env.reset())
    tp.free()
    assert all(np.isfinite(v).all() for k, v in out.items() if v.dtype == np.float32), [k for k, v in out.items() if v.dtype == np.float32 and not np.isfinite(v).all()]
    eps_ref = ar.draws(SEED, 0, n, NU, 0, T) if head != ar.DETERMINISTIC else np.zeros((T, n, NU))
    worst = {"mean": 0.0, "log_std": 0.0, "eps": 0.0, "action": 0.0}
    for t in range(T):
        ref = ar.actor(out["obs"][t], ws, bs, head, log_std=ls, eps=eps_ref[t])  # on the device's own recorded observations
        worst["mean"] = max(worst["mean"], float((np.abs(out["mean"][t] - ref["mean"]) / np.maximum(1.0, np.abs(ref["mean"]))).max()))
        if head == ar.SQUASHED:
            worst["log_std"] = max(worst["log_std"], float((np.abs(out["log_std"][t] - ref["log_std"]) / np.maximum(1.0, np.abs(ref["log_std"]))).max()))
        worst["eps"] = max(worst["eps"], float(np.abs(out["eps"][t] - eps_ref[t]).max()))
        # the head on the device's own tapes
        mean64, eps64 = out["mean"][t].astype(np.float64), out["eps"][t].astype(np.float64)
        ls64 = out["log_std"][t].astype(np.float64) if head == ar.SQUASHED else np.broadcast_to(ls.astype(np.float64), mean64.shape)
        act = ar.head_action(head, mean64, ls64, eps64)
        if head == ar.DETERMINISTIC:
            assert np.array_equal(out["action"][t], out["mean"][t]) and not out["eps"][t].any()
        else:
            scale = np.maximum(1.0, np.maximum(np.abs(act), np.exp(ls64) * np.abs(eps64))) if head == ar.GAUSSIAN else 1.0
            worst["action"] = max(worst["action"], float((np.abs(out["action"][t] - act) / scale).max()))
    _report("actor head %d, %d envs, %s: mean %.3g (bound %.0e), log_std %.3g (%.0e), eps %.3g (%.0e), action %.3g (%.0e); |mean| max %.2f, log_std range [%.2f, %.2f]"
            % (head, n, "-".join(map(str, sizes)), worst["mean"], MEAN_TOL, worst["log_std"], MEAN_TOL, worst["eps"], EPS_TOL, worst["action"], ACT_TOL,
               np.abs(out["mean"]).max(), out["log_std"].min() if head == ar.SQUASHED else ls.min(), out["log_std"].max() if head == ar.SQUASHED else ls.max()))
    assert worst["mean"] < MEAN_TOL and worst["log_std"] < MEAN_TOL
    assert worst["eps"] < EPS_TOL
    assert worst["action"] < ACT_TOL
    if head == ar.SQUASHED:
        assert np.abs(out["action"]).max() <= 1.0 and out["log_std"].min() >= -20.0 and out["log_std"].max() <= 2.0
    if head != ar.DETERMINISTIC:
        assert np.abs(out["eps"]).std() > 0.5 and np.abs(out["action"] - out["mean"]).max() > 0.1
    env.close()


_replays = {}


def _replay(hbmod, gpu, kind):
    """One collection and its replay through hb_env_step_dev with the recorded actions, on two batches set up alike; computed once per kind
    and shared (read only) by the tests below.  kind: "plain" (64 envs), "pipelined" (128 envs in two segments: a pipelined batch of 64
    steps in one segment, so 128 is the smallest that is cut), "team" (the reference's robot, 16 envs, T = 4, squashed head)."""
    if kind in _replays:
        return _replays[kind]
    team = kind == "team"
    m = hbmod.Model.load(TEAM_HBM if team else HUMANOID_HBM)
    n, steps, head = (16, 4, ar.SQUASHED) if team else (128 if kind == "pipelined" else 64, T, ar.GAUSSIAN)
    envs = [hbmod.VecEnv(m, n, gpu, team=True) if team else _make_env(hbmod, m, n, gpu) for _ in range(2)]
    if kind == "pipelined":
        for e in envs:
            e.batch.pipeline(2)
            assert e.batch.segments == 2
    a, c = envs
    sizes = [m.nobs, 32, 2 * m.nu] if team else _sizes(head)
    if team:
        assert sizes == [30, 32, 24]
    ws, bs = ar.make_actor(sizes, seed=5, scale=0.3)
    a.batch.actor_set(sizes, ws, bs, head=head, log_std=None if team else _log_std(), seed=SEED)
    o0, o0c = a.reset(), c.reset()
    assert np.array_equal(o0, o0c)
    launches0 = a.batch.step_launches()
    tp = Tapes(a.batch, steps, m.nobs, m.nu, log_std=team, terminal_obs=True)
    out = tp.collect(o0, a.n_substeps)
    tp.free()
    launches = a.batch.step_launches() - launches0
    kernel = a.batch.last_kernel()
    # the replay: the same steps driven from Python, one hb_env_step_dev per recorded action row
    b = c.batch
    nb = {"action": n * m.nu * 4, "obs": n * m.nobs * 4, "reward": n * 4, "terminated": n, "truncated": n}
    ptr = {k: b.dev_alloc(v) for k, v in nb.items()}
    rep = {"obs": [], "reward": [], "terminated": [], "truncated": [], "terminal_obs": []}
    launches0 = b.step_launches()
    for t in range(steps):
        b.to_dev(ptr["action"], out["action"][t])
        b.env_step_dev(ptr["action"], ptr["obs"], ptr["reward"], ptr["terminated"], ptr["truncated"], c.n_substeps)
        rep["obs"].append(b.from_dev(ptr["obs"], (n, m.nobs)))
        rep["reward"].append(b.from_dev(ptr["reward"], (n,)))
        rep["terminated"].append(b.from_dev(ptr["terminated"], (n,), np.uint8))
        rep["truncated"].append(b.from_dev(ptr["truncated"], (n,), np.uint8))
        rep["terminal_obs"].append(b.env_terminal_obs())
    rep = {k: np.stack(v) for k, v in rep.items()}
    res = dict(out=out, rep=rep, obs0=o0, state_a=a.batch.get_state(hbmod.STATE_INTEGRATION), state_c=b.get_state(hbmod.STATE_INTEGRATION),
               launches=(launches, b.step_launches() - launches0), kernels=(kernel, b.last_kernel()), n=n, T=steps)
    for p in ptr.values():
        b.dev_free(p)
    a.close(); c.close()
    _replays[kind] = res
    return res


def _assert_replay_identical(r):
    out, rep = r["out"], r["rep"]
    assert np.array_equal(out["obs"][0], r["obs0"])
    for k in ("reward", "terminated", "truncated"):
        assert np.array_equal(out[k], rep[k]), k
    assert np.array_equal(out["obs"][1:], rep["obs"])
    assert np.array_equal(r["state_a"], r["state_c"])
    assert set(np.unique(out["terminated"])) <= {0, 1} and set(np.unique(out["truncated"])) <= {0, 1}
    assert r["launches"][0] == r["launches"][1] and r["kernels"][0] == r["kernels"][1] and r["kernels"][0].startswith("hb_")


@pytest.mark.parametrize("kind", ["plain", "pipelined"])
def test_collection_replays_as_env_step_dev(hbmod, gpu, kind):
    r = _replay(hbmod, gpu, kind)
    _assert_replay_identical(r)
    done = (r["out"]["terminated"] | r["out"]["truncated"]).astype(bool)
    assert done[:-1].any(), "no env finished and was reset inside the window"  # (and stepped on in its new episode)
    assert not done.all()


def test_terminal_observations(hbmod, gpu):
    r = _replay(hbmod, gpu, "plain")
    done = (r["out"]["terminated"] | r["out"]["truncated"]).astype(bool)
    assert done.sum() >= 1
    got, want = r["out"]["terminal_obs"], r["rep"]["terminal_obs"]
    assert np.isfinite(got).all()
    assert np.array_equal(got[done], want[done])
    assert np.array_equal(got, want)  # (the whole table: rows of envs that did not finish keep their older values in both)


def test_team_robot_collection(hbmod, gpu):
    """the reference's robot: the staged step under the collector"""
    r = _replay(hbmod, gpu, "team")
    assert r["n"] == 16 and r["T"] == 4
    for k, v in r["out"].items():
        if v.dtype == np.float32:
            assert np.isfinite(v).all(), k
    assert np.abs(r["out"]["action"]).max() <= 1.0 and r["out"]["log_std"].min() >= -20.0 and r["out"]["log_std"].max() <= 2.0
    _assert_replay_identical(r)


def test_determinism_counter_and_sharding(hbmod, humanoid_model, gpu):
    m = humanoid_model
    n = 64
    sizes = _sizes(ar.GAUSSIAN)
    ws, bs = ar.make_actor(sizes, seed=11, scale=0.35)
    ls = _log_std()
    runs = []
    for _ in range(2):
        env = _make_env(hbmod, m, n, gpu)
        env.batch.actor_set(sizes, ws, bs, head="gaussian", log_std=ls, seed=SEED)
        tp = Tapes(env.batch, T, NOBS, NU)
        first = tp.collect(env.reset())
        second = tp.collect(first["obs"][T])  # row T of the previous collection is the next one's input
        runs.append((first, second, env.batch.get_state(hbmod.STATE_INTEGRATION)))
        tp.free()
        env.close()
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]) and np.array_equal(runs[0][1][k], runs[1][1][k]), k
    assert np.array_equal(runs[0][2], runs[1][2])
    first, second = runs[0][0], runs[0][1]
    assert np.abs(first["eps"] - second["eps"]).max() > 0.1
    assert np.abs(second["eps"] - ar.draws(SEED, 0, n, NU, T, T)).max() < EPS_TOL  # the counter went on at draw0 = T
    assert np.abs(first["eps"] - ar.draws(SEED, 0, n, NU, 0, T)).max() < EPS_TOL
    # sharding: 37 envs at env offset 27 are envs 27..63 of the 64-env batch
    obs0 = np.random.default_rng(3).uniform(-1, 1, size=(n, NOBS)).astype(np.float32)
    rows = []
    for n_part, off in ((64, 0), (37, 27)):
        b = hbmod.Batch(m, n_part, gpu)
        b.reset(perturb=True, env_offset=off)
        b.actor_set(sizes, ws, bs, head="gaussian", log_std=ls, seed=SEED)
        tp = Tapes(b, 1, NOBS, NU)
        rows.append(tp.collect(obs0[off:]))
        tp.free()
        b.close()
    for k in ("eps", "action", "mean"):
        assert np.array_equal(rows[0][k][0, 27:], rows[1][k][0]), k
    assert np.abs(rows[0]["eps"][0, :37] - rows[1]["eps"][0]).max() > 0.1  # (and not the rows of envs 0..36)


@pytest.mark.parametrize("head", [ar.DETERMINISTIC, ar.GAUSSIAN, ar.SQUASHED])
def test_deterministic_flag(hbmod, humanoid_model, gpu, head):
    m = humanoid_model
    n = 37
    sizes = _sizes(head)
    ws, bs = ar.make_actor(sizes, seed=11, scale=0.35)
    env = _make_env(hbmod, m, n, gpu)
    env.batch.actor_set(sizes, ws, bs, head=head, log_std=_log_std() if head == ar.GAUSSIAN else None, seed=SEED, deterministic=True)
    tp = Tapes(env.batch, 2, NOBS, NU, log_std=head == ar.SQUASHED)
    out = tp.collect(env.reset())
    tp.free()
    env.close()
    assert not out["eps"].any()
    if head == ar.SQUASHED:
        assert np.abs(out["action"] - np.tanh(out["mean"].astype(np.float64))).max() < ACT_TOL
    else:
        assert np.array_equal(out["action"], out["mean"])


def test_head0_is_the_existing_policy(hbmod, humanoid_model, gpu):
    m = humanoid_model
    n = 37
    sizes = _sizes(ar.DETERMINISTIC)
    ws, bs = ar.make_actor(sizes, seed=11, scale=0.35)
    env = hbmod.VecEnv(m, n, gpu)  # realism off: the observation is the true state's, which is what hb_policy_eval reads
    b = env.batch
    obs0 = env.reset()
    b.set_policy_mlp(ws, bs)
    ctrl = b.policy_eval()
    b.actor_set(sizes, ws, bs, head="deterministic")
    tp = Tapes(b, 1, NOBS, NU, only=("obs", "action"))  # (and the minimal set of tapes)
    out = tp.collect(obs0)
    tp.free()
    assert np.abs(out["action"][0] - ctrl).max() < MEAN_TOL
    assert np.abs(ctrl - ar.network(obs0, ws, bs, ar.DETERMINISTIC)).max() < MEAN_TOL
    # either network is replaced without touching the other (the collection above has stepped the envs: a new evaluation)
    ctrl = b.policy_eval()
    ws2, bs2 = ar.make_actor(sizes, seed=12, scale=0.35)
    b.actor_set(sizes, ws2, bs2, head="deterministic")
    assert np.array_equal(b.policy_eval(), ctrl)
    b.set_policy_mlp(ws2, bs2)
    b.actor_set(sizes, ws, bs, head="deterministic")
    b.set_policy_mlp(ws, bs)
    assert np.array_equal(b.policy_eval(), ctrl)
    env.close()


def test_collect_torch_and_numpy_forms(hbmod, humanoid_model, gpu):
    """VecEnv.collect / collect_torch: the dict of tapes, the default obs0 (what the VecEnv last returned), and chaining"""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    m = humanoid_model
    n = 37
    sizes = _sizes(ar.SQUASHED)
    ws, bs = ar.make_actor(sizes, seed=11, scale=0.35)
    envs = [_make_env(hbmod, m, n, gpu) for _ in range(2)]
    for e in envs:
        e.actor_set(sizes, ws, bs, head="squashed", seed=SEED)
    a, c = envs
    o0 = a.reset()
    c.reset()
    r1 = a.collect(4, terminal_obs=True)  # starts from reset()'s observation
    assert sorted(r1) == sorted(["obs", "action", "mean", "eps", "log_std", "reward", "terminated", "truncated", "terminal_obs"])
    assert r1["obs"].shape == (5, n, NOBS) and r1["action"].shape == (4, n, NU) and r1["reward"].shape == (4, n) and r1["terminated"].dtype == bool
    assert np.array_equal(r1["obs"][0], o0)
    t2 = a.collect_torch(4)  # continues from row T of the collection before it
    assert t2["obs"].is_cuda and t2["terminated"].dtype == torch.bool and "terminal_obs" not in t2
    r2 = {k: v.cpu().numpy() for k, v in t2.items()}
    assert np.array_equal(r2["obs"][0], r1["obs"][4])
    tp = Tapes(c.batch, 8, NOBS, NU, log_std=True)
    ref = tp.collect(o0)
    tp.free()
    for k in ("obs", "action", "eps", "reward"):
        assert np.array_equal(np.concatenate([r1[k][:4], r2[k]]), ref[k]), k  # (obs: rows 0..3, then the second collection's five)
    # a step in between: the next collection starts from its observation
    obs, *_ = a.step_arrays(np.zeros((n, NU), np.float32))
    r3 = a.collect(1)
    assert np.array_equal(r3["obs"][0], obs)
    for e in envs:
        e.close()


def test_argument_checks(hbmod, humanoid_model, gpu):
    import ctypes
    m = humanoid_model
    L = hbmod.lib()
    env = hbmod.VecEnv(m, 8, gpu)
    b = env.batch
    obs0 = env.reset()
    tp = Tapes(b, 2, NOBS, NU, log_std=True)

    def collect(T=2, sub=1, **drop):
        p = {k: (None if k in drop else v) for k, v in tp.ptr.items()}
        return L.hb_env_collect_dev(b._h, T, sub, ctypes.byref(hbmod.HbCollectOut(**p)))

    def install(sizes, head, log_std=None, batch=b, cfg=True):
        ws = [np.zeros((a, c), np.float32) for a, c in zip(sizes[:-1], sizes[1:])]
        bs = [np.zeros(c, np.float32) for c in sizes[1:]]
        conf = hbmod.HbActorConfig()
        conf.head = head
        if log_std is not None:
            conf.log_std[:len(log_std)] = list(log_std)
        csz = (ctypes.c_int * len(sizes))(*sizes)
        wp = (ctypes.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
        bp = (ctypes.c_void_p * len(bs))(*[x.ctypes.data for x in bs])
        return L.hb_actor_set_mlp(batch._h if batch is not None else None, len(ws), csz, wp, bp, ctypes.byref(conf) if cfg else None)

    EINVAL, EUNSUPPORTED = -1, -4
    assert collect(log_std=1) == EINVAL  # no actor installed
    # hb_actor_set_mlp
    assert install([NOBS, 32, NU], 1, batch=None) == EINVAL
    assert install([NOBS, 32, NU], 1, cfg=False) == EINVAL
    assert L.hb_actor_set_mlp(b._h, 0, None, None, None, ctypes.byref(hbmod.HbActorConfig())) == EINVAL
    assert install([NOBS, 8, 8, 8, 8, NU], 1) == EINVAL           # five layers
    assert install([NOBS + 1, 32, NU], 1) == EINVAL               # input width
    assert install([NOBS, 32, NU + 1], 1) == EINVAL               # output width
    assert install([NOBS, 32, NU], 2) == EINVAL                   # the squashed head is 2 nu wide
    assert install([NOBS, 32, 2 * NU], 1) == EINVAL
    assert install([NOBS, 32, NU], 3) == EINVAL                   # no such head
    assert install([NOBS, 32, NU], 1, log_std=[0.0] * 20 + [float("nan")]) == EINVAL
    assert install([NOBS, 32, NU], 1, log_std=[float("inf")]) == EINVAL
    assert install([NOBS, 257, NU], 1) == EUNSUPPORTED            # wider than the fused kernel's tiles: no fallback
    assert install([NOBS, 256, 2 * NU], 2) == 0
    assert collect(log_std=1) == 0 and collect() == 0             # squashed head: with and without its log_std tape
    wide = hbmod.Model.from_xml_string(_wide_xml(33))             # 33 actuators: more than hb_actor_config.log_std holds
    wb = hbmod.Batch(wide, 4, gpu)
    assert wide.nu == 33 and install([wide.nobs, 16, 33], 1, batch=wb) == EINVAL
    wb.close()
    # hb_env_collect_dev
    assert install([NOBS, 32, NU], 1, log_std=[0.0] * NU) == 0
    assert L.hb_env_collect_dev(None, 2, 1, ctypes.byref(hbmod.HbCollectOut(**tp.ptr))) == EINVAL
    assert L.hb_env_collect_dev(b._h, 2, 1, None) == EINVAL
    assert collect(T=0, log_std=1) == EINVAL and collect(sub=0, log_std=1) == EINVAL
    assert collect(obs=1, log_std=1) == EINVAL and collect(action=1, log_std=1) == EINVAL
    assert collect() == EINVAL                                    # a log_std tape with the Gaussian head
    with pytest.raises(hbmod.HbError):
        b.env_collect_dev(2, 1, **tp.ptr)
    with pytest.raises(hbmod.HbError):
        b.actor_set([NOBS, 300, NU], [np.zeros((NOBS, 300)), np.zeros((300, NU))], [np.zeros(300), np.zeros(NU)], head="gaussian", log_std=0.0)
    # the batch still steps and collects
    b.to_dev(tp.ptr["obs"], obs0)
    assert collect(log_std=1, mean=1, eps=1, reward=1, terminated=1, truncated=1) == 0
    got = tp.read()
    assert np.isfinite(got["obs"]).all() and np.isfinite(got["action"]).all()
    o, r, te, tr, _ = env.step_arrays(np.zeros((8, NU), np.float32))
    assert np.isfinite(o).all() and np.isfinite(r).all()
    tp.free()
    env.close()


def _wide_xml(nu):
    """a pendulum with nu motors on its one joint"""
    body = '<body><joint name="j0" type="hinge" axis="0 1 0"/><geom type="sphere" size="0.02" mass="0.1"/></body>'
    return '<mujoco><worldbody>%s</worldbody><actuator>%s</actuator></mujoco>' % (body, '<motor joint="j0"/>' * nu)
