"""stable-baselines3 VecEnv contract over the env entry points of libhb.so.

Replaces the stack ``DummyVecEnv([CPUEnv, ...])`` the reference trains and benchmarks with (rl/train.py:123-136,169-232,
simulation/benchmark.py:37-53; env contract simulation/cpu_env.py:374-416,676-693).  What SB3's learners and callbacks use of a VecEnv:
  ``reset() -> obs[N, nobs]``
  ``step_async(actions)``, ``step_wait() -> (obs, rewards, dones, infos)`` and ``step(actions)`` = the two in a row, finished envs reset
      in place; ``infos`` is a list of N dicts, and for an env that finished this step
          infos[i]["terminal_observation"]  the observation of the state the episode ended in (DummyVecEnv.step_wait; SAC / PPO bootstrap
                                            from it),
          infos[i]["TimeLimit.truncated"]   = truncated and not terminated (the learner bootstraps only then),
          infos[i]["is_success"]            (cpu_env.py:688-689: the env's `truncated` - in standupReward that IS success);
  ``num_envs``, ``observation_space`` / ``action_space`` (Box-like: low, high, shape, dtype, sample(), contains()), ``get_attr``,
  ``set_attr`` (rl/randomization_adaptation_callback.py:53-54 sets "randomization_factor"), ``env_method``, ``seed``, ``env_is_wrapped``,
  ``close``.
``step_arrays(actions) -> (obs, reward, terminated, truncated, infos)`` is the array form (gymnasium's vector-env tuple, infos a dict of
arrays) for callers that do not want N dicts per step; ``step_torch`` keeps everything on the GPU.  All arithmetic is in the HIP kernels.
"""
import numpy as np

from .engine import STATE_TIME, WARN_BADQACC, WARN_BADQPOS, WARN_BADQVEL, WARN_CNSTRFULL, WARN_CONTACTFULL, Batch, Model, height_scan_rays


class Box:
    """what SB3 reads of a gymnasium.spaces.Box (gymnasium is not a dependency of this package): cpu_env.py:56-63"""

    def __init__(self, low, high, shape, dtype=np.float32, seed=0):
        self.low = np.full(shape, low, dtype=dtype)
        self.high = np.full(shape, high, dtype=dtype)
        self.shape = tuple(shape)
        self.dtype = np.dtype(dtype)
        self._rng = np.random.default_rng(seed)

    def sample(self):
        return self._rng.uniform(self.low, self.high).astype(self.dtype)

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))

    def seed(self, seed=None):
        self._rng = np.random.default_rng(seed)
        return [seed]

    def __repr__(self):
        return "Box(%g, %g, %r, %s)" % (float(self.low.flat[0]), float(self.high.flat[0]), self.shape, self.dtype.name)


_NO_INFO = {}  # (shared by the envs that did not finish an episode this step: SB3 copies an info dict before it adds to one)


class VecEnv:
    def __init__(self, model, n_envs, device=0, n_substeps=1, randomization_factor=1.0, realism=False, domain_randomization=False, seed=0, team=False,
                 contact_forces=False, body_accelerations=False, height_scan=None, normalize=None, obs_extend=None, commands=None, box_manifold=False, feet=None, **reward_overrides):
        """realism=True adds CPUEnv's sensor/action noise, delay FIFOs and pushes (hb_env_randomization), scaled by
        randomization_factor exactly like the reset perturbation; domain_randomization=True draws per-env masses, floor
        friction, joint and actuator parameters at every reset (hb_domain_randomization).  team=True: the reference's own
        constants for its own robot (hb_env_team_config: obs[30] in JOINT_NAMES order, action[12], standup reset, kp = 2).
        contact_forces=True: the physics steps also write every body's contact wrench (hb_contact_readout), read with
        body_contact_forces(); such steps run the full step kernel.  body_accelerations=True: likewise every body's acceleration
        (hb_body_acc_readout), read with body_accelerations().  height_scan=dict(body=..., xs=..., ys=..., z0=1.0, cutoff=2 * z0): a grid
        of downward rays from z0 above `body` (id or name) at the offsets xs (forward) x ys (left) of its heading frame, at the geoms of the
        world body only (hb_ray_configure: yaw frame, static), read with height_scan() / height_scan_torch(); the observation is unchanged
        unless obs_extend asks for the scan.
        obs_extend=dict(prev_action=True, height_scan=dict(offset=z0, scale=1.0, clip=(lo, hi))) (any subset): every observation this
        VecEnv produces - reset, step*, step_torch, the tapes of collect*, terminal observations - gains, behind the model's nobs entries,
        the action the env last applied (zero after a reset) and one entry per ray of height_scan=..., clamp(scale * (offset - distance),
        lo, hi) - with offset = z0 the terrain height relative to the body (hb_env_obs_extend); `nobs`, observation_shape and
        obs_layout() describe the row, and actor, critic, Q networks, normaliser, learners and ReplayBuffer are sized by it.  Extension
        entries carry no sensor noise and no delay.  obs_extend=None, or a dict with everything off: the observation is the model's.
        commands=dict(vx_min=..., vx_max=..., vy_min=..., vy_max=..., yaw_min=..., yaw_max=..., resample_time=..., zero_fraction=...,
        w_yaw=..., frame=1, observe=1, seed=...) (any subset; {} for the defaults of hb_env_default_commands, seed defaulting to this
        VecEnv's): every env follows its own commanded planar velocity and yaw rate, drawn on the device at every episode start and every
        resample_time seconds, rewarded by the linear and the yaw term (target_velocity is ignored) and - with observe - seen as the
        last three entries of every row, behind the extension: obs_layout()["command"]; commands() and set_commands() read and override
        them.  set_attr("randomization_factor", ...) does NOT scale the command ranges: they are the task, not a disturbance.
        feet=dict(bodies=("foot_right", "foot_left"), penalised=(...), terminal=(...), contact_threshold=..., w_air_time=...,
        air_time_target=..., air_gate=1, air_cmd_min=..., w_force=..., force_max=..., w_stumble=..., stumble_ratio=..., w_collision=...,
        observe=1) (bodies by name or id; the rest any subset of hb_env_feet, defaults of hb_env_default_feet): the foot-contact terms of
        the env kernel (hb_env_feet_configure) - an air-time reward paid at touchdown, penalties on hard impacts, on stumbling and on
        contacts of the penalised bodies, the end of the episode when a terminal body touches anything - read from the contact read-out on
        the device (contact_forces is switched on); with observe the n_feet contact flags sit directly in front of the command:
        obs_layout()["foot_contact"]; foot_contacts() and foot_air_time() read the state.
        normalize=dict(norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8) (any subset; {} for the
        defaults): stable-baselines3's VecNormalize over a VecMonitor on the device (hb_norm_*): reset, step*, step_torch and collect*
        return normalised observations and rewards, finished envs' infos carry "episode": {"r", "l"} and a normalised
        terminal_observation; `training`, normalize_obs, get_original_obs / get_original_reward, save_normalization / load_normalization as
        in VecNormalize.  normalize=None: every path is unchanged.
        box_manifold=True: box - box pairs give a clipped face manifold of up to eight contacts (Model.box_manifold) in place of the
        portal search's one; set on the model before the batch is built.  False leaves the model as it came."""
        self.model = model if isinstance(model, Model) else Model.load(model)
        if box_manifold:
            self.model.box_manifold(1)
        self.batch = Batch(self.model, n_envs, device)
        self.num_envs = int(n_envs)
        self.n_substeps = int(n_substeps)
        self.copy_outputs = True  # False: step() returns views of the page-locked transfer record, valid until the next step() (saves four host copies)
        self.cfg = self.batch.env_team_config() if team else self.batch.env_default_config()
        self.team = bool(team)
        self.cfg.reset_perturb = float(randomization_factor)
        for k, v in reward_overrides.items():
            if not hasattr(self.cfg, k):
                raise AttributeError("unknown env parameter %r" % k)
            setattr(self.cfg, k, v)
        self.batch.env_configure(self.cfg)
        self.contact_forces = bool(contact_forces)
        if self.contact_forces:
            self.batch.contact_readout(True)
        self._body_accelerations = bool(body_accelerations)
        if self._body_accelerations:
            self.batch.body_acc_readout(True)
        self._scan = None
        self._last_obs = None  # the observation last returned (host array or CUDA tensor): collect()'s default starting point
        self._device = int(device)
        if height_scan is not None:
            hs = dict(height_scan)
            body = hs.pop("body")
            body = self.model.name2id("body", body) if isinstance(body, str) else int(body)
            xs, ys = np.asarray(hs.pop("xs"), dtype=np.float32).reshape(-1), np.asarray(hs.pop("ys"), dtype=np.float32).reshape(-1)
            z0 = float(hs.pop("z0", 1.0))
            cutoff = float(hs.pop("cutoff", 2.0 * z0))
            if hs or cutoff <= 0:
                raise ValueError("height_scan: body, xs, ys, z0 and a cutoff > 0 (got %r)" % sorted(hs))
            pnt, vec = height_scan_rays(xs, ys, z0)
            self.batch.ray_configure(pnt, vec, frame="yaw", frame_body=body, static=True, moving=False, cutoff=cutoff)
            self._scan = (len(ys), len(xs), cutoff)
        # the extension of the observation, ahead of everything that is sized by it (the terminal-observation table, the normaliser)
        ext = dict(obs_extend or {})
        ext_scan, ext_act = ext.pop("height_scan", None), bool(ext.pop("prev_action", False))
        if ext:
            raise TypeError("obs_extend: unknown option(s) %s" % sorted(ext))
        if ext_scan is not None and self._scan is None:
            raise ValueError("obs_extend: height_scan needs the VecEnv's height_scan=dict(body=..., xs=..., ys=...)")
        if ext_act or ext_scan is not None:
            self.batch.obs_extend(prev_action=ext_act, height_scan=ext_scan)
        # velocity commands: with observe they widen the row too, so they also come before everything sized by it
        self.commands_cfg = None
        if commands is not None:
            self.commands_cfg = self.batch.default_commands()
            self.commands_cfg.seed = int(seed)
            for k, v in dict(commands).items():
                if not hasattr(self.commands_cfg, k):
                    raise TypeError("commands: unknown option %r" % k)
                setattr(self.commands_cfg, k, v)
            self.batch.commands_configure(self.commands_cfg)
        # foot-contact terms: with observe they widen the row as well
        self.feet_cfg = None
        if feet is not None:
            opts = dict(feet)
            self.feet_cfg = self.batch.default_feet()
            ids = {k: [self.model.name2id("body", b) if isinstance(b, str) else int(b) for b in opts.pop(k)]
                   for k in ("bodies", "penalised", "terminal") if k in opts}
            if any(i < 0 for v in ids.values() for i in v):
                raise ValueError("feet: a body name is not in the model")
            self.feet_cfg.set_bodies(**ids)
            for k, v in opts.items():
                if not hasattr(self.feet_cfg, k) or k.endswith("_body"):
                    raise TypeError("feet: unknown option %r" % k)
                setattr(self.feet_cfg, k, v)
            self.batch.feet_configure(self.feet_cfg)
            self.contact_forces = True  # (the terms read the contact read-out, so body_contact_forces() is there too)
        self.nobs = self.batch.env_nobs
        row = self.batch.env_row()
        self._layout = {"base": slice(0, row.base)}
        for key, part in (("prev_action", "prev_action"), ("height_scan", "scan"), ("foot_contact", "foot_contact"), ("command", "command")):
            at, count = getattr(row, part), getattr(row, "n_" + part)
            if count:
                self._layout[key] = slice(at, at + count)
        self.realism = None
        if realism:
            self.realism = self.batch.env_default_randomization()
            self.realism.seed = int(seed)
            self.realism.control_timestep = float(self.model.opt.timestep * self.n_substeps)
            self._apply_realism()
        self.domain = None
        if domain_randomization:
            self.domain = self.batch.env_default_domain_randomization()
            self.domain.seed = int(seed)
            if self.team:
                self.domain.kp_nominal = 2.0  # JOINT_P_GAIN (simulation_parameters.py:35): CPUEnv overwrites the motors' gain at every reset
                self.domain.floor_bump_max = 0.1  # MAX_FLOOR_BUMP_HEIGHT
            self._apply_domain()
        # gymnasium-style space descriptions (cpu_env.py:56-63: Box(-1,1,(nu,)), Box(-10,10,(nobs,)))
        self.action_shape = (self.model.nu,)
        self.observation_shape = (self.nobs,)
        self.action_low, self.action_high = -1.0, 1.0
        self.action_space = Box(-1.0, 1.0, self.action_shape, seed=seed)
        self.observation_space = Box(-10.0, 10.0, self.observation_shape, seed=seed)
        self.seed_value = int(seed)
        self.render_mode = None
        self.batch.env_terminal_obs(fetch=False)  # the env kernel records the observation an episode ends in (hb_env_terminal_obs)
        self._norm = None
        if normalize is not None:
            opts = dict(norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8)
            unknown = set(normalize) - set(opts)
            if unknown:
                raise TypeError("normalize: unknown option(s) %s" % sorted(unknown))
            opts.update(normalize)
            self._norm = opts
            self._training = True
            self._orig_obs = self._orig_reward = None
            self.batch.norm_configure(training=True, **opts)

    def obs_layout(self):
        """the columns of an observation row as slices: "base" (the model's nobs entries), and with obs_extend "prev_action" (nu) and
        "height_scan" (len(ys) * len(xs) entries, row-major over ys then xs like height_scan()), with observed feet "foot_contact" (n_feet
        flags, 0 or 1, directly in front of the command) and with observed commands "command" (vx, vy, yaw rate: the last three entries)"""
        return dict(self._layout)

    def _need_feet(self, what):
        if self.feet_cfg is None:
            raise RuntimeError("%s: create the VecEnv with feet=dict(bodies=...)" % what)

    def foot_contacts(self):
        """[num_envs, n_feet] bool: the feet in contact at the last step evaluation (ones at an episode start; Batch.feet)"""
        self._need_feet("foot_contacts")
        return self.batch.feet()[1].astype(bool)

    def foot_air_time(self):
        """[num_envs, n_feet] float32: the state time minus the time each foot was last evaluated in contact (0 while it stands)"""
        self._need_feet("foot_air_time")
        return self.batch.get_state(STATE_TIME).reshape(-1, 1) - self.batch.feet()[0]

    def commands(self):
        """[num_envs, 3] float32: every env's current (vx, vy, yaw rate) command (Batch.commands)"""
        return self.batch.commands()

    def set_commands(self, cmd, mask=None):
        """overrides the current command of the envs of `mask` (None: all) until their next scheduled draw (Batch.set_commands)"""
        self.batch.set_commands(cmd, mask)

    # ---- VecNormalize's surface (normalize=...)
    def _need_norm(self, what):
        if self._norm is None:
            raise RuntimeError("%s: create the VecEnv with normalize=dict(...)" % what)

    @property
    def training(self):
        """VecNormalize.training: False freezes the running statistics (evaluation); the monitor keeps counting"""
        self._need_norm("training")
        return self._training

    @training.setter
    def training(self, on):
        self._need_norm("training")
        self._training = bool(on)
        self.batch.norm_configure(training=self._training, **self._norm)

    def _norm_host(self):
        """the device block the host paths stage a step in: obs | reward | ep_return | ep_length | terminal_obs | terminated | truncated"""
        h = getattr(self, "_norm_dev", None)
        if h is None:
            n, nobs = self.num_envs, self.nobs
            ob, rb = n * nobs * 4, n * 4
            base = self.batch.dev_alloc(2 * ob + 3 * rb + 2 * n)
            h = self._norm_dev = dict(obs=base, reward=base + ob, ep_ret=base + ob + rb, ep_len=base + ob + 2 * rb, tobs=base + ob + 3 * rb,
                                      term=base + 2 * ob + 3 * rb, trunc=base + 2 * ob + 3 * rb + n, ob=ob, rb=rb)
        return h

    def _norm_reset_host(self, obs):
        h = self._norm_host()
        self._orig_obs, self._orig_reward = obs, None
        self.batch.to_dev(h["obs"], obs)
        self.batch.norm_reset_dev(h["obs"], h["obs"])
        return self.batch.from_dev(h["obs"], obs.shape)

    def _norm_step_host(self, obs, rew, term, trunc):
        """one normaliser step on host arrays: (obs, reward, ep_return, ep_length), and the normalised terminal observations kept for
        _sb3 when an env finished"""
        h, n, nobs = self._norm_host(), self.num_envs, self.nobs
        self._orig_obs, self._orig_reward = obs, rew
        done = term | trunc
        self.batch.to_dev(h["obs"], np.concatenate([np.ascontiguousarray(obs, np.float32).reshape(-1), np.ascontiguousarray(rew, np.float32)]))
        self.batch.to_dev(h["term"], np.concatenate([term.astype(np.uint8), trunc.astype(np.uint8)]))
        tobs = None
        if done.any():
            self.batch.to_dev(h["tobs"], self.batch.env_terminal_obs())
            tobs = h["tobs"]
        self.batch.norm_step_dev(h["obs"], h["obs"], h["reward"], h["term"], h["trunc"], reward_out=h["reward"], terminal_obs_in=tobs,
                                 terminal_obs_out=tobs, ep_return_out=h["ep_ret"], ep_length_out=h["ep_len"])
        out = self.batch.from_dev(h["obs"], (n * nobs + 3 * n,))
        self._norm_tobs = self.batch.from_dev(h["tobs"], (n, nobs)) if tobs else None
        return out[:n * nobs].reshape(n, nobs), out[n * nobs:n * nobs + n], out[n * nobs + n:n * nobs + 2 * n], out[n * nobs + 2 * n:].view(np.int32)

    def normalize_obs(self, x):
        """VecNormalize.normalize_obs: x [..., nobs] (array or CUDA tensor) with the current statistics, no update (hb_norm_obs_dev)"""
        self._need_norm("normalize_obs")
        nobs = self.nobs
        if isinstance(x, np.ndarray) or not hasattr(x, "data_ptr"):
            a = np.ascontiguousarray(x, dtype=np.float32)
            assert a.shape[-1] == nobs and a.size, a.shape
            p = self.batch.dev_alloc(a.nbytes)
            try:
                self.batch.to_dev(p, a)
                self.batch.norm_obs_dev(p, p, a.size // nobs)
                return self.batch.from_dev(p, a.shape)
            finally:
                self.batch.dev_free(p)
        import torch
        a = x.contiguous()
        assert a.dtype == torch.float32 and a.shape[-1] == nobs and a.numel(), tuple(a.shape)
        out = torch.empty_like(a)
        stream = torch.cuda.ExternalStream(self.batch.stream, device=a.device)
        cur = torch.cuda.current_stream(a.device)
        stream.wait_stream(cur)
        self.batch.norm_obs_dev(a.data_ptr(), out.data_ptr(), a.numel() // nobs)
        cur.wait_stream(stream)  # (whatever the caller's stream does with either tensor next is ordered behind the kernel)
        return out

    def get_original_obs(self):
        """VecNormalize.get_original_obs: the raw observations of the last reset / step* / step_torch (array or CUDA tensor)"""
        self._need_norm("get_original_obs")
        return self._orig_obs

    def get_original_reward(self):
        """VecNormalize.get_original_reward: the raw rewards of the last step* / step_torch"""
        self._need_norm("get_original_reward")
        return self._orig_reward

    def save_normalization(self, path):
        """VecNormalize.save: the flat statistics record (hb_norm_get_stats) as an .npz"""
        self._need_norm("save_normalization")
        np.savez(path, record=self.batch.norm_stats(), nobs=self.nobs)

    def load_normalization(self, path):
        self._need_norm("load_normalization")
        with np.load(path if str(path).endswith(".npz") else str(path) + ".npz") as z:
            if int(z["nobs"]) != self.nobs:
                raise ValueError("load_normalization: the record is for %d observations, this env has %d" % (int(z["nobs"]), self.nobs))
            self.batch.norm_set_stats(z["record"])

    @property
    def randomization_factor(self):
        return float(self.cfg.reset_perturb)

    def _apply_realism(self):
        self.realism.factor = float(self.cfg.reset_perturb)
        self.batch.env_randomize(self.realism if self.realism.factor > 0 else None)

    def _apply_domain(self):
        self.domain.factor = float(self.cfg.reset_perturb)
        self.batch.env_domain_randomize(self.domain if self.domain.factor > 0 else None)

    ATTRS = ("randomization_factor", "num_envs", "n_substeps", "reward_kind", "max_time", "seed_value", "render_mode")

    def get_attr(self, name, indices=None):
        """VecEnv.get_attr: the attribute of every (selected) env - all envs of a batch share their parameters"""
        if name not in self.ATTRS:
            raise AttributeError(name)
        v = getattr(self.cfg, name) if name in ("reward_kind", "max_time") else getattr(self, name)
        return [v] * len(self._indices(indices))

    def set_attr(self, name, value, indices=None):
        if name != "randomization_factor":
            raise AttributeError(name)
        self.cfg.reset_perturb = float(np.clip(value, 0.0, 1.0))
        self.batch.env_configure(self.cfg)
        if self.realism is not None:
            self._apply_realism()
        if self.domain is not None:
            self._apply_domain()

    def env_method(self, method_name, *args, indices=None, **kwargs):
        """VecEnv.env_method: the per-env methods SB3's tooling calls on CPUEnv: its reward / termination functions are the batch's"""
        if method_name == "get_wrapper_attr":
            return self.get_attr(args[0], indices)
        raise AttributeError("env method %r: the envs of a batch live on the GPU (hb_env_*), not in Python objects" % method_name)

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False] * len(self._indices(indices))

    def seed(self, seed=None):
        """VecEnv.seed: env i is seeded seed + i in SB3; here the counter-based generators take (seed, global env index) themselves"""
        self.seed_value = int(0 if seed is None else seed)
        for r in (self.realism, self.domain):
            if r is not None:
                r.seed = self.seed_value
        if self.realism is not None:
            self._apply_realism()
        if self.domain is not None:
            self._apply_domain()
        self.action_space.seed(self.seed_value)
        return [self.seed_value + i for i in range(self.num_envs)]

    def _indices(self, indices):
        if indices is None:
            return range(self.num_envs)
        return [indices] if isinstance(indices, int) else list(indices)

    def reset(self):
        self._last_obs = self.batch.env_reset()  # (a reference only: what collect() starts from when it is given no obs0)
        if self._norm is not None:
            self._last_obs = self._norm_reset_host(self._last_obs)
        return self._last_obs

    def step_async(self, actions):
        """stable-baselines3's VecEnv.step_async: the step is enqueued (actions up, physics, observations down) and the host returns at once"""
        self.batch.env_step(actions, self.n_substeps, wait=False)
        self._pending = True

    def step_wait(self):
        """VecEnv.step_wait: (obs, rewards, dones, infos) of the step_async before it, infos a list of dicts (module docstring)"""
        assert getattr(self, "_pending", False), "step_wait without step_async"
        self._pending = False
        self.batch.sync()
        return self._sb3(*self._finish(*self.batch.env_step_result(getattr(self, "copy_outputs", True))))

    def step(self, actions):
        """VecEnv.step = step_async + step_wait"""
        self.step_async(actions)
        return self.step_wait()

    def step_arrays(self, actions):
        """the same step as arrays: (obs, reward, terminated, truncated, infos) with infos a dict of arrays"""
        return self._finish(*self.batch.env_step(actions, self.n_substeps, copy=getattr(self, "copy_outputs", True)))

    def _sb3(self, obs, rew, term, trunc, arr):
        done = arr["done"]
        infos = [_NO_INFO] * self.num_envs
        if done.any():
            tobs = self.batch.env_terminal_obs() if self._norm is None else self._norm_tobs  # one more transfer, only on the steps an episode ends
            for i in np.flatnonzero(done):
                infos[i] = {"terminal_observation": tobs[i].copy(), "TimeLimit.truncated": bool(trunc[i] and not term[i]), "is_success": bool(trunc[i]),
                            "warnings": int(arr["warnings"][i])}
                if self._norm is not None:
                    infos[i]["episode"] = {"r": float(arr["ep_return"][i]), "l": int(arr["ep_length"][i])}  # (Monitor's)
        return obs, rew, done, infos

    def _finish(self, obs, rew, term, trunc):
        if self._norm is not None:
            obs, rew, ep_ret, ep_len = self._norm_step_host(obs, rew, term, trunc)
        self._last_obs = obs
        done = term | trunc
        # "warnings": the per-env HB_WARN_* bits (mjData.warning, mjdata.h:54-65): a contact or constraint-row overflow (rows were dropped for
        # that env-step) or a bad-state reset is visible to the training loop instead of silently changing that env's physics.  Polled every
        # `warning_period`-th step (default 16: the poll is one more stream synchronisation and device-to-host copy on the host-action path)
        # through hb_env_warnings, which also keeps the bits of episodes that ended - and were reset in place - between two polls: nothing is
        # lost, a bit is reported at the poll after it was raised.  A fresh array at every poll.
        self._steps = getattr(self, "_steps", 0) + 1
        if getattr(self, "_warn", None) is None or self._steps % max(1, int(getattr(self, "warning_period", 16))) == 0:
            self._warn = self.batch.env_warnings()
        w = self._warn
        infos = {"is_success": trunc.copy(), "done": done, "warnings": w,  # cpu_env.py:688-689
                 "overflow": (w & (WARN_CONTACTFULL | WARN_CNSTRFULL)) != 0}
        if self._norm is not None:
            infos["ep_return"], infos["ep_length"] = ep_ret, ep_len  # (of the episodes that ended at this step, 0 elsewhere)
        return obs, rew, term, trunc, infos

    def body_contact_forces(self):
        """[n_envs, nbody, 6]: force | torque about the body's xipos (world axes) of the contacts on every body, from the last physics
        substep of the last step (an env that finished there and was reset in place: from its reset's settle step, if it has one)."""
        if not self.contact_forces:
            raise RuntimeError("body_contact_forces: create the VecEnv with contact_forces=True")
        return self.batch.body_contact()

    def body_accelerations(self):
        """[n_envs, nbody, 6]: angular | linear acceleration of every body's xipos (world axes, gravity pseudo-acceleration included:
        +|g| upward at rest), from the last physics substep of the last step (as body_contact_forces)."""
        if not self._body_accelerations:
            raise RuntimeError("body_accelerations: create the VecEnv with body_accelerations=True")
        return self.batch.body_acc()

    def body_poses(self):
        """[n_envs, nbody, 10]: xpos | xquat (w x y z) | xipos of every body at the envs' current states - the states the last returned
        observations describe (Batch.kinematics; computed on demand from qpos)"""
        return self.batch.kinematics(pose=True, vel=False)["pose"]

    def body_velocities(self):
        """[n_envs, nbody, 6]: angular velocity | velocity of every body's xipos, world axes, at the envs' current states"""
        return self.batch.kinematics(pose=False, vel=True)["vel"]

    def geom_poses(self):
        """[n_envs, ngeom, 7]: geom_xpos | orientation quaternion (w x y z) of every geom at the envs' current states"""
        return self.batch.kinematics(pose=False, vel=False, geoms=True)["geoms"]

    def height_scan(self):
        """[n_envs, len(ys), len(xs)] float32: the distance from each point of the scan grid (z0 above the body, in its heading frame)
        down to the terrain at the envs' current states, `cutoff` where nothing is hit (Batch.rays; computed on demand from qpos)"""
        if self._scan is None:
            raise RuntimeError("height_scan: create the VecEnv with height_scan=dict(body=..., xs=..., ys=...)")
        ny, nx, cutoff = self._scan
        dist, gid = self.batch.rays()
        return np.where(gid >= 0, dist, np.float32(cutoff)).astype(np.float32).reshape(self.num_envs, ny, nx)

    def height_scan_torch(self):
        """The same as a float32 CUDA tensor, without a host transfer or synchronisation (hb_rays_dev): ordered behind the steps made so
        far on the batch's stream and visible to the caller's current torch stream, like step_torch's outputs."""
        import torch
        if self._scan is None:
            raise RuntimeError("height_scan_torch: create the VecEnv with height_scan=dict(body=..., xs=..., ys=...)")
        ny, nx, cutoff = self._scan
        dev = torch.device("cuda", self._device)
        if getattr(self, "_t_scan", None) is None:
            self._t_scan = (torch.empty((self.num_envs, ny * nx), dtype=torch.float32, device=dev), torch.empty((self.num_envs, ny * nx), dtype=torch.int32, device=dev))
        stream = torch.cuda.ExternalStream(self.batch.stream, device=dev)  # (fetching the stream launches held step calls and joins the pipes)
        cur = torch.cuda.current_stream(dev)
        stream.wait_stream(cur)  # whoever still reads the previous scan is done before it is rewritten
        dist, gid = self._t_scan
        self.batch.rays_dev(dist.data_ptr(), gid.data_ptr())
        cur.wait_stream(stream)
        return torch.where(gid >= 0, dist, torch.full_like(dist, cutoff)).reshape(self.num_envs, ny, nx)

    def dynamics(self, M=True, bias=True, passive=True, jac=None):
        """dict of float32 arrays, those asked for: "M" [n_envs, nv, nv], "bias" and "passive" [n_envs, nv], "jac" [n_envs, jac.n, 6, nv]
        (jac: a Batch.jac_spec) at the envs' current states - the states the last returned observations describe (Batch.dynamics)"""
        return self.batch.dynamics(M=M, bias=bias, passive=passive, jac=jac)

    def dynamics_torch(self, M=True, bias=True, passive=True, jac=None):
        """The same as float32 CUDA tensors, without a host transfer or synchronisation (hb_dynamics_dev): ordered behind the steps made
        so far on the batch's stream and visible to the caller's current torch stream, like step_torch's outputs.  The tensors are
        rewritten by the next call that asks for the same outputs."""
        import torch
        nv, n = self.batch.model.nv, self.num_envs
        dev = torch.device("cuda", self._device)
        shapes = {"M": (n, nv, nv) if M else None, "bias": (n, nv) if bias else None, "passive": (n, nv) if passive else None,
                  "jac": (n, jac.n, 6, nv) if jac is not None else None}
        if getattr(self, "_t_dyn", None) is None:
            self._t_dyn = {}
        out = {}
        for k, shape in shapes.items():
            if shape is not None:
                if k not in self._t_dyn or tuple(self._t_dyn[k].shape) != shape:
                    self._t_dyn[k] = torch.empty(shape, dtype=torch.float32, device=dev)
                out[k] = self._t_dyn[k]
        stream = torch.cuda.ExternalStream(self.batch.stream, device=dev)  # (fetching the stream launches held step calls and joins the pipes)
        cur = torch.cuda.current_stream(dev)
        stream.wait_stream(cur)  # whoever still reads the previous tensors is done before they are rewritten
        ptr = {k: out[k].data_ptr() if k in out else None for k in shapes}
        self.batch.dynamics_dev(ptr["M"], ptr["bias"], ptr["passive"], jac, ptr["jac"])
        cur.wait_stream(stream)
        return out

    def warning_counts(self):
        """Number of envs currently carrying each warning bit."""
        w = self.batch.status()
        return {"contact_full": int(((w & WARN_CONTACTFULL) != 0).sum()), "constraint_full": int(((w & WARN_CNSTRFULL) != 0).sum()),
                "bad_qpos": int(((w & WARN_BADQPOS) != 0).sum()), "bad_qvel": int(((w & WARN_BADQVEL) != 0).sum()), "bad_qacc": int(((w & WARN_BADQACC) != 0).sum())}

    def step_torch(self, actions):
        """The same step with the policy on the GPU: `actions` is a float32 CUDA tensor [n_envs, nu]; returns CUDA tensors
        (obs, reward, terminated, truncated) that are rewritten by the next call.  No host transfer and no host
        synchronisation: the batch's stream waits for the caller's current torch stream, and the caller's stream for the step."""
        import torch
        a = actions.contiguous()
        if getattr(self, "_t_out", None) is None:
            dev = a.device
            self._t_out = (torch.empty((self.num_envs, self.nobs), dtype=torch.float32, device=dev), torch.empty(self.num_envs, dtype=torch.float32, device=dev),
                           torch.empty(self.num_envs, dtype=torch.uint8, device=dev), torch.empty(self.num_envs, dtype=torch.uint8, device=dev))
            self._t_stream = torch.cuda.ExternalStream(self.batch.stream, device=dev)  # the batch's own HIP stream, seen by torch
        assert a.dtype == torch.float32 and tuple(a.shape) == (self.num_envs, self.model.nu)
        cur = torch.cuda.current_stream(a.device)
        self._t_stream.wait_stream(cur)   # the policy's output is complete before the step reads it
        o, r, te, tr = self._t_out
        if self._norm is None:
            self.batch.env_step_dev(a.data_ptr(), o.data_ptr(), r.data_ptr(), te.data_ptr(), tr.data_ptr(), self.n_substeps)
        else:  # the step writes the raw tensors (get_original_*), the normaliser the returned ones, on the same stream
            if getattr(self, "_t_raw", None) is None:
                self._t_raw = (torch.empty_like(o), torch.empty_like(r))
            self._orig_obs, self._orig_reward = self._t_raw
            self.batch.env_step_dev(a.data_ptr(), self._orig_obs.data_ptr(), self._orig_reward.data_ptr(), te.data_ptr(), tr.data_ptr(), self.n_substeps)
            self.batch.norm_step_dev(self._orig_obs.data_ptr(), o.data_ptr(), self._orig_reward.data_ptr(), te.data_ptr(), tr.data_ptr(), reward_out=r.data_ptr())
        cur.wait_stream(self._t_stream)   # and the caller's stream sees the results
        a.record_stream(self._t_stream)
        self._last_obs = o
        return o, r, te.view(torch.bool), tr.view(torch.bool)  # (the kernel writes 0 / 1 bytes: a view, not two conversion kernels)

    def actor_set(self, sizes, weights, biases, head="gaussian", log_std=None, seed=None, deterministic=False, activation="tanh"):
        """Installs the sampling actor collect() / collect_torch() run in the env loop (Batch.actor_set: weights[l] is [in, out], the
        transpose of torch.nn.Linear.weight; heads "deterministic", "gaussian", "squashed"; hidden activation
        "tanh", "relu" or "elu").  seed defaults to this VecEnv's seed; its
        draws are a random stream of their own, independent of the realism layer's."""
        self.batch.actor_set(sizes, weights, biases, head=head, log_std=log_std, seed=self.seed_value if seed is None else seed, deterministic=deterministic,
                             activation=activation)

    def critic_set(self, sizes, weights, biases, activation="tanh"):
        """Installs the critic collect() / collect_torch() evaluate with gae=... (Batch.critic_set: sizes [nobs, hidden..., 1], weights[l] is
        [in, out], the transpose of torch.nn.Linear.weight; hidden layers with `activation` - "tanh", "relu" or "elu" -, linear
        output)."""
        self.batch.critic_set(sizes, weights, biases, activation=activation)

    def collect_torch(self, T, obs0=None, terminal_obs=False, gae=None, raw=False):
        """T steps of the installed actor in the env loop on the device (hb_env_collect_dev): no host transfer, no host synchronisation,
        one Python call.  Returns a dict of CUDA tensors: "obs" [T + 1, n, nobs] (row 0 is obs0; row t + 1 the observation after step t,
        for an env that finished there the first of its new episode), "action", "mean", "eps" [T, n, nu] (and "log_std" with the squashed
        head), "reward" [T, n] float32, "terminated", "truncated" [T, n] bool, and with terminal_obs=True "terminal_obs" [T, n, nobs], whose
        row (t, e) is the observation of the state env e's episode ended in where terminated | truncated is set at (t, e) and an older
        value elsewhere.  obs0: the observation the envs last returned, [n, nobs] as a CUDA tensor or array; default: what this VecEnv
        last returned from reset / step* / collect* (uploaded here if it lives on the host).  The tensors are rewritten by the next
        collection of the same T.  Streams are ordered as in step_torch.
        gae=dict(gamma=..., lam=..., bootstrap_truncated=True): the PPO buffer behind the collection on the same stream (hb_collect_gae_dev,
        needs critic_set): adds "value" [T + 1, n], "advantage" and "returns" [T, n], and with the gaussian and squashed heads "log_prob"
        [T, n]; with bootstrap_truncated (the default) the terminal_obs tape is recorded whether asked for or not, and V of it is folded
        into the reward of envs cut by truncation alone, as stable-baselines3's collect_rollouts does.  gae=None: exactly the call above.
        With normalize=... (hb_env_collect_norm_dev): "obs" and "reward" are normalised, so are the rows of "terminal_obs" whose env
        finished; obs0 is a NORMALISED observation (what reset / step* / collect* returned); the dict gains "ep_return" float32 and
        "ep_length" int32 [T, n] (the return and length of the episode that ended at (t, e), 0 elsewhere), and with raw=True "raw_obs"
        [T, n, nobs] (row t: the raw form of obs[t + 1]) and "raw_reward" [T, n]; gae=... then works on the normalised tapes."""
        import torch
        T = int(T)
        if gae is not None:
            gae = dict(gae)
            g_gamma, g_lam, g_boot = float(gae.pop("gamma")), float(gae.pop("lam")), bool(gae.pop("bootstrap_truncated", True))
            if gae:
                raise TypeError("collect: unknown gae option(s) %s" % sorted(gae))
            gae = True
            terminal_obs = terminal_obs or g_boot
        n, nobs, nu = self.num_envs, self.nobs, self.model.nu
        dev = torch.device("cuda", self._device)
        squashed = getattr(self.batch, "actor_head", None) == 2
        key = (T, bool(terminal_obs), squashed)
        cache = getattr(self, "_t_collect", None)
        if cache is None:
            cache = self._t_collect = {}
        if key not in cache:
            f32 = dict(dtype=torch.float32, device=dev)
            t = {"obs": torch.empty((T + 1, n, nobs), **f32), "action": torch.empty((T, n, nu), **f32), "mean": torch.empty((T, n, nu), **f32),
                 "eps": torch.empty((T, n, nu), **f32), "reward": torch.empty((T, n), **f32),
                 "terminated": torch.empty((T, n), dtype=torch.uint8, device=dev), "truncated": torch.empty((T, n), dtype=torch.uint8, device=dev)}
            if squashed:
                t["log_std"] = torch.empty((T, n, nu), **f32)
            if terminal_obs:
                t["terminal_obs"] = torch.empty((T, n, nobs), **f32)
            cache[key] = t
        t = cache[key]
        src = self._last_obs if obs0 is None else obs0
        if src is None:
            raise RuntimeError("collect: no observation to start from - call reset() first or pass obs0")
        stream = torch.cuda.ExternalStream(self.batch.stream, device=dev)  # (fetching the stream launches held step calls and joins the pipes)
        cur = torch.cuda.current_stream(dev)
        src = torch.as_tensor(src, dtype=torch.float32)
        assert tuple(src.shape) == (n, nobs), tuple(src.shape)
        t["obs"][0].copy_(src)  # on the caller's stream, behind whatever produced src (a host array: uploaded here)
        stream.wait_stream(cur)   # obs[0] is complete, and whoever still reads the previous tapes is done, before they are rewritten
        out = dict(t)
        if self._norm is None:
            if raw:
                raise RuntimeError("collect: raw=True needs normalize=dict(...)")
            self.batch.env_collect_dev(T, self.n_substeps, **{k: v.data_ptr() for k, v in t.items()})
        else:
            akey = ("norm", T, bool(raw))
            if akey not in cache:
                aux = {"ep_return": torch.empty((T, n), dtype=torch.float32, device=dev), "ep_length": torch.empty((T, n), dtype=torch.int32, device=dev)}
                if raw:
                    aux["raw_obs"] = torch.empty((T, n, nobs), dtype=torch.float32, device=dev)
                    aux["raw_reward"] = torch.empty((T, n), dtype=torch.float32, device=dev)
                cache[akey] = aux
            aux = cache[akey]
            self.batch.env_collect_norm_dev(T, self.n_substeps, **{k: v.data_ptr() for k, v in t.items()}, **{k: v.data_ptr() for k, v in aux.items()})
            out.update(aux)
        if gae:
            gkey = ("gae", T)
            if gkey not in cache:
                cache[gkey] = {k: torch.empty((T + 1 if k == "value" else T, n), dtype=torch.float32, device=dev) for k in ("value", "log_prob", "advantage", "returns")}
            g = dict(cache[gkey])
            if getattr(self.batch, "actor_head", None) not in (1, 2):
                del g["log_prob"]  # (the deterministic head has no density)
            self.batch.collect_gae_dev(T, g_gamma, g_lam, g_boot, **{k: v.data_ptr() for k, v in t.items()}, **{k: v.data_ptr() for k, v in g.items()})
            out.update(g)
        cur.wait_stream(stream)   # and the caller's stream sees the results
        self._last_obs = t["obs"][T]
        out["terminated"], out["truncated"] = t["terminated"].view(torch.bool), t["truncated"].view(torch.bool)
        return out

    def collect(self, T, obs0=None, terminal_obs=False, gae=None, raw=False):
        """collect_torch with numpy arrays: the same dict, copied to the host (one synchronisation at the end)."""
        return {k: v.cpu().numpy() for k, v in self.collect_torch(T, obs0=obs0, terminal_obs=terminal_obs, gae=gae, raw=raw).items()}

    # ---- the PPO learner on the device (Batch.learner_create, ppo_minibatch_dev)
    def learner(self, **cfg):
        """Creates the PPO learner over the networks of actor_set (Gaussian head) and critic_set, which become the trainable parameters:
        what collect_torch runs afterwards is whatever ppo_update left.  cfg: clip_range, ent_coef, vf_coef, max_grad_norm,
        normalize_advantage, lr, beta1, beta2, eps - stable-baselines3's defaults where not given (Batch.learner_configure changes them
        later, e.g. for a learning-rate schedule)."""
        self.batch.learner_create(**cfg)
        self._ppo_updates = self._ppo_epochs = 0

    def ppo_minibatches(self, n_rows, batch_size, n_epochs, seed=None, update=None):
        """The minibatches ppo_update visits: a list, one entry per epoch, of (perm, [(start, mb), ...]) - perm a CUDA int32 permutation of the
        n_rows rows drawn with torch.randperm from a device generator seeded by (seed, update), one draw per epoch in order; minibatch k
        of the epoch is perm[start:start + mb]: consecutive stretches of batch_size, the last one shorter."""
        import torch
        dev = torch.device("cuda", self._device)
        seed = self.seed_value if seed is None else int(seed)
        update = getattr(self, "_ppo_updates", 0) if update is None else int(update)
        g = torch.Generator(device=dev)
        g.manual_seed((seed * 1000003 + update) % (1 << 62))
        cuts = [(s0, min(int(batch_size), n_rows - s0)) for s0 in range(0, n_rows, int(batch_size))]
        return [(torch.randperm(n_rows, generator=g, device=dev).to(torch.int32), cuts) for _ in range(int(n_epochs))]

    def ppo_update(self, buf, n_epochs=10, batch_size=64, target_kl=None, seed=None):
        """stable-baselines3's PPO.train over the dict collect_torch(T, gae=...) returned, on the device: the first T rows of its tapes are
        flattened to T n rows (views, no copy), and every epoch visits them in the minibatches of ppo_minibatches, one
        Batch.ppo_minibatch_dev (seven launches) each, all on the batch's stream.  Without target_kl nothing in the loop touches the host:
        the statistics of every minibatch stay on the device and are read once at the end.  With target_kl the approx_kl of each minibatch
        is read before its step, as SB3 does, and the update stops (without that step) when it exceeds 1.5 target_kl.  Returns the means
        of the statistics (engine.PPO_STATS): the losses, approx_kl, clip_fraction, the advantage moments and ratio_max over every
        minibatch EVALUATED - the one that stopped the update included, as in SB3's logs -, grad_norm and skipped over the minibatches
        STEPPED (NaN when none was); "n_minibatches" (steps taken in this call), "early_stop", "n_updates" (epochs begun since the learner
        was created, SB3's counter) and "explained_variance" of the buffer's value against its returns.  Streams are ordered as in
        collect_torch."""
        import torch
        from .engine import PPO_STATS
        if batch_size < 1 or n_epochs < 1:
            raise ValueError("ppo_update: n_epochs and batch_size must be at least 1")
        for k in ("obs", "action", "log_prob", "advantage", "returns", "value"):
            if k not in buf:
                raise ValueError("ppo_update: the buffer has no %r - collect with gae=dict(...) and the gaussian head" % k)
        T, n = buf["advantage"].shape
        R = T * n
        dev = torch.device("cuda", self._device)
        plan = self.ppo_minibatches(R, batch_size, n_epochs, seed=seed)
        stats = torch.zeros((sum(len(c) for _, c in plan), 16), dtype=torch.float32, device=dev)
        tapes = [buf["obs"][:T], buf["action"], buf["log_prob"], buf["advantage"], buf["returns"]]
        assert all(x.is_contiguous() and x.dtype == torch.float32 for x in tapes)
        ptrs = [x.data_ptr() for x in tapes]
        stream = torch.cuda.ExternalStream(self.batch.stream, device=dev)  # (fetching the stream launches held step calls and joins the pipes)
        cur = torch.cuda.current_stream(dev)
        stream.wait_stream(cur)  # the buffer, the permutations and the zeroed statistics are complete
        done, stopped = 0, False
        for perm, cuts in plan:
            self._ppo_epochs = getattr(self, "_ppo_epochs", 0) + 1
            for s0, mb in cuts:
                sp = stats[done].data_ptr()
                if target_kl is None:
                    self.batch.ppo_minibatch_dev(*ptrs, R, mb, index=perm.data_ptr() + 4 * s0, stats=sp)
                else:
                    self.batch.ppo_grad_dev(*ptrs, R, mb, index=perm.data_ptr() + 4 * s0, stats=sp)
                    if float(self.batch.from_dev(sp + 4 * 4, (1,))[0]) > 1.5 * float(target_kl):
                        stopped = True
                        break
                    self.batch.ppo_adam_dev(stats=sp)
                done += 1
            if stopped:
                break
        cur.wait_stream(stream)  # the caller's stream is behind the update: the tapes and permutations may be reused or freed on it
        self._ppo_updates = getattr(self, "_ppo_updates", 0) + 1
        ret, val = buf["returns"].reshape(-1), buf["value"][:T].reshape(-1)
        var = ret.var()
        log = {"explained_variance": float("nan") if float(var) == 0.0 else float(1.0 - (ret - val).var() / var)}
        rows = stats[:done + (1 if stopped else 0)].double().cpu().numpy()
        for i, k in enumerate(PPO_STATS):
            part = rows[:done] if k in ("grad_norm", "skipped") else rows
            log[k] = float(part[:, i].mean()) if len(part) else float("nan")
        log.update(n_minibatches=done, n_updates=self._ppo_epochs, early_stop=stopped)
        return log

    # ---- the SAC learner on the device (Batch.sac_create, sac_step_dev)
    def q_set(self, k, sizes, weights, biases, activation="tanh"):
        """Installs Q network k (0 or 1) of the SAC learner (Batch.q_set: sizes [nobs + nu, hidden..., 1] over the row obs | action,
        weights[l] is [in, out], the transpose of torch.nn.Linear.weight; hidden layers with `activation` - "tanh", "relu" or "elu" -, linear
        output; both Q networks of a learner share it)."""
        self.batch.q_set(k, sizes, weights, biases, activation=activation)

    def sac_learner(self, **cfg):
        """Creates the SAC learner over the networks of actor_set (squashed head) and q_set, which become the trainable parameters: what
        collect_torch runs afterwards is whatever sac_update left, with no actor_set in between.  cfg: the fields of hb_sac_config -
        stable-baselines3's defaults where not given; seed defaults to this VecEnv's seed."""
        cfg.setdefault("seed", self.seed_value & 0xFFFFFFFF)
        self.batch.sac_create(**cfg)
        self._sac_updates = self._sac_steps = 0

    def sac_update(self, replay, gradient_steps, batch_size=256, seed=None):
        """stable-baselines3's SAC.train over a ReplayBuffer on this VecEnv's device: gradient_steps calls of Batch.sac_step_dev (sixteen
        launches each), every one on batch_size rows drawn uniformly from the filled part of the ring (torch.randint from a device
        generator seeded by (seed, the number of sac_update calls so far)), all on the batch's stream.  Nothing in the loop touches the
        host: the statistics of every step stay on the device and are read once at the end.  Returns their means (engine.SAC_STATS) and
        "n_updates" (gradient steps since the learner was created, SB3's counter).  Streams are ordered as in ppo_update."""
        import torch
        from .engine import SAC_STATS
        if batch_size < 1 or gradient_steps < 1:
            raise ValueError("sac_update: gradient_steps and batch_size must be at least 1")
        dev = torch.device("cuda", self._device)
        if replay.device != dev:
            raise ValueError("sac_update: the replay buffer lives on %s, the learner on %s" % (replay.device, dev))
        seed = self.seed_value if seed is None else int(seed)
        g = torch.Generator(device=dev)
        g.manual_seed((seed * 1000003 + getattr(self, "_sac_updates", 0)) % (1 << 62))
        index = replay.sample_index(int(gradient_steps) * int(batch_size), g)
        stats = torch.zeros((int(gradient_steps), 16), dtype=torch.float32, device=dev)
        ptrs = [x.data_ptr() for x in (replay.obs, replay.action, replay.reward, replay.next_obs, replay.done)]
        stream = torch.cuda.ExternalStream(self.batch.stream, device=dev)  # (fetching the stream launches held step calls and joins the pipes)
        cur = torch.cuda.current_stream(dev)
        stream.wait_stream(cur)  # the ring, the indices and the zeroed statistics are complete
        for k in range(int(gradient_steps)):
            self.batch.sac_step_dev(*ptrs, replay.capacity, int(batch_size), index=index.data_ptr() + 4 * k * int(batch_size), stats=stats[k].data_ptr())
        cur.wait_stream(stream)  # the caller's stream is behind the update: the ring and the indices may be reused on it
        self._sac_updates = getattr(self, "_sac_updates", 0) + 1
        rows = stats.double().mean(dim=0).cpu().numpy()
        log = {k: float(rows[i]) for i, k in enumerate(SAC_STATS)}
        self._sac_steps = getattr(self, "_sac_steps", 0) + int(gradient_steps)
        log["n_updates"] = self._sac_steps
        return log

    def close(self):
        if getattr(self, "_norm_dev", None) is not None:
            self.batch.dev_free(self._norm_dev["obs"])
            self._norm_dev = None
        self.batch.close()
