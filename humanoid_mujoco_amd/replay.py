"""ReplayBuffer: the off-policy store between VecEnv.collect_torch and VecEnv.sac_update - a ring of transitions in torch tensors on the
device the collection's tapes live on (or on the CPU), filled by index arithmetic alone."""


class ReplayBuffer:
    """A ring of `capacity` transitions: obs, next_obs [capacity, nobs], action [capacity, nu], reward [capacity] float32 and done
    [capacity] uint8.  Pure torch: it runs on any device, the CPU included, and never synchronises with the host - `size` and `pos` are
    host integers advanced by the number of rows added, which is known from the tapes' shapes.
    With VecEnv(normalize=...) the ring holds the normalised tapes as collected; stable-baselines3 stores raw values and normalises on
    sampling, which this buffer does not do."""

    def __init__(self, capacity, nobs, nu=None, device="cpu"):
        """nobs: the width of an observation row, or the VecEnv the transitions come from - the buffer then takes its widths from the
        env (env.nobs, the model's observation and what obs_extend appends, and the model's nu)"""
        import torch
        if capacity < 1:
            raise ValueError("ReplayBuffer: capacity must be at least 1")
        if hasattr(nobs, "nobs"):
            nobs, nu = nobs.nobs, (nobs.model.nu if nu is None else nu)
        if nu is None:
            raise TypeError("ReplayBuffer: nu is required with a numeric nobs")
        self.capacity, self.nobs, self.nu = int(capacity), int(nobs), int(nu)
        self.device = torch.device(device)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.obs = torch.zeros((self.capacity, self.nobs), **f32)
        self.next_obs = torch.zeros((self.capacity, self.nobs), **f32)
        self.action = torch.zeros((self.capacity, self.nu), **f32)
        self.reward = torch.zeros((self.capacity,), **f32)
        self.done = torch.zeros((self.capacity,), dtype=torch.uint8, device=self.device)
        self.pos = self.size = 0

    def add(self, buf):
        """Appends the T n transitions of the dict collect_torch(T, terminal_obs=True) returned, in (t, e) order (step by step, env by env):
        next_obs is terminal_obs[t] where terminated | truncated (the observation the episode ended in, not the first of the next
        episode), else obs[t + 1]; done is terminated alone - SB3's dones * (1 - timeouts): an env cut by truncation alone bootstraps
        from its terminal observation.  More rows than the capacity: the last `capacity` of them stay."""
        import torch
        for k in ("obs", "action", "reward", "terminated", "truncated", "terminal_obs"):
            if k not in buf:
                raise ValueError("ReplayBuffer.add: the buffer has no %r - collect with terminal_obs=True" % k)
        T, n = buf["reward"].shape
        ended = (buf["terminated"].bool() | buf["truncated"].bool()).unsqueeze(-1)
        nxt = torch.where(ended, buf["terminal_obs"], buf["obs"][1:T + 1])
        part = {"obs": buf["obs"][:T].reshape(T * n, self.nobs), "next_obs": nxt.reshape(T * n, self.nobs),
                "action": buf["action"].reshape(T * n, self.nu), "reward": buf["reward"].reshape(T * n),
                "done": buf["terminated"].reshape(T * n).to(torch.uint8)}
        R = T * n
        skip = max(0, R - self.capacity)  # (rows that would be overwritten within this call)
        pos = (self.pos + skip) % self.capacity
        idx = (torch.arange(R - skip, device=self.device) + pos) % self.capacity
        for k, v in part.items():
            getattr(self, k).index_copy_(0, idx, v[skip:].to(self.device))
        self.pos = (self.pos + R) % self.capacity
        self.size = min(self.capacity, self.size + R)

    def sample_index(self, batch_size, generator=None):
        """int32 [batch_size] row numbers, uniform over the filled part (with replacement, as SB3 samples)"""
        import torch
        if self.size < 1:
            raise RuntimeError("ReplayBuffer.sample_index: the buffer is empty")
        return torch.randint(0, self.size, (int(batch_size),), generator=generator, device=self.device, dtype=torch.int32)
