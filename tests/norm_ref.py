"""fp64 numpy restatement of the normaliser of include/hb.h (hb_norm_*): stable-baselines3's VecNormalize over a VecMonitor.

[recall] stable-baselines3 and gymnasium are not installed here; this restates, from their documented behaviour, RunningMeanStd
(update_from_moments), VecNormalize.step_wait / reset / normalize_obs / normalize_reward and Monitor's info["episode"] = {"r", "l"}:

    update(batch of n rows, mean mb, biased variance vb):   d = mb - mean; tot = count + n
        mean += d n / tot;  var = (var count + vb n + d d count n / tot) / tot;  count = tot
    step(obs, reward, terminated, truncated, terminal_obs), done = terminated | truncated:
        1. training and norm_obs: obs_rms.update(obs)                     (terminal observations never enter an update)
        2. obs_out = clip((obs - mean) / sqrt(var + epsilon), +-clip_obs)
        3. training: ret = ret gamma + reward; ret_rms.update(ret)         (whether or not norm_reward is set)
        4. norm_reward: reward_out = clip(reward / sqrt(ret_var + epsilon), +-clip_reward)
        5. the terminal-observation rows of done envs are normalised as in 2
        6. ep_ret += reward (raw), ep_len += 1; where done they are reported, added to the totals and cleared
        7. ret = 0 where done
    reset(obs): ret = ep_ret = ep_len = 0; training and norm_obs: obs_rms.update(obs); normalise.

Outputs are rounded to float32 once and clipped in float32, as the kernels do.
"""
import numpy as np

DEFAULTS = dict(norm_obs=True, norm_reward=True, training=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8)


class RunningMeanStd:
    def __init__(self, shape=()):
        self.mean = np.zeros(shape, np.float64)
        self.var = np.ones(shape, np.float64)
        self.count = 1e-4

    def update_from_moments(self, mb, vb, n):
        d = mb - self.mean
        tot = self.count + n
        self.mean = self.mean + d * n / tot
        self.var = (self.var * self.count + vb * n + d * d * self.count * n / tot) / tot
        self.count = tot

    def update(self, x):
        x = np.asarray(x, np.float64)
        self.update_from_moments(x.mean(axis=0), x.var(axis=0), x.shape[0])


def merge_records(a, b, nobs):
    """the host merge of two flat records obs_mean[nobs] | obs_var[nobs] | obs_count | ret_mean | ret_var | ret_count: record b enters
    record a as one update with n = its count (the multi-GPU recipe of include/hb.h)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = a.copy()
    o = RunningMeanStd((nobs,))
    o.mean, o.var, o.count = a[:nobs].copy(), a[nobs:2 * nobs].copy(), a[2 * nobs]
    o.update_from_moments(b[:nobs], b[nobs:2 * nobs], b[2 * nobs])
    r = RunningMeanStd()
    r.mean, r.var, r.count = a[2 * nobs + 1], a[2 * nobs + 2], a[2 * nobs + 3]
    r.update_from_moments(b[2 * nobs + 1], b[2 * nobs + 2], b[2 * nobs + 3])
    out[:nobs], out[nobs:2 * nobs], out[2 * nobs] = o.mean, o.var, o.count
    out[2 * nobs + 1], out[2 * nobs + 2], out[2 * nobs + 3] = r.mean, r.var, r.count
    return out


def _clip32(x, c):
    return np.clip(np.asarray(x, np.float64).astype(np.float32), np.float32(-c), np.float32(c))


class NormRef:
    def __init__(self, n_env, nobs, **cfg):
        c = dict(DEFAULTS)
        c.update(cfg)
        self.__dict__.update(c)
        # (the C struct holds float32 constants: the reference computes with the same numbers)
        self.gamma, self.epsilon = float(np.float32(self.gamma)), float(np.float32(self.epsilon))
        self.clip_obs, self.clip_reward = float(np.float32(self.clip_obs)), float(np.float32(self.clip_reward))
        self.n_env, self.nobs = n_env, nobs
        self.obs_rms, self.ret_rms = RunningMeanStd((nobs,)), RunningMeanStd()
        self.ret = np.zeros(n_env)
        self.ep_ret = np.zeros(n_env)
        self.ep_len = np.zeros(n_env, np.int32)
        self.totals = np.zeros(4)  # episodes, sum of returns, sum of squared returns, sum of lengths

    def record(self):
        return np.concatenate([self.obs_rms.mean, self.obs_rms.var, [self.obs_rms.count, self.ret_rms.mean, self.ret_rms.var, self.ret_rms.count]])

    def set_record(self, rec):
        n = self.nobs
        rec = np.asarray(rec, np.float64)
        self.obs_rms.mean, self.obs_rms.var, self.obs_rms.count = rec[:n].copy(), rec[n:2 * n].copy(), float(rec[2 * n])
        self.ret_rms.mean, self.ret_rms.var, self.ret_rms.count = float(rec[2 * n + 1]), float(rec[2 * n + 2]), float(rec[2 * n + 3])

    def normalize_obs(self, obs):
        obs = np.asarray(obs, np.float32)
        if not self.norm_obs:
            return obs.copy()
        return _clip32((obs.astype(np.float64) - self.obs_rms.mean) / np.sqrt(self.obs_rms.var + self.epsilon), self.clip_obs)

    def normalize_reward(self, reward):
        reward = np.asarray(reward, np.float32)
        if not self.norm_reward:
            return reward.copy()
        return _clip32(reward.astype(np.float64) / np.sqrt(self.ret_rms.var + self.epsilon), self.clip_reward)

    def reset(self, obs):
        self.ret[:] = 0.0
        self.ep_ret[:] = 0.0
        self.ep_len[:] = 0
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        return self.normalize_obs(obs)

    def step(self, obs, reward, terminated, truncated, terminal_obs=None):
        """returns dict(obs, reward, terminal_obs, ep_return float32, ep_length int32); terminal_obs: the rows of done envs normalised,
        the others as given"""
        done = np.asarray(terminated, bool) | np.asarray(truncated, bool)
        r64 = np.asarray(reward, np.float32).astype(np.float64)
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        out = {"obs": self.normalize_obs(obs)}
        if self.training:
            self.ret = self.ret * self.gamma + r64
            self.ret_rms.update(self.ret)
        out["reward"] = self.normalize_reward(reward)
        if terminal_obs is not None:
            t = np.asarray(terminal_obs, np.float32).copy()
            if done.any():
                t[done] = self.normalize_obs(t[done])
            out["terminal_obs"] = t
        self.ep_ret += r64
        self.ep_len += 1
        out["ep_return"] = np.where(done, self.ep_ret, 0.0).astype(np.float32)
        out["ep_length"] = np.where(done, self.ep_len, 0).astype(np.int32)
        fin = self.ep_ret[done]
        self.totals += [done.sum(), fin.sum(), (fin * fin).sum(), self.ep_len[done].sum()]
        self.ep_ret[done] = 0.0
        self.ep_len[done] = 0
        self.ret[done] = 0.0
        return out


U64 = 2.0 ** -53


class ErrorBound:
    """Forward bound on how far two fp64 evaluations of the SAME running statistics can drift apart when they differ only in the order of
    the sums over a batch's rows (one pass over n rows, or chunks of 64 merged in chunk order with the update formula) and in whether a
    product feeds an addition fused - what separates the device from NormRef.  Each evaluation is within `mean`, `var` of the exact
    value; two of them differ by at most twice that.  Per update with n rows of magnitude at most S = max |x| and nchunk chunks, with
    u = 2^-53 and A = n + 6 nchunk + 8 roundings in a chain (an n-term sum in any order: n - 1; a Chan merge per chunk: 6; the rest: 8):
        e_mb  = A u S                                        the batch mean
        e_vb  = 2 A u vb + e_mb^2                            two-pass deviations: sum (x - m)^2 = sum (x - mu)^2 + n (m - mu)^2 exactly
        e_d   = e_mb + e_mean                                d = mb - mean cancels: its ABSOLUTE error is what is carried
        e_mean' = e_mean + e_mb + 4 u (|mean| + |d|)
        e_var'  = (e_var count + e_vb n) / tot + (2 |d| e_d + e_d^2) count n / tot^2 + 8 u var'
    (every term of var' is non-negative, so the merge itself loses 8 u var' at most).  x_err: an absolute error the rows themselves carry
    (the discounted returns, which are computed values) - it enters e_mb directly and e_vb through the deviations."""

    def __init__(self, shape=()):
        self.mean = np.zeros(shape)
        self.var = np.zeros(shape)

    def update(self, rms_before, rms_after, x, x_err=0.0):
        x = np.asarray(x, np.float64)
        n = x.shape[0]
        nchunk = (n + 63) // 64
        A = n + 6 * nchunk + 8
        S = np.abs(x).max(axis=0)
        mb, vb = x.mean(axis=0), x.var(axis=0)
        d = np.abs(mb - rms_before.mean)
        count, tot = rms_before.count, rms_before.count + n
        e_mb = A * U64 * S + x_err
        e_vb = 2 * A * U64 * vb + e_mb ** 2 + 2 * np.sqrt(vb) * x_err + x_err ** 2
        e_d = e_mb + self.mean
        self.var = (self.var * count + e_vb * n) / tot + (2 * d * e_d + e_d ** 2) * count * n / tot ** 2 + 8 * U64 * rms_after.var
        self.mean = self.mean + e_mb + 4 * U64 * (np.abs(rms_before.mean) + d)
