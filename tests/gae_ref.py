"""fp64 reference of the PPO buffer (include/hb.h: hb_critic_set_mlp, hb_collect_gae_dev): critic values, log-probabilities of the recorded
draws, and GAE(gamma, lambda) both as stable-baselines3's backward recurrence and as the definition, explicit sums per episode.  Test
infrastructure: the package never imports it."""
import numpy as np

import actor_ref as ar

LOG_2PI = np.log(2.0 * np.pi)


def values(obs, ws, bs):
    """V(obs) in fp64 for observations [..., nobs]: tanh hidden layers, linear last layer of width 1; shape [...]"""
    return ar.network(obs, ws, bs, ar.GAUSSIAN)[..., 0]


def boot_mask(terminated, truncated, bootstrap_truncated=True):
    """where an env is bootstrapped: cut by truncation alone (VecEnv's TimeLimit.truncated)"""
    te, tr = np.asarray(terminated).astype(bool), np.asarray(truncated).astype(bool)
    return (tr & ~te) if bootstrap_truncated else np.zeros_like(te)


def squash_correction(x):
    """log(1 - tanh(x)^2) = 2 (log 2 - x - softplus(-2 x)), the form that does not cancel at large |x|"""
    x = np.asarray(x, dtype=np.float64)
    return 2.0 * (np.log(2.0) - x - np.logaddexp(0.0, -2.0 * x))


def log_prob_terms(head, eps, log_std, mean=None):
    """the per-actuator terms [..., nu] of log_prob"""
    eps = np.asarray(eps, dtype=np.float64)
    ls = np.broadcast_to(np.asarray(log_std, dtype=np.float64), eps.shape)
    term = -0.5 * eps * eps - ls - 0.5 * LOG_2PI
    if head == ar.SQUASHED:
        x = np.asarray(mean, dtype=np.float64) + np.exp(ls) * eps
        term = term - squash_correction(x)
    elif head != ar.GAUSSIAN:
        raise ValueError("head %r has no density" % (head,))
    return term


def log_prob(head, eps, log_std, mean=None):
    """log pi(action | obs) [...] of the action the head formed from eps [..., nu]"""
    return log_prob_terms(head, eps, log_std, mean).sum(axis=-1)


def shaped_reward(reward, terminal_value, terminated, truncated, gamma, bootstrap_truncated=True):
    """r' = reward + gamma terminal_value where the env is bootstrapped (terminal_value is not read elsewhere: it may hold anything)"""
    boot = boot_mask(terminated, truncated, bootstrap_truncated)
    tv = np.where(boot, np.asarray(terminal_value, dtype=np.float64), 0.0) if bootstrap_truncated else 0.0
    return np.asarray(reward, dtype=np.float64) + gamma * tv


def deltas(reward, value, terminal_value, terminated, truncated, gamma, bootstrap_truncated=True):
    """TD residuals [T, n]: r' + gamma nt value[t+1] - value[t]"""
    value = np.asarray(value, dtype=np.float64)
    done = np.asarray(terminated).astype(bool) | np.asarray(truncated).astype(bool)
    rp = shaped_reward(reward, terminal_value, terminated, truncated, gamma, bootstrap_truncated)
    return rp + gamma * np.where(done, 0.0, value[1:]) - value[:-1]


def gae(reward, value, terminal_value, terminated, truncated, gamma, lam, bootstrap_truncated=True):
    """(advantage, returns) [T, n] by the backward recurrence of RolloutBuffer.compute_returns_and_advantage; value is [T + 1, n]"""
    value = np.asarray(value, dtype=np.float64)
    done = np.asarray(terminated).astype(bool) | np.asarray(truncated).astype(bool)
    d = deltas(reward, value, terminal_value, terminated, truncated, gamma, bootstrap_truncated)
    T = d.shape[0]
    adv = np.zeros_like(d)
    nxt = np.zeros(d.shape[1:])
    for t in range(T - 1, -1, -1):
        nxt = d[t] + gamma * lam * np.where(done[t], 0.0, nxt)
        adv[t] = nxt
    return adv, adv + value[:-1]


def gae_by_episode(reward, value, terminal_value, terminated, truncated, gamma, lam, bootstrap_truncated=True):
    """the definition: advantage[t] = sum_k (gamma lam)^k delta[t + k] over the steps of t's own episode (up to and including the step it
    ends at, or the end of the tape)"""
    value = np.asarray(value, dtype=np.float64)
    done = np.asarray(terminated).astype(bool) | np.asarray(truncated).astype(bool)
    d = deltas(reward, value, terminal_value, terminated, truncated, gamma, bootstrap_truncated)
    T, n = d.shape
    adv = np.zeros_like(d)
    for e in range(n):
        for t in range(T):
            w = 1.0
            for k in range(t, T):
                adv[t, e] += w * d[k, e]
                if done[k, e]:
                    break
                w *= gamma * lam
    return adv, adv + value[:-1]
