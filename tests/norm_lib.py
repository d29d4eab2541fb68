"""The normaliser's reference and its derived bounds, advanced together (Tracker), and the measured / bound ratio the tests assert
(ratio): the harness of tests/test_gpu_norm.py that the observation extension's test (tests/test_gpu_obs_ext.py) runs too.  The
derivation of the bounds is in tests/test_gpu_norm.py's docstring.

TEST INFRASTRUCTURE: the product package never imports this module.
"""
import numpy as np

import norm_ref as nr

V32 = 2.0 ** -24


class Tracker:
    """the reference and the bounds of tests/test_gpu_norm.py's docstring, advanced together"""

    def __init__(self, n, nobs, **cfg):
        self.ref = nr.NormRef(n, nobs, **cfg)
        self.eo, self.er = nr.ErrorBound((nobs,)), nr.ErrorBound()
        self.k, self.ret_max, self.tot_mag, self.count_adds = 0, 0.0, np.zeros(4), 0

    def _obs_update(self, obs):
        before = nr.RunningMeanStd((self.ref.nobs,))
        before.mean, before.var, before.count = self.ref.obs_rms.mean.copy(), self.ref.obs_rms.var.copy(), self.ref.obs_rms.count
        return before

    def reset(self, obs):
        upd = self.ref.training and self.ref.norm_obs
        before = self._obs_update(obs)
        out = self.ref.reset(obs)
        if upd:
            self.eo.update(before, self.ref.obs_rms, obs)
            self.count_adds += (self.ref.n_env + 63) // 64 + 1
        return out

    def step(self, obs, rew, term, trunc, tobs=None):
        ref = self.ref
        before = self._obs_update(obs)
        rb = nr.RunningMeanStd()
        rb.mean, rb.var, rb.count = ref.ret_rms.mean, ref.ret_rms.var, ref.ret_rms.count
        ret_new = ref.ret * ref.gamma + np.asarray(rew, np.float64)
        out = ref.step(obs, rew, term, trunc, tobs)
        self.k += 1
        if ref.training:
            self.count_adds += (ref.n_env + 63) // 64 + 1
            if ref.norm_obs:
                self.eo.update(before, ref.obs_rms, obs)
            self.ret_max = max(self.ret_max, float(np.abs(ret_new).max()))
            self.er.update(rb, ref.ret_rms, ret_new, x_err=2 * self.k * nr.U64 * self.ret_max)
        done = np.asarray(term, bool) | np.asarray(trunc, bool)
        er = out["ep_return"].astype(np.float64)[done]
        self.tot_mag += [0.0, np.abs(er).sum(), (er * er).sum(), 0.0]
        return out

    def dz_obs(self, x):
        """the bound on |out_dev - out_ref| for rows x [.., nobs] normalised with the CURRENT statistics"""
        ref = self.ref
        if not ref.norm_obs:
            return np.zeros(np.shape(x))
        x = np.asarray(x, np.float64)
        inv = 1.0 / np.sqrt(ref.obs_rms.var + ref.epsilon)
        z = (x - ref.obs_rms.mean) * inv
        dz = np.abs(z) * (2 * self.eo.var) / (2 * (ref.obs_rms.var + ref.epsilon)) + 2 * self.eo.mean * inv + 6 * nr.U64 * np.abs(z)
        return 2 * V32 * np.minimum(np.abs(z), ref.clip_obs) + dz

    def dz_rew(self, r):
        ref = self.ref
        if not ref.norm_reward:
            return np.zeros(np.shape(r))
        z = np.asarray(r, np.float64) / np.sqrt(ref.ret_rms.var + ref.epsilon)
        dz = np.abs(z) * (2 * self.er.var) / (2 * (ref.ret_rms.var + ref.epsilon)) + 6 * nr.U64 * np.abs(z)
        return 2 * V32 * np.minimum(np.abs(z), ref.clip_reward) + dz

    def stats_ratio(self, rec):
        """largest |device - reference| / bound over the record's means and variances (counts must be equal)"""
        n, ref = self.ref.nobs, self.ref.record()
        for i in (2 * n, 2 * n + 3):
            assert abs(rec[i] - ref[i]) <= self.count_adds * nr.U64 * ref[i], "counts"
        tiny = 1e-300
        r = [np.abs(rec[:n] - ref[:n]) / (2 * self.eo.mean + tiny), np.abs(rec[n:2 * n] - ref[n:2 * n]) / (2 * self.eo.var + tiny),
             [abs(rec[2 * n + 1] - ref[2 * n + 1]) / (2 * self.er.mean + tiny)], [abs(rec[2 * n + 2] - ref[2 * n + 2]) / (2 * self.er.var + tiny)]]
        return float(max(np.max(x) for x in r))


def ratio(got, want, bound):
    """largest |got - want| / bound; where the bound is 0 the values must be equal"""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    err = np.abs(got - want)
    assert np.all(err[bound == 0] == 0)
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
