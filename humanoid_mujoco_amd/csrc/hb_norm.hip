// hb_norm.hip - running observation / reward normalisation and episode statistics (include/hb.h: hb_norm_*, hb_env_collect_norm_dev):
// VecNormalize over a VecMonitor in two launches per env step.  hb_norm_moments_kernel reduces the batch's rows in fixed chunks of 64
// consecutive envs to one fp64 partial per chunk and advances the per-env accumulators; hb_norm_apply_kernel merges the partials in
// chunk order into the running statistics - every block for itself, all to the same bits - and normalises its rows.  No atomics, no
// fences, no block waits for another: the order is the stream's.  A translation unit of its own: no other kernel compiles differently
// for it.
#include <hip/hip_runtime.h>
#include "hb_device.hpp"
#include "hb_launch.hpp"

namespace hb {

// the update of a running (mean, var, count) with n rows of mean mb and biased variance vb (include/hb.h)
__device__ __forceinline__ void norm_update(double& mean, double& var, double& count, double mb, double vb, double n) {
  const double d = mb - mean, tot = count + n;
  mean += d * n / tot;
  var = (var * count + vb * n + d * d * count * n / tot) / tot;
  count = tot;
}

// Block c takes the envs [64 c, 64 c + 64) whatever the grid is.  Its rows go to LDS once (consecutive lanes read consecutive floats of
// the contiguous [n_env][nobs] array); lane e of wave 0 advances env 64 c + e's accumulators; then one thread per column walks the
// chunk's rows in row order twice - mean, then squared deviations about it (never E[x^2] - E[x]^2) - in fp64, column c of LDS row r at
// tile[r nobs + c]: consecutive threads, consecutive banks.  Column nobs is the updated discounted return, column nobs + 1 the four
// episode-total terms.  Partial of the chunk: norm_part_doubles(nobs) doubles (hb_device.hpp).
__global__ __launch_bounds__(256) void hb_norm_moments_kernel(const NormDesc d) {
  extern __shared__ __attribute__((aligned(16))) double sm_moments[];
  double* sret = sm_moments;                                // [64] the updated discounted return
  double* sepr = sm_moments + kNormChunk;                   // [64] the return of the episode that ended here, else 0
  int* sepl = reinterpret_cast<int*>(sm_moments + 2 * kNormChunk);  // [64] its length, else 0 (an episode has at least one step)
  float* tile = reinterpret_cast<float*>(sm_moments + 2 * kNormChunk + kNormChunk / 2);  // [64][nobs]
  const int tid = threadIdx.x, nobs = d.nobs;
  const long long e0 = (long long)blockIdx.x * kNormChunk;
  const int cnt = (int)min((long long)kNormChunk, d.n_rows - e0);
  if (d.upd_obs) {
    const float* src = d.obs_in + (size_t)e0 * nobs;
    for (int idx = tid; idx < cnt * nobs; idx += 256) tile[idx] = src[idx];
  }
  if (tid < kNormChunk) {
    double rn = 0.0, er = 0.0;
    int el = 0;
    if (tid < cnt) {
      const long long e = e0 + tid;
      if (d.reset) {
        d.ret[e] = 0.0; d.ep_ret[e] = 0.0; d.ep_len[e] = 0;
      } else {
        const double r = (double)d.reward_in[e];
        const bool done = (d.term[e] | d.trunc[e]) != 0;
        if (d.upd_ret) {
          rn = d.ret[e] * d.gamma + r;
          d.ret[e] = done ? 0.0 : rn;
        } else if (done) {
          d.ret[e] = 0.0;
        }
        // (the episode's return and length stay in the accumulators until the apply kernel has written them out and cleared them)
        const double ern = d.ep_ret[e] + r;
        const int eln = d.ep_len[e] + 1;
        d.ep_ret[e] = ern; d.ep_len[e] = eln;
        if (done) { er = ern; el = eln; }
      }
    }
    sret[tid] = rn; sepr[tid] = er; sepl[tid] = el;
  }
  __syncthreads();
  double* part = d.part + (size_t)blockIdx.x * norm_part_doubles(nobs);
  for (int c = tid; c < nobs + 2; c += 256) {
    if (c == nobs + 1) {
      double ne = 0.0, sr = 0.0, sr2 = 0.0, sl = 0.0;
      for (int r = 0; r < cnt; r++)
        if (sepl[r] > 0) { ne += 1.0; sr += sepr[r]; sr2 += sepr[r] * sepr[r]; sl += (double)sepl[r]; }
      part[0] = (double)cnt; part[1] = ne; part[2] = sr; part[3] = sr2; part[4] = sl;
    } else if (c == nobs ? d.upd_ret : d.upd_obs) {
      double s = 0.0;
      if (c == nobs) for (int r = 0; r < cnt; r++) s += sret[r];
      else for (int r = 0; r < cnt; r++) s += (double)tile[r * nobs + c];
      const double m = s / (double)cnt;
      double m2 = 0.0;
      if (c == nobs) for (int r = 0; r < cnt; r++) { const double dv = sret[r] - m; m2 += dv * dv; }
      else for (int r = 0; r < cnt; r++) { const double dv = (double)tile[r * nobs + c] - m; m2 += dv * dv; }
      part[5 + 2 * c] = m; part[6 + 2 * c] = m2 / (double)cnt;  // (the chunk's biased variance: divided here once, not in every merging block)
    }
  }
}

hipError_t launch_norm_moments(const NormDesc& d, hipStream_t stream) {
  (void)hipGetLastError();
  if (d.nobs < 1 || d.nobs > kNormMaxObs || d.n_rows < 1 || !d.part || !d.ret || !d.ep_ret || !d.ep_len || (d.upd_obs && !d.obs_in) ||
      (!d.reset && (!d.reward_in || !d.term || !d.trunc)))
    return hipErrorInvalidValue;
  const long long nblk = (d.n_rows + kNormChunk - 1) / kNormChunk;
  if (nblk != d.nchunk) return hipErrorInvalidValue;
  const size_t shmem = (2 * kNormChunk + kNormChunk / 2) * sizeof(double) + (size_t)kNormChunk * d.nobs * sizeof(float);
  hipLaunchKernelGGL(hb_norm_moments_kernel, dim3((unsigned)nblk), dim3(256), shmem, stream, d);
  return hipGetLastError();
}

__device__ __forceinline__ float norm_clip(float v, float c) { return v < -c ? -c : (v > c ? c : v); }  // (a NaN passes through, as in numpy's clip)

// Every block merges the nchunk partials in chunk order into the statistics of slot k (one thread per column; the counts are the same
// in every column, each thread carries its own) and keeps mean and 1 / sqrt(var + epsilon) of every column in LDS; block 0 alone writes
// the merged record to slot k ^ 1, which the next launch reads (the host flips k).  Then the block's 64 rows: (float)((x - mean) *
// inv_std) in fp64 per element, clipped in fp32; the rewards; the terminal-observation rows of envs that finished; the episode outputs,
// after which a finished env's episode accumulators are cleared.  Every element is read and written by the same thread: in place works.
__global__ __launch_bounds__(256) void hb_norm_apply_kernel(const NormDesc d) {
  extern __shared__ __attribute__((aligned(16))) double sm_apply[];
  const int tid = threadIdx.x, nobs = d.nobs;
  double* smean = sm_apply;            // [nobs]
  double* sinv = sm_apply + nobs;      // [nobs + 1]: the obs columns, then the discounted return
  int* sdone = reinterpret_cast<int*>(sm_apply + 2 * nobs + 2);  // [64]
  const int R = norm_rec_doubles(nobs), P = norm_part_doubles(nobs);
  const double* cur = d.rec + (size_t)d.k * R;
  double* nxt = d.rec + (size_t)(d.k ^ 1) * R;
  const bool store = d.store && blockIdx.x == 0;
  for (int c = tid; c < nobs + 2; c += 256) {
    if (c == nobs + 1) {
      if (store) {
        double t0 = cur[2 * nobs + 4], t1 = cur[2 * nobs + 5], t2 = cur[2 * nobs + 6], t3 = cur[2 * nobs + 7];
        if (!d.reset)
          for (int ch = 0; ch < d.nchunk; ch++) {
            const double* p = d.part + (size_t)ch * P;
            t0 += p[1]; t1 += p[2]; t2 += p[3]; t3 += p[4];
          }
        nxt[2 * nobs + 4] = t0; nxt[2 * nobs + 5] = t1; nxt[2 * nobs + 6] = t2; nxt[2 * nobs + 7] = t3;
      }
    } else {
      const bool obs = c < nobs;
      double mean = obs ? cur[c] : cur[2 * nobs + 1], var = obs ? cur[nobs + c] : cur[2 * nobs + 2], count = obs ? cur[2 * nobs] : cur[2 * nobs + 3];
      if (obs ? d.upd_obs : d.upd_ret)
        // (the merge is a serial chain, the partials are not: sixteen chunks' loads are in flight at once, then merged in chunk order)
        for (int ch0 = 0; ch0 < d.nchunk; ch0 += 16) {
          double n[16], mb[16], vb[16];
#pragma unroll
          for (int u = 0; u < 16; u++) {
            const double* p = d.part + (size_t)min(ch0 + u, d.nchunk - 1) * P;
            n[u] = p[0]; mb[u] = p[5 + 2 * c]; vb[u] = p[6 + 2 * c];
          }
#pragma unroll
          for (int u = 0; u < 16; u++)
            if (ch0 + u < d.nchunk) norm_update(mean, var, count, mb[u], vb[u], n[u]);
        }
      if (obs) smean[c] = mean;
      sinv[c] = 1.0 / sqrt(var + d.epsilon);
      if (store) {
        if (obs) { nxt[c] = mean; nxt[nobs + c] = var; if (c == 0) nxt[2 * nobs] = count; }
        else { nxt[2 * nobs + 1] = mean; nxt[2 * nobs + 2] = var; nxt[2 * nobs + 3] = count; }
      }
    }
  }
  const long long r0 = (long long)blockIdx.x * kNormChunk;
  const int cnt = (int)min((long long)kNormChunk, d.n_rows - r0);
  if (tid < kNormChunk) sdone[tid] = (d.term && tid < cnt) ? ((d.term[r0 + tid] | d.trunc[r0 + tid]) != 0) : 0;
  __syncthreads();
  if (d.norm_obs || d.obs_out != d.obs_in) {
    const float* src = d.obs_in + (size_t)r0 * nobs;
    float* dst = d.obs_out + (size_t)r0 * nobs;
    for (int idx = tid; idx < cnt * nobs; idx += 256) {
      const int c = idx % nobs;
      const float x = src[idx];
      dst[idx] = d.norm_obs ? norm_clip((float)(((double)x - smean[c]) * sinv[c]), d.clip_obs) : x;
    }
  }
  if (d.tobs_in && (d.norm_obs || d.tobs_out != d.tobs_in)) {
    const float* src = d.tobs_in + (size_t)r0 * nobs;
    float* dst = d.tobs_out + (size_t)r0 * nobs;
    for (int idx = tid; idx < cnt * nobs; idx += 256) {
      const int row = idx / nobs, c = idx - row * nobs;
      if (sdone[row]) {
        const float x = src[idx];
        dst[idx] = d.norm_obs ? norm_clip((float)(((double)x - smean[c]) * sinv[c]), d.clip_obs) : x;
      }
    }
  }
  if (tid < cnt && d.reward_in) {
    const long long e = r0 + tid;
    if (d.reward_out) {
      const float r = d.reward_in[e];
      d.reward_out[e] = d.norm_reward ? norm_clip((float)((double)r * sinv[nobs]), d.clip_reward) : r;
    }
    const bool done = sdone[tid] != 0;
    if (d.ep_return_out) d.ep_return_out[e] = done ? (float)d.ep_ret[e] : 0.f;
    if (d.ep_length_out) d.ep_length_out[e] = done ? d.ep_len[e] : 0;
    if (done) { d.ep_ret[e] = 0.0; d.ep_len[e] = 0; }
  }
}

hipError_t launch_norm_apply(const NormDesc& d, hipStream_t stream) {
  (void)hipGetLastError();
  if (d.nobs < 1 || d.nobs > kNormMaxObs || d.n_rows < 1 || !d.rec || !d.obs_in || !d.obs_out || (d.nchunk > 0 && !d.part) ||
      (d.tobs_in == nullptr) != (d.tobs_out == nullptr) || (d.reward_in && (!d.term || !d.trunc || !d.ep_ret || !d.ep_len)) || (d.tobs_in && !d.term))
    return hipErrorInvalidValue;
  const long long nblk = (d.n_rows + kNormChunk - 1) / kNormChunk;
  if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t shmem = (size_t)(2 * d.nobs + 2) * sizeof(double) + kNormChunk * sizeof(int);
  hipLaunchKernelGGL(hb_norm_apply_kernel, dim3((unsigned)nblk), dim3(256), shmem, stream, d);
  return hipGetLastError();
}

}  // namespace hb
