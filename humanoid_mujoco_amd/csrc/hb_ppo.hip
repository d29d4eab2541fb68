// hb_ppo.hip - the PPO learner of hb_ppo_grad_dev / hb_ppo_adam_dev: the clipped surrogate of stable-baselines3's PPO.train for the
// Gaussian head, the backward pass through actor and critic, global-norm clipping and Adam.  A translation unit of its own: no other
// kernel compiles differently for it.
//
// hb_ppo_grad_dev is FIVE launches, whatever the minibatch size:
//   1. hb_ppo_forward_kernel   grid (tiles, 3): y = 0 the actor, y = 1 the critic over 16 gathered rows each - hb_actor_kernel's layer
//      loop (hb_mlp_layers.inl), whose hook also stores every layer's activation to the scratch [mb][width]; y = 2: the first nchunk
//      blocks form the chunk sums of the advantage.
//   2. hb_ppo_head_kernel      one lane per row: log-probability, ratio, the loss terms by row, dloss/dmean (the actor's top dZ),
//      dloss/dvalue (the critic's top dZ), dloss/dlog_std by row.
//   3. hb_ppo_backprop_kernel  grid (tiles, 2): dZ_{l-1} = (dZ_l W_l^T) (1 - a^2), top layer down to layer 1 - the SAME layer loop on the
//      reversed network, B operand = a second packing of the transposed weights; every layer's dZ goes to the scratch.
//   4. hb_ppo_wgrad_kernel     grid (chunks, layers of both networks + 1): dW_l = A_l^T dZ_l and db_l = colsum dZ_l over the chunk's rows,
//      16 rows at a time through LDS, 32 accumulator tiles per wave; the last y: the chunk sums of dlog_std and of the loss terms.
//   5. hb_ppo_reduce_kernel    one lane per entry of the flat record: the chunk partials summed in chunk order; one more block merges
//      the statistics.
// hb_ppo_adam_dev is TWO: hb_ppo_norm_kernel (chunk sums of squares over the flat gradient), hb_ppo_adam_kernel (every block merges
// them in order, then clipping, Adam and the refresh of the packed operands, one lane per entry).
// All matrix products are v_mfma_f32_16x16x4_f32 (exact f32).  No atomics, no cross-block communication inside a launch: every
// reduction has an order fixed by (mb, sizes) alone (hb_device.hpp: ppo_row_chunk), so the same inputs give the same bits.
// What this learner's kernels and the SAC learner's (hb_sac.hip) do alike is one piece of code: the row gather, the dW / db sweep, the
// merge of the partials and Adam's step in hb_learn_core.hpp, the refresh of the packed operands in hb_device.hpp (learn_refresh).
#include <hip/hip_runtime.h>
#include "hb_learn_core.hpp"
#include "hb_launch.hpp"

namespace hb {

// the moments of the minibatch's advantages from the chunk partials, merged in chunk order (fp64): mean, unbiased std (0 for mb = 1)
__device__ __forceinline__ void ppo_adv_moments(const PpoDesc& d, double& mean, double& sd) {
  double s = 0.0, q = 0.0;
  for (int c = 0; c < d.nchunk; c++) { s += d.advpart[2 * c]; q += d.advpart[2 * c + 1]; }
  mean = s / d.mb;
  const double var = d.mb > 1 ? fmax(0.0, (q - s * mean) / (d.mb - 1)) : 0.0;
  sd = sqrt(var);
}

// hb_ppo_forward_kernel, hb_ppo_backprop_kernel and their twins for networks that are not tanh
#define HB_ACT_ANY 0
#include "hb_ppo_mlp.inl"
#undef HB_ACT_ANY
#define HB_ACT_ANY 1
#include "hb_ppo_mlp.inl"
#undef HB_ACT_ANY

// One lane per minibatch row.  Roundings are fp32 unless said otherwise; A_r is formed in fp64 from the fp64 moments and rounded once.
__global__ __launch_bounds__(256) void hb_ppo_head_kernel(const PpoDesc d) {
  __shared__ double mom[2];
  if (threadIdx.x == 0) ppo_adv_moments(d, mom[0], mom[1]);
  __syncthreads();
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= d.mb) return;
  const long long src = learn_src_row(d.index, d.first, r);
  const int nu = d.nu;
  const float half_log_2pi = 0.91893853320467274178f;
  const float* ls = d.param + d.off_log_std;
  const float* mu = d.net[0].out + (size_t)r * nu;
  const float* act = d.action + (size_t)src * nu;
  float lp = 0.f;
  for (int i = 0; i < nu; i++) {
    const float z = (act[i] - mu[i]) * expf(-ls[i]);
    lp += __fmaf_rn(-0.5f * z, z, -ls[i]) - half_log_2pi;
  }
  float A = d.advantage[src];
  if (d.normalize && d.mb > 1) A = (float)(((double)A - mom[0]) / (mom[1] + 1e-8));
  const float dl = lp - d.old_log_prob[src];
  const float ratio = expf(dl);
  const float lo = 1.f - d.clip_range, hi = 1.f + d.clip_range;
  const float s1 = A * ratio, s2 = A * fminf(fmaxf(ratio, lo), hi);
  const bool inside = ratio >= lo && ratio <= hi;
  const float inv_mb = 1.f / (float)d.mb;
  const float glp = (inside || s1 < s2) ? -s1 * inv_mb : 0.f;  // dloss / dlp_r (autograd's torch.min over torch.clamp, ties included)
  float* dmu = d.net[0].dz[d.net[0].fwd.nl - 1] + (size_t)r * nu;
  float* gl = d.gls + (size_t)r * nu;
  for (int i = 0; i < nu; i++) {
    const float is = expf(-ls[i]);
    const float z = (act[i] - mu[i]) * is;
    dmu[i] = glp * (z * is);
    gl[i] = glp * __fmaf_rn(z, z, -1.f);
  }
  const float v = d.net[1].out[r], e = v - d.returns[src];
  d.net[1].dz[d.net[1].fwd.nl - 1][r] = 2.f * d.vf_coef * e * inv_mb;
  float* sr = d.srow + (size_t)r * 5;
  sr[0] = -fminf(s1, s2);
  sr[1] = e * e;
  sr[2] = (ratio - 1.f) - dl;
  sr[3] = fabsf(ratio - 1.f) > d.clip_range ? 1.f : 0.f;
  sr[4] = ratio;
}

// dW = A^T dZ and db over one chunk of rows (learn_wgrad_chunk), one layer of one network per blockIdx.y; the block behind the layers
// sums what only this learner has
__global__ __launch_bounds__(512) void hb_ppo_wgrad_kernel(const PpoDesc d) {
  __shared__ float sA[16 * 272], sZ[16 * 272];
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int r0 = c * d.chunk, r1 = min(d.mb, r0 + d.chunk);
  float* out = d.part + (size_t)c * d.P;
  const int La = d.net[0].fwd.nl, Lc = d.net[1].fwd.nl;
  int y = blockIdx.y;
  if (y == La + Lc) {
    // the chunk sums of dlog_std by column and of the loss terms, in row order (fp64, rounded once)
    if (tid < d.nu) {
      double s = 0.0;
      for (int r = r0; r < r1; r++) s += (double)d.gls[(size_t)r * d.nu + tid];
      out[d.off_log_std + tid] = (float)s;
    } else if (tid >= 64 && tid < 69) {
      const int j = tid - 64;
      double s = 0.0;
      for (int r = r0; r < r1; r++) { const double x = (double)d.srow[(size_t)r * 5 + j]; s = j == 4 ? fmax(s, x) : s + x; }
      d.statpart[8 * c + j] = s;
    }
    return;
  }
  const PpoNet& nw = d.net[y < La ? 0 : 1];
  const int l = y < La ? y : y - La;
  learn_wgrad_chunk(nw.act[l], nw.dz[l], nw.fwd.sizes[l], nw.fwd.sizes[l + 1], r0, r1, out + nw.off_w[l], out + nw.off_b[l], sA, sZ);
}

__global__ __launch_bounds__(256) void hb_ppo_reduce_kernel(const PpoDesc d) {
  if (blockIdx.x == gridDim.x - 1) {
    // the statistics (fp64 sums in chunk order); grad_norm [6] and skipped [10] belong to hb_ppo_adam_dev
    if (threadIdx.x != 0 || !d.stats) return;
    double s[5] = {0, 0, 0, 0, 0};
    for (int c = 0; c < d.nchunk; c++)
      for (int j = 0; j < 5; j++) s[j] = j == 4 ? fmax(s[j], d.statpart[8 * c + j]) : s[j] + d.statpart[8 * c + j];
    double ent = 0.0;
    for (int i = 0; i < d.nu; i++) ent -= 0.5 + 0.91893853320467274178 + (double)d.param[d.off_log_std + i];
    double mean, sd;
    ppo_adv_moments(d, mean, sd);
    const double pl = s[0] / d.mb, vl = s[1] / d.mb;
    for (int j = 0; j < 16; j++) d.stats[j] = 0.f;
    d.stats[0] = (float)pl; d.stats[1] = (float)vl; d.stats[2] = (float)ent;
    d.stats[3] = (float)(pl + (double)d.ent_coef * ent + (double)d.vf_coef * vl);
    d.stats[4] = (float)(s[2] / d.mb); d.stats[5] = (float)(s[3] / d.mb);
    d.stats[7] = (float)mean; d.stats[8] = (float)sd; d.stats[9] = (float)s[4];
    return;
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.P) return;
  float g = learn_partials_sum(d.part, d.P, d.nchunk, i);
  if (i >= d.off_log_std && i < d.off_log_std + d.nu) g -= d.ent_coef;  // the entropy bonus
  d.grad[i] = g;
}

__global__ __launch_bounds__(256) void hb_ppo_norm_kernel(const PpoAdamDesc d) {
  __shared__ double red[256];
  const int base = blockIdx.x * kPpoNormChunk;
  double s = 0.0;
  for (int j = 0; j < kPpoNormChunk / 256; j++) {
    const int i = base + j * 256 + threadIdx.x;
    if (i < d.P) { const double g = (double)d.grad[i]; s += g * g; }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double S = 0.0;
    for (int t = 0; t < 256; t++) S += red[t];
    d.normpart[blockIdx.x] = S;
  }
}

// One lane per entry of the flat record.  Every block forms the same norm (the partials in order); the step on the clipped gradient is
// learn_adam_entry's.  A W entry is also written to its place in the packed B operand of the forward kernels and in the packed
// transpose (learn_refresh).
__global__ __launch_bounds__(256) void hb_ppo_adam_kernel(const PpoAdamDesc d) {
  __shared__ double gsh;
  if (threadIdx.x == 0) {
    double S = 0.0;
    for (int c = 0; c < d.nnorm; c++) S += d.normpart[c];
    gsh = sqrt(S);
  }
  __syncthreads();
  const double gn = gsh;
  const bool skip = !(gn <= 1.7976931348623157e308);  // NaN or infinity
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    if (d.stats) { d.stats[6] = (float)gn; d.stats[10] = skip ? 1.f : 0.f; }
  }
  if (skip) {
    // (every block takes this branch or none; only this lane touches the counter, and nobody reads it in this launch)
    if (i == 0) d.nskip[0] = d.nskip[0] + 1;
    return;
  }
  if (i >= d.P) return;
  const double t = (double)(d.calls - (long long)d.nskip[0]);
  const double scale = d.max_grad_norm > 0.f ? fmin(1.0, (double)d.max_grad_norm / (gn + 1e-6)) : 1.0;
  const double g = (double)d.grad[i] * scale;
  learn_refresh(d.seg, d.nseg, i, learn_adam_entry(g, d.lr, t, d.beta1, d.beta2, d.eps, d.m, d.v, d.param, i));
}

hipError_t launch_ppo_grad(const PpoDesc& d, hipStream_t stream) {
  (void)hipGetLastError();
  if (d.mb < 1 || d.nchunk < 1 || d.nchunk > 64 || d.nu < 1 || d.nu > kActorMaxNu || d.P < 1) return hipErrorInvalidValue;
  const int tiles = (d.mb + 15) / 16;
  int ldx = 1;
  for (int k = 0; k < 2; k++) ldx = max(ldx, max(d.net[k].fwd.ldx, d.net[k].bwd.ldx));
  const size_t shmem = ((size_t)32 * ldx + 8 * 256) * sizeof(float);  // two activation tiles + the split-K partial tiles (>= the 8 KB of the advantage blocks)
  if (shmem > 64 * 1024 || tiles < d.nchunk) return hipErrorInvalidValue;
  const int nlay = d.net[0].fwd.nl + d.net[1].fwd.nl;
  const bool tanh_only = d.net[0].fwd.act == kActTanh && d.net[1].fwd.act == kActTanh;
  if (tanh_only) hipLaunchKernelGGL(hb_ppo_forward_kernel, dim3(tiles, 3), dim3(512), shmem, stream, d);
  else hipLaunchKernelGGL(hb_ppo_forward_act_kernel, dim3(tiles, 3), dim3(512), shmem, stream, d);
  hipLaunchKernelGGL(hb_ppo_head_kernel, dim3((d.mb + 255) / 256), dim3(256), 0, stream, d);
  if (tanh_only) hipLaunchKernelGGL(hb_ppo_backprop_kernel, dim3(tiles, 2), dim3(512), shmem, stream, d);
  else hipLaunchKernelGGL(hb_ppo_backprop_act_kernel, dim3(tiles, 2), dim3(512), shmem, stream, d);
  hipLaunchKernelGGL(hb_ppo_wgrad_kernel, dim3(d.nchunk, nlay + 1), dim3(512), 0, stream, d);
  hipLaunchKernelGGL(hb_ppo_reduce_kernel, dim3((d.P + 255) / 256 + 1), dim3(256), 0, stream, d);
  return hipGetLastError();
}

hipError_t launch_ppo_adam(const PpoAdamDesc& d, hipStream_t stream) {
  (void)hipGetLastError();
  if (d.P < 1 || d.nseg < 1 || d.nseg > kLearnMaxSeg || d.nnorm != (d.P + kPpoNormChunk - 1) / kPpoNormChunk) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hb_ppo_norm_kernel, dim3(d.nnorm), dim3(256), 0, stream, d);
  hipLaunchKernelGGL(hb_ppo_adam_kernel, dim3((d.P + 255) / 256), dim3(256), 0, stream, d);
  return hipGetLastError();
}

}  // namespace hb
