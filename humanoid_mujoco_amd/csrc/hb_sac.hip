// hb_sac.hip - the SAC learner of hb_sac_step_dev: stable-baselines3's SAC.train for the squashed Gaussian actor (HB_ACTOR_SQUASHED), twin
// Q networks over obs | action, their Polyak-averaged targets and the entropy coefficient.  A translation unit of its own: no other
// kernel compiles differently for it.  The design is hb_ppo.hip's - 16 gathered rows per block through hb_mlp_layers.inl, activations and
// dZ in a learner-owned scratch [mb][width], the reversed network for dA = dZ W^T, 32 accumulator tiles per wave for dW = A^T dZ over a
// chunk of rows, chunk partials merged in order - with the launches described job by job (hb_device.hpp: Sac*Desc), so that three
// kernels serve five networks.  What the two learners' kernels do alike is one piece of code: the row gather, the dW / db sweep, the
// merge of the partials and Adam's step in hb_learn_core.hpp, the refresh of the packed operands in hb_device.hpp (learn_refresh).
//
// hb_sac_step_dev is SIXTEEN launches whatever the minibatch size (fifteen on a step the target update interval skips):
//   1. hb_sac_forward_kernel   grid (tiles, 4): the actor on obs (activations kept) and on next_obs (nothing kept), Q1 and Q2 on
//      obs | action (input rows and activations kept)
//   2. hb_sac_sample_kernel    one lane per row: eps_pi, eps_next (drawn or read), a_pi, a', lp_pi, lp'; alpha = exp(log_ent_coef)
//   3. hb_sac_forward_kernel   grid (tiles, 2): Q1', Q2' on next_obs | a', nothing kept
//   4. hb_sac_critic_head_kernel  one lane per row: y, the top dZ of Q1 and Q2, the by-row terms of the statistics
//   5. hb_sac_backprop_kernel  grid (tiles, 2): dZ of Q1 and Q2 down to layer 0
//   6. hb_sac_wgrad_kernel     grid (chunks, layers of Q1 and Q2 + 1): dW, db by chunk; the last y: the chunk sums of the by-row terms
//   7. hb_sac_reduce_kernel    the chunk partials in chunk order; the statistics and dloss / dlog_ent_coef
//   8. hb_sac_adam_kernel      Q1, Q2 (and log_ent_coef), with the refresh of every packed operand
//   9. hb_sac_forward_kernel   grid (tiles, 2): the UPDATED Q1, Q2 on obs | a_pi, activations kept
//  10. hb_sac_backprop_kernel  grid (tiles, 2): from a top gradient of 1 down INTO the action inputs: dQ1 / da, dQ2 / da (no dZ stored)
//  11. hb_sac_actor_head_kernel  one lane per row: min Q, the actor's top dZ (mean | log_std), the by-row terms
//  12. hb_sac_backprop_kernel  grid (tiles, 1): the actor's dZ
//  13. hb_sac_wgrad_kernel     grid (chunks, layers of the actor + 1)
//  14. hb_sac_reduce_kernel
//  15. hb_sac_adam_kernel      the actor
//  16. hb_sac_polyak_kernel    Q' = tau Q + (1 - tau) Q', one lane per entry, with the refresh of the targets' packed operands
// All matrix products are v_mfma_f32_16x16x4_f32 (exact f32).  No atomics, no cross-block communication inside a launch: every reduction
// has an order fixed by (mb, sizes) alone, so the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include "hb_learn_core.hpp"
#include "hb_launch.hpp"

namespace hb {

// hb_sac_forward_kernel, hb_sac_backprop_kernel and their twins for launches with a job whose network is not tanh
#define HB_ACT_ANY 0
#include "hb_sac_mlp.inl"
#undef HB_ACT_ANY
#define HB_ACT_ANY 1
#include "hb_sac_mlp.inl"
#undef HB_ACT_ANY

// One lane per minibatch row, both branches (0: pi on obs, 1: next on next_obs).  Roundings are fp32 and follow hb_log_prob_kernel
// (hb_gae.hip) term by term; the draw of (row r, element i) is rng_normal(seed, r, 0, t, stream, i).
__global__ __launch_bounds__(256) void hb_sac_sample_kernel(const SacHeadDesc d) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r == 0) d.alpha[0] = (float)exp((double)d.param[d.P - 1]);
  if (r >= d.mb) return;
  const int nu = d.nu;
  const float half_log_2pi = 0.91893853320467274178f, log2f_ = 0.69314718055994530942f;
  for (int br = 0; br < 2; br++) {
    const float* out = (br ? d.nx_out : d.pi_out) + (size_t)r * 2 * nu;
    float* user = br ? d.eps_next : d.eps_pi;
    float* act = (br ? d.a_nx : d.a_pi) + (size_t)r * nu;
    float sum = 0.f;
    for (int i = 0; i < nu; i++) {
      const size_t o = (size_t)r * nu + i;
      float eps;
      if (d.eps_given) eps = user[o];
      else {
        eps = rng_normal(d.seed, (unsigned)r, 0u, d.t, br ? RS_SAC_NEXT : RS_SAC_PI, (unsigned)i);
        if (user) user[o] = eps;
      }
      if (!br) d.eps[o] = eps;
      const float ls = fminf(2.f, fmaxf(-20.f, out[nu + i]));
      float term = __fsub_rn(__fmaf_rn(-0.5f * eps, eps, -ls), half_log_2pi);
      const float x = __fmaf_rn(expf(ls), eps, out[i]);
      const float a = fabsf(x);
      const float corr = 2.f * __fsub_rn(__fsub_rn(log2f_, a), log1pf(expf(-2.f * a)));
      term = __fsub_rn(term, corr);
      sum = __fadd_rn(sum, term);
      act[i] = tanhf(x);
    }
    (br ? d.lp_nx : d.lp_pi)[r] = sum;
  }
}

// y = reward + (1 - done) gamma (min(Q1', Q2') - alpha lp'); dloss / dQk = (Qk - y) / mb
__global__ __launch_bounds__(256) void hb_sac_critic_head_kernel(const SacHeadDesc d) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= d.mb) return;
  const long long src = learn_src_row(d.index, d.first, r);
  const float alpha = d.alpha[0];
  const float tq = __fmaf_rn(-alpha, d.lp_nx[r], fminf(d.qt[0][r], d.qt[1][r]));
  const float rew = d.reward[src];
  const float y = d.done[src] ? rew : __fmaf_rn(d.gamma, tq, rew);
  const float inv_mb = 1.f / (float)d.mb;
  const float q1 = d.q[0][r], q2 = d.q[1][r];
  const float e1 = q1 - y, e2 = q2 - y;
  d.dzq[0][r] = e1 * inv_mb;
  d.dzq[1][r] = e2 * inv_mb;
  float* sr = d.srow + (size_t)r * kSacSrow;
  sr[0] = e1 * e1; sr[1] = e2 * e2; sr[2] = d.lp_pi[r]; sr[3] = q1; sr[4] = q2; sr[5] = y;
}

// The actor's top dZ.  g = d min(Q1, Q2) / da: the smaller network's, and on a tie half of each (torch.min's backward).
// mb dL/dmean_i = 2 alpha a_i - g_i (1 - a_i^2);  mb dL/dls_i = alpha (-1 + 2 a_i s_i eps_i) - g_i (1 - a_i^2) s_i eps_i where the clamp passes
__global__ __launch_bounds__(256) void hb_sac_actor_head_kernel(const SacHeadDesc d) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= d.mb) return;
  const int nu = d.nu;
  const float alpha = d.alpha[0], inv_mb = 1.f / (float)d.mb;
  const float q1 = d.qpi[0][r], q2 = d.qpi[1][r];
  const float w1 = q1 < q2 ? 1.f : (q1 == q2 ? 0.5f : 0.f), w2 = 1.f - w1;
  const float* out = d.pi_out + (size_t)r * 2 * nu;
  float* dz = d.dza + (size_t)r * 2 * nu;
  for (int i = 0; i < nu; i++) {
    const size_t o = (size_t)r * nu + i;
    const float g = w1 * d.da[0][o] + w2 * d.da[1][o];
    const float a = d.a_pi[o], eps = d.eps[o];
    const float raw = out[nu + i];
    const float se = expf(fminf(2.f, fmaxf(-20.f, raw))) * eps;
    const float gx = g * __fmaf_rn(-a, a, 1.f);  // through tanh
    const float aa = 2.f * alpha * a;
    dz[i] = (aa - gx) * inv_mb;
    const bool pass = raw >= -20.f && raw <= 2.f;
    dz[nu + i] = pass ? (__fmaf_rn(aa, se, -alpha) - gx * se) * inv_mb : 0.f;
  }
  const float mq = fminf(q1, q2);
  float* sr = d.srow + (size_t)r * kSacSrow;
  sr[0] = __fmaf_rn(alpha, d.lp_pi[r], -mq);
  sr[1] = mq;
}

// dW = A^T dZ and db over one chunk of rows (learn_wgrad_chunk), one job per blockIdx.y; the block behind the jobs sums the by-row terms
__global__ __launch_bounds__(512) void hb_sac_wgrad_kernel(const SacWgDesc d) {
  __shared__ float sA[16 * 272], sZ[16 * 272];
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int r0 = c * d.chunk, r1 = min(d.mb, r0 + d.chunk);
  float* out = d.part + (size_t)c * d.P;
  if ((int)blockIdx.y == d.njob) {
    // the chunk sums of the by-row terms, in row order (fp64)
    if (tid < d.ncol) {
      double s = 0.0;
      for (int r = r0; r < r1; r++) s += (double)d.srow[(size_t)r * kSacSrow + tid];
      d.statpart[kSacSrow * c + tid] = s;
    }
    return;
  }
  const SacWgJob& jb = d.job[blockIdx.y];
  learn_wgrad_chunk(jb.A, jb.Z, jb.K, jb.N, r0, r1, out + jb.off_w, out + jb.off_b, sA, sZ);
}

// One lane per entry of [lo, hi): the chunk partials summed in chunk order.  One more block merges the by-row terms (fp64 sums in chunk
// order, rounded once): phase 0 - critic_loss, ent_coef_loss, the alpha used, the means of lp_pi, Q1, Q2, y, and dloss / dlog_ent_coef =
// -(mean lp_pi + target_entropy) into the record's last entry; phase 1 - actor_loss and the mean of min Q(obs, a_pi).
__global__ __launch_bounds__(256) void hb_sac_reduce_kernel(const SacReduceDesc d) {
  if (blockIdx.x == gridDim.x - 1) {
    if (threadIdx.x != 0) return;
    double s[6] = {0, 0, 0, 0, 0, 0};
    const int ncol = d.phase == 0 ? 6 : 2;
    for (int c = 0; c < d.nchunk; c++)
      for (int j = 0; j < ncol; j++) s[j] += d.statpart[kSacSrow * c + j];
    const double inv = 1.0 / d.mb;
    if (d.phase == 0) {
      const double mlp = s[2] * inv, te = (double)d.target_entropy;
      d.grad[d.P - 1] = (float)(-(mlp + te));
      if (d.stats) {
        for (int j = 0; j < 16; j++) d.stats[j] = 0.f;
        d.stats[1] = (float)(0.5 * (s[0] * inv + s[1] * inv));
        d.stats[2] = (float)(-(double)d.param[d.P - 1] * (mlp + te));
        d.stats[3] = d.alpha[0];
        d.stats[4] = (float)mlp; d.stats[5] = (float)(s[3] * inv); d.stats[6] = (float)(s[4] * inv); d.stats[7] = (float)(s[5] * inv);
      }
    } else if (d.stats) {
      d.stats[0] = (float)(s[0] * inv);
      d.stats[8] = (float)(s[1] * inv);
    }
    return;
  }
  const int i = d.lo + blockIdx.x * 256 + threadIdx.x;
  if (i >= d.hi) return;
  d.grad[i] = learn_partials_sum(d.part, d.P, d.nchunk, i);
}

// torch.optim.Adam, one lane per entry of [lo, hi) (learn_adam_entry), with the refresh of the packed operands (learn_refresh)
__global__ __launch_bounds__(256) void hb_sac_adam_kernel(const SacAdamDesc d) {
  const int i = d.lo + blockIdx.x * 256 + threadIdx.x;
  if (i >= d.hi) return;
  const float& lr = i == d.ent_index ? d.lr_ent : d.lr;
  learn_refresh(d.seg, d.nseg, i, learn_adam_entry((double)d.grad[i], lr, (double)d.t, d.beta1, d.beta2, d.eps, d.m, d.v, d.param, i));
}

// Q' = tau Q + (1 - tau) Q' in fp64, rounded once, one lane per entry of the targets' record
__global__ __launch_bounds__(256) void hb_sac_polyak_kernel(const SacPolyakDesc d) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.n) return;
  const double tau = (double)d.tau;
  const float pf = (float)(tau * (double)d.src[i] + (1.0 - tau) * (double)d.target[i]);
  d.target[i] = pf;
  learn_refresh(d.seg, d.nseg, i, pf);
}

static size_t sac_shmem(int ldx) { return ((size_t)32 * ldx + 8 * 256) * sizeof(float); }  // two activation tiles + the split-K partial tiles

hipError_t launch_sac_forward(const SacFwdDesc& d, int njob, hipStream_t stream) {
  (void)hipGetLastError();
  if (d.mb < 1 || njob < 1 || njob > 4) return hipErrorInvalidValue;
  int ldx = 1;
  for (int j = 0; j < njob; j++) {
    const SacFwdJob& jb = d.job[j];
    if (jb.net.nl < 1 || jb.net.nl > 4 || jb.n0 < 1 || jb.n1 < 0 || jb.n0 + jb.n1 != jb.net.sizes[0] || !jb.x0 || (jb.n1 && !jb.x1) || !jb.out) return hipErrorInvalidValue;
    for (int l = 0; l <= jb.net.nl; l++) if (jb.net.sizes[l] < 1 || jb.net.sizes[l] + 4 > jb.net.ldx) return hipErrorInvalidValue;
    ldx = max(ldx, jb.net.ldx);
  }
  if (sac_shmem(ldx) > 64 * 1024) return hipErrorInvalidValue;
  bool tanh_only = true;
  for (int j = 0; j < njob; j++) tanh_only = tanh_only && d.job[j].net.act == kActTanh;
  if (tanh_only) hipLaunchKernelGGL(hb_sac_forward_kernel, dim3((d.mb + 15) / 16, njob), dim3(512), sac_shmem(ldx), stream, d);
  else hipLaunchKernelGGL(hb_sac_forward_act_kernel, dim3((d.mb + 15) / 16, njob), dim3(512), sac_shmem(ldx), stream, d);
  return hipGetLastError();
}

hipError_t launch_sac_head(const SacHeadDesc& d, int what, hipStream_t stream) {
  (void)hipGetLastError();
  if (d.mb < 1 || d.nu < 1 || d.nu > kActorMaxNu || d.P < 1 || what < 0 || what > 2) return hipErrorInvalidValue;
  if (d.eps_given && (!d.eps_pi || !d.eps_next)) return hipErrorInvalidValue;
  const dim3 grid((d.mb + 255) / 256);
  if (what == 0) hipLaunchKernelGGL(hb_sac_sample_kernel, grid, dim3(256), 0, stream, d);
  else if (what == 1) hipLaunchKernelGGL(hb_sac_critic_head_kernel, grid, dim3(256), 0, stream, d);
  else hipLaunchKernelGGL(hb_sac_actor_head_kernel, grid, dim3(256), 0, stream, d);
  return hipGetLastError();
}

hipError_t launch_sac_backprop(const SacBwdDesc& d, int njob, hipStream_t stream) {
  (void)hipGetLastError();
  if (d.mb < 1 || njob < 1 || njob > 2) return hipErrorInvalidValue;
  int ldx = 1;
  for (int j = 0; j < njob; j++) {
    const SacBwdJob& jb = d.job[j];
    if (jb.net.nl < 0 || jb.net.nl > jb.L || jb.L < 1 || jb.L > 4 || (!jb.unit_top && !jb.top) || (jb.net.nl == jb.L && !jb.da)) return hipErrorInvalidValue;
    for (int l = 0; l <= jb.net.nl; l++) if (jb.net.sizes[l] < 1 || jb.net.sizes[l] + 4 > jb.net.ldx) return hipErrorInvalidValue;
    ldx = max(ldx, jb.net.ldx);
  }
  if (sac_shmem(ldx) > 64 * 1024) return hipErrorInvalidValue;
  bool tanh_only = true;
  for (int j = 0; j < njob; j++) tanh_only = tanh_only && d.job[j].activation == kActTanh;
  if (tanh_only) hipLaunchKernelGGL(hb_sac_backprop_kernel, dim3((d.mb + 15) / 16, njob), dim3(512), sac_shmem(ldx), stream, d);
  else hipLaunchKernelGGL(hb_sac_backprop_act_kernel, dim3((d.mb + 15) / 16, njob), dim3(512), sac_shmem(ldx), stream, d);
  return hipGetLastError();
}

hipError_t launch_sac_wgrad(const SacWgDesc& d, hipStream_t stream) {
  (void)hipGetLastError();
  if (d.mb < 1 || d.njob < 1 || d.njob > 8 || d.chunk < 1 || d.nchunk != (d.mb + d.chunk - 1) / d.chunk || d.nchunk > 64 || d.ncol < 1 || d.ncol > kSacSrow) return hipErrorInvalidValue;
  for (int j = 0; j < d.njob; j++) {
    const SacWgJob& jb = d.job[j];
    if (jb.K < 1 || jb.K > 256 || jb.N < 1 || jb.N > 256 || jb.off_w < 0 || jb.off_b < 0 || jb.off_w + jb.K * jb.N > d.P || jb.off_b + jb.N > d.P) return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(hb_sac_wgrad_kernel, dim3(d.nchunk, d.njob + 1), dim3(512), 0, stream, d);
  return hipGetLastError();
}

hipError_t launch_sac_reduce(const SacReduceDesc& d, hipStream_t stream) {
  (void)hipGetLastError();
  if (d.lo < 0 || d.hi <= d.lo || d.hi > d.P || d.nchunk < 1 || d.nchunk > 64 || d.mb < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hb_sac_reduce_kernel, dim3((d.hi - d.lo + 255) / 256 + 1), dim3(256), 0, stream, d);
  return hipGetLastError();
}

hipError_t launch_sac_adam(const SacAdamDesc& d, hipStream_t stream) {
  (void)hipGetLastError();
  if (d.lo < 0 || d.hi <= d.lo || d.nseg < 1 || d.nseg > kLearnMaxSeg || d.seg[0].start != d.lo || d.t < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hb_sac_adam_kernel, dim3((d.hi - d.lo + 255) / 256), dim3(256), 0, stream, d);
  return hipGetLastError();
}

hipError_t launch_sac_polyak(const SacPolyakDesc& d, hipStream_t stream) {
  (void)hipGetLastError();
  if (d.n < 1 || d.nseg < 1 || d.nseg > kLearnMaxSeg || d.seg[0].start != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hb_sac_polyak_kernel, dim3((d.n + 255) / 256), dim3(256), 0, stream, d);
  return hipGetLastError();
}

}  // namespace hb
