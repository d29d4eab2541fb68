// hb_actor.hip - the sampling actor of hb_env_collect_dev: observation rows -> MLP -> head (deterministic / Gaussian / squashed Gaussian)
// -> action and the tapes of what was drawn, one launch per env step.  A translation unit of its own: the kernels of hb_env.hip compile
// exactly as they did without it.
#include <hip/hip_runtime.h>
#include "hb_kcommon.hpp"
#include "hb_launch.hpp"

namespace hb {

// hb_policy_kernel's design (hb_env.hip): 16 envs per block, activations ping-pong between two LDS tiles of 16 rows, eight waves share the
// 16-column output tiles of a layer, each sweeping K four columns per v_mfma_f32_16x16x4_f32 (exact f32) with the A operand from LDS and
// the B operand from weights the host packed in operand order (wp[tile][k/4][lane] = W[4(k/4) + lane/16][16 tile + lane%16], one coalesced
// 256-byte wave load per MFMA); a layer with fewer than eight tiles splits K across the idle waves and the partial tiles are summed in a
// fixed order (deterministic, no atomics).  That layer loop is hb_mlp_layers.inl, included in place by the three kernels that run it
// (here, hb_policy_kernel, hb_value_kernel): "head 0 is the existing policy" holds because it is the same source.  What differs:
//  - the input tile is read from an observation row [n_env][nobs] - the env adapter's noisy, delayed observation - in one coalesced pass;
//  - the last layer leaves its pre-activations (bias added) in the LDS tile, and a head pass with one lane per (env, actuator) forms
//    mean, log_std, the N(0, 1) draw and the action and stores them: the block's 16 rows are one contiguous stretch of every tape, so
//    consecutive lanes write consecutive floats.
// The draw of (env, actuator) depends on the env's GLOBAL index and the step counter only (rng_normal, hb_kcommon.hpp): the same on any
// split of a batch, whatever block or lane computes it.
__global__ __launch_bounds__(512) void hb_actor_kernel(const ActorDesc ad, const float* obs, const ActorTapes tp, int n_env, unsigned env_global0, unsigned draw) {
  extern __shared__ __attribute__((aligned(16))) float sm_actor[];
  const PolicyDesc& pd = ad.net;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * 16, ldx = pd.ldx;
  const int live = min(16, n_env - m0);  // rows of this block that are envs
  float* cur = sm_actor;
  float* nxt = sm_actor + 16 * ldx;
  float* part = sm_actor + 32 * ldx;  // [8][16][16] partial tiles
  {
    // observation tile: the block's rows are one contiguous stretch of obs; rows past n_env and the K pad columns are zero (finite)
    const int nobs = pd.sizes[0];
    const float* src = obs + (size_t)m0 * nobs;
    for (int idx = tid; idx < 16 * nobs; idx += 512) {
      const int row = idx / nobs, c = idx - row * nobs;
      cur[row * ldx + c] = row < live ? src[idx] : 0.f;
    }
    if (tid < 48) cur[(tid / 3) * ldx + nobs + tid % 3] = 0.f;
  }
  __syncthreads();
#define HB_MLP_EMIT(row, n, v) nxt[(row) * ldx + (n)] = last ? (v) : tanhf(v)  // (the last layer's activation belongs to the head)
#include "hb_mlp_layers.inl"
#undef HB_MLP_EMIT
  // the head: cur holds the last layer's pre-activations [16][nu] (head 2: [16][2 nu], mean | log_std)
  const int nu = ad.nu;
  for (int idx = tid; idx < live * nu; idx += 512) {
    const int row = idx / nu, i = idx - row * nu;
    const float v = cur[row * ldx + i];
    float mean, ls = 0.f, eps = 0.f, action;
    if (ad.head == kActorDeterministic) {
      mean = action = tanhf(v);
    } else {
      mean = v;
      ls = ad.head == kActorSquashed ? fminf(2.f, fmaxf(-20.f, cur[row * ldx + nu + i])) : ad.log_std[i];
      if (!ad.deterministic) eps = rng_normal(ad.seed, env_global0 + (unsigned)(m0 + row), 0u, draw, RS_ACTOR, (unsigned)i);
      const float pre = mean + expf(ls) * eps;
      action = ad.head == kActorSquashed ? tanhf(pre) : pre;
    }
    const size_t o = (size_t)m0 * nu + idx;
    tp.action[o] = action;
    if (tp.mean) tp.mean[o] = mean;
    if (tp.log_std) tp.log_std[o] = ls;
    if (tp.eps) tp.eps[o] = eps;
  }
}

hipError_t launch_actor(const ActorDesc& ad, const float* obs, const ActorTapes& tp, int n_env, unsigned env_global0, unsigned draw, hipStream_t stream) {
  (void)hipGetLastError();
  if (n_env < 1 || !obs || !tp.action) return hipErrorInvalidValue;
  const size_t shmem = ((size_t)32 * ad.net.ldx + 8 * 256) * sizeof(float);  // two activation tiles + the split-K partial tiles
  if (shmem > 64 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hb_actor_kernel, dim3((n_env + 15) / 16), dim3(512), shmem, stream, ad, obs, tp, n_env, env_global0, draw);
  return hipGetLastError();
}

}  // namespace hb
