// hb_actor.hip - the sampling actor of hb_env_collect_dev: observation rows -> MLP -> head (deterministic / Gaussian / squashed Gaussian)
// -> action and the tapes of what was drawn, one launch per env step.  A translation unit of its own: the kernels of hb_env.hip and hb_policy.hip compile
// exactly as they did without it.
#include <hip/hip_runtime.h>
#include "hb_kcommon.hpp"
#include "hb_launch.hpp"

namespace hb {

// hb_policy_kernel's design (hb_policy.hip): 16 envs per block, activations ping-pong between two LDS tiles of 16 rows, eight waves share the
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
#define HB_ACT_ANY 0
#include "hb_actor_kernel.inl"
#undef HB_ACT_ANY
#define HB_ACT_ANY 1
#include "hb_actor_kernel.inl"
#undef HB_ACT_ANY

hipError_t launch_actor(const ActorDesc& ad, const float* obs, const ActorTapes& tp, int n_env, unsigned env_global0, unsigned draw, hipStream_t stream) {
  (void)hipGetLastError();
  if (n_env < 1 || !obs || !tp.action) return hipErrorInvalidValue;
  const size_t shmem = ((size_t)32 * ad.net.ldx + 8 * 256) * sizeof(float);  // two activation tiles + the split-K partial tiles
  if (shmem > 64 * 1024) return hipErrorInvalidValue;
  if (ad.net.act == kActTanh) hipLaunchKernelGGL(hb_actor_kernel, dim3((n_env + 15) / 16), dim3(512), shmem, stream, ad, obs, tp, n_env, env_global0, draw);
  else hipLaunchKernelGGL(hb_actor_act_kernel, dim3((n_env + 15) / 16), dim3(512), shmem, stream, ad, obs, tp, n_env, env_global0, draw);
  return hipGetLastError();
}

}  // namespace hb
