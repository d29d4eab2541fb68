// hb_actor_kernel.inl - included twice by hb_actor.hip (HB_ACT_ANY 0, then 1): the kernels as they were for tanh networks - tanhf written into the hooks, the
// text, registers and bits they had before a network could choose its hidden activation - and their *_act_kernel twins with the
// block-uniform run-time choice of mlp_act / mlp_act_slope (hb_kcommon.hpp), which costs a hook two to four registers and some scalar
// work (profiles/act_kernel_resources.txt, profiles/act_bench.txt).  The launchers pick the twin when a network is not tanh.
#if HB_ACT_ANY
#define HB_ACTOR_KERNEL hb_actor_act_kernel
#define HB_HIDDEN(act, v) mlp_act(act, v)
#else
#define HB_ACTOR_KERNEL hb_actor_kernel
#define HB_HIDDEN(act, v) tanhf(v)
#endif

__global__ __launch_bounds__(512) void HB_ACTOR_KERNEL(const ActorDesc ad, const float* obs, const ActorTapes tp, int n_env, unsigned env_global0, unsigned draw) {
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
#define HB_MLP_EMIT(row, n, v) nxt[(row) * ldx + (n)] = last ? (v) : HB_HIDDEN(pd.act, v)  // (the last layer's activation belongs to the head)
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

#undef HB_ACTOR_KERNEL
#undef HB_HIDDEN
