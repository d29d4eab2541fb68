// hb_sac_mlp.inl - included twice by hb_sac.hip (HB_ACT_ANY 0, then 1): the kernels as they were for tanh networks - tanhf written into the hooks, the
// text, registers and bits they had before a network could choose its hidden activation - and their *_act_kernel twins with the
// block-uniform run-time choice of mlp_act / mlp_act_slope (hb_kcommon.hpp), which costs a hook two to four registers and some scalar
// work (profiles/act_kernel_resources.txt, profiles/act_bench.txt).  The launchers pick the twin when a network is not tanh.
#if HB_ACT_ANY
#define HB_SAC_FORWARD_KERNEL hb_sac_forward_act_kernel
#define HB_SAC_BACKPROP_KERNEL hb_sac_backprop_act_kernel
#define HB_HIDDEN(act, v) mlp_act(act, v)
#define HB_SLOPE(act, a) mlp_act_slope(act, a)
#else
#define HB_SAC_FORWARD_KERNEL hb_sac_forward_kernel
#define HB_SAC_BACKPROP_KERNEL hb_sac_backprop_kernel
#define HB_HIDDEN(act, v) tanhf(v)
#define HB_SLOPE(act, a) __fmaf_rn(-(a), (a), 1.f)
#endif

__global__ __launch_bounds__(512) void HB_SAC_FORWARD_KERNEL(const SacFwdDesc d) {
  extern __shared__ __attribute__((aligned(16))) float sm_sac[];
  const SacFwdJob& jb = d.job[blockIdx.y];
  const PolicyDesc& pd = jb.net;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * 16, ldx = pd.ldx;
  const int live = min(16, d.mb - m0);
  float* cur = sm_sac;
  float* nxt = sm_sac + 16 * ldx;
  float* part = sm_sac + 32 * ldx;  // [8][16][16] partial tiles
  {
    // the input tile from its two sources; rows past mb and the K pad columns are zero
    const int n0 = jb.n0, n1 = jb.n1, nin = n0 + n1;
    for (int idx = tid; idx < 16 * nin; idx += 512) {
      const int row = idx / nin, c = idx - row * nin;
      float x = 0.f;
      if (row < live) {
        const int r = m0 + row;
        if (c < n0) x = jb.x0[(size_t)(jb.gather0 ? learn_src_row(d.index, d.first, r) : (long long)r) * n0 + c];
        else x = jb.x1[(size_t)(jb.gather1 ? learn_src_row(d.index, d.first, r) : (long long)r) * n1 + (c - n0)];
        if (jb.in_store) jb.in_store[(size_t)r * nin + c] = x;
      }
      cur[row * ldx + c] = x;
    }
    if (tid < 48) cur[(tid / 3) * ldx + nin + tid % 3] = 0.f;
  }
  __syncthreads();
  // (l: the layer index of the loop)
#define HB_MLP_EMIT(row, n, v) do { \
    const float a_ = last ? (v) : HB_HIDDEN(pd.act, v); \
    nxt[(row) * ldx + (n)] = a_; \
    if ((row) < live) { \
      if (last) jb.out[(size_t)(m0 + (row)) * N + (n)] = a_; \
      else if (jb.act[1]) jb.act[l + 1][(size_t)(m0 + (row)) * N + (n)] = a_; \
    } \
  } while (0)
#include "hb_mlp_layers.inl"
#undef HB_MLP_EMIT
}

__global__ __launch_bounds__(512) void HB_SAC_BACKPROP_KERNEL(const SacBwdDesc d) {
  extern __shared__ __attribute__((aligned(16))) float sm_sac[];
  const SacBwdJob& jb = d.job[blockIdx.y];
  const PolicyDesc& pd = jb.net;
  if (pd.nl < 1) return;  // one layer and no input gradient: its dZ is the head's
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * 16, ldx = pd.ldx, L = jb.L;
  const int live = min(16, d.mb - m0);
  float* cur = sm_sac;
  float* nxt = sm_sac + 16 * ldx;
  float* part = sm_sac + 32 * ldx;
  {
    const int n0 = pd.sizes[0];
    for (int idx = tid; idx < 16 * n0; idx += 512) {
      const int row = idx / n0;
      cur[row * ldx + (idx - row * n0)] = row < live ? (jb.unit_top ? 1.f : jb.top[(size_t)m0 * n0 + idx]) : 0.f;
    }
    if (tid < 48) cur[(tid / 3) * ldx + n0 + tid % 3] = 0.f;
  }
  __syncthreads();
  // step l of the loop multiplies by the transpose of layer L - 1 - l: v is dloss / dact[L - 1 - l] - an output of the hidden activation, or
  // for L - 1 - l == 0 (a Q network's nl = L) the action inputs, which are no activation's output: no derivative
#define HB_MLP_EMIT(row, n, v) do { \
    float g_ = 0.f; \
    if ((row) < live) { \
      const size_t o_ = (size_t)(m0 + (row)) * N + (n); \
      if (L - 1 - l == 0) { \
        g_ = (v); \
        jb.da[o_] = g_; \
      } else { \
        const float a_ = jb.act[L - 1 - l][o_]; \
        g_ = (v) * HB_SLOPE(jb.activation, a_); \
        if (jb.dz[0]) jb.dz[L - 2 - l][o_] = g_; \
      } \
    } \
    nxt[(row) * ldx + (n)] = g_; \
  } while (0)
#include "hb_mlp_layers.inl"
#undef HB_MLP_EMIT
}

#undef HB_SAC_FORWARD_KERNEL
#undef HB_SAC_BACKPROP_KERNEL
#undef HB_HIDDEN
#undef HB_SLOPE
