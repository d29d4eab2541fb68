// hb_ppo_mlp.inl - included twice by hb_ppo.hip (HB_ACT_ANY 0, then 1): the kernels as they were for tanh networks - tanhf written into the hooks, the
// text, registers and bits they had before a network could choose its hidden activation - and their *_act_kernel twins with the
// block-uniform run-time choice of mlp_act / mlp_act_slope (hb_kcommon.hpp), which costs a hook two to four registers and some scalar
// work (profiles/act_kernel_resources.txt, profiles/act_bench.txt).  The launchers pick the twin when a network is not tanh.
#if HB_ACT_ANY
#define HB_PPO_FORWARD_KERNEL hb_ppo_forward_act_kernel
#define HB_PPO_BACKPROP_KERNEL hb_ppo_backprop_act_kernel
#define HB_HIDDEN(act, v) mlp_act(act, v)
#define HB_SLOPE(act, a) mlp_act_slope(act, a)
#else
#define HB_PPO_FORWARD_KERNEL hb_ppo_forward_kernel
#define HB_PPO_BACKPROP_KERNEL hb_ppo_backprop_kernel
#define HB_HIDDEN(act, v) tanhf(v)
#define HB_SLOPE(act, a) __fmaf_rn(-(a), (a), 1.f)
#endif

__global__ __launch_bounds__(512) void HB_PPO_FORWARD_KERNEL(const PpoDesc d) {
  extern __shared__ __attribute__((aligned(16))) float sm_ppo[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (blockIdx.y == 2) {
    // chunk sums of the advantage: lane t takes rows t, t + 512, ... of the chunk, lane 0 adds the 512 sums in lane order
    const int c = blockIdx.x;
    if (c >= d.nchunk) return;
    double* red = (double*)sm_ppo;
    const int r1 = min(d.mb, (c + 1) * d.chunk);
    double s = 0.0, q = 0.0;
    for (int r = c * d.chunk + tid; r < r1; r += 512) {
      const double a = (double)d.advantage[learn_src_row(d.index, d.first, r)];
      s += a; q += a * a;
    }
    red[tid] = s; red[512 + tid] = q;
    __syncthreads();
    if (tid == 0) {
      double S = 0.0, Q = 0.0;
      for (int t = 0; t < 512; t++) { S += red[t]; Q += red[512 + t]; }
      d.advpart[2 * c] = S; d.advpart[2 * c + 1] = Q;
    }
    return;
  }
  const PpoNet& nw = d.net[blockIdx.y];
  const PolicyDesc& pd = nw.fwd;
  const int m0 = blockIdx.x * 16, ldx = pd.ldx;
  const int live = min(16, d.mb - m0);
  float* cur = sm_ppo;
  float* nxt = sm_ppo + 16 * ldx;
  float* part = sm_ppo + 32 * ldx;  // [8][16][16] partial tiles
  {
    // the gathered observation tile; rows past mb and the K pad columns are zero.  The actor's blocks keep it as act[0] for the dW pass.
    const int nobs = pd.sizes[0];
    for (int idx = tid; idx < 16 * nobs; idx += 512) {
      const int row = idx / nobs, c = idx - row * nobs;
      float x = 0.f;
      if (row < live) {
        x = d.obs[(size_t)learn_src_row(d.index, d.first, m0 + row) * nobs + c];
        if (blockIdx.y == 0) nw.act[0][(size_t)(m0 + row) * nobs + c] = x;
      }
      cur[row * ldx + c] = x;
    }
    if (tid < 48) cur[(tid / 3) * ldx + nobs + tid % 3] = 0.f;
  }
  __syncthreads();
  // (l: the layer index of the loop)
#define HB_MLP_EMIT(row, n, v) do { \
    const float a_ = last ? (v) : HB_HIDDEN(pd.act, v); \
    nxt[(row) * ldx + (n)] = a_; \
    if ((row) < live) { \
      if (last) nw.out[(size_t)(m0 + (row)) * N + (n)] = a_; \
      else nw.act[l + 1][(size_t)(m0 + (row)) * N + (n)] = a_; \
    } \
  } while (0)
#include "hb_mlp_layers.inl"
#undef HB_MLP_EMIT
}

__global__ __launch_bounds__(512) void HB_PPO_BACKPROP_KERNEL(const PpoDesc d) {
  extern __shared__ __attribute__((aligned(16))) float sm_ppo[];
  const PpoNet& nw = d.net[blockIdx.y];
  const PolicyDesc& pd = nw.bwd;
  if (pd.nl < 1) return;  // one layer: its dZ is the head's
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * 16, ldx = pd.ldx, L = nw.fwd.nl;
  const int live = min(16, d.mb - m0);
  float* cur = sm_ppo;
  float* nxt = sm_ppo + 16 * ldx;
  float* part = sm_ppo + 32 * ldx;
  {
    const int n0 = pd.sizes[0];
    const float* src = nw.dz[L - 1] + (size_t)m0 * n0;
    for (int idx = tid; idx < 16 * n0; idx += 512) {
      const int row = idx / n0, c = idx - row * n0;
      cur[row * ldx + c] = row < live ? src[idx] : 0.f;
    }
    if (tid < 48) cur[(tid / 3) * ldx + n0 + tid % 3] = 0.f;
  }
  __syncthreads();
  // step l of the loop multiplies by the transpose of layer L - 1 - l: v is dloss / dact[L - 1 - l], an output of the hidden activation
#define HB_MLP_EMIT(row, n, v) do { \
    float g_ = 0.f; \
    if ((row) < live) { \
      const size_t o_ = (size_t)(m0 + (row)) * N + (n); \
      const float a_ = nw.act[L - 1 - l][o_]; \
      g_ = (v) * HB_SLOPE(nw.fwd.act, a_); \
      nw.dz[L - 2 - l][o_] = g_; \
    } \
    nxt[(row) * ldx + (n)] = g_; \
  } while (0)
#include "hb_mlp_layers.inl"
#undef HB_MLP_EMIT
}

#undef HB_PPO_FORWARD_KERNEL
#undef HB_PPO_BACKPROP_KERNEL
#undef HB_HIDDEN
#undef HB_SLOPE
