// hb_value_kernel.inl - included twice by hb_gae.hip (HB_ACT_ANY 0, then 1): the kernels as they were for tanh networks - tanhf written into the hooks, the
// text, registers and bits they had before a network could choose its hidden activation - and their *_act_kernel twins with the
// block-uniform run-time choice of mlp_act / mlp_act_slope (hb_kcommon.hpp), which costs a hook two to four registers and some scalar
// work (profiles/act_kernel_resources.txt, profiles/act_bench.txt).  The launchers pick the twin when a network is not tanh.
#if HB_ACT_ANY
#define HB_VALUE_KERNEL hb_value_act_kernel
#define HB_HIDDEN(act, v) mlp_act(act, v)
#else
#define HB_VALUE_KERNEL hb_value_kernel
#define HB_HIDDEN(act, v) tanhf(v)
#endif

__global__ __launch_bounds__(512) void HB_VALUE_KERNEL(const PolicyDesc pd, const float* rows, const uint8_t* term, const uint8_t* trunc, long long n_rows, float* out) {
  extern __shared__ __attribute__((aligned(16))) float sm_value[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.x * 16;
  const int ldx = pd.ldx;
  const int live = (int)min(16LL, n_rows - m0);  // rows of this block that exist
  // bit r: row m0 + r is evaluated (every wave forms the same word)
  unsigned sel = (1u << live) - 1u;
  if (term) sel = (unsigned)__ballot(lane < live && trunc[m0 + min(lane, live - 1)] && !term[m0 + min(lane, live - 1)]) & 0xffffu;
  if (!sel) {
    if (tid < live) out[m0 + tid] = 0.f;
    return;
  }
  float* cur = sm_value;
  float* nxt = sm_value + 16 * ldx;
  float* part = sm_value + 32 * ldx;  // [8][16][16] partial tiles
  {
    const int nobs = pd.sizes[0];
    const float* src = rows + (size_t)m0 * nobs;
    for (int idx = tid; idx < 16 * nobs; idx += 512) {
      const int row = idx / nobs, c = idx - row * nobs;
      cur[row * ldx + c] = (sel >> row & 1u) ? src[idx] : 0.f;
    }
    if (tid < 48) cur[(tid / 3) * ldx + nobs + tid % 3] = 0.f;
  }
  __syncthreads();
#define HB_MLP_EMIT(row, n, v) nxt[(row) * ldx + (n)] = last ? (v) : HB_HIDDEN(pd.act, v)  // (the critic is linear at the top)
#include "hb_mlp_layers.inl"
#undef HB_MLP_EMIT
  // cur holds the last layer's output, column 0 of every row
  if (tid < live) out[m0 + tid] = (sel >> tid & 1u) ? cur[tid * ldx] : 0.f;
}

#undef HB_VALUE_KERNEL
#undef HB_HIDDEN
