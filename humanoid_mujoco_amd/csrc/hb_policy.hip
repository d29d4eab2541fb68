// hb_policy.hip - the policy MLP (hb_policy_*): the layer-by-layer kernel of wide networks and the fused kernels of hb_policy_kernels.inl,
// and their launchers.
#include <hip/hip_runtime.h>
#include "hb_kcommon.hpp"
#include "hb_launch.hpp"

namespace hb {

// One dense layer of the policy MLP on the matrix cores: Y[M][N] = act(X[M][K] W[K][N] + b[N]); act 0: none, else 1 + kAct*.
// One wave per 32x32 output tile, K swept two columns per v_mfma_f32_32x32x2_f32 (exact f32); the X tile
// is staged through LDS (row stride K+1: conflict-free A-operand reads), W streams from L2 coalesced.
__global__ __launch_bounds__(kGroup) void hb_mlp_layer_kernel(const float* X, const float* W, const float* bias, float* Y, int Mrows, int K, int N, int act) {
  extern __shared__ float xs[];
  const int lane = threadIdx.x, m0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
  const int ks = K + 1;
  for (int idx = lane; idx < 32 * K; idx += kGroup) {
    const int r = idx / K, c = idx - r * K;
    xs[r * ks + c] = (m0 + r < Mrows) ? X[(size_t)(m0 + r) * K + c] : 0.f;
  }
  __syncthreads();
  const int col = lane & 31, half = lane >> 5;
  const bool nvld = n0 + col < N;
  f32x16 D;
#pragma unroll
  for (int r = 0; r < 16; r++) D[r] = 0.f;
  for (int k0 = 0; k0 < K; k0 += 2) {
    const int k = k0 + half;
    const float a = k < K ? xs[col * ks + k] : 0.f;
    const float bv = (nvld && k < K) ? W[(size_t)k * N + n0 + col] : 0.f;
    D = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, D, 0, 0, 0);
  }
  const float bn = nvld ? bias[n0 + col] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int row = m0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (row < Mrows && nvld) {
      float v = D[r] + bn;
      Y[(size_t)row * N + n0 + col] = act ? mlp_act(act - 1, v) : v;
    }
  }
}

// hb_policy_kernel, hb_policy_lean_kernel and their twins for networks that are not tanh
#define HB_ACT_ANY 0
#include "hb_policy_kernels.inl"
#undef HB_ACT_ANY
#define HB_ACT_ANY 1
#include "hb_policy_kernels.inl"
#undef HB_ACT_ANY

hipError_t launch_mlp_layer(const float* X, const float* W, const float* bias, float* Y, int Mrows, int K, int N, int act, hipStream_t stream) {
  (void)hipGetLastError();  // the result below must be this launch's, not an older call's sticky error
  hipLaunchKernelGGL(hb_mlp_layer_kernel, dim3((Mrows + 31) / 32, (N + 31) / 32), dim3(kGroup), (size_t)32 * (K + 1) * sizeof(float), stream, X, W, bias, Y, Mrows, K, N, act);
  return hipGetLastError();
}
hipError_t launch_policy_lean(const DevModel& M, const PolicyDesc& pd, const float* state, float* ctrl, float* act, int n_env, hipStream_t stream) {
  (void)hipGetLastError();
  if (pd.act == kActTanh) hipLaunchKernelGGL(hb_policy_lean_kernel, dim3((n_env + 15) / 16), dim3(256), 0, stream, M, pd, state, ctrl, act, n_env);
  else hipLaunchKernelGGL(hb_policy_lean_act_kernel, dim3((n_env + 15) / 16), dim3(256), 0, stream, M, pd, state, ctrl, act, n_env);
  return hipGetLastError();
}
hipError_t launch_policy(const DevModel& M, const PolicyDesc& pd, const float* state, float* ctrl, int n_env, hipStream_t stream) {
  const size_t shmem = ((size_t)32 * pd.ldx + 8 * 256) * sizeof(float);
  (void)hipGetLastError();  // the result below must be this launch's, not an older call's sticky error
  if (pd.act == kActTanh) hipLaunchKernelGGL(hb_policy_kernel, dim3((n_env + 15) / 16), dim3(512), shmem, stream, M, pd, state, ctrl, n_env);
  else hipLaunchKernelGGL(hb_policy_act_kernel, dim3((n_env + 15) / 16), dim3(512), shmem, stream, M, pd, state, ctrl, n_env);
  return hipGetLastError();
}
}  // namespace hb
