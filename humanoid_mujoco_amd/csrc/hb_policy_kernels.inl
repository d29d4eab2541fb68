// hb_policy_kernels.inl - included twice by hb_policy.hip (HB_ACT_ANY 0, then 1): the kernels as they were for tanh networks - tanhf written into the hooks, the
// text, registers and bits they had before a network could choose its hidden activation - and their *_act_kernel twins with the
// block-uniform run-time choice of mlp_act / mlp_act_slope (hb_kcommon.hpp), which costs a hook two to four registers and some scalar
// work (profiles/act_kernel_resources.txt, profiles/act_bench.txt).  The launchers pick the twin when a network is not tanh.
#if HB_ACT_ANY
#define HB_POLICY_KERNEL hb_policy_act_kernel
#define HB_POLICY_LEAN_KERNEL hb_policy_lean_act_kernel
#define HB_POLICY_ACT(v) mlp_act(last ? kActTanh : pd.act, v)
#else
#define HB_POLICY_KERNEL hb_policy_kernel
#define HB_POLICY_LEAN_KERNEL hb_policy_lean_kernel
#define HB_POLICY_ACT(v) tanhf(v)
#endif

// The whole policy in one launch: observation -> every MLP layer -> controls, for 16 envs per block (4096 envs = 256
// blocks: one per CU; f32 MFMA throughput per CU is the bound, so the batch is spread over the whole chip).
// Activations never leave LDS (two ping-pong tiles of 16 rows); eight waves share the 16-column output tiles of a
// layer, each sweeping K four columns per v_mfma_f32_16x16x4_f32 (exact f32) with the A operand from LDS and the
// B operand from weights pre-packed on the host in operand order (one coalesced 256-byte wave load per MFMA:
// wp[tile][k/4][lane] = W[4(k/4) + lane/16][16 tile + lane%16]).  A layer with fewer than eight tiles (the
// nu-wide output layer) splits K across the idle waves instead; the partial tiles are summed in a fixed order
// (deterministic, no atomics).  The layer loop is hb_mlp_layers.inl, shared with hb_actor_kernel and hb_value_kernel.
__global__ __launch_bounds__(512) void HB_POLICY_KERNEL(const DevModel M, const PolicyDesc pd, const float* state, float* ctrl, int n_env) {
  extern __shared__ float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * 16, ldx = pd.ldx;
  float* cur = sm;
  float* nxt = sm + 16 * ldx;
  float* part = sm + 32 * ldx;  // [8][16][16] partial tiles
  // observation tile: 32 threads per env row gather the copied entries through the gather table (independent loads,
  // all in flight at once), one thread per row derives the gravity direction from the root quaternion
  {
    const int row = tid >> 5, sub = tid & 31;
    float* o = cur + row * ldx;
    const bool live = m0 + row < n_env;
    const float* s = state + (size_t)(m0 + row) * M.nstate;
    const int ncopy = M.nobs - 3;
    for (int k = sub; k < ncopy; k += 32) {
      const int src = M.obs_src[k];
      o[k] = (live && src >= 0) ? s[src] : 0.f;
    }
    if (sub == 0) {
      Q4 q = {1.f, 0.f, 0.f, 0.f};
      if (live && M.obs_root_qadr >= 0) q = qnormalize(ldq(s + 1 + M.obs_root_qadr + 3));
      float mm[9];
      q2mat(mm, q);
      o[ncopy] = live ? -mm[6] : 0.f; o[ncopy + 1] = live ? -mm[7] : 0.f; o[ncopy + 2] = live ? -mm[8] : 0.f;
      for (int k = M.nobs; k < M.nobs + 3; k++) o[k] = 0.f;  // K is swept four at a time: the pad columns must be finite
    }
  }
  __syncthreads();
  // the installed activation behind every hidden layer, tanh behind the last; its outputs are the controls of the rows that are envs
#define HB_MLP_EMIT(row, n, v)                                                                     \
  do {                                                                                             \
    const float y_ = HB_POLICY_ACT(v);                                                             \
    if (!last) nxt[(row) * ldx + (n)] = y_;                                                        \
    else if (m0 + (row) < n_env) ctrl[(size_t)(m0 + (row)) * N + (n)] = y_;                        \
  } while (0)
#include "hb_mlp_layers.inl"
#undef HB_MLP_EMIT
}

// The same policy without LDS and inside 64 VGPRs: four waves per block of sixteen envs, activations ping-pong through an L2-resident
// scratch (the waves of a block share the CU's vector L1).  Two step-kernel waves per SIMD leave 64 VGPRs, six wave slots and no LDS:
// blocks of THIS kernel run beside them (measured: 6 us slower beside a chip full of step waves than alone), where the LDS variant
// (33 KB per block) waits for two step blocks of a CU to retire (config 4, pipelined: its 10 us became 43).
// Activations are stored in the A-operand order of v_mfma_f32_16x16x4_f32 - element (env row, k) at [k / 4][k % 4][row] - so that a
// k-step's operand is one contiguous 256-byte wave load like the host-packed weights (row-major rows 260 floats apart cost sixteen
// cache lines per load: 52 us for 4096 envs).
// (amdgpu_num_vgpr counts per half of the unified register file: 32 -> 64 registers in all, tools/kernel_resources.sh; with 48 - what
// is left beside two 232-register waves - the kernel spills 23 values and the loop runs 3.10e7 instead of 3.20e7 env-steps/s)
__attribute__((amdgpu_num_vgpr(32))) __global__ __launch_bounds__(256) void HB_POLICY_LEAN_KERNEL(const DevModel M, const PolicyDesc pd, const float* state, float* ctrl,
                                                                                                  float* act, int n_env) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * 16, ldx = pd.ldx;
  float* cur = act + (size_t)blockIdx.x * 32 * ldx;  // [ldx / 4][4][16]
  float* nxt = cur + 16 * ldx;
  {
    const int row = tid & 15, sub = tid >> 4;  // sixteen threads per observation column stride, consecutive threads = consecutive rows
    const bool live = m0 + row < n_env;
    const float* s = state + (size_t)(live ? m0 + row : 0) * M.nstate;
    const int ncopy = M.nobs - 3;
    for (int k = sub; k < ncopy; k += 16) {
      const int src = M.obs_src[k];
      cur[(k >> 2) * 64 + (k & 3) * 16 + row] = (live && src >= 0) ? s[src] : 0.f;
    }
    if (sub == 0) {
      Q4 q = {1.f, 0.f, 0.f, 0.f};
      if (live && M.obs_root_qadr >= 0) q = qnormalize(ldq(s + 1 + M.obs_root_qadr + 3));
      // third row of the rotation matrix of q (q2mat's m[6..8])
      const float m6 = 2.f * (q.x * q.z - q.w * q.y), m7 = 2.f * (q.y * q.z + q.w * q.x), m8 = q.w * q.w - q.x * q.x - q.y * q.y + q.z * q.z;
      const float g3[3] = {live ? -m6 : 0.f, live ? -m7 : 0.f, live ? -m8 : 0.f};
      for (int c = 0; c < 3; c++) { const int k = ncopy + c; cur[(k >> 2) * 64 + (k & 3) * 16 + row] = g3[c]; }
      for (int k = M.nobs; k < ((M.nobs + 3) & ~3); k++) cur[(k >> 2) * 64 + (k & 3) * 16 + row] = 0.f;  // K is swept four at a time: the pad columns must be finite
    }
  }
  __syncthreads();
  const int col = lane & 15, quad = lane >> 4;  // B: k offset = quad, column = col;  D: rows 4 quad + r, column col
  for (int l = 0; l < pd.nl; l++) {
    const int K = pd.sizes[l], N = pd.sizes[l + 1], KK = (K + 3) / 4, ntile = (N + 15) / 16;
    const bool last = l + 1 == pd.nl;
    const float* wp = pd.w[l];
    const float* bias = pd.b[l];
    if (!last && tid < 16 * (((N + 3) & ~3) - N)) { const int k = N + tid / 16; nxt[(k >> 2) * 64 + (k & 3) * 16 + (tid & 15)] = 0.f; }  // pad columns of the next layer's input
    // two output tiles per wave and pass: they share the A operand, and their accumulators are two independent MFMA chains
    for (int nt = 2 * wave; nt < ntile; nt += 8) {
      const bool two = nt + 1 < ntile;
      f32x4 D0 = {0.f, 0.f, 0.f, 0.f}, D1 = {0.f, 0.f, 0.f, 0.f};
      const float* ap = cur + lane;
      const float* bp0 = wp + (size_t)nt * KK * 64 + lane;
      const float* bp1 = bp0 + (two ? (size_t)KK * 64 : 0);
      int kk = 0;
      for (; kk + 4 <= KK; kk += 4) {  // four k-steps of operands in flight per batch of MFMAs (measured: three are slower; loading the next batch under this one's MFMAs changes nothing)
        float a[4], w0[4], w1[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { a[u] = ap[(kk + u) * 64]; w0[u] = bp0[(kk + u) * 64]; w1[u] = bp1[(kk + u) * 64]; }
#pragma unroll
        for (int u = 0; u < 4; u++) {
          D0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w0[u], D0, 0, 0, 0);
          D1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w1[u], D1, 0, 0, 0);
        }
      }
      for (; kk < KK; kk++) {
        const float a = ap[kk * 64];
        D0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp0[kk * 64], D0, 0, 0, 0);
        D1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp1[kk * 64], D1, 0, 0, 0);
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        if (h == 1 && !two) break;
        const int n = (nt + h) * 16 + col;
        const float bn = n < N ? bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = 4 * quad + r;
          if (n < N) {
            const float v = HB_POLICY_ACT((h ? D1[r] : D0[r]) + bn);
            if (!last) nxt[(n >> 2) * 64 + (n & 3) * 16 + row] = v;
            else if (m0 + row < n_env) ctrl[(size_t)(m0 + row) * N + n] = v;
          }
        }
      }
    }
    __syncthreads();
    float* t = cur; cur = nxt; nxt = t;
  }
}

#undef HB_POLICY_KERNEL
#undef HB_POLICY_LEAN_KERNEL
#undef HB_POLICY_ACT
