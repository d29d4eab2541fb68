// hb_learn_core.hpp - what the learners' kernels share (hb_ppo.hip, hb_sac.hip): the gather of a minibatch row, dW = A^T dZ and db over a
// chunk of rows, the merge of the chunk partials, and Adam's step on one entry.  Each learner stays a translation unit of its own and
// keeps its kernels; these are their bodies.  The refresh of the packed operands behind a step (ParamSeg, learn_refresh) is
// hb_device.hpp's, where the host can run it too.
#pragma once
#include "hb_kcommon.hpp"

namespace hb {

// minibatch row r of the tapes
__device__ __forceinline__ long long learn_src_row(const int* index, long long first, int r) { return index ? (long long)index[r] : first + r; }

// dW = A^T dZ and db = colsum dZ over the rows [r0, r1) of A [mb][K] and Z [mb][N], by one block of 512 lanes: the A operand of the MFMA
// is A^T (row i = input column, k = minibatch row), the B operand dZ (k = minibatch row, column = output column), both read from the
// block's 16-row LDS tiles sA, sZ [16 * 272].  Wave w owns the output tiles (kt, nt), kt = w and w + 8, nt = 0 .. 15: 32 accumulators,
// which cover the widest layer (256 x 256).  db: lane n adds column n of every dZ tile in row order.  gw [K][N] and gb [N] are written.
__device__ __forceinline__ void learn_wgrad_chunk(const float* A, const float* Z, int K, int N, int r0, int r1, float* gw, float* gb, float* sA, float* sZ) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Kp = (K + 15) / 16 * 16, Np = (N + 15) / 16 * 16, lda = ppo_ld(K), ldz = ppo_ld(N);
  const int ktiles = Kp / 16, ntiles = Np / 16;
  const int col = lane & 15, quad = lane >> 4;
  f32x4 acc[2][16];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 16; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  for (int t0 = r0; t0 < r1; t0 += 16) {
    for (int idx = tid; idx < 16 * Kp; idx += 512) {
      const int row = idx / Kp, k = idx - row * Kp;
      sA[row * lda + k] = (t0 + row < r1 && k < K) ? A[(size_t)(t0 + row) * K + k] : 0.f;
    }
    for (int idx = tid; idx < 16 * Np; idx += 512) {
      const int row = idx / Np, n = idx - row * Np;
      sZ[row * ldz + n] = (t0 + row < r1 && n < N) ? Z[(size_t)(t0 + row) * N + n] : 0.f;
    }
    __syncthreads();
    if (wave < ktiles) {
      const bool two = wave + 8 < ktiles;
      for (int s = 0; s < 4; s++) {
        const float a0 = sA[(4 * s + quad) * lda + wave * 16 + col];
        const float a1 = two ? sA[(4 * s + quad) * lda + (wave + 8) * 16 + col] : 0.f;
        const float* zp = sZ + (4 * s + quad) * ldz + col;
#pragma unroll
        for (int nt = 0; nt < 16; nt++) {
          if (nt < ntiles) {
            const float z = zp[nt * 16];
            acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, z, acc[0][nt], 0, 0, 0);
            if (two) acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, z, acc[1][nt], 0, 0, 0);
          }
        }
      }
    }
    if (tid < N) {
      for (int row = 0; row < 16; row++) bsum += sZ[row * ldz + tid];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int kt = wave + 8 * i;
    if (kt < ktiles) {
#pragma unroll
      for (int nt = 0; nt < 16; nt++) {
        if (nt < ntiles) {
          const int n = nt * 16 + col;
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int k = kt * 16 + 4 * quad + r;
            if (k < K && n < N) gw[(size_t)k * N + n] = acc[i][nt][r];
          }
        }
      }
    }
  }
  if (tid < N) gb[tid] = bsum;
}

// entry i of the gradient: the chunk partials part [nchunk][P] summed in chunk order
__device__ __forceinline__ float learn_partials_sum(const float* part, int P, int nchunk, int i) {
  float g = 0.f;
  for (int c = 0; c < nchunk; c++) g += part[(size_t)c * P + i];
  return g;
}

// torch.optim.Adam's step t on entry i: fp64 on the fp32 gradient g, moments and parameter, each result rounded to fp32 once and written
// back; the rounded parameter is returned.  (The arrays with the index, and lr by reference - it may differ by lane, and is read where it
// is used, behind the pow()s -: in this shape both Adam kernels keep the registers they had with the text in place.)
__device__ __forceinline__ float learn_adam_entry(double g, const float& lr, double t, float beta1, float beta2, float eps, float* m_io, float* v_io, float* param_io, int i) {
  const double b1 = (double)beta1, b2 = (double)beta2;
  const double m = b1 * (double)m_io[i] + (1.0 - b1) * g;
  const double v = b2 * (double)v_io[i] + (1.0 - b2) * g * g;
  const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
  const double p = (double)param_io[i] - (double)lr / bc1 * m / (sqrt(v) / sqrt(bc2) + (double)eps);
  const float pf = (float)p;
  m_io[i] = (float)m; v_io[i] = (float)v; param_io[i] = pf;
  return pf;
}

}  // namespace hb
