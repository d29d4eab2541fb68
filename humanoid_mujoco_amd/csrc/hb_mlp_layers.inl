// hb_mlp_layers.inl - the layer loop of the 16-row fused MLP kernels: hb_policy_kernel (hb_policy_kernels.inl), hb_actor_kernel
// (hb_actor_kernel.inl), hb_value_kernel (hb_value_kernel.inl) and the learners' forward and backward kernels (hb_ppo_mlp.inl,
// hb_sac_mlp.inl) include it in place, once each, inside the kernel body.  Text, not a function: as a __device__ function
// with an epilogue functor the same loop costs the policy kernel its 64th register step and a wave per SIMD
// (profiles/mlp_shared_loop.txt).  Its contract:
//  - in scope: pd (PolicyDesc), tid, lane, wave, ldx = pd.ldx, and the LDS pointers cur (the input tile [16][ldx], its three pad
//    columns behind sizes[0] zero), nxt (the other tile) and part (the split-K partial tiles [8][16][16]); all 512 threads arrive,
//    behind a __syncthreads() that covers the input tile;
//  - the hook HB_MLP_EMIT(row, n, v), which the kernel defines before the include and undefines behind it: called once per output
//    (row 0..15, column n < N) of every layer with the pre-activation v = sum + bias, with last (this is the last layer), N (the
//    layer's width) and nxt visible; on a layer that is not the last it has to store the activation - the network's own, pd.act - to nxt[row * ldx + n];
//  - behind it cur is the tile the last layer's hook wrote (where it wrote to nxt), and every thread is past the last barrier.
// Eight waves share the 16-column output tiles of a layer, each sweeping K four columns per v_mfma_f32_16x16x4_f32 (exact f32) with the
// A operand from LDS and the B operand from the packed weights (DevMlp, hb_batch.hpp); a layer with fewer than eight tiles splits K
// across the idle waves, and the partial tiles are summed in a fixed order (deterministic, no atomics).
const int col = lane & 15, quad = lane >> 4;  // A: row = col, k offset = quad;  B: k offset = quad, column = col;  D: rows 4 quad + r, column col
for (int l = 0; l < pd.nl; l++) {
  const int K = pd.sizes[l], N = pd.sizes[l + 1], KK = (K + 3) / 4, ntile = (N + 15) / 16;
  const bool last = l + 1 == pd.nl;
  int S = 1;  // K slices per tile
  while (S * 2 * ntile <= 8) S *= 2;
  const float* wp = pd.w[l];
  const float* bias = pd.b[l];
  if (!last && tid < 48) nxt[(tid / 3) * ldx + N + tid % 3] = 0.f;  // pad columns of the next layer's input
  for (int it = wave; it < ntile * S; it += 8) {
    const int nt = it / S, sl = it - nt * S;
    const int kb = KK * sl / S, ke = KK * (sl + 1) / S;
    f32x4 D = {0.f, 0.f, 0.f, 0.f};
    const float* ap = cur + col * ldx + quad;
    const float* bp = wp + (size_t)nt * KK * 64 + lane;
    int kk = kb;
    for (; kk + 8 <= ke; kk += 8) {  // eight operand pairs in flight per batch of MFMAs
      float a[8], w[8];
#pragma unroll
      for (int u = 0; u < 8; u++) { a[u] = ap[4 * (kk + u)]; w[u] = bp[(size_t)(kk + u) * 64]; }
#pragma unroll
      for (int u = 0; u < 8; u++) D = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u], D, 0, 0, 0);
    }
    for (; kk < ke; kk++) D = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[4 * kk], bp[(size_t)kk * 64], D, 0, 0, 0);
    const int n = nt * 16 + col;
    if (S == 1) {
      if (n < N) {
        const float bn = bias[n];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const float v = D[r] + bn;
          HB_MLP_EMIT(4 * quad + r, n, v);
        }
      }
    } else {
      float* pp = part + it * 256;
#pragma unroll
      for (int r = 0; r < 4; r++) pp[(4 * quad + r) * 16 + col] = D[r];
    }
  }
  __syncthreads();
  if (S > 1) {
    for (int idx = tid; idx < ntile * 256; idx += 512) {
      const int nt = idx >> 8, rc = idx & 255, row = rc >> 4, n = nt * 16 + (rc & 15);
      if (n < N) {
        float v = bias[n];
        for (int sl = 0; sl < S; sl++) v += part[(nt * S + sl) * 256 + rc];
        HB_MLP_EMIT(row, n, v);
      }
    }
    __syncthreads();
  }
  float* t = cur; cur = nxt; nxt = t;
}
