// hb_gae.hip - the PPO buffer of hb_collect_gae_dev over the tapes of a collection: the critic over rows of observations (hb_value_kernel),
// the GAE(gamma, lambda) scan (hb_gae_scan_kernel) and the log-probabilities of the recorded draws (hb_log_prob_kernel).  A translation
// unit of its own: no other kernel compiles differently for it.
#include <hip/hip_runtime.h>
#include "hb_kcommon.hpp"
#include "hb_launch.hpp"

namespace hb {

// hb_actor_kernel's design (hb_actor.hip) on a row array [n_rows][nobs]: 16 rows per block, activations ping-pong between two LDS tiles,
// eight waves share the 16-column output tiles of a layer, each sweeping K four columns per v_mfma_f32_16x16x4_f32 (exact f32), B operand
// from the packed weights; a layer with fewer than eight tiles splits K across the idle waves and the partial tiles are summed in a fixed
// order.  The layer loop is hb_actor_kernel's: both include hb_mlp_layers.inl with the same hook (as text, not as a shared __device__
// function, which cost the actor three registers: profiles/gae_kernel_resources.txt, profiles/mlp_shared_loop.txt).
// What differs from the actor:
//  - term / trunc null: every row is evaluated (the obs tape).  Both given: row i is evaluated where trunc[i] && !term[i] - the rows
//    that are bootstrapped - and every other row is NOT READ (it holds stale or arbitrary data), loads as zeros and gets out[i] = 0; a
//    block with no selected row writes its zeros and returns;
//  - the last layer has one output column: one tile, split-K across the eight waves; out[i] is its pre-activation (the critic is linear
//    at the top).
// A row's value does not depend on the other rows of its tile nor on where in the tile it stands (every D[i][j] of an MFMA is its own
// chain over k), so V is the same bits however the rows are cut into batches.
#define HB_ACT_ANY 0
#include "hb_value_kernel.inl"
#undef HB_ACT_ANY
#define HB_ACT_ANY 1
#include "hb_value_kernel.inl"
#undef HB_ACT_ANY

hipError_t launch_value(const PolicyDesc& pd, const float* rows, const uint8_t* term, const uint8_t* trunc, long long n_rows, float* out, hipStream_t stream) {
  (void)hipGetLastError();
  if (n_rows < 1 || !rows || !out || (term == nullptr) != (trunc == nullptr) || pd.nl < 1 || pd.sizes[pd.nl] != 1) return hipErrorInvalidValue;
  const size_t shmem = ((size_t)32 * pd.ldx + 8 * 256) * sizeof(float);  // two activation tiles + the split-K partial tiles
  const long long nblk = (n_rows + 15) / 16;
  if (shmem > 64 * 1024 || nblk > 0x7fffffffLL) return hipErrorInvalidValue;
  if (pd.act == kActTanh) hipLaunchKernelGGL(hb_value_kernel, dim3((unsigned)nblk), dim3(512), shmem, stream, pd, rows, term, trunc, n_rows, out);
  else hipLaunchKernelGGL(hb_value_act_kernel, dim3((unsigned)nblk), dim3(512), shmem, stream, pd, rows, term, trunc, n_rows, out);
  return hipGetLastError();
}

// One lane per env, t = T-1 .. 0; every tape is [t][n_env], so the lanes of a wave read consecutive floats.  No cross-lane operation: env
// e's results are the same bits whatever n_env is and wherever e stands.  The arithmetic, with its fp32 roundings (tests/test_gpu_gae.py
// derives its bound from this count): r' = fma(gamma, tv, reward) [1]; q = fma(gamma nt, V[t+1], r') [1]; delta = q - V[t] [1];
// A = fma(gl nt, A, delta) [1], gl = gamma lam rounded once on the host [1]; returns = A + V[t] [1, not fed back].  nt is applied as a
// select (the coefficient is gamma or 0, gl or 0), not as a product; terminal values are read only where the env is bootstrapped.
__global__ __launch_bounds__(64) void hb_gae_scan_kernel(const GaeScan g) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= g.n_env) return;
  const size_t n = (size_t)g.n_env;
  float adv = 0.f;
  float vnext = g.value[(size_t)g.T * n + e];
  for (int t = g.T - 1; t >= 0; t--) {
    const size_t o = (size_t)t * n + e;
    const bool te = g.terminated[o] != 0, tr = g.truncated[o] != 0;
    const bool done = te || tr;
    const float v = g.value[o];
    float rp = g.reward[o];
    if (g.term_value && tr && !te) rp = __fmaf_rn(g.gamma, g.term_value[o], rp);
    const float q = __fmaf_rn(done ? 0.f : g.gamma, vnext, rp);
    const float delta = __fsub_rn(q, v);
    adv = __fmaf_rn(done ? 0.f : g.gl, adv, delta);
    if (g.advantage) g.advantage[o] = adv;
    if (g.returns) g.returns[o] = __fadd_rn(adv, v);
    vnext = v;
  }
}

hipError_t launch_gae_scan(const GaeScan& g, hipStream_t stream) {
  (void)hipGetLastError();
  if (g.n_env < 1 || g.T < 1 || !g.reward || !g.value || !g.terminated || !g.truncated || (!g.advantage && !g.returns)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hb_gae_scan_kernel, dim3((g.n_env + 63) / 64), dim3(64), 0, stream, g);
  return hipGetLastError();
}

// One lane per tape row (t, e): the sum over the actuators in index order, no cross-lane operation.  Per actuator (roundings in
// brackets): term = fma(-eps / 2, eps, -ls) [1] - log(2 pi) / 2 [1, the constant 1]; head 2: x = fma(exp(ls), eps, mean) [expf, 1],
// a = |x|, corr = 2 ((log 2 - a) [1, the constant 1] - log1p(exp(-2 a)) [expf, log1pf, 1]), term -= corr [1]; sum += term [1].
// log 2 - |x| - log1p(exp(-2 |x|)) is log 2 - x - softplus(-2 x) (even in x) without the overflow of exp(-2 x) at large negative x.
__global__ __launch_bounds__(256) void hb_log_prob_kernel(const LogProbDesc d, long long n_rows) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= n_rows) return;
  const size_t o = (size_t)row * d.nu;
  const float half_log_2pi = 0.91893853320467274178f, log2f_ = 0.69314718055994530942f;
  float sum = 0.f;
  for (int i = 0; i < d.nu; i++) {
    const float eps = d.eps[o + i];
    const float ls = d.head == kActorSquashed ? d.ls[o + i] : d.log_std[i];
    float term = __fsub_rn(__fmaf_rn(-0.5f * eps, eps, -ls), half_log_2pi);
    if (d.head == kActorSquashed) {
      const float a = fabsf(__fmaf_rn(expf(ls), eps, d.mean[o + i]));
      const float corr = 2.f * __fsub_rn(__fsub_rn(log2f_, a), log1pf(expf(-2.f * a)));
      term = __fsub_rn(term, corr);
    }
    sum = __fadd_rn(sum, term);
  }
  d.out[row] = sum;
}

hipError_t launch_log_prob(const LogProbDesc& d, long long n_rows, hipStream_t stream) {
  (void)hipGetLastError();
  if (n_rows < 1 || d.nu < 1 || d.nu > kActorMaxNu || !d.eps || !d.out || (d.head != kActorGaussian && d.head != kActorSquashed) ||
      (d.head == kActorSquashed && (!d.mean || !d.ls)))
    return hipErrorInvalidValue;
  const long long nblk = (n_rows + 255) / 256;
  if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hb_log_prob_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, d, n_rows);
  return hipGetLastError();
}

}  // namespace hb
