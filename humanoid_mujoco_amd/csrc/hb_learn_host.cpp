// hb_learn_host.cpp - LearnerCore (hb_batch.hpp): what the PPO and the SAC learner do alike on the host with their flat record and the
// device operands that follow it.  The arithmetic that needs no device is hb_learn_host.hpp's.
#include "hb_batch.hpp"

namespace hb {

int learner_idle(hb_batch* b) {
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

LearnNet LearnerCore::view(const LearnNets& ns, int k, bool with_t) const {
  const DevMlp& n = *ns.net[k];
  LearnNet v;
  memset(&v, 0, sizeof v);
  v.layers = n.layers; v.ldx = n.desc().ldx; v.k0 = ns.k0[k];
  for (int l = 0; l <= n.layers; l++) v.sizes[l] = n.sizes[l];
  for (int l = 0; l < n.layers; l++) {
    v.off_w[l] = off_w[k][l]; v.off_b[l] = off_b[k][l];
    v.w[l] = n.wp[l]; v.b[l] = n.b[l];
    v.wt[l] = with_t && v.has_t(l) ? d_wt[k][l].get() : nullptr;
  }
  return v;
}

int LearnerCore::alloc_record(size_t ndbl) {
  int rc = d_param.alloc(P);
  if (rc == HB_OK) rc = d_grad.alloc(P, true);
  if (rc == HB_OK) rc = d_m.alloc(P, true);
  if (rc == HB_OK) rc = d_v.alloc(P, true);
  if (rc == HB_OK) rc = d_zero.alloc(256, true);
  if (rc == HB_OK) rc = d_dbl.alloc(ndbl, true);
  return rc;
}

int LearnerCore::read_installed(const LearnNets& ns, std::vector<float>& flat) const {
  flat.assign(P, 0.f);
  for (int k = 0; k < ns.n; k++) {
    const DevMlp& n = *ns.net[k];
    for (int l = 0; l < n.layers; l++) {
      const int K = n.sizes[l], N = n.sizes[l + 1];
      std::vector<float> packed(n.wp[l].capacity());
      HB_HIP(hipMemcpy(packed.data(), n.wp[l], packed.size() * sizeof(float), hipMemcpyDeviceToHost));
      const std::vector<float> W = DevMlp::unpack_mfma_b(packed, K, N);
      memcpy(&flat[off_w[k][l]], W.data(), W.size() * sizeof(float));
      HB_HIP(hipMemcpy(&flat[off_b[k][l]], n.b[l], N * sizeof(float), hipMemcpyDeviceToHost));
    }
  }
  return HB_OK;
}

int LearnerCore::write_params(const LearnNets& ns, const float* flat, bool forward) {
  HB_HIP(hipMemcpy(d_param, flat, (size_t)P * sizeof(float), hipMemcpyHostToDevice));
  for (int k = 0; k < ns.n; k++) {
    const DevMlp& n = *ns.net[k];
    const LearnNet v = view(ns, k);
    for (int l = 0; l < n.layers; l++) {
      const int K = n.sizes[l], N = n.sizes[l + 1];
      const float* W = flat + off_w[k][l];
      if (forward) {
        const std::vector<float> packed = DevMlp::pack_mfma_b(W, K, N);
        HB_HIP(hipMemcpy(n.wp[l], packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(n.b[l], flat + off_b[k][l], N * sizeof(float), hipMemcpyHostToDevice));
      }
      if (!v.has_t(l)) continue;
      // the packed transpose of rows k0 .. K - 1 of W[K][N]
      const int k0 = v.t0(l), Ka = K - k0;
      std::vector<float> Wt((size_t)N * Ka);
      for (int kk = 0; kk < Ka; kk++) for (int nn = 0; nn < N; nn++) Wt[(size_t)nn * Ka + kk] = W[(size_t)(k0 + kk) * N + nn];
      const std::vector<float> packed = DevMlp::pack_mfma_b(Wt.data(), N, Ka);
      if (d_wt[k][l].reserve(packed.size()) != HB_OK) return HB_ENOMEM;
      HB_HIP(hipMemcpy(d_wt[k][l], packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  return HB_OK;
}

int LearnerCore::reserve_scratch(size_t need, int nchunk, hipStream_t st) {
  if (need > d_scratch.capacity() || (size_t)nchunk * P > d_part.capacity()) {
    HB_HIP(hipStreamSynchronize(st));
    if (d_scratch.reserve(need) != HB_OK || d_part.reserve((size_t)nchunk * P) != HB_OK) return HB_ENOMEM;
  }
  return HB_OK;
}

int LearnerCore::download(hb_batch* b, const float* dev, float* out, long long count) const {
  if (!out || !on || count != P) return HB_EINVAL;
  const int rc = learner_idle(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipMemcpy(out, dev, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
  return HB_OK;
}

int LearnerCore::get_record(hb_batch* b, float* params, float* m, float* v) const {
  const int rc = learner_idle(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipMemcpy(params, d_param, (size_t)P * sizeof(float), hipMemcpyDeviceToHost));
  HB_HIP(hipMemcpy(m, d_m, (size_t)P * sizeof(float), hipMemcpyDeviceToHost));
  HB_HIP(hipMemcpy(v, d_v, (size_t)P * sizeof(float), hipMemcpyDeviceToHost));
  return HB_OK;
}

int LearnerCore::set_moments(const float* m, const float* v) {
  HB_HIP(hipMemcpy(d_m, m, (size_t)P * sizeof(float), hipMemcpyHostToDevice));
  HB_HIP(hipMemcpy(d_v, v, (size_t)P * sizeof(float), hipMemcpyHostToDevice));
  return HB_OK;
}

}  // namespace hb
