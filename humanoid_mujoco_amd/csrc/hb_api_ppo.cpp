// hb_api_ppo.cpp - the C-ABI of the PPO learner (include/hb.h: hb_learner_*, hb_ppo_*): the owner of the flat parameter record, its
// gradient and Adam moments, the packed transposes of the backward pass, and the launches of hb_ppo.hip.
#include "hb_batch.hpp"

namespace {

const DevMlp& net_of(const hb_batch* b, int k) { return k == 0 ? b->actor : b->critic; }

bool cfg_ok(const hb_ppo_config* c) {
  const float f[] = {c->clip_range, c->ent_coef, c->vf_coef, c->max_grad_norm, c->lr, c->beta1, c->beta2, c->eps};
  for (float x : f) if (!std::isfinite(x)) return false;
  return c->clip_range > 0.f && c->beta1 >= 0.f && c->beta1 < 1.f && c->beta2 >= 0.f && c->beta2 < 1.f && c->lr >= 0.f && c->eps > 0.f;
}

// the flat layout (include/hb.h): the actor's layers W | b, log_std, the critic's layers
void layout(hb_batch* b) {
  Learner& L = b->learner;
  int o = 0;
  for (int k = 0; k < 2; k++) {
    const DevMlp& n = net_of(b, k);
    for (int l = 0; l < n.layers; l++) {
      L.off_w[k][l] = o; o += n.sizes[l] * n.sizes[l + 1];
      L.off_b[k][l] = o; o += n.sizes[l + 1];
    }
    if (k == 0) { L.off_log_std = o; o += b->D.dm.nu; }
  }
  L.P = o;
}

// the flat record of what is installed: the networks' packed operands read back from the device, log_std from the actor's config
int read_installed(hb_batch* b, std::vector<float>& flat) {
  const Learner& L = b->learner;
  flat.assign(L.P, 0.f);
  for (int k = 0; k < 2; k++) {
    const DevMlp& n = net_of(b, k);
    for (int l = 0; l < n.layers; l++) {
      const int K = n.sizes[l], N = n.sizes[l + 1];
      std::vector<float> packed(n.wp[l].capacity());
      HB_HIP(hipMemcpy(packed.data(), n.wp[l], packed.size() * sizeof(float), hipMemcpyDeviceToHost));
      const std::vector<float> W = DevMlp::unpack_mfma_b(packed, K, N);
      memcpy(&flat[L.off_w[k][l]], W.data(), W.size() * sizeof(float));
      HB_HIP(hipMemcpy(&flat[L.off_b[k][l]], n.b[l], N * sizeof(float), hipMemcpyDeviceToHost));
    }
  }
  memcpy(&flat[L.off_log_std], b->actor_cfg.log_std, b->D.dm.nu * sizeof(float));
  return HB_OK;
}

// the flat record to the device: the master copy and every operand the kernels read (forward: only with `forward`; the packed
// transposes always), and the actor's log_std.  The stream is idle.
int write_params(hb_batch* b, const float* flat, bool forward) {
  Learner& L = b->learner;
  HB_HIP(hipMemcpy(L.d_param, flat, (size_t)L.P * sizeof(float), hipMemcpyHostToDevice));
  for (int k = 0; k < 2; k++) {
    const DevMlp& n = net_of(b, k);
    for (int l = 0; l < n.layers; l++) {
      const int K = n.sizes[l], N = n.sizes[l + 1];
      const float* W = flat + L.off_w[k][l];
      if (forward) {
        const std::vector<float> packed = DevMlp::pack_mfma_b(W, K, N);
        HB_HIP(hipMemcpy(n.wp[l], packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(n.b[l], flat + L.off_b[k][l], N * sizeof(float), hipMemcpyHostToDevice));
      }
      if (l > 0) {
        std::vector<float> Wt((size_t)N * K);
        for (int kk = 0; kk < K; kk++) for (int nn = 0; nn < N; nn++) Wt[(size_t)nn * K + kk] = W[(size_t)kk * N + nn];
        const std::vector<float> packed = DevMlp::pack_mfma_b(Wt.data(), N, K);
        if (L.d_wt[k][l].reserve(packed.size()) != HB_OK) return HB_ENOMEM;
        HB_HIP(hipMemcpy(L.d_wt[k][l], packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
      }
    }
  }
  memcpy(b->actor_cfg.log_std, flat + L.off_log_std, b->D.dm.nu * sizeof(float));
  L.log_std_dirty = false;
  return HB_OK;
}

int idle(hb_batch* b) {
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

int set_t(hb_batch* b, long long t) {
  const int zero = 0;
  HB_HIP(hipMemcpy(b->learner.d_nskip, &zero, sizeof zero, hipMemcpyHostToDevice));
  b->learner.calls = t;
  return HB_OK;
}

}  // namespace

namespace hb {

int learner_sync_log_std(hb_batch* b) {
  Learner& L = b->learner;
  if (!L.on || !L.log_std_dirty) return HB_OK;
  int rc = idle(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipMemcpy(b->actor_cfg.log_std, L.d_param + L.off_log_std, b->D.dm.nu * sizeof(float), hipMemcpyDeviceToHost));
  L.log_std_dirty = false;
  return HB_OK;
}

int learner_net_replaced(hb_batch* b, int net, bool shapes_same) {
  Learner& L = b->learner;
  if (!L.on) return HB_OK;
  int rc = idle(b);
  if (rc != HB_OK) return rc;
  // a new actor brings its own log_std; behind a new critic the actor keeps running the TRAINED one, whether or not the learner stays
  if (net == 0) L.log_std_dirty = false;
  else if ((rc = learner_sync_log_std(b)) != HB_OK) return rc;
  if (!shapes_same || b->actor_cfg.head != HB_ACTOR_GAUSSIAN) { L.clear(); return HB_OK; }
  std::vector<float> flat;
  if ((rc = read_installed(b, flat)) != HB_OK || (rc = write_params(b, flat.data(), false)) != HB_OK) { L.clear(); return rc; }
  // that network's moments start over: the actor's stretch of the record ends behind log_std, the critic's begins there
  const size_t cut = (size_t)L.off_log_std + b->D.dm.nu;
  const size_t lo = net == 0 ? 0 : cut, n = net == 0 ? cut : (size_t)L.P - cut;
  HB_HIP(hipMemset(L.d_m + lo, 0, n * sizeof(float)));
  HB_HIP(hipMemset(L.d_v + lo, 0, n * sizeof(float)));
  return HB_OK;
}

int learner_activation_changed(hb_batch* b) {
  Learner& L = b->learner;
  if (!L.on) return HB_OK;
  int rc = learner_sync_log_std(b);
  if (rc == HB_OK) rc = idle(b);
  if (rc != HB_OK) return rc;
  L.clear();
  return HB_OK;
}

}  // namespace hb

extern "C" {

int hb_ppo_default_config(hb_ppo_config* c) {
  if (!c) return HB_EINVAL;
  c->clip_range = 0.2f; c->ent_coef = 0.f; c->vf_coef = 0.5f; c->max_grad_norm = 0.5f; c->normalize_advantage = 1;
  c->lr = 3e-4f; c->beta1 = 0.9f; c->beta2 = 0.999f; c->eps = 1e-5f;
  return HB_OK;
}

int hb_ppo_row_chunk(int mb) { return mb < 1 ? 0 : ppo_row_chunk(mb); }

int hb_learner_create(hb_batch* b, const hb_ppo_config* cfg) {
  if (!b || !cfg || !cfg_ok(cfg) || b->actor.layers < 1 || b->critic.layers < 1) return HB_EINVAL;
  if (b->actor_cfg.head != HB_ACTOR_GAUSSIAN) return HB_EUNSUPPORTED;  // (the deterministic head has no density; the squashed head is SAC's)
  int rc = learner_sync_log_std(b);  // (a learner that is replaced: its trained log_std is the actor's, as its weights are)
  if (rc == HB_OK) rc = idle(b);
  if (rc != HB_OK) return rc;
  Learner& L = b->learner;
  L.clear();
  layout(b);
  const size_t P = L.P, nnorm = (P + kPpoNormChunk - 1) / kPpoNormChunk;
  rc = L.d_param.alloc(P);
  if (rc == HB_OK) rc = L.d_grad.alloc(P, true);
  if (rc == HB_OK) rc = L.d_m.alloc(P, true);
  if (rc == HB_OK) rc = L.d_v.alloc(P, true);
  if (rc == HB_OK) rc = L.d_zero.alloc(256, true);
  if (rc == HB_OK) rc = L.d_dbl.alloc(64 * 2 + 64 * 8 + nnorm, true);
  if (rc == HB_OK) rc = L.d_nskip.alloc(1, true);
  std::vector<float> flat;
  if (rc == HB_OK) rc = read_installed(b, flat);
  if (rc == HB_OK) rc = write_params(b, flat.data(), false);
  if (rc != HB_OK) { L.clear(); return rc; }
  L.cfg = *cfg;
  L.on = true;
  return HB_OK;
}

int hb_learner_configure(hb_batch* b, const hb_ppo_config* cfg) {
  if (!b || !cfg || !b->learner.on || !cfg_ok(cfg)) return HB_EINVAL;
  b->learner.cfg = *cfg;
  return HB_OK;
}

int hb_learner_destroy(hb_batch* b) {
  if (!b || !b->learner.on) return HB_EINVAL;
  int rc = learner_sync_log_std(b);  // (the actor keeps running the trained log_std)
  if (rc == HB_OK) rc = idle(b);
  if (rc != HB_OK) return rc;
  b->learner.clear();
  return HB_OK;
}

long long hb_learner_param_count(hb_batch* b) { return b && b->learner.on ? b->learner.P : HB_EINVAL; }

static int get_flat(hb_batch* b, const float* dev, float* out, long long count) {
  if (!b || !out || !b->learner.on || count != b->learner.P) return HB_EINVAL;
  const int rc = idle(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipMemcpy(out, dev, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
  return HB_OK;
}

int hb_learner_get_params(hb_batch* b, float* out, long long count) { return get_flat(b, b ? b->learner.d_param.get() : nullptr, out, count); }
int hb_learner_get_grads(hb_batch* b, float* out, long long count) { return get_flat(b, b ? b->learner.d_grad.get() : nullptr, out, count); }

int hb_learner_set_params(hb_batch* b, const float* in, long long count) {
  if (!b || !in || !b->learner.on || count != b->learner.P) return HB_EINVAL;
  const int rc = idle(b);
  if (rc != HB_OK) return rc;
  return write_params(b, in, true);
}

int hb_learner_get_state(hb_batch* b, float* params, float* m, float* v, long long count, long long* t) {
  if (!b || !params || !m || !v || !t || !b->learner.on || count != b->learner.P) return HB_EINVAL;
  Learner& L = b->learner;
  const int rc = idle(b);
  if (rc != HB_OK) return rc;
  int nskip = 0;
  HB_HIP(hipMemcpy(params, L.d_param, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
  HB_HIP(hipMemcpy(m, L.d_m, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
  HB_HIP(hipMemcpy(v, L.d_v, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
  HB_HIP(hipMemcpy(&nskip, L.d_nskip, sizeof nskip, hipMemcpyDeviceToHost));
  *t = L.calls - nskip;
  return HB_OK;
}

int hb_learner_set_state(hb_batch* b, const float* params, const float* m, const float* v, long long count, long long t) {
  if (!b || !params || !m || !v || !b->learner.on || count != b->learner.P || t < 0) return HB_EINVAL;
  Learner& L = b->learner;
  int rc = idle(b);
  if (rc != HB_OK) return rc;
  if ((rc = write_params(b, params, true)) != HB_OK) return rc;
  HB_HIP(hipMemcpy(L.d_m, m, (size_t)count * sizeof(float), hipMemcpyHostToDevice));
  HB_HIP(hipMemcpy(L.d_v, v, (size_t)count * sizeof(float), hipMemcpyHostToDevice));
  return set_t(b, t);
}

int hb_learner_grad_dev(hb_batch* b, float** ptr, long long* count) {
  if (!b || !ptr || !count || !b->learner.on) return HB_EINVAL;
  *ptr = b->learner.d_grad;
  *count = b->learner.P;
  return HB_OK;
}

int hb_ppo_grad_dev(hb_batch* b, const hb_ppo_rows* rows, float* stats_dev) {
  if (!b || !rows || !b->learner.on) return HB_EINVAL;
  if (!rows->obs || !rows->action || !rows->old_log_prob || !rows->advantage || !rows->returns) return HB_EINVAL;
  if (rows->mb < 1 || rows->n_rows < 1) return HB_EINVAL;
  if (!rows->index && (rows->first < 0 || rows->first + rows->mb > rows->n_rows)) return HB_EINVAL;
  Learner& L = b->learner;
  HB_HIP(hipSetDevice(b->device));
  hipStream_t st = main_stream(b);
  const size_t mb = rows->mb, nu = b->D.dm.nu, nobs = b->D.dm.nobs;
  auto r4 = [](size_t x) { return (x + 3) & ~(size_t)3; };
  const int chunk = ppo_row_chunk(rows->mb), nchunk = (rows->mb + chunk - 1) / chunk;
  // the scratch: act[0] | per network: act[1..], dz[0..], out | gls | srow
  size_t need = r4(mb * nobs) + r4(mb * nu) + r4(mb * 5);
  for (int k = 0; k < 2; k++) {
    const DevMlp& n = net_of(b, k);
    for (int l = 1; l <= n.layers; l++) need += 2 * r4(mb * n.sizes[l]);
  }
  if (need > L.d_scratch.capacity() || (size_t)nchunk * L.P > L.d_part.capacity()) {
    HB_HIP(hipStreamSynchronize(st));  // (a call still in flight uses the buffers that are replaced)
    if (L.d_scratch.reserve(need) != HB_OK || L.d_part.reserve((size_t)nchunk * L.P) != HB_OK) return HB_ENOMEM;
  }
  PpoDesc d;
  memset(&d, 0, sizeof d);
  float* p = L.d_scratch;
  float* act0 = p; p += r4(mb * nobs);
  for (int k = 0; k < 2; k++) {
    const DevMlp& n = net_of(b, k);
    PpoNet& w = d.net[k];
    const int nl = n.layers;
    w.fwd = n.desc();
    w.bwd.nl = nl - 1;
    w.bwd.ldx = w.fwd.ldx;
    for (int j = 0; j <= nl - 1; j++) w.bwd.sizes[j] = n.sizes[nl - j];
    for (int j = 0; j < nl - 1; j++) { w.bwd.w[j] = L.d_wt[k][nl - 1 - j]; w.bwd.b[j] = L.d_zero; }
    w.act[0] = act0;
    for (int l = 1; l < nl; l++) { w.act[l] = p; p += r4(mb * n.sizes[l]); }
    for (int l = 0; l < nl; l++) { w.dz[l] = p; p += r4(mb * n.sizes[l + 1]); }
    w.out = p; p += r4(mb * n.sizes[nl]);
    for (int l = 0; l < nl; l++) { w.off_w[l] = L.off_w[k][l]; w.off_b[l] = L.off_b[k][l]; }
  }
  d.gls = p; p += r4(mb * nu);
  d.srow = p;
  d.obs = rows->obs; d.action = rows->action; d.old_log_prob = rows->old_log_prob; d.advantage = rows->advantage; d.returns = rows->returns;
  d.index = rows->index; d.first = rows->first;
  d.mb = rows->mb; d.nobs = (int)nobs; d.nu = (int)nu; d.chunk = chunk; d.nchunk = nchunk; d.P = L.P; d.off_log_std = L.off_log_std;
  d.normalize = L.cfg.normalize_advantage != 0;
  d.clip_range = L.cfg.clip_range; d.ent_coef = L.cfg.ent_coef; d.vf_coef = L.cfg.vf_coef;
  d.param = L.d_param;
  d.advpart = L.d_dbl; d.statpart = L.d_dbl + 128;
  d.part = L.d_part; d.grad = L.d_grad; d.stats = stats_dev;
  HB_HIP(launch_ppo_grad(d, st));
  return HB_OK;
}

int hb_ppo_adam_dev(hb_batch* b, float* stats_dev) {
  if (!b || !b->learner.on) return HB_EINVAL;
  Learner& L = b->learner;
  HB_HIP(hipSetDevice(b->device));
  hipStream_t st = main_stream(b);
  PpoAdamDesc d;
  memset(&d, 0, sizeof d);
  for (int k = 0; k < 2; k++) {
    const DevMlp& n = net_of(b, k);
    for (int l = 0; l < n.layers; l++) {
      d.seg[d.nseg++] = PpoSeg{L.off_w[k][l], n.sizes[l], n.sizes[l + 1], n.wp[l].get(), l > 0 ? L.d_wt[k][l].get() : nullptr};
      d.seg[d.nseg++] = PpoSeg{L.off_b[k][l], 0, n.sizes[l + 1], n.b[l].get(), nullptr};
    }
    if (k == 0) d.seg[d.nseg++] = PpoSeg{L.off_log_std, 0, b->D.dm.nu, nullptr, nullptr};
  }
  d.P = L.P; d.nnorm = (L.P + kPpoNormChunk - 1) / kPpoNormChunk;
  d.param = L.d_param; d.m = L.d_m; d.v = L.d_v; d.grad = L.d_grad;
  d.normpart = L.d_dbl + 128 + 512; d.nskip = L.d_nskip;
  d.calls = L.calls + 1;
  d.lr = L.cfg.lr; d.beta1 = L.cfg.beta1; d.beta2 = L.cfg.beta2; d.eps = L.cfg.eps; d.max_grad_norm = L.cfg.max_grad_norm;
  d.stats = stats_dev;
  HB_HIP(launch_ppo_adam(d, st));
  L.calls++;
  L.log_std_dirty = true;
  return HB_OK;
}

int hb_ppo_minibatch_dev(hb_batch* b, const hb_ppo_rows* rows, float* stats_dev) {
  const int rc = hb_ppo_grad_dev(b, rows, stats_dev);
  return rc != HB_OK ? rc : hb_ppo_adam_dev(b, stats_dev);
}

}  // extern "C"
