// hb_api_ppo.cpp - the C-ABI of the PPO learner (include/hb.h: hb_learner_*, hb_ppo_*): the owner of the flat parameter record, its
// gradient and Adam moments, the packed transposes of the backward pass, and the launches of hb_ppo.hip.
#include "hb_batch.hpp"

namespace {

// the networks of the flat record: the actor, the critic; layer 0 of either needs no transpose
LearnNets nets_of(const hb_batch* b) { return LearnNets{2, {&b->actor, &b->critic, nullptr}, {-1, -1, -1}}; }

bool cfg_ok(const hb_ppo_config* c) {
  const float f[] = {c->clip_range, c->ent_coef, c->vf_coef, c->max_grad_norm, c->lr, c->beta1, c->beta2, c->eps};
  for (float x : f) if (!std::isfinite(x)) return false;
  return c->clip_range > 0.f && c->beta1 >= 0.f && c->beta1 < 1.f && c->beta2 >= 0.f && c->beta2 < 1.f && c->lr >= 0.f && c->eps > 0.f;
}

// the flat layout (include/hb.h): the actor's layers W | b, log_std, the critic's layers
void layout(hb_batch* b) {
  Learner& L = b->learner;
  const LearnNets ns = nets_of(b);
  L.off_log_std = L.layout(ns, 0, 0);
  L.P = L.layout(ns, 1, L.off_log_std + b->D.dm.nu);
}

// the flat record of what is installed: the networks' operands, log_std from the actor's config
int read_installed(hb_batch* b, std::vector<float>& flat) {
  const int rc = b->learner.read_installed(nets_of(b), flat);
  if (rc != HB_OK) return rc;
  memcpy(&flat[b->learner.off_log_std], b->actor_cfg.log_std, b->D.dm.nu * sizeof(float));
  return HB_OK;
}

// the flat record to the device (LearnerCore::write_params), and the actor's log_std.  The stream is idle.
int write_params(hb_batch* b, const float* flat, bool forward) {
  Learner& L = b->learner;
  const int rc = L.write_params(nets_of(b), flat, forward);
  if (rc != HB_OK) return rc;
  memcpy(b->actor_cfg.log_std, flat + L.off_log_std, b->D.dm.nu * sizeof(float));
  L.log_std_dirty = false;
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
  int rc = learner_idle(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipMemcpy(b->actor_cfg.log_std, L.d_param + L.off_log_std, b->D.dm.nu * sizeof(float), hipMemcpyDeviceToHost));
  L.log_std_dirty = false;
  return HB_OK;
}

int learner_net_replaced(hb_batch* b, int net, bool shapes_same) {
  Learner& L = b->learner;
  if (!L.on) return HB_OK;
  int rc = learner_idle(b);
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
  if (rc == HB_OK) rc = learner_idle(b);
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
  if (rc == HB_OK) rc = learner_idle(b);
  if (rc != HB_OK) return rc;
  Learner& L = b->learner;
  L.clear();
  layout(b);
  const size_t nnorm = ((size_t)L.P + kPpoNormChunk - 1) / kPpoNormChunk;
  rc = L.alloc_record(64 * 2 + 64 * 8 + nnorm);
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
  if (rc == HB_OK) rc = learner_idle(b);
  if (rc != HB_OK) return rc;
  b->learner.clear();
  return HB_OK;
}

long long hb_learner_param_count(hb_batch* b) { return b && b->learner.on ? b->learner.P : HB_EINVAL; }

int hb_learner_get_params(hb_batch* b, float* out, long long count) { return b ? b->learner.download(b, b->learner.d_param, out, count) : HB_EINVAL; }
int hb_learner_get_grads(hb_batch* b, float* out, long long count) { return b ? b->learner.download(b, b->learner.d_grad, out, count) : HB_EINVAL; }

int hb_learner_set_params(hb_batch* b, const float* in, long long count) {
  if (!b || !in || !b->learner.on || count != b->learner.P) return HB_EINVAL;
  const int rc = learner_idle(b);
  if (rc != HB_OK) return rc;
  return write_params(b, in, true);
}

int hb_learner_get_state(hb_batch* b, float* params, float* m, float* v, long long count, long long* t) {
  if (!b || !params || !m || !v || !t || !b->learner.on || count != b->learner.P) return HB_EINVAL;
  Learner& L = b->learner;
  const int rc = L.get_record(b, params, m, v);
  if (rc != HB_OK) return rc;
  int nskip = 0;
  HB_HIP(hipMemcpy(&nskip, L.d_nskip, sizeof nskip, hipMemcpyDeviceToHost));
  *t = L.calls - nskip;
  return HB_OK;
}

int hb_learner_set_state(hb_batch* b, const float* params, const float* m, const float* v, long long count, long long t) {
  if (!b || !params || !m || !v || !b->learner.on || count != b->learner.P || t < 0) return HB_EINVAL;
  Learner& L = b->learner;
  int rc = learner_idle(b);
  if (rc != HB_OK) return rc;
  if ((rc = write_params(b, params, true)) != HB_OK || (rc = L.set_moments(m, v)) != HB_OK) return rc;
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
  const size_t mb = rows->mb, nu = b->D.dm.nu, nobs = b->row.width;
  const int chunk = ppo_row_chunk(rows->mb), nchunk = (rows->mb + chunk - 1) / chunk;
  const LearnNets ns = nets_of(b);
  PpoDesc d;
  memset(&d, 0, sizeof d);
  // the scratch: act[0] | per network: act[1..], dz[0..], out | gls | srow
  auto carve = [&](ScratchCarve c) {
    float* act0 = c.take(mb * nobs);
    for (int k = 0; k < 2; k++) {
      const DevMlp& n = *ns.net[k];
      PpoNet& w = d.net[k];
      w.act[0] = act0;
      for (int l = 1; l < n.layers; l++) w.act[l] = c.take(mb * n.sizes[l]);
      for (int l = 0; l < n.layers; l++) w.dz[l] = c.take(mb * n.sizes[l + 1]);
      w.out = c.take(mb * n.sizes[n.layers]);
    }
    d.gls = c.take(mb * nu);
    d.srow = c.take(mb * 5);
    return c.used;
  };
  const int rc = L.reserve_scratch(carve(ScratchCarve{}), nchunk, st);
  if (rc != HB_OK) return rc;
  carve(ScratchCarve{L.d_scratch, 0});
  for (int k = 0; k < 2; k++) {
    PpoNet& w = d.net[k];
    w.fwd = ns.net[k]->desc();
    w.bwd = learn_reversed(L.view(ns, k), 0, L.d_zero);
    for (int l = 0; l < w.fwd.nl; l++) { w.off_w[l] = L.off_w[k][l]; w.off_b[l] = L.off_b[k][l]; }
  }
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
  const LearnNets ns = nets_of(b);
  d.nseg = learn_segments(L.view(ns, 0), 0, d.seg);
  d.seg[d.nseg++] = ParamSeg{L.off_log_std, 0, b->D.dm.nu, 0, nullptr, nullptr};
  d.nseg += learn_segments(L.view(ns, 1), 0, d.seg + d.nseg);
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
