// hb_api_collect.cpp — the C-ABI of libhb.so (include/hb.h), collecting rollouts through the env adapter: the sampling actor with its
// collection loop, the critic with the PPO buffer over the tapes (values, log-probabilities, GAE), the hidden activation of an installed
// network, and the running observation / reward normaliser with its episode statistics.  The actor and the critic are each a DevMlp
// (hb_batch.hpp): one owner packs, uploads and describes an installed network, and one check (mlp_args_ok) covers the arrays of the
// hb_*_set_mlp entry points; their kernels share one layer loop (hb_mlp_layers.inl).
#include "hb_batch.hpp"

extern "C" {

// ---- actor and rollout collection

// the sizes of an installed network are those of the arguments (a learner on the batch keeps its state then: learner_net_replaced)
static bool mlp_same_shape(const DevMlp& n, int n_layers, const int* sizes) {
  if (n.layers != n_layers) return false;
  for (int l = 0; l <= n_layers; l++) if (n.sizes[l] != sizes[l]) return false;
  return true;
}

int hb_actor_set_mlp(hb_batch* b, int n_layers, const int* sizes, const float* const* weights, const float* const* biases, const hb_actor_config* cfg) {
  if (!b || !cfg || !mlp_args_ok(n_layers, sizes, weights, biases)) return HB_EINVAL;
  const int nu = b->D.dm.nu;
  if (cfg->head != HB_ACTOR_DETERMINISTIC && cfg->head != HB_ACTOR_GAUSSIAN && cfg->head != HB_ACTOR_SQUASHED) return HB_EINVAL;
  if (nu < 1 || nu > kActorMaxNu) return HB_EINVAL;
  if (sizes[0] != b->row.width || sizes[n_layers] != (cfg->head == HB_ACTOR_SQUASHED ? 2 * nu : nu)) return HB_EINVAL;
  if (cfg->head == HB_ACTOR_GAUSSIAN) for (int i = 0; i < nu; i++) if (!std::isfinite(cfg->log_std[i])) return HB_EINVAL;
  for (int l = 0; l <= n_layers; l++) if (sizes[l] > 256) return HB_EUNSUPPORTED;  // (the fused kernel's LDS tiles; no layer-by-layer fallback)
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));  // (a collection still in flight reads the buffers that are replaced below)
  // (every argument check is behind us: from here on only the device can fail, and then no actor is installed)
  const bool same = mlp_same_shape(b->actor, n_layers, sizes);
  b->sac.clear();  // (a SAC learner does not outlive the actor it trained: hb_sac_create again)
  if ((rc = b->actor.install(n_layers, sizes, weights, biases)) != HB_OK) { b->learner.clear(); return rc; }
  b->actor_cfg = *cfg;
  b->actor_draw0 = 0;
  return learner_net_replaced(b, 0, same);
}

static int norm_step_impl(hb_batch* b, const hb_norm_io& io);

// the loop of hb_env_collect_dev; norm: one normaliser step behind every env step (hb_env_collect_norm_dev), aux: its tapes or null
static int collect_impl(hb_batch* b, int T, int n_substeps, const hb_collect_out* out, bool norm, const hb_norm_tapes* aux) {
  if (!b || T < 1 || n_substeps < 1 || !out || !out->obs || !out->action || b->actor.layers < 1) return HB_EINVAL;
  if (out->log_std && b->actor_cfg.head != HB_ACTOR_SQUASHED) return HB_EINVAL;
  if (norm && !b->norm_on) return HB_EINVAL;
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipSetDevice(b->device));
  const DevModel& dm = b->D.dm;
  const size_t n = b->n_env, nu = dm.nu, nobs = b->row.width;
  if (out->terminal_obs && !b->d_term_obs && (rc = hb_env_terminal_obs(b, nullptr)) != HB_OK) return rc;
  if ((rc = learner_sync_log_std(b)) != HB_OK) return rc;  // (a learner's Adam steps moved log_std on the device: hb_ppo_adam_dev)
  ActorDesc ad;
  memset(&ad, 0, sizeof ad);
  ad.net = b->actor.desc();
  ad.head = b->actor_cfg.head; ad.deterministic = b->actor_cfg.deterministic != 0; ad.nu = dm.nu; ad.seed = b->actor_cfg.seed;
  memcpy(ad.log_std, b->actor_cfg.log_std, sizeof ad.log_std);
  for (int t = 0; t < T; t++) {
    const size_t row = (size_t)t * n;
    ActorTapes tp;
    tp.action = out->action + row * nu;
    tp.mean = out->mean ? out->mean + row * nu : nullptr;
    tp.log_std = out->log_std ? out->log_std + row * nu : nullptr;
    tp.eps = out->eps ? out->eps + row * nu : nullptr;
    HB_HIP(launch_actor(ad, out->obs + row * nobs, tp, b->n_env, (unsigned)b->env_offset, b->actor_draw0, main_stream(b)));
    b->actor_draw0++;
    // (outputs of the step that have no tape land in the batch's own record, hb_env_step's device buffers; with the normaliser the raw
    // observations and rewards go to their aux tapes where those are given, else to the main tapes, which are then normalised in place)
    float* obs_next = out->obs + (row + n) * nobs;
    float* raw_obs = norm && aux && aux->raw_obs ? aux->raw_obs + row * nobs : obs_next;
    float* reward = out->reward ? out->reward + row : nullptr;
    float* raw_reward = norm && aux && aux->raw_reward ? aux->raw_reward + row : (reward ? reward : b->d_reward);
    uint8_t* term = out->terminated ? out->terminated + row : b->d_term;
    uint8_t* trunc = out->truncated ? out->truncated + row : b->d_trunc;
    rc = env_step_impl(b, tp.action, n_substeps, nullptr, true, raw_obs, raw_reward, term, trunc);
    if (rc != HB_OK) return rc;
    if (out->terminal_obs)
      HB_HIP(hipMemcpyAsync(out->terminal_obs + row * nobs, b->d_term_obs, n * nobs * sizeof(float), hipMemcpyDeviceToDevice, main_stream(b)));
    if (norm) {
      hb_norm_io io;
      memset(&io, 0, sizeof io);
      io.obs_in = raw_obs; io.obs_out = obs_next; io.reward_in = raw_reward; io.reward_out = reward; io.terminated = term; io.truncated = trunc;
      if (out->terminal_obs) io.terminal_obs_in = io.terminal_obs_out = out->terminal_obs + row * nobs;
      io.ep_return_out = aux && aux->ep_return ? aux->ep_return + row : nullptr;
      io.ep_length_out = aux && aux->ep_length ? aux->ep_length + row : nullptr;
      if ((rc = norm_step_impl(b, io)) != HB_OK) return rc;
    }
  }
  return HB_OK;
}

int hb_env_collect_dev(hb_batch* b, int T, int n_substeps, const hb_collect_out* out) { return collect_impl(b, T, n_substeps, out, false, nullptr); }

// ---- critic and the PPO buffer over a collection's tapes

int hb_critic_set_mlp(hb_batch* b, int n_layers, const int* sizes, const float* const* weights, const float* const* biases) {
  if (!b || !mlp_args_ok(n_layers, sizes, weights, biases)) return HB_EINVAL;
  if (sizes[0] != b->row.width || sizes[n_layers] != 1) return HB_EINVAL;
  for (int l = 0; l <= n_layers; l++) if (sizes[l] > 256) return HB_EUNSUPPORTED;  // (the fused kernel's LDS tiles; no layer-by-layer fallback)
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));  // (a call still in flight reads the buffers that are replaced below)
  // (every argument check is behind us: from here on only the device can fail, and then no critic is installed)
  const bool same = mlp_same_shape(b->critic, n_layers, sizes);
  int rc = learner_sync_log_std(b);  // (whatever becomes of a learner below, the actor keeps the log_std it trained)
  if (rc != HB_OK) return rc;
  rc = b->critic.install(n_layers, sizes, weights, biases);
  if (rc != HB_OK) { b->learner.clear(); return rc; }
  return learner_net_replaced(b, 1, same);
}

// ---- the hidden activation of an installed network

static DevMlp* mlp_of(hb_batch* b, int net) {
  switch (net) {
    case HB_NET_POLICY: return &b->policy;
    case HB_NET_ACTOR: return &b->actor;
    case HB_NET_CRITIC: return &b->critic;
    case HB_NET_Q1: return &b->q[0];
    case HB_NET_Q2: return &b->q[1];
    default: return nullptr;
  }
}

int hb_mlp_get_activation(hb_batch* b, int net) {
  const DevMlp* n = b ? mlp_of(b, net) : nullptr;
  return n && n->layers >= 1 ? n->act : HB_EINVAL;
}

int hb_mlp_set_activation(hb_batch* b, int net, int activation) {
  DevMlp* n = b ? mlp_of(b, net) : nullptr;
  if (!n || n->layers < 1) return HB_EINVAL;
  if (activation != HB_ACT_TANH && activation != HB_ACT_RELU && activation != HB_ACT_ELU) return HB_EINVAL;
  if (n->act == activation) return HB_OK;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));  // (a learner step still in flight uses the buffers that are released below)
  // a learner does not outlive the network it trained, as behind the network's set_mlp; the actor's draw counter goes on
  if (net == HB_NET_ACTOR || net == HB_NET_CRITIC) {
    const int rc = learner_activation_changed(b);
    if (rc != HB_OK) return rc;
  }
  if (net == HB_NET_ACTOR || net == HB_NET_Q1 || net == HB_NET_Q2) b->sac.clear();
  n->act = activation;
  return HB_OK;
}

int hb_collect_gae_dev(hb_batch* b, int T, const hb_collect_out* tapes, const hb_gae_config* cfg, const hb_gae_out* out) {
  if (!b || !tapes || !cfg || !out || T < 1) return HB_EINVAL;
  if (!out->value && !out->terminal_value && !out->log_prob && !out->advantage && !out->returns) return HB_EINVAL;
  if (!std::isfinite(cfg->gamma) || !std::isfinite(cfg->lam) || cfg->gamma < 0.f || cfg->gamma > 1.f || cfg->lam < 0.f || cfg->lam > 1.f) return HB_EINVAL;
  const bool boot = cfg->bootstrap_truncated != 0, scan = out->advantage || out->returns;
  const bool want_value = out->value || scan, want_tv = out->terminal_value || (scan && boot);
  if ((want_value || want_tv) && b->critic.layers < 1) return HB_EINVAL;
  if (want_value && !tapes->obs) return HB_EINVAL;
  if (scan && (!tapes->reward || !tapes->terminated || !tapes->truncated)) return HB_EINVAL;
  if (want_tv && (!tapes->terminal_obs || !tapes->terminated || !tapes->truncated)) return HB_EINVAL;
  const int head = b->actor_cfg.head;
  if (out->log_prob) {
    if (b->actor.layers < 1 || head == HB_ACTOR_DETERMINISTIC || !tapes->eps) return HB_EINVAL;
    if (head == HB_ACTOR_SQUASHED && (!tapes->mean || !tapes->log_std)) return HB_EINVAL;
  }
  HB_HIP(hipSetDevice(b->device));
  const size_t n = b->n_env;
  const long long rows = (long long)T * b->n_env;
  // value and terminal-value tapes the caller did not ask for but the scan needs: the batch's scratch
  float* value = out->value;
  float* tv = out->terminal_value;
  const size_t need = (want_value && !value ? (size_t)(T + 1) * n : 0) + (want_tv && !tv ? (size_t)T * n : 0);
  if (need) {
    if (need > b->d_gae.capacity()) HB_HIP(hipStreamSynchronize(main_stream(b)));  // (a call still in flight writes the buffer that is replaced)
    const int rc = b->d_gae.reserve(need);
    if (rc != HB_OK) return rc;
    float* p = b->d_gae;
    if (want_value && !value) { value = p; p += (size_t)(T + 1) * n; }
    if (want_tv && !tv) tv = p;
  }
  hipStream_t st = main_stream(b);
  const PolicyDesc pd = b->critic.desc();  // (read only where there is a critic: checked above)
  if (want_value) HB_HIP(launch_value(pd, tapes->obs, nullptr, nullptr, rows + b->n_env, value, st));
  if (want_tv) {
    if (boot) HB_HIP(launch_value(pd, tapes->terminal_obs, tapes->terminated, tapes->truncated, rows, tv, st));
    else HB_HIP(hipMemsetAsync(tv, 0, (size_t)rows * sizeof(float), st));  // (only as an output: the scan does not read it then)
  }
  if (scan) {
    GaeScan g;
    memset(&g, 0, sizeof g);
    g.reward = tapes->reward; g.value = value; g.term_value = boot ? tv : nullptr;
    g.terminated = tapes->terminated; g.truncated = tapes->truncated;
    g.advantage = out->advantage; g.returns = out->returns;
    g.gamma = cfg->gamma; g.gl = (float)((double)cfg->gamma * (double)cfg->lam);
    g.T = T; g.n_env = b->n_env;
    HB_HIP(launch_gae_scan(g, st));
  }
  if (out->log_prob) {
    const int rc = learner_sync_log_std(b);  // (as in the collection)
    if (rc != HB_OK) return rc;
    LogProbDesc d;
    memset(&d, 0, sizeof d);
    d.head = head; d.nu = b->D.dm.nu;
    memcpy(d.log_std, b->actor_cfg.log_std, sizeof d.log_std);
    d.eps = tapes->eps; d.mean = tapes->mean; d.ls = tapes->log_std; d.out = out->log_prob;
    HB_HIP(launch_log_prob(d, rows, st));
  }
  return HB_OK;
}

// ---- running observation / reward normalisation and episode statistics (hb_norm.hip)

int hb_norm_default_config(hb_norm_config* c) {
  if (!c) return HB_EINVAL;
  c->norm_obs = c->norm_reward = c->training = 1;
  c->clip_obs = c->clip_reward = 10.f; c->gamma = 0.99f; c->epsilon = 1e-8f;
  return HB_OK;
}

int hb_norm_configure(hb_batch* b, const hb_norm_config* cfg) {
  if (!b) return HB_EINVAL;
  if (cfg && (!std::isfinite(cfg->clip_obs) || !(cfg->clip_obs > 0.f) || !std::isfinite(cfg->clip_reward) || !(cfg->clip_reward > 0.f) ||
              !std::isfinite(cfg->epsilon) || !(cfg->epsilon > 0.f) || !std::isfinite(cfg->gamma) || cfg->gamma < 0.f || cfg->gamma > 1.f))
    return HB_EINVAL;
  const int nobs = b->row.width;
  if (cfg && (nobs < 1 || nobs > kNormMaxObs)) return HB_EUNSUPPORTED;
  HB_HIP(hipSetDevice(b->device));
  if (!cfg) {
    HB_HIP(hipStreamSynchronize(main_stream(b)));  // (a step still in flight uses the buffers that are released)
    reset_all(b->d_norm_rec, b->d_norm_env, b->d_norm_part, b->d_norm_len);
    b->norm_on = false;
    return HB_OK;
  }
  if (!b->norm_on) {
    const size_t n = b->n_env, R = norm_rec_doubles(nobs), nchunk = (n + kNormChunk - 1) / kNormChunk;
    int rc = b->d_norm_rec.alloc(2 * R);
    if (rc == HB_OK) rc = b->d_norm_env.alloc(2 * n, /*zero=*/true);
    if (rc == HB_OK) rc = b->d_norm_len.alloc(n, /*zero=*/true);
    if (rc == HB_OK) rc = b->d_norm_part.reserve(nchunk * norm_part_doubles(nobs));
    std::vector<double> rec(2 * R, 0.0);
    for (int c = 0; c < nobs; c++) rec[nobs + c] = 1.0;
    rec[2 * nobs] = 1e-4; rec[2 * nobs + 2] = 1.0; rec[2 * nobs + 3] = 1e-4;
    if (rc == HB_OK && hipMemcpy(b->d_norm_rec, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = HB_ENODEVICE;
    if (rc != HB_OK) { reset_all(b->d_norm_rec, b->d_norm_env, b->d_norm_part, b->d_norm_len); return rc; }
    b->norm_k = 0;
    b->norm_on = true;
  }
  b->norm_cfg = *cfg;
  return HB_OK;
}

int hb_norm_get_stats(hb_batch* b, double* out) {
  if (!b || !out || !b->norm_on) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  const int nobs = b->row.width;
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  HB_HIP(hipMemcpy(out, b->d_norm_rec + (size_t)b->norm_k * norm_rec_doubles(nobs), (size_t)(2 * nobs + 4) * sizeof(double), hipMemcpyDeviceToHost));
  return HB_OK;
}

int hb_norm_set_stats(hb_batch* b, const double* in) {
  if (!b || !in || !b->norm_on) return HB_EINVAL;
  const int nobs = b->row.width;
  for (int i = 0; i < 2 * nobs + 4; i++) if (!std::isfinite(in[i])) return HB_EINVAL;
  for (int c = 0; c < nobs; c++) if (in[nobs + c] < 0.0) return HB_EINVAL;
  if (in[2 * nobs] < 0.0 || in[2 * nobs + 2] < 0.0 || in[2 * nobs + 3] < 0.0) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  HB_HIP(hipMemcpy(b->d_norm_rec + (size_t)b->norm_k * norm_rec_doubles(nobs), in, (size_t)(2 * nobs + 4) * sizeof(double), hipMemcpyHostToDevice));
  return HB_OK;
}

int hb_norm_get_env(hb_batch* b, double* disc_return, double* ep_return, int32_t* ep_length) {
  if (!b || !b->norm_on) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  const size_t n = b->n_env;
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  if (disc_return) HB_HIP(hipMemcpy(disc_return, b->d_norm_env, n * sizeof(double), hipMemcpyDeviceToHost));
  if (ep_return) HB_HIP(hipMemcpy(ep_return, b->d_norm_env + n, n * sizeof(double), hipMemcpyDeviceToHost));
  if (ep_length) HB_HIP(hipMemcpy(ep_length, b->d_norm_len, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return HB_OK;
}

int hb_norm_episode_totals(hb_batch* b, double out[4]) {
  if (!b || !out || !b->norm_on) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  const int nobs = b->row.width;
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  HB_HIP(hipMemcpy(out, b->d_norm_rec + (size_t)b->norm_k * norm_rec_doubles(nobs) + 2 * nobs + 4, 4 * sizeof(double), hipMemcpyDeviceToHost));
  return HB_OK;
}

// the fields every launch of the normaliser shares
static NormDesc norm_desc(hb_batch* b) {
  const hb_norm_config& c = b->norm_cfg;
  NormDesc d;
  memset(&d, 0, sizeof d);
  d.nobs = b->row.width;
  d.norm_obs = c.norm_obs != 0; d.norm_reward = c.norm_reward != 0;
  d.k = b->norm_k;
  d.clip_obs = c.clip_obs; d.clip_reward = c.clip_reward; d.gamma = (double)c.gamma; d.epsilon = (double)c.epsilon;
  d.rec = b->d_norm_rec; d.part = b->d_norm_part;
  d.ret = b->d_norm_env; d.ep_ret = b->d_norm_env + b->n_env; d.ep_len = b->d_norm_len;
  return d;
}

// a step (io.reward_in given) or a reset over the batch's n_env rows: the moments launch, the apply launch, and the slot flips
static int norm_step_impl(hb_batch* b, const hb_norm_io& io) {
  const hb_norm_config& c = b->norm_cfg;
  NormDesc d = norm_desc(b);
  d.n_rows = b->n_env; d.nchunk = (b->n_env + kNormChunk - 1) / kNormChunk;
  d.reset = io.reward_in == nullptr;
  d.upd_obs = c.training && c.norm_obs; d.upd_ret = c.training && !d.reset;
  d.store = 1;
  d.obs_in = io.obs_in; d.obs_out = io.obs_out; d.reward_in = io.reward_in; d.reward_out = io.reward_out;
  d.term = io.terminated; d.trunc = io.truncated; d.tobs_in = io.terminal_obs_in; d.tobs_out = io.terminal_obs_out;
  d.ep_return_out = io.ep_return_out; d.ep_length_out = io.ep_length_out;
  hipStream_t st = main_stream(b);
  HB_HIP(launch_norm_moments(d, st));
  HB_HIP(launch_norm_apply(d, st));
  b->norm_k ^= 1;
  return HB_OK;
}

int hb_norm_step_dev(hb_batch* b, const hb_norm_io* io) {
  if (!b || !io || !b->norm_on || !io->obs_in || !io->obs_out || !io->reward_in || !io->terminated || !io->truncated) return HB_EINVAL;
  if ((io->terminal_obs_in == nullptr) != (io->terminal_obs_out == nullptr)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  return norm_step_impl(b, *io);
}

int hb_norm_reset_dev(hb_batch* b, const float* obs_in, float* obs_out) {
  if (!b || !b->norm_on || !obs_in || !obs_out) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  hb_norm_io io;
  memset(&io, 0, sizeof io);
  io.obs_in = obs_in; io.obs_out = obs_out;
  return norm_step_impl(b, io);
}

int hb_norm_obs_dev(hb_batch* b, const float* in, float* out, long long n_rows) {
  if (!b || !b->norm_on || !in || !out || n_rows < 1) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  NormDesc d = norm_desc(b);
  d.n_rows = n_rows;
  d.obs_in = in; d.obs_out = out;
  HB_HIP(launch_norm_apply(d, main_stream(b)));
  return HB_OK;
}

int hb_env_collect_norm_dev(hb_batch* b, int T, int n_substeps, const hb_collect_out* out, const hb_norm_tapes* aux) {
  return collect_impl(b, T, n_substeps, out, true, aux);
}

}  // extern "C"
