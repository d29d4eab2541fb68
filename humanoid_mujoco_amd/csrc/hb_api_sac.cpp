// hb_api_sac.cpp - the C-ABI of the SAC learner (include/hb.h: hb_q_*, hb_sac_*): the owner of the flat parameter record, its gradient
// and Adam moments, the targets, the packed transposes of the backward pass, and the sixteen launches of hb_sac.hip.
#include "hb_batch.hpp"

namespace {

// the networks of the flat record: the actor, Q1, Q2; layer 0 of a Q network has the transpose of its action rows (dQ / da)
LearnNets nets_of(const hb_batch* b) {
  const int nobs = b->row.width;
  return LearnNets{3, {&b->actor, &b->q[0], &b->q[1]}, {-1, nobs, nobs}};
}
// the same with the targets in the Q networks' places (their tensors stand where their Q network's do)
LearnNets target_nets_of(hb_batch* b) {
  LearnNets ns = nets_of(b);
  ns.net[1] = &b->sac.tq[0]; ns.net[2] = &b->sac.tq[1];
  return ns;
}

bool cfg_ok(const hb_sac_config* c) {
  const float f[] = {c->gamma, c->tau, c->lr_actor, c->lr_critic, c->lr_ent, c->beta1, c->beta2, c->eps, c->ent_coef_init, c->target_entropy};
  for (float x : f) if (!std::isfinite(x)) return false;
  return c->gamma >= 0.f && c->gamma <= 1.f && c->tau >= 0.f && c->tau <= 1.f && c->lr_actor >= 0.f && c->lr_critic >= 0.f && c->lr_ent >= 0.f &&
         c->beta1 >= 0.f && c->beta1 < 1.f && c->beta2 >= 0.f && c->beta2 < 1.f && c->eps > 0.f && c->ent_coef_init > 0.f && c->target_update_interval >= 1;
}

// the flat layout (include/hb.h): the actor's layers W | b, Q1's, Q2's, log_ent_coef
void layout(hb_batch* b) {
  SacLearner& L = b->sac;
  const LearnNets ns = nets_of(b);
  L.off_q = L.layout(ns, 0, 0);
  const int end = L.layout(ns, 2, L.layout(ns, 1, L.off_q));
  L.PT = end - L.off_q;
  L.P = end + 1;
}

// the targets' record to the device, and the operands of their forward pass
int write_targets(hb_batch* b, const float* rec) {
  SacLearner& L = b->sac;
  HB_HIP(hipMemcpy(L.d_target, rec, (size_t)L.PT * sizeof(float), hipMemcpyHostToDevice));
  for (int k = 0; k < 2; k++) {
    const DevMlp& n = b->q[k];
    const float *w[4], *bias[4];
    for (int l = 0; l < n.layers; l++) { w[l] = rec + (L.off_w[k + 1][l] - L.off_q); bias[l] = rec + (L.off_b[k + 1][l] - L.off_q); }
    const int rc = L.tq[k].install(n.layers, n.sizes, w, bias);
    if (rc != HB_OK) return rc;
    L.tq[k].act = n.act;  // (a target runs its Q network's activation; a change of that one destroys the learner)
  }
  return HB_OK;
}

float target_entropy(const hb_batch* b) { return b->sac.cfg.target_entropy_auto ? -(float)b->D.dm.nu : b->sac.cfg.target_entropy; }

}  // namespace

extern "C" {

int hb_q_set_mlp(hb_batch* b, int k, int n_layers, const int* sizes, const float* const* weights, const float* const* biases) {
  if (!b || k < 0 || k > 1 || !mlp_args_ok(n_layers, sizes, weights, biases)) return HB_EINVAL;
  if (sizes[0] != b->row.width + b->D.dm.nu || sizes[n_layers] != 1) return HB_EINVAL;
  for (int l = 0; l <= n_layers; l++) if (sizes[l] > 256) return HB_EUNSUPPORTED;  // (the fused kernel's LDS tiles; no layer-by-layer fallback)
  const int rc = learner_idle(b);  // (a call still in flight reads the buffers that are replaced below)
  if (rc != HB_OK) return rc;
  b->sac.clear();
  return b->q[k].install(n_layers, sizes, weights, biases);
}

int hb_q_values_dev(hb_batch* b, const float* obs, const float* action, long long n_rows, float* q1_out, float* q2_out) {
  if (!b || !obs || !action || (!q1_out && !q2_out) || n_rows < 1 || n_rows > 0x7fffffffLL) return HB_EINVAL;
  if ((q1_out && b->q[0].layers < 1) || (q2_out && b->q[1].layers < 1)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  hipStream_t st = main_stream(b);
  SacFwdDesc d;
  memset(&d, 0, sizeof d);
  d.mb = (int)n_rows;
  int nj = 0;
  float* outs[2] = {q1_out, q2_out};
  for (int k = 0; k < 2; k++) {
    if (!outs[k]) continue;
    SacFwdJob& j = d.job[nj++];
    j.net = b->q[k].desc();
    j.x0 = obs; j.n0 = b->row.width; j.x1 = action; j.n1 = b->D.dm.nu;
    j.out = outs[k];
  }
  HB_HIP(launch_sac_forward(d, nj, st));
  return HB_OK;
}

int hb_sac_default_config(hb_sac_config* c) {
  if (!c) return HB_EINVAL;
  memset(c, 0, sizeof *c);
  c->gamma = 0.99f; c->tau = 0.005f; c->lr_actor = c->lr_critic = c->lr_ent = 3e-4f; c->beta1 = 0.9f; c->beta2 = 0.999f; c->eps = 1e-8f;
  c->ent_coef_init = 1.f; c->auto_ent = 1; c->target_entropy_auto = 1; c->target_entropy = 0.f; c->target_update_interval = 1; c->seed = 0;
  return HB_OK;
}

int hb_sac_create(hb_batch* b, const hb_sac_config* cfg) {
  if (!b || !cfg || !cfg_ok(cfg) || b->actor.layers < 1 || b->q[0].layers < 1 || b->q[1].layers < 1) return HB_EINVAL;
  if (b->q[0].layers != b->q[1].layers) return HB_EINVAL;
  for (int l = 0; l <= b->q[0].layers; l++) if (b->q[0].sizes[l] != b->q[1].sizes[l]) return HB_EINVAL;
  if (b->q[0].act != b->q[1].act) return HB_EINVAL;  // (the actor's may differ)
  if (b->actor_cfg.head != HB_ACTOR_SQUASHED) return HB_EUNSUPPORTED;
  const int nu = b->D.dm.nu;
  if (nu < 1 || nu > kActorMaxNu) return HB_EINVAL;
  int rc = learner_idle(b);
  if (rc != HB_OK) return rc;
  SacLearner& L = b->sac;
  L.clear();
  layout(b);
  const LearnNets ns = nets_of(b);
  rc = L.alloc_record(64 * kSacSrow);
  if (rc == HB_OK) rc = L.d_target.alloc(L.PT);
  if (rc == HB_OK) rc = L.d_alpha.alloc(4, true);
  std::vector<float> flat;
  if (rc == HB_OK) rc = L.read_installed(ns, flat);
  if (rc == HB_OK) {
    flat[L.P - 1] = (float)std::log((double)cfg->ent_coef_init);
    rc = L.write_params(ns, flat.data(), false);
  }
  if (rc == HB_OK) rc = write_targets(b, flat.data() + L.off_q);
  if (rc != HB_OK) { L.clear(); return rc; }
  L.cfg = *cfg;
  L.on = true;
  return HB_OK;
}

int hb_sac_configure(hb_batch* b, const hb_sac_config* cfg) {
  if (!b || !cfg || !b->sac.on || !cfg_ok(cfg)) return HB_EINVAL;
  b->sac.cfg = *cfg;
  return HB_OK;
}

int hb_sac_destroy(hb_batch* b) {
  if (!b || !b->sac.on) return HB_EINVAL;
  const int rc = learner_idle(b);
  if (rc != HB_OK) return rc;
  b->sac.clear();
  return HB_OK;
}

long long hb_sac_param_count(hb_batch* b) { return b && b->sac.on ? b->sac.P : HB_EINVAL; }
long long hb_sac_target_count(hb_batch* b) { return b && b->sac.on ? b->sac.PT : HB_EINVAL; }

int hb_sac_get_params(hb_batch* b, float* out, long long count) { return b ? b->sac.download(b, b->sac.d_param, out, count) : HB_EINVAL; }
int hb_sac_get_grads(hb_batch* b, float* out, long long count) { return b ? b->sac.download(b, b->sac.d_grad, out, count) : HB_EINVAL; }

int hb_sac_set_params(hb_batch* b, const float* in, long long count) {
  if (!b || !in || !b->sac.on || count != b->sac.P) return HB_EINVAL;
  const int rc = learner_idle(b);
  if (rc != HB_OK) return rc;
  return b->sac.write_params(nets_of(b), in, true);
}

int hb_sac_get_state(hb_batch* b, float* params, float* m, float* v, long long count, float* targets, long long target_count, long long* t) {
  if (!b || !params || !m || !v || !targets || !t || !b->sac.on || count != b->sac.P || target_count != b->sac.PT) return HB_EINVAL;
  SacLearner& L = b->sac;
  const int rc = L.get_record(b, params, m, v);
  if (rc != HB_OK) return rc;
  HB_HIP(hipMemcpy(targets, L.d_target, (size_t)target_count * sizeof(float), hipMemcpyDeviceToHost));
  *t = L.t;
  return HB_OK;
}

int hb_sac_set_state(hb_batch* b, const float* params, const float* m, const float* v, long long count, const float* targets, long long target_count, long long t) {
  if (!b || !params || !m || !v || !targets || !b->sac.on || count != b->sac.P || target_count != b->sac.PT || t < 0) return HB_EINVAL;
  SacLearner& L = b->sac;
  int rc = learner_idle(b);
  if (rc != HB_OK) return rc;
  if ((rc = L.write_params(nets_of(b), params, true)) != HB_OK) return rc;
  if ((rc = write_targets(b, targets)) != HB_OK) return rc;
  if ((rc = L.set_moments(m, v)) != HB_OK) return rc;
  L.t = t;
  return HB_OK;
}

int hb_sac_step_dev(hb_batch* b, const hb_sac_rows* rows, float* stats_dev) {
  if (!b || !rows || !b->sac.on) return HB_EINVAL;
  if (!rows->obs || !rows->action || !rows->reward || !rows->next_obs || !rows->done) return HB_EINVAL;
  if (rows->mb < 1 || rows->n_rows < 1) return HB_EINVAL;
  if (!rows->index && (rows->first < 0 || rows->first + rows->mb > rows->n_rows)) return HB_EINVAL;
  if (rows->eps_given && (!rows->eps_pi || !rows->eps_next)) return HB_EINVAL;
  SacLearner& L = b->sac;
  HB_HIP(hipSetDevice(b->device));
  hipStream_t st = main_stream(b);
  const size_t mb = rows->mb, nu = b->D.dm.nu, nobs = b->row.width;
  const DevMlp& A = b->actor;
  const DevMlp& Q = b->q[0];
  const int La = A.layers, Lq = Q.layers;
  const int chunk = ppo_row_chunk(rows->mb), nchunk = (rows->mb + chunk - 1) / chunk;
  const LearnNets ns = nets_of(b), ts = target_nets_of(b);
  // the scratch: the actor's input rows, activations, dZ and its two outputs | the samples | the Q networks' input rows | per Q network:
  // activations, dZ, the three outputs and dQ / da | the by-row terms
  float *a_act[4] = {}, *a_dz[4] = {}, *q_act[2][4] = {}, *q_dz[2][4] = {};
  float *pi_out, *nx_out, *a_pi, *a_nx, *eps, *lp_pi, *lp_nx, *q_in, *q_out[2], *qt_out[2], *qpi_out[2], *q_da[2], *srow;
  auto carve = [&](ScratchCarve c) {
    a_act[0] = c.take(mb * nobs);
    for (int l = 1; l < La; l++) a_act[l] = c.take(mb * A.sizes[l]);
    for (int l = 0; l < La; l++) a_dz[l] = c.take(mb * A.sizes[l + 1]);
    pi_out = c.take(mb * 2 * nu);
    nx_out = c.take(mb * 2 * nu);
    a_pi = c.take(mb * nu);
    a_nx = c.take(mb * nu);
    eps = c.take(mb * nu);
    lp_pi = c.take(mb);
    lp_nx = c.take(mb);
    q_in = c.take(mb * (nobs + nu));
    for (int k = 0; k < 2; k++) {
      q_act[k][0] = q_in;
      for (int l = 1; l < Lq; l++) q_act[k][l] = c.take(mb * Q.sizes[l]);
      for (int l = 0; l < Lq; l++) q_dz[k][l] = c.take(mb * Q.sizes[l + 1]);
      q_out[k] = c.take(mb); qt_out[k] = c.take(mb); qpi_out[k] = c.take(mb);
      q_da[k] = c.take(mb * nu);
    }
    srow = c.take(mb * kSacSrow);
    return c.used;
  };
  const int rc = L.reserve_scratch(carve(ScratchCarve{}), nchunk, st);
  if (rc != HB_OK) return rc;
  carve(ScratchCarve{L.d_scratch, 0});

  // the reversed network of net k (0 actor, 1 Q1, 2 Q2): L - 1 steps down to dZ_0, or L steps into the action inputs
  auto reversed = [&](int k, bool to_input) { return learn_reversed(L.view(ns, k), to_input ? (int)nu : 0, L.d_zero); };
  auto fwd_job = [&](SacFwdJob& j, const DevMlp& n, const float* x0, const float* x1, bool gather1, float* in_store, float* const* act, float* out) {
    j.net = n.desc();
    j.x0 = x0; j.n0 = (int)nobs; j.gather0 = 1;
    j.x1 = x1; j.n1 = x1 ? (int)nu : 0; j.gather1 = gather1 ? 1 : 0;
    j.in_store = in_store;
    if (act) for (int l = 1; l < n.layers; l++) j.act[l] = act[l];
    j.out = out;
  };
  auto wg_jobs = [&](SacWgDesc& w, int k, float* const* act, float* const* dz) {
    const DevMlp& n = *ns.net[k];
    for (int l = 0; l < n.layers; l++) w.job[w.njob++] = SacWgJob{act[l], dz[l], n.sizes[l], n.sizes[l + 1], L.off_w[k][l], L.off_b[k][l]};
  };
  const long long t1 = L.t + 1;

  SacHeadDesc h;
  memset(&h, 0, sizeof h);
  h.mb = rows->mb; h.nu = (int)nu; h.eps_given = rows->eps_given != 0;
  h.seed = L.cfg.seed; h.t = (unsigned)L.t;
  h.index = rows->index; h.first = rows->first;
  h.gamma = L.cfg.gamma; h.target_entropy = target_entropy(b);
  h.param = L.d_param; h.P = L.P; h.alpha = L.d_alpha;
  h.reward = rows->reward; h.done = rows->done;
  h.eps_pi = rows->eps_pi; h.eps_next = rows->eps_next; h.eps = eps;
  h.pi_out = pi_out; h.nx_out = nx_out; h.a_pi = a_pi; h.a_nx = a_nx; h.lp_pi = lp_pi; h.lp_nx = lp_nx;
  for (int k = 0; k < 2; k++) { h.q[k] = q_out[k]; h.qt[k] = qt_out[k]; h.qpi[k] = qpi_out[k]; h.da[k] = q_da[k]; h.dzq[k] = q_dz[k][Lq - 1]; }
  h.dza = a_dz[La - 1];
  h.srow = srow;

  SacFwdDesc f;
  memset(&f, 0, sizeof f);
  f.index = rows->index; f.first = rows->first; f.mb = rows->mb;
  // 1. the actor on obs and on next_obs, Q1 and Q2 on obs | action
  fwd_job(f.job[0], A, rows->obs, nullptr, false, a_act[0], a_act, pi_out);
  fwd_job(f.job[1], A, rows->next_obs, nullptr, false, nullptr, nullptr, nx_out);
  fwd_job(f.job[2], b->q[0], rows->obs, rows->action, true, q_in, q_act[0], q_out[0]);
  fwd_job(f.job[3], b->q[1], rows->obs, rows->action, true, nullptr, q_act[1], q_out[1]);
  HB_HIP(launch_sac_forward(f, 4, st));
  // 2. the samples
  HB_HIP(launch_sac_head(h, 0, st));
  // 3. the targets on next_obs | a'
  memset(f.job, 0, sizeof f.job);
  fwd_job(f.job[0], L.tq[0], rows->next_obs, a_nx, false, nullptr, nullptr, qt_out[0]);
  fwd_job(f.job[1], L.tq[1], rows->next_obs, a_nx, false, nullptr, nullptr, qt_out[1]);
  HB_HIP(launch_sac_forward(f, 2, st));
  // 4. y and the critics' top dZ
  HB_HIP(launch_sac_head(h, 1, st));
  // 5. the critics' dZ
  SacBwdDesc bw;
  memset(&bw, 0, sizeof bw);
  bw.mb = rows->mb;
  for (int k = 0; k < 2; k++) {
    SacBwdJob& j = bw.job[k];
    j.net = reversed(k + 1, false); j.L = Lq; j.activation = Q.act; j.top = q_dz[k][Lq - 1];
    for (int l = 1; l < Lq; l++) j.act[l] = q_act[k][l];
    for (int l = 0; l < Lq - 1; l++) j.dz[l] = q_dz[k][l];
  }
  if (Lq > 1) HB_HIP(launch_sac_backprop(bw, 2, st));
  // 6. - 8. dW, db by chunk; their merge, the statistics and dloss / dlog_ent_coef; Adam
  SacWgDesc w;
  memset(&w, 0, sizeof w);
  w.mb = rows->mb; w.chunk = chunk; w.nchunk = nchunk; w.P = L.P; w.part = L.d_part; w.srow = srow; w.statpart = L.d_dbl;
  wg_jobs(w, 1, q_act[0], q_dz[0]);
  wg_jobs(w, 2, q_act[1], q_dz[1]);
  w.ncol = 6;
  HB_HIP(launch_sac_wgrad(w, st));
  SacReduceDesc rd;
  memset(&rd, 0, sizeof rd);
  rd.lo = L.off_q; rd.hi = L.P - 1; rd.P = L.P; rd.nchunk = nchunk; rd.mb = rows->mb; rd.phase = 0;
  rd.target_entropy = h.target_entropy; rd.part = L.d_part; rd.param = L.d_param; rd.alpha = L.d_alpha; rd.statpart = L.d_dbl;
  rd.grad = L.d_grad; rd.stats = stats_dev;
  HB_HIP(launch_sac_reduce(rd, st));
  SacAdamDesc ad;
  memset(&ad, 0, sizeof ad);
  ad.param = L.d_param; ad.m = L.d_m; ad.v = L.d_v; ad.grad = L.d_grad; ad.t = t1;
  ad.beta1 = L.cfg.beta1; ad.beta2 = L.cfg.beta2; ad.eps = L.cfg.eps; ad.lr_ent = L.cfg.lr_ent;
  ad.lo = L.off_q; ad.hi = L.cfg.auto_ent ? L.P : L.P - 1; ad.ent_index = L.P - 1; ad.lr = L.cfg.lr_critic;
  ad.nseg = learn_segments(L.view(ns, 1), 0, ad.seg);
  ad.nseg += learn_segments(L.view(ns, 2), 0, ad.seg + ad.nseg);
  ad.seg[ad.nseg++] = ParamSeg{L.P - 1, 0, 1, 0, nullptr, nullptr};
  HB_HIP(launch_sac_adam(ad, st));
  // 9. the updated Q1, Q2 on obs | a_pi
  memset(f.job, 0, sizeof f.job);
  fwd_job(f.job[0], b->q[0], rows->obs, a_pi, false, nullptr, q_act[0], qpi_out[0]);
  fwd_job(f.job[1], b->q[1], rows->obs, a_pi, false, nullptr, q_act[1], qpi_out[1]);
  HB_HIP(launch_sac_forward(f, 2, st));
  // 10. dQ1 / da, dQ2 / da from a top gradient of 1
  memset(&bw, 0, sizeof bw);
  bw.mb = rows->mb;
  for (int k = 0; k < 2; k++) {
    SacBwdJob& j = bw.job[k];
    j.net = reversed(k + 1, true); j.L = Lq; j.activation = Q.act; j.unit_top = 1; j.da = q_da[k];
    for (int l = 1; l < Lq; l++) j.act[l] = q_act[k][l];
  }
  HB_HIP(launch_sac_backprop(bw, 2, st));
  // 11. the actor's top dZ
  HB_HIP(launch_sac_head(h, 2, st));
  // 12. the actor's dZ
  memset(&bw, 0, sizeof bw);
  bw.mb = rows->mb;
  {
    SacBwdJob& j = bw.job[0];
    j.net = reversed(0, false); j.L = La; j.activation = A.act; j.top = a_dz[La - 1];
    for (int l = 1; l < La; l++) j.act[l] = a_act[l];
    for (int l = 0; l < La - 1; l++) j.dz[l] = a_dz[l];
  }
  if (La > 1) HB_HIP(launch_sac_backprop(bw, 1, st));
  // 13. - 15. the actor's dW, db; merge; Adam
  memset(w.job, 0, sizeof w.job);
  w.njob = 0;
  wg_jobs(w, 0, a_act, a_dz);
  w.ncol = 2;
  HB_HIP(launch_sac_wgrad(w, st));
  rd.lo = 0; rd.hi = L.off_q; rd.phase = 1;
  HB_HIP(launch_sac_reduce(rd, st));
  ad.lo = 0; ad.hi = L.off_q; ad.ent_index = -1; ad.lr = L.cfg.lr_actor;
  memset(ad.seg, 0, sizeof ad.seg);
  ad.nseg = learn_segments(L.view(ns, 0), 0, ad.seg);
  HB_HIP(launch_sac_adam(ad, st));
  // 16. the targets
  if (t1 % L.cfg.target_update_interval == 0) {
    SacPolyakDesc pk;
    memset(&pk, 0, sizeof pk);
    pk.n = L.PT; pk.src = L.d_param + L.off_q; pk.target = L.d_target; pk.tau = L.cfg.tau;
    pk.nseg = learn_segments(L.view(ts, 1, false), L.off_q, pk.seg);
    pk.nseg += learn_segments(L.view(ts, 2, false), L.off_q, pk.seg + pk.nseg);
    HB_HIP(launch_sac_polyak(pk, st));
  }
  L.t = t1;
  return HB_OK;
}

}  // extern "C"
