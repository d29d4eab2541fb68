// hb_api.cpp — the C-ABI of libhb.so (include/hb.h), first part: model handles, the batch lifecycle and pipeline, reset / step / forward /
// inverse / kinematics, status, counts and read-outs, memory helpers and timing.  Rollouts and tasks are in hb_api_rollout.cpp, the env
// adapter in hb_api_env.cpp, the policy in hb_api_policy.cpp, the collection loop in hb_api_collect.cpp; the device model tables in
// hb_tables.cpp and the launch plumbing around the kernel translation units (hb_step.hip, hb_narrow.hip, hb_env.hip, hb_rollout.hip, hb_kin.hip) in
// hb_batch.cpp.
//
// Host C++ only; no PyTorch.  One hb_batch owns one HIP stream and all device memory of its
// envs; the model is immutable and shareable (reference ownership rules: SURVEY.md §8b).
#include "hb_batch.hpp"
#include "hb_tables.hpp"

// the names of one kind of model element (null: no such kind)
static const std::vector<std::string>* names_of(const Model& m, const std::string& k) {
  if (k == "body") return &m.body_name;
  if (k == "joint") return &m.jnt_name;
  if (k == "geom") return &m.geom_name;
  if (k == "actuator") return &m.actuator_name;
  if (k == "tendon") return &m.tendon_name;
  if (k == "key") return &m.key_name;
  if (k == "equality") return &m.eq_name;
  return nullptr;
}

extern "C" {

const char* hb_version(void) { return "hb 0.1 (gfx950)"; }

hb_model* hb_model_load(const char* path, char* err, int err_sz) {
  if (!path) { set_err(err, err_sz, "null path"); return nullptr; }
  hb_model* h = nullptr;
  try {  // nothing may propagate through the C boundary (a malformed file can make the loaders throw bad_alloc / length_error)
    h = new hb_model;
    std::string e, p = path;
    bool ok = (p.size() > 4 && p.substr(p.size() - 4) == ".hbm") ? load_hbm(p, h->m, e) : compile_mjcf_file(p, h->m, e);
    if (!ok) { set_err(err, err_sz, e); delete h; return nullptr; }
    return h;
  } catch (const std::exception& ex) {
    set_err(err, err_sz, std::string("model load failed: ") + ex.what());
    delete h;
    return nullptr;
  }
}

hb_model* hb_model_load_xml_string(const char* xml, char* err, int err_sz) {
  if (!xml) { set_err(err, err_sz, "null xml"); return nullptr; }
  hb_model* h = nullptr;
  try {
    h = new hb_model;
    std::string e;
    if (!compile_mjcf_string(xml, h->m, e)) { set_err(err, err_sz, e); delete h; return nullptr; }
    return h;
  } catch (const std::exception& ex) {
    set_err(err, err_sz, std::string("model load failed: ") + ex.what());
    delete h;
    return nullptr;
  }
}

int hb_model_save(const hb_model* m, const char* path, char* err, int err_sz) {
  if (!m || !path) return HB_EINVAL;
  std::string e;
  if (!save_hbm(m->m, path, e)) { set_err(err, err_sz, e); return HB_EIO; }
  return HB_OK;
}

void hb_model_free(hb_model* m) { delete m; }

int hb_model_sizes(const hb_model* h, hb_sizes* out) {
  if (!h || !out) return HB_EINVAL;
  const Model& m = h->m;
  out->nq = m.nq; out->nv = m.nv; out->nu = m.nu; out->nbody = m.nbody; out->njnt = m.njnt; out->ngeom = m.ngeom; out->ntendon = m.ntendon;
  out->nM = m.nM; out->nkey = m.nkey; out->npair = m.npair;
  out->nobs = model_nobs(m);
  { int variant; std::string e; if (!model_variant(m, variant, out->ncon_max, out->nefc_max, e)) { out->ncon_max = kNconMax; out->nefc_max = kNefcMax; } }
  return HB_OK;
}

int hb_options_get(const hb_model* h, hb_options* o) {
  if (!h || !o) return HB_EINVAL;
  const Model& m = h->m;
  o->timestep = m.timestep; memcpy(o->gravity, m.gravity, sizeof o->gravity); o->impratio = m.impratio; o->tolerance = m.tolerance;
  o->iterations = m.iterations; o->solver = m.solver; o->cone = m.cone; o->integrator = m.integrator; o->disableflags = m.disableflags;
  o->ls_iterations = m.ls_iterations; o->ls_tolerance = m.ls_tolerance;
  return HB_OK;
}

int hb_options_set(hb_model* h, const hb_options* o) {
  if (!h || !o) return HB_EINVAL;
  if ((o->solver != SOL_PGS && o->solver != SOL_NEWTON) || o->cone != 0 || (o->integrator != INT_EULER && o->integrator != INT_RK4)) return HB_EUNSUPPORTED;
  if (!(o->timestep > 0) || !(o->impratio > 0) || o->iterations < 0 || o->ls_iterations < 0 || !(o->ls_tolerance >= 0)) return HB_EINVAL;
  Model& m = h->m;
  m.timestep = o->timestep; memcpy(m.gravity, o->gravity, sizeof o->gravity); m.impratio = o->impratio; m.tolerance = o->tolerance;
  m.iterations = o->iterations; m.disableflags = o->disableflags; m.solver = o->solver; m.integrator = o->integrator;
  m.ls_iterations = o->ls_iterations; m.ls_tolerance = o->ls_tolerance;
  return HB_OK;
}

int hb_model_pair_order(hb_model* h, int order) {
  if (!h) return HB_EINVAL;
  if (order == 0 || order == 1) sort_pairs(h->m, order);
  else if (order != -1) return HB_EINVAL;
  return h->m.pair_order;
}

int hb_model_box_manifold(hb_model* h, int mode) {
  if (!h) return refuse_with("hb_model_box_manifold: NULL model");
  if (mode == 0 || mode == 1) h->m.box_manifold = mode;
  else if (mode != -1) return refuse_with("hb_model_box_manifold: mode must be 1 (on), 0 (off) or -1 (query)");
  return h->m.box_manifold;
}

int hb_model_name2id(const hb_model* h, const char* kind, const char* name) {
  if (!h || !kind || !name) return -1;
  const std::vector<std::string>* v = names_of(h->m, kind);
  if (!v) return -1;
  for (size_t i = 0; i < v->size(); i++) if ((*v)[i] == name) return (int)i;
  return -1;
}

int hb_model_id2name(const hb_model* h, const char* kind, int id, char* out, int cap) {
  if (!h || !kind || !out || cap <= 0) return HB_EINVAL;
  const std::vector<std::string>* v = names_of(h->m, kind);
  if (!v || id < 0 || (size_t)id >= v->size() || (*v)[id].size() >= (size_t)cap) return HB_EINVAL;
  memcpy(out, (*v)[id].c_str(), (*v)[id].size() + 1);
  return (int)(*v)[id].size();
}

int hb_model_get_array(const hb_model* h, const char* field, double* out, int cap) {
  if (!h || !field) return HB_EINVAL;
  struct Finder {
    const char* want; const vecd* found = nullptr; const veci* foundi = nullptr;
    bool optional(bool) { return true; }
    void operator()(const char* n, vecd& v) { if (!strcmp(n, want)) found = &v; }
    void operator()(const char* n, veci& v) { if (!strcmp(n, want)) foundi = &v; }
    void operator()(const char*, int&) {}
    void operator()(const char*, double&) {}
    void operator()(const char*, double*, int) {}
    void operator()(const char*, std::vector<std::string>&) {}
  } f;
  f.want = field;
  const_cast<Model&>(h->m).visit(f);
  if (f.found) { int n = (int)f.found->size(); if (out) for (int i = 0; i < n && i < cap; i++) out[i] = (*f.found)[i]; return n; }
  if (f.foundi) { int n = (int)f.foundi->size(); if (out) for (int i = 0; i < n && i < cap; i++) out[i] = (*f.foundi)[i]; return n; }
  return HB_EINVAL;
}

hb_batch* hb_batch_create(const hb_model* m, int n_env, int device, char* err, int err_sz) {
  if (!m || n_env <= 0) { set_err(err, err_sz, "bad arguments"); return nullptr; }
  int ndev = 0;
  if (device < 0 || hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device >= ndev) {
    set_err(err, err_sz, "no HIP device available: this engine has no CPU backend (device=" + std::to_string(device) + ", visible=" + std::to_string(ndev) + ")");
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) { set_err(err, err_sz, "hipSetDevice failed"); return nullptr; }
  hb_batch* b = new hb_batch;
  b->model = m; b->n_env = n_env; b->device = device;
  std::string e;
  if (!build_device_model(m->m, b->D, e)) { set_err(err, err_sz, e); delete b; return nullptr; }
  const DevModel& dm = b->D.dm;
  b->row = env_row(dm.nobs, 0, 0, 0, false);  // (until hb_env_obs_extend and the observed features widen the adapter's rows)
  bool ok = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming) == hipSuccess;
  // (the pipes' streams are created when hb_batch_pipeline asks for them: the runtime maps streams
  // onto four hardware queues, and streams that share one serialise - a batch should not own more streams than it uses)
  ok = ok && b->d_state.alloc((size_t)n_env * dm.nstate) == HB_OK;
  ok = ok && b->d_status.alloc((size_t)n_env) == HB_OK;
  ok = ok && b->d_counts.alloc((size_t)n_env * kCountStride, /*zero=*/true) == HB_OK;
  ok = ok && ensure_ctrl(b, (size_t)n_env * std::max(1, dm.nu)) == HB_OK;
  ok = ok && b->d_order.alloc((size_t)2 * n_env) == HB_OK;  // the permutation | the sort keys of a pass
  ok = ok && b->d_order2.alloc((size_t)2 * n_env) == HB_OK;
  // general variants: the staged step (pose -> narrowphase -> step kernels); hb_batch_tune(HB_TUNE_STAGED, 0) keeps everything in the step kernel
  if (dm.variant != 0) {
    StageBufs& sb = b->stage;
    ok = ok && b->d_stage_geom.alloc((size_t)n_env * std::max(1, dm.ngeom) * 10) == HB_OK;
    ok = ok && b->d_stage_item.alloc((size_t)n_env * kWorkMax) == HB_OK;
    ok = ok && b->d_stage_nwork.alloc((size_t)n_env, /*zero=*/true) == HB_OK;
    ok = ok && b->d_stage_nsearch.alloc((size_t)n_env * 2, /*zero=*/true) == HB_OK;
    ok = ok && b->d_stage_result.alloc((size_t)n_env * kWorkMax * 4) == HB_OK;
    sb.geom = b->d_stage_geom; sb.item = b->d_stage_item; sb.nwork = b->d_stage_nwork; sb.nsearch = b->d_stage_nsearch; sb.result = b->d_stage_result;
    sb.nq = dm.nq; sb.nv = dm.nv; sb.nu = dm.nu;
    sb.no_mesh = b->model->m.nmesh == 0 ? 1 : 0;
    sb.has_box = dm.box_manifold ? 2 : dm.has_box;
    sb.pose_lds = pose_lds_floats(dm.nq, dm.nbody, dm.ngeom) * (int)sizeof(float);
    if (dm.variant == 1 || b->D.d_dm_fast) {
      ok = ok && b->d_stage_defer.alloc((size_t)n_env * 3, /*zero=*/true) == HB_OK;  // flags | list | counters (StageBufs)
      if (ok) { sb.defer = b->d_stage_defer; sb.defer_list = sb.defer + n_env; sb.defer_count = sb.defer + 2 * (size_t)n_env; }
      if (dm.variant == 2 || dm.variant == 3) { sb.dm_fast = b->D.d_dm_fast; sb.fast_lds = b->D.fast_lds_floats * (int)sizeof(float); }
      if (ok && sb.fast_lds > 64 * 1024) ok = set_step_lds_limit(sb.fast_lds) == hipSuccess;
    }
  }
  if (hb_debug()) fprintf(stderr, "[hb] LDS per env: %d bytes (%d envs per CU)\n", dm.lds_floats * 4, 160 * 1024 / (dm.lds_floats * 4));
  if (hb_debug()) fprintf(stderr, "[hb] tree levels %d, limit candidates %d, trees %d; size-specialised kernel: %s\n", dm.nlevel, dm.nlimcand, dm.ntree, (b->D.sized_h27 || b->D.sized_team) ? "yes" : "no");
  if (hb_debug() && b->D.fast_lds_floats) fprintf(stderr, "[hb] LDS per env of the staged step's fast kernel: %d bytes (%d envs per CU)\n", b->D.fast_lds_floats * 4, 160 * 1024 / (b->D.fast_lds_floats * 4));
  if (ok && dm.lds_floats * 4 > 64 * 1024) ok = set_step_lds_limit(dm.lds_floats * 4) == hipSuccess;
  if (!ok) { set_err(err, err_sz, "device allocation failed"); hb_batch_free(b); return nullptr; }
  if (hb_reset(b, nullptr, -1, 0, 0) != HB_OK) { set_err(err, err_sz, "initial reset failed"); hb_batch_free(b); return nullptr; }
  return b;
}

void hb_batch_free(hb_batch* b) {
  if (!b) return;
  b->fold_n = 0;  // (step calls nobody will read the results of)
  HB_IGN(hipSetDevice(b->device));
  for (int c = 0; c < hb_batch::kPipes; c++) {
    if (b->pipe[c] && b->pipe[c] != b->stream) { HB_IGN(hipStreamSynchronize(b->pipe[c])); HB_IGN(hipStreamDestroy(b->pipe[c])); }
    if (b->ev_pipe[c]) HB_IGN(hipEventDestroy(b->ev_pipe[c]));
  }
  if (b->ev_fork) HB_IGN(hipEventDestroy(b->ev_fork));
  if (b->stream) { HB_IGN(hipStreamSynchronize(b->stream)); HB_IGN(hipStreamDestroy(b->stream)); }
  for (auto e : b->tev) HB_IGN(hipEventDestroy(e));
  if (b->ev0) HB_IGN(hipEventDestroy(b->ev0));
  if (b->ev1) HB_IGN(hipEventDestroy(b->ev1));
  delete b;  // (the device buffers: every stream was waited for above, and the device is still set)
}

int hb_batch_n_env(const hb_batch* b) { return b ? b->n_env : HB_EINVAL; }
void* hb_batch_stream(hb_batch* b) { return b ? (void*)main_stream(b) : nullptr; }
int hb_batch_sync(hb_batch* b) {
  if (!b) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  if (b->join_error) { b->join_error = 0; return HB_ENODEVICE; }
  return HB_OK;
}
// the streams of the first n segments, created on first use.  Segment 0 runs on the batch's own stream: one stream fewer for the
// process' hardware queues (below), and nothing else is enqueued there while steps are in flight
static int make_pipes(hb_batch* b, int n) {
  for (int c = 0; c < n; c++) {
    if (!b->pipe[c] && c == 0) b->pipe[0] = b->stream;
    if (!b->pipe[c]) {
      // (streams of different priorities - ROCm keeps one pool of hardware queues per priority level - were measured too: 95 us per step for three
      // segments against 88)
      const hipError_t e = hipStreamCreateWithFlags(&b->pipe[c], hipStreamNonBlocking);
      if (e != hipSuccess) return HB_ENOMEM;
    }
    if (!b->ev_pipe[c] && hipEventCreateWithFlags(&b->ev_pipe[c], hipEventDisableTiming) != hipSuccess) return HB_ENOMEM;
  }
  return HB_OK;
}
// Do kernels on the first n segment streams run at the same time?  ROCm maps a process' streams onto GPU_MAX_HW_QUEUES (default 4)
// hardware queues, the null stream included, and two streams on one queue run their kernels one after the other: three segments
// of which two share a queue step 4096 envs in 147 us instead of 88.  Nothing in HIP tells which queue a stream got, so this looks:
// one idling wave per stream (60 us each), all n overlapping pairwise in the GPU's own clock or not.
// returns -1 when all n run side by side, else the higher stream index of the first pair that does not (-2: the probe itself failed)
static int pipes_conflict(hb_batch* b, int n) {
  DevBuf<unsigned long long> d;
  unsigned long long h[2 * hb_batch::kPipes] = {};
  if (hipStreamSynchronize(b->stream) != hipSuccess || d.alloc(2 * hb_batch::kPipes, /*zero=*/true) != HB_OK) return -2;
  bool ok = true;
  for (int c = 0; c < n && ok; c++) ok = launch_probe_spin(d + 2 * c, 6000, b->pipe[c]) == hipSuccess;
  for (int c = 0; c < n; c++) ok = hipStreamSynchronize(b->pipe[c]) == hipSuccess && ok;
  ok = ok && hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) == hipSuccess;
  if (!ok) return -2;
  for (int i = 0; i < n; i++)
    for (int j = i + 1; j < n; j++)
      if (!(h[2 * i] < h[2 * j + 1] && h[2 * j] < h[2 * i + 1] && h[2 * i + 1] > h[2 * i] && h[2 * j + 1] > h[2 * j])) return j;
  return -1;
}
int hb_batch_pipeline(hb_batch* b, int on) {
  if (!b) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  (void)main_stream(b);
  if (on < 0 || on > hb_batch::kPipes) return HB_EINVAL;
  // 1: default segment count.  Measured on MI355X, 4096 envs, us per step (tools/gpu_pipeline_queues.py, every case a fresh process):
  // 2 segments 92, 3 segments 88, 4 segments 87 with GPU_MAX_HW_QUEUES >= 5 and 142 without, 5 and more 107 - 170 however many queues
  // the runtime is given (a fifth active queue is multiplexed).  Three it is, when the three streams are seen to run side by side
  // (other streams of the process can take the queues: pipes_conflict); two otherwise.  No environment is set here.
  int want = on == 1 ? 3 : on;
  int rc = make_pipes(b, want);
  if (rc != HB_OK) return rc;
  if (on == 1 && b->probed_segments) want = b->probed_segments;  // (probed before on these very streams: no second probe, the same shape every time)
  else if (on == 1) {
    // a stream that shares its queue is replaced by a fresh one (the runtime deals queues out in turn: the next stream lands on another
    // one) while the old one still holds its place; a few tries, then two segments
    hipStream_t spare[4] = {};
    int bad = pipes_conflict(b, want);
    for (int t = 0; t < 4 && bad > 0; t++) {
      hipStream_t s = nullptr;
      if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) break;
      spare[t] = b->pipe[bad];
      b->pipe[bad] = s;
      bad = pipes_conflict(b, want);
    }
    for (hipStream_t s : spare) if (s) HB_IGN(hipStreamDestroy(s));
    if (bad == -2) return HB_ENODEVICE;  // the probe itself failed (a HIP error, not a shared queue): an error, not a quiet two segments
    if (bad != -1) want = 2;
    b->probed_segments = want;
    if (hb_debug()) fprintf(stderr, "[hb] hb_batch_pipeline: %d env segments (%s)\n", want, bad == -1 ? "every segment stream has a hardware queue of its own" : "two of three segment streams share a hardware queue");
  }
  b->npipe = want;
  if (b->order_mode == 2) b->order_mode = 0;  // segment boundaries changed: per-segment permutations are stale (one of the whole batch stays good for unsegmented launches)
  return HB_OK;
}
int hb_batch_segments(const hb_batch* b) { return b ? segment_count(b) : HB_EINVAL; }
int hb_batch_join(hb_batch* b) {
  if (!b) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  (void)main_stream(b);  // (launches the step calls held back, then joins the segments' streams)
  return b->join_error ? HB_ENODEVICE : HB_OK;
}

int hb_reset(hb_batch* b, const uint8_t* mask, int keyframe, int perturb, int env_offset) {
  return reset_impl(b, mask, keyframe, perturb ? 1.f : 0.f, env_offset);
}

int hb_step_dev(hb_batch* b, const float* ctrl_dev, int n_substeps) {
  if (!b || n_substeps < 1 || (!ctrl_dev && b->D.dm.nu > 0)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  BatchPtrs P = make_ptrs(b);
  P.ctrl = ctrl_dev; P.ctrl_mode = 0;
  return launch_steps(b, P, n_substeps, /*foldable=*/true);
}

int hb_step(hb_batch* b, const float* ctrl, int n_substeps) {
  if (!b || n_substeps < 1 || (!ctrl && b->D.dm.nu > 0)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  size_t n = (size_t)b->n_env * b->D.dm.nu;
  if (n) HB_HIP(hipMemcpyAsync(ctrl_for_write(b), ctrl, n * sizeof(float), hipMemcpyHostToDevice, main_stream(b)));
  int rc = hb_step_dev(b, b->d_ctrl, n_substeps);
  if (rc != HB_OK) return rc;
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

int hb_forward(hb_batch* b, const float* ctrl) {
  if (!b) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  size_t n = (size_t)b->n_env * b->D.dm.nu;
  if (ctrl && n) HB_HIP(hipMemcpyAsync(ctrl_for_write(b), ctrl, n * sizeof(float), hipMemcpyHostToDevice, main_stream(b)));
  else if (n) HB_HIP(hipMemsetAsync(ctrl_for_write(b), 0, n * sizeof(float), main_stream(b)));
  BatchPtrs P = make_ptrs(b);
  P.ctrl = b->d_ctrl; P.ctrl_mode = 0; P.integrate = 0;
  HB_HIP(launch_batch_step(b, P, 1, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

int hb_inverse_dev(hb_batch* b, const float* qacc_dev, int flags, float* qfrc_inverse_dev, int* warnings_dev) {
  if (!b || !qacc_dev || !qfrc_inverse_dev || (flags & ~HB_INV_DISCRETE)) return HB_EINVAL;
  if ((flags & HB_INV_DISCRETE) && b->D.dm.integrator != INT_EULER) return HB_EUNSUPPORTED;  // (the discrete inverse is that of the Euler step)
  HB_HIP(hipSetDevice(b->device));
  const hipStream_t stream = main_stream(b);  // (held step calls launched, pipes joined: the inverse sees the state they leave)
  // a launch of its own, not make_ptrs: nothing of the batch's state, status, counts, orders or noise process is written
  // (the pose and narrowphase kernels of a general variant write per-env counts and status bits: here into scratch, which the inverse
  // kernel reads back into the warnings)
  const size_t ncount = (size_t)b->n_env * kCountStride;
  if (b->d_inv_scratch.alloc(ncount + (size_t)b->n_env) != HB_OK) return HB_ENOMEM;
  HB_HIP(hipMemsetAsync(b->d_inv_scratch + ncount, 0, (size_t)b->n_env * sizeof(int), stream));
  BatchPtrs P;
  memset(&P, 0, sizeof P);
  P.state = b->d_state; P.counts = b->d_inv_scratch; P.status = b->d_inv_scratch + ncount;
  P.ctrl = b->d_ctrl;  // (never applied: mj_inverse leaves the actuators out)
  P.n_env = b->n_env; P.blk0 = 0; P.nblk = b->n_env;
  P.dr = b->d_dr; P.dr_stride = b->dr_stride;
  P.stage = b->stage;  // general variants: the narrowphase of a staged step into the batch's stage buffers, which every step rewrites
  P.stage.defer = nullptr; P.stage.defer_list = nullptr; P.stage.defer_count = nullptr; P.stage.dm_fast = nullptr; P.stage.fast_lds = 0;
  P.inv_qacc = qacc_dev; P.inv_out = qfrc_inverse_dev; P.inv_warn = warnings_dev; P.inv_flags = flags;
  HB_HIP(launch_inverse(b->D.d_dm, b->D.dm, P, stream, &b->last_kernel));
  return HB_OK;
}

int hb_inverse(hb_batch* b, const float* qacc, int flags, float* qfrc_inverse, int* warnings) {
  if (!b || !qacc || !qfrc_inverse || (flags & ~HB_INV_DISCRETE)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  const size_t n = (size_t)b->n_env * b->D.dm.nv;
  if (b->d_inv.alloc(2 * n + (size_t)b->n_env) != HB_OK) return HB_ENOMEM;
  float* d_qacc = b->d_inv;
  float* d_out = b->d_inv + n;
  int* d_warn = reinterpret_cast<int*>(b->d_inv + 2 * n);
  if (n) HB_HIP(hipMemcpyAsync(d_qacc, qacc, n * sizeof(float), hipMemcpyHostToDevice, main_stream(b)));
  const int rc = hb_inverse_dev(b, d_qacc, flags, d_out, warnings ? d_warn : nullptr);
  if (rc != HB_OK) return rc;
  if (n) HB_HIP(hipMemcpyAsync(qfrc_inverse, d_out, n * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  if (warnings) HB_HIP(hipMemcpyAsync(warnings, d_warn, (size_t)b->n_env * sizeof(int), hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

// ---- whole-body kinematics read-out (hb_kin.hip) -----------------------------------------------------------------
namespace {
int kinematics_launch(hb_batch* b, const float* qpos, const float* qvel, int qpos_stride, int qvel_stride, long long n, float* body_pose, float* body_vel,
                      float* geom_pose, hipStream_t stream) {
  KinArgs A;
  A.qpos = qpos; A.qvel = qvel; A.qpos_stride = qpos_stride; A.qvel_stride = qvel_stride; A.n = n;
  A.body_pose = body_pose; A.body_vel = body_vel; A.geom_pose = geom_pose;
  HB_HIP(launch_kinematics(b->D.d_dm, b->D.dm, A, b->tune[HB_TUNE_KIN_PACK], stream, &b->last_kernel));
  return HB_OK;
}
// host form: the outputs asked for (and qpos / qvel when given) staged in d_kin, one launch, copied back
int kinematics_host(hb_batch* b, const float* qpos, const float* qvel, long long n, float* body_pose, float* body_vel, float* geom_pose) {
  const DevModel& dm = b->D.dm;
  const size_t sn = (size_t)n;
  StageBlock blk[5] = {{body_pose ? sn * dm.nbody * 10 : 0, nullptr, body_pose}, {body_vel ? sn * dm.nbody * 6 : 0, nullptr, body_vel},
                       {geom_pose ? sn * dm.ngeom * 7 : 0, nullptr, geom_pose}, {qpos ? sn * dm.nq : 0, qpos, nullptr}, {qpos && qvel ? sn * dm.nv : 0, qvel, nullptr}};
  const hipStream_t stream = main_stream(b);  // (held step calls launched, pipes joined)
  return staged_call(b->d_kin, blk, 5, stream, [&] {
    if (qpos) return kinematics_launch(b, blk[3].dev, blk[4].dev, dm.nq, dm.nv, n, blk[0].dev, blk[1].dev, blk[2].dev, stream);
    return kinematics_launch(b, b->d_state + 1, b->d_state + 1 + dm.nq, dm.nstate, dm.nstate, n, blk[0].dev, blk[1].dev, blk[2].dev, stream);
  });
}
}  // namespace

int hb_kinematics_dev(hb_batch* b, float* body_pose_dev, float* body_vel_dev, float* geom_pose_dev) {
  if (!b || (!body_pose_dev && !body_vel_dev && !geom_pose_dev)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  const hipStream_t stream = main_stream(b);  // (held step calls launched, pipes joined: the read-out sees the state they leave)
  const DevModel& dm = b->D.dm;
  return kinematics_launch(b, b->d_state + 1, b->d_state + 1 + dm.nq, dm.nstate, dm.nstate, b->n_env, body_pose_dev, body_vel_dev, geom_pose_dev, stream);
}
int hb_kinematics(hb_batch* b, float* body_pose, float* body_vel, float* geom_pose) {
  if (!b || (!body_pose && !body_vel && !geom_pose)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  return kinematics_host(b, nullptr, nullptr, b->n_env, body_pose, body_vel, geom_pose);
}
int hb_kinematics_states_dev(hb_batch* b, const float* qpos_dev, const float* qvel_dev, int n, float* body_pose_dev, float* body_vel_dev, float* geom_pose_dev) {
  if (!b || !qpos_dev || n <= 0 || (!body_pose_dev && !body_vel_dev && !geom_pose_dev) || (body_vel_dev && !qvel_dev)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  const hipStream_t stream = main_stream(b);
  return kinematics_launch(b, qpos_dev, qvel_dev, b->D.dm.nq, b->D.dm.nv, n, body_pose_dev, body_vel_dev, geom_pose_dev, stream);
}
int hb_kinematics_states(hb_batch* b, const float* qpos, const float* qvel, int n, float* body_pose, float* body_vel, float* geom_pose) {
  if (!b || !qpos || n <= 0 || (!body_pose && !body_vel && !geom_pose) || (body_vel && !qvel)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  return kinematics_host(b, qpos, body_vel ? qvel : nullptr, n, body_pose, body_vel, geom_pose);
}

// ---- ray casting (hb_ray.hip) ----------------------------------------------------------------------------------------
int hb_ray_configure(hb_batch* b, const hb_ray_spec* spec, const float* pnt, const float* vec, int n_ray) {
  if (!b) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  // while the scan is part of the observation (hb_env_obs_extend) the rays may move, their number may not: every row is sized by it
  if (b->obs_ext.height_scan && (!spec || n_ray != b->n_ray || !(spec->cutoff > 0.f))) return HB_EINVAL;
  if (!spec || n_ray == 0) {  // remove: rays in flight (hb_rays_dev) read the buffers until the stream has run dry
    HB_HIP(hipStreamSynchronize(main_stream(b)));
    b->n_ray = 0;
    reset_all(b->d_ray, b->d_ray_kin, b->d_ray_out, b->d_ray_geoms);
    return HB_OK;
  }
  const Model& m = b->model->m;
  if (!pnt || !vec || n_ray < 1 || n_ray > kRayMax) return HB_EINVAL;
  if (spec->frame < HB_RAY_FRAME_WORLD || spec->frame > HB_RAY_FRAME_YAW || spec->frame_body < 0 || spec->frame_body >= m.nbody) return HB_EINVAL;
  if (spec->bodyexclude < -1 || spec->bodyexclude >= m.nbody) return HB_EINVAL;
  if (!(spec->flags & (HB_RAY_STATIC | HB_RAY_MOVING)) || (spec->flags & ~(HB_RAY_STATIC | HB_RAY_MOVING)) || !std::isfinite(spec->cutoff)) return HB_EINVAL;
  std::vector<float> h(6 * (size_t)n_ray);
  for (int i = 0; i < n_ray; i++) {
    const double x = vec[3 * i], y = vec[3 * i + 1], z = vec[3 * i + 2], n = std::sqrt(x * x + y * y + z * z);
    if (!std::isfinite(n) || !(n > 0) || !std::isfinite(pnt[3 * i]) || !std::isfinite(pnt[3 * i + 1]) || !std::isfinite(pnt[3 * i + 2])) return HB_EINVAL;
    for (int k = 0; k < 3; k++) { h[3 * i + k] = pnt[3 * i + k]; h[3 * (size_t)n_ray + 3 * i + k] = (float)(vec[3 * i + k] / n); }
  }
  // the eligible geoms; one whose surface has no intersection routine refuses the whole configuration (Batch.ray_configure names it)
  std::vector<int> geoms;
  bool moving = false, hfield = false;
  for (int g = 0; g < m.ngeom; g++) {
    const int body = m.geom_bodyid[g], type = m.geom_type[g];
    if (body == spec->bodyexclude || !(spec->flags & (body == 0 ? HB_RAY_STATIC : HB_RAY_MOVING))) continue;
    if (type != GEOM_PLANE && type != GEOM_HFIELD && type != GEOM_SPHERE && type != GEOM_CAPSULE && type != GEOM_BOX) {
      if (!m.geom_contype[g] && !m.geom_conaffinity[g]) continue;  // (a visual marker: it collides with nothing, and no ray sees it)
      return HB_EUNSUPPORTED;
    }
    geoms.push_back(g);
    moving |= body != 0; hfield |= type == GEOM_HFIELD;
  }
  // from here on the previous configuration is replaced: nothing of it may still be in use
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  b->n_ray = 0;
  const size_t nkin = spec->frame != HB_RAY_FRAME_WORLD || moving ? (size_t)b->n_env * ((size_t)m.nbody * 10 + (size_t)m.ngeom * 7) : 0;
  if (b->d_ray.reserve(h.size()) != HB_OK || b->d_ray_geoms.reserve(geoms.size() + 1) != HB_OK || (nkin && b->d_ray_kin.reserve(nkin) != HB_OK)) return HB_ENOMEM;
  HB_HIP(hipMemcpy(b->d_ray, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  if (!geoms.empty()) HB_HIP(hipMemcpy(b->d_ray_geoms, geoms.data(), geoms.size() * sizeof(int), hipMemcpyHostToDevice));
  b->ray_spec = *spec; b->ray_ngeom = (int)geoms.size(); b->ray_moving = moving; b->ray_hfield = hfield;
  b->n_ray = n_ray;
  return HB_OK;
}
// the poses the installed rays need and the ray kernel, on the batch's stream: A's outputs (and mask, transform) are the caller's
static int rays_launch(hb_batch* b, RayArgs A) {
  const hipStream_t stream = main_stream(b);  // (held step calls launched, pipes joined: the rays see the state they leave)
  const DevModel& dm = b->D.dm;
  const bool framed = b->ray_spec.frame != HB_RAY_FRAME_WORLD;
  float* d_body = b->d_ray_kin;
  float* d_geom = d_body ? d_body + (size_t)b->n_env * dm.nbody * 10 : nullptr;
  if (framed || b->ray_moving) {  // the poses the rays need, by the kinematics read-out's own launch; world-frame rays at static geoms need none
    const int rc = kinematics_launch(b, b->d_state + 1, b->d_state + 1 + dm.nq, dm.nstate, dm.nstate, b->n_env, framed ? d_body : nullptr, nullptr,
                                     b->ray_moving ? d_geom : nullptr, stream);
    if (rc != HB_OK) return rc;
  }
  A.pnt = b->d_ray; A.vec = b->d_ray + 3 * (size_t)b->n_ray; A.geoms = b->d_ray_geoms;
  A.n_ray = b->n_ray; A.n_geom = b->ray_ngeom; A.n_env = b->n_env;
  A.frame = b->ray_spec.frame; A.frame_body = b->ray_spec.frame_body; A.cutoff = b->ray_spec.cutoff;
  A.body_pose = framed ? d_body : nullptr; A.geom_pose = b->ray_moving ? d_geom : nullptr;
  A.dr = b->d_dr; A.dr_stride = b->dr_stride; A.has_hfield = b->ray_hfield ? 1 : 0;
  HB_HIP(launch_rays(b->D.d_dm, dm, A, stream, &b->last_kernel));
  return HB_OK;
}
int hb_rays_dev(hb_batch* b, float* dist_dev, int* geomid_dev) {
  if (!b || (!dist_dev && !geomid_dev) || b->n_ray < 1) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  RayArgs A;
  memset(&A, 0, sizeof A);
  A.dist = dist_dev; A.geomid = geomid_dev;
  return rays_launch(b, A);
}
extern "C++" {
namespace hb {
int rays_scan_launch(hb_batch* b, const uint8_t* mask, float* rows) {
  if (b->n_ray < 1 || !b->obs_ext.height_scan) return HB_EINVAL;
  RayArgs A;
  memset(&A, 0, sizeof A);
  A.dist = rows ? rows : b->d_ext_scan.get(); A.env_mask = mask;
  A.xform = 1; A.out_stride = rows ? b->row.width : b->n_ray; A.out_col = rows ? b->row.scan : 0;
  A.x_offset = b->obs_ext.scan_offset; A.x_scale = b->obs_ext.scan_scale; A.x_lo = b->obs_ext.scan_lo; A.x_hi = b->obs_ext.scan_hi;
  const char* name = b->last_kernel;  // (hb_last_kernel goes on naming the step kernel of the env step this is part of)
  const int rc = rays_launch(b, A);
  b->last_kernel = name;
  return rc;
}
}  // namespace hb
}  // extern "C++"
int hb_rays(hb_batch* b, float* dist, int* geomid) {
  if (!b || (!dist && !geomid) || b->n_ray < 1) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  const size_t n = (size_t)b->n_env * b->n_ray;
  const hipStream_t stream = main_stream(b);  // (d_ray_out is idle: the host form before this one ended synchronised)
  if (b->d_ray_out.reserve(2 * n) != HB_OK) return HB_ENOMEM;
  float* d_dist = b->d_ray_out;
  int* d_id = reinterpret_cast<int*>(d_dist + n);
  const int rc = hb_rays_dev(b, dist ? d_dist : nullptr, geomid ? d_id : nullptr);
  if (rc != HB_OK) return rc;
  if (dist) HB_HIP(hipMemcpyAsync(dist, d_dist, n * sizeof(float), hipMemcpyDeviceToHost, stream));
  if (geomid) HB_HIP(hipMemcpyAsync(geomid, d_id, n * sizeof(int), hipMemcpyDeviceToHost, stream));
  HB_HIP(hipStreamSynchronize(stream));
  return HB_OK;
}

int hb_get_status(hb_batch* b, int* status) {
  if (!b || !status) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  HB_HIP(hipMemcpy(status, b->d_status, (size_t)b->n_env * sizeof(int), hipMemcpyDeviceToHost));
  return HB_OK;
}

int hb_get_counts(hb_batch* b, int* ncon, int* nefc, int* niter) {
  if (!b) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  std::vector<int> h((size_t)b->n_env * kCountStride);
  HB_HIP(hipMemcpy(h.data(), b->d_counts, h.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int e = 0; e < b->n_env; e++) {
    if (ncon) ncon[e] = h[kCountStride * e];
    if (nefc) nefc[e] = h[kCountStride * e + 1];
    if (niter) niter[e] = h[kCountStride * e + 2];
  }
  return HB_OK;
}

int hb_get_collision_counts(hb_batch* b, int* nwork, int* nsearch, int* kcycles) {
  if (!b) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  std::vector<int> h((size_t)b->n_env * kCountStride);
  HB_HIP(hipMemcpy(h.data(), b->d_counts, h.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int e = 0; e < b->n_env; e++) {
    if (nwork) nwork[e] = h[kCountStride * e + 5];
    if (nsearch) nsearch[e] = h[kCountStride * e + 6];
    if (kcycles) kcycles[e] = h[kCountStride * e + 7];
  }
  return HB_OK;
}

const char* hb_last_kernel(hb_batch* b) {
  if (!b) return "";
  if (b->fold_n && flush_steps(b) != HB_OK) b->join_error = 1;  // (step calls held back: launched now, so that the name is theirs)
  return b->last_kernel;
}
long long hb_batch_step_launches(hb_batch* b) {
  if (!b) return HB_EINVAL;
  if (b->fold_n && flush_steps(b) != HB_OK) b->join_error = 1;
  return b->launch_count;
}
int hb_batch_device_name(const hb_batch* b, char* out, int cap) {
  if (!b || !out || cap < 2) return HB_EINVAL;
  hipDeviceProp_t prop;
  HB_HIP(hipGetDeviceProperties(&prop, b->device));
  snprintf(out, (size_t)cap, "%s (%s, %d CUs) #%d", prop.name, prop.gcnArchName, prop.multiProcessorCount, b->device);
  return HB_OK;
}
int hb_batch_tune(hb_batch* b, int knob, int value) {
  if (!b || knob < 0 || knob >= HB_TUNE_COUNT || value < 0) return HB_EINVAL;
  if (knob == HB_TUNE_DUO && value > 2) return HB_EINVAL;
  if (knob == HB_TUNE_FOLD && (value < 1 || value > kFoldMax)) return HB_EINVAL;
  if (knob == HB_TUNE_KIN_PACK && value > 1) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  (void)main_stream(b);  // the choice holds from the next launch on: whatever is in flight on the segments' streams is joined first
  b->tune[knob] = value;
  if (knob == HB_TUNE_SCHEDULE) { b->schedule = value != 0; b->order_mode = 0; }
  if (knob == HB_TUNE_STAGED || knob == HB_TUNE_FASTPASS) b->order_mode = 0;
  return HB_OK;
}

int hb_diag_enable(hb_batch* b, int on) {
  if (!b) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  const size_t n = b->n_env;
  if (on && (b->d_diag_qacc.alloc(n * b->D.dm.nv) != HB_OK || b->d_diag_force.alloc(n * b->D.dm.nefc_max) != HB_OK ||
             b->d_diag_contact.alloc(n * b->D.dm.ncon_max * kDiagConStride) != HB_OK)) {
    reset_all(b->d_diag_qacc, b->d_diag_force, b->d_diag_contact);
    return HB_ENOMEM;
  }
  b->diag = on != 0;
  return HB_OK;
}

int hb_contact_readout(hb_batch* b, int on) {
  refuse_clear();
  if (!b) return refuse_with("hb_contact_readout: NULL batch");
  HB_HIP(hipSetDevice(b->device));
  if (!on && b->d_feet) return refuse_with("hb_contact_readout: the installed foot-contact terms (hb_env_feet_configure) read it");
  (void)main_stream(b);  // from the next launch on: step calls held back are launched as they were made
  if (on && alloc_contact_readout(b) != HB_OK) return HB_ENOMEM;
  b->contact_readout = on != 0;
  return HB_OK;
}
static int contact_out(hb_batch* b, float* out, const float* dev, size_t n) {
  if (!b || !out || !b->contact_readout || !dev) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  HB_HIP(hipMemcpy(out, dev, n * sizeof(float), hipMemcpyDeviceToHost));
  return HB_OK;
}
int hb_get_contact_force(hb_batch* b, float* out) { return contact_out(b, out, b ? b->d_contact_force.get() : nullptr, b ? (size_t)b->n_env * b->D.dm.ncon_max * 6 : 0); }
int hb_get_body_contact(hb_batch* b, float* out) { return contact_out(b, out, b ? b->d_body_contact.get() : nullptr, b ? (size_t)b->n_env * b->D.dm.nbody * 6 : 0); }
int hb_contact_readout_dev(hb_batch* b, const float** contact_force_dev, const float** body_contact_dev) {
  if (!b || !b->contact_readout) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  (void)main_stream(b);  // (joins like hb_batch_stream: work enqueued on the batch's stream from here on follows every step call made so far)
  if (contact_force_dev) *contact_force_dev = b->d_contact_force;
  if (body_contact_dev) *body_contact_dev = b->d_body_contact;
  return HB_OK;
}

int hb_body_acc_readout(hb_batch* b, int on) {
  if (!b) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  if (on && (b->D.dm.nfric || b->D.dm.neq_rows)) return HB_EUNSUPPORTED;  // (a model with friction loss or equality rows: no step kernel has both those rows and this read-out)
  (void)main_stream(b);  // from the next launch on: step calls held back are launched as they were made
  if (on && alloc_body_acc_readout(b) != HB_OK) return HB_ENOMEM;
  b->body_acc_readout = on != 0;
  return HB_OK;
}
int hb_get_body_acc(hb_batch* b, float* out) {
  if (!b || !out || !b->body_acc_readout || !b->d_body_acc.get()) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  HB_HIP(hipMemcpy(out, b->d_body_acc.get(), (size_t)b->n_env * b->D.dm.nbody * 6 * sizeof(float), hipMemcpyDeviceToHost));
  return HB_OK;
}
int hb_body_acc_readout_dev(hb_batch* b, const float** body_acc_dev) {
  if (!b || !b->body_acc_readout) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  (void)main_stream(b);  // (joins like hb_batch_stream)
  if (body_acc_dev) *body_acc_dev = b->d_body_acc;
  return HB_OK;
}

static int copy_out(hb_batch* b, float* out, const float* dev, size_t n) {
  if (!b || !out) return HB_EINVAL;
  if (!b->diag || !dev) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  HB_HIP(hipMemcpy(out, dev, n * sizeof(float), hipMemcpyDeviceToHost));
  return HB_OK;
}
int hb_get_qacc(hb_batch* b, float* qacc) { return copy_out(b, qacc, b ? b->d_diag_qacc.get() : nullptr, b ? (size_t)b->n_env * b->D.dm.nv : 0); }
int hb_get_efc_force(hb_batch* b, float* f) { return copy_out(b, f, b ? b->d_diag_force.get() : nullptr, b ? (size_t)b->n_env * b->D.dm.nefc_max : 0); }
int hb_get_contacts(hb_batch* b, float* c) { return copy_out(b, c, b ? b->d_diag_contact.get() : nullptr, b ? (size_t)b->n_env * b->D.dm.ncon_max * kDiagConStride : 0); }

void* hb_dev_alloc(hb_batch* b, uint64_t bytes) {
  if (!b || hipSetDevice(b->device) != hipSuccess) return nullptr;
  void* p = nullptr;
  if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
  return p;
}
void hb_dev_free(hb_batch* b, void* p) {
  if (!b || !p) return;
  HB_IGN(hipSetDevice(b->device));
  HB_IGN(hipStreamSynchronize(main_stream(b)));  // (step calls held back, fold_steps, may read the buffer: launched and waited for)
  HB_IGN(hipFree(p));
}
void* hb_host_alloc(uint64_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}
void hb_host_free(void* p) { if (p) HB_IGN(hipHostFree(p)); }
int hb_memcpy_h2d(hb_batch* b, void* dst_dev, const void* src, uint64_t bytes) {
  if (!b || !dst_dev || !src) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}
int hb_memcpy_d2h(hb_batch* b, void* dst, const void* src_dev, uint64_t bytes) {
  if (!b || !dst || !src_dev) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}
int hb_get_stamps(hb_batch* b, unsigned long long* out) {
#ifdef HB_STAMPS
  if (!b || !out) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  if (!b->d_stamps) return b->d_stamps.alloc((size_t)b->n_env * 16, /*zero=*/true);  // first call arms the stamps; call again after a step to read them
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  HB_HIP(hipMemcpy(out, b->d_stamps, (size_t)b->n_env * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return HB_OK;
#else
  (void)b; (void)out;
  return HB_EUNSUPPORTED;
#endif
}
int hb_step_timing(hb_batch* b, int enable) {
  if (!b) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  if (enable && b->tev.empty()) {
    b->tev.resize(512);
    for (auto& e : b->tev) HB_HIP(hipEventCreate(&e));
  }
  b->time_steps = enable != 0;
  b->tev_used = 0;
  return HB_OK;
}
int hb_step_timing_read(hb_batch* b, float* mean_us, int* samples) {
  if (!b || !mean_us) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  double tot = 0;
  int n = 0;
  for (int i = 0; i + 1 < b->tev_used; i += 2) {
    float ms = 0;
    HB_HIP(hipEventElapsedTime(&ms, b->tev[i], b->tev[i + 1]));
    tot += ms; n++;
  }
  *mean_us = n ? (float)(1e3 * tot / n) : 0.f;
  if (samples) *samples = n;
  b->tev_used = 0;
  return HB_OK;
}
int hb_timer_start(hb_batch* b) {
  if (!b) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  if (!b->ev0) { HB_HIP(hipEventCreate(&b->ev0)); HB_HIP(hipEventCreate(&b->ev1)); }
  HB_HIP(hipEventRecord(b->ev0, main_stream(b)));
  return HB_OK;
}
int hb_timer_stop(hb_batch* b, float* elapsed_ms) {
  if (!b || !elapsed_ms || !b->ev0) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipEventRecord(b->ev1, main_stream(b)));
  HB_HIP(hipEventSynchronize(b->ev1));
  HB_HIP(hipEventElapsedTime(elapsed_ms, b->ev0, b->ev1));
  return HB_OK;
}

}  // extern "C"
