// hb_batch.cpp — the launch plumbing behind the C-ABI (hb_batch.hpp): the upload of the device model tables (hb_tables.cpp builds them),
// the step launches with their pipes, segments and folded step calls, and the state I/O.  launch_steps and everything it calls is in
// this one file.
#include "hb_batch.hpp"
#include "hb_tables.hpp"

namespace hb {

// The model's tables onto the device: hb_tables.cpp builds them (and refuses what this build cannot run), this uploads the three flat
// arrays, points every pointer field of the DevModel into them, and uploads the qpos sources and the DevModel itself - for variants 2 / 3
// also the fast one: the same model, so the same pointers, with the variant-1 layout.
bool build_device_model(const Model& m, DeviceModel& D, std::string& err) {
  HostTables H;
  if (!build_model_tables(m, H, err)) return false;
  DevModel& dm = D.dm;
  dm = H.dm;
  if (D.d_int.alloc(H.iv.size()) != HB_OK || D.d_flt.alloc(H.fv.size()) != HB_OK || D.d_u64.alloc(H.uv.size()) != HB_OK) { err = "hipMalloc failed for model tables"; return false; }
  if (hipMemcpy(D.d_int, H.iv.data(), H.iv.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(D.d_flt, H.fv.data(), H.fv.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(D.d_u64, H.uv.data(), H.uv.size() * sizeof(unsigned long long), hipMemcpyHostToDevice) != hipSuccess) { err = "hipMemcpy failed for model tables"; return false; }
  for (const TableFixup& x : H.fix) {
    const void* p = x.array == kTabInt ? (const void*)(D.d_int + x.off) : x.array == kTabFloat ? (const void*)(D.d_flt + x.off) : (const void*)(D.d_u64 + x.off);
    memcpy((char*)&dm + x.field, &p, sizeof p);
  }
  D.obs_jnt_joint = dm.obs_jnt; D.obs_src_joint = dm.obs_src;
  D.obs_jnt_act = D.d_int + H.o_obs_jnt_act; D.obs_src_act = D.d_int + H.o_obs_src_act;
  D.has_act_order = H.has_act_order;
  if (D.d_qpos_src.alloc(H.qsrc.size()) != HB_OK ||
      hipMemcpy(D.d_qpos_src, H.qsrc.data(), H.qsrc.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { err = "hipMalloc failed for qpos sources"; return false; }
  if (D.d_dm.alloc(1) != HB_OK || hipMemcpy(D.d_dm, &dm, sizeof(DevModel), hipMemcpyHostToDevice) != hipSuccess) { err = "hipMalloc failed for the device model"; return false; }
  D.sized_h27 = H.sized_h27; D.sized_team = H.sized_team; D.fast_lds_floats = H.fast_lds_floats;
  if (H.fast_lds_floats) {
    DevModel fm = dm;
    fm.variant = 1; fm.ncon_max = kNconMax; fm.nefc_max = kNefcMax;
    set_layout(fm, H.fast_lay);
    if (D.d_dm_fast.alloc(1) != HB_OK || hipMemcpy(D.d_dm_fast, &fm, sizeof(DevModel), hipMemcpyHostToDevice) != hipSuccess) { err = "hipMalloc failed for the device model"; return false; }
  }
  return true;
}

int ensure_ctrl(hb_batch* b, size_t floats) {
  if (floats > b->d_ctrl.capacity()) b->tape_steps = 0;  // a regrown control buffer no longer holds a spline tape
  return b->d_ctrl.reserve(floats);
}

// the staged step's buffers as this launch sees them (HB_TUNE_STAGED / FASTPASS / NARROW_PRIM switch parts of it off: all null = the fused step)
static StageBufs staged(const hb_batch* b) {
  StageBufs sb = b->stage;
  if (!b->tune[HB_TUNE_STAGED]) { sb = StageBufs{}; return sb; }
  if (!b->tune[HB_TUNE_FASTPASS]) { sb.defer = nullptr; sb.defer_list = nullptr; sb.defer_count = nullptr; sb.dm_fast = nullptr; sb.fast_lds = 0; }
  if (!b->tune[HB_TUNE_NARROW_PRIM]) sb.no_mesh = 0;
  return sb;
}
bool staged_on(const hb_batch* b) { return b->stage.result && b->tune[HB_TUNE_STAGED]; }

BatchPtrs make_ptrs(hb_batch* b) {
  BatchPtrs P;
  memset(&P, 0, sizeof P);
  P.state = b->d_state; P.status = b->d_status; P.counts = b->d_counts; P.xfrc = b->d_xfrc; P.qfrc_out = b->d_qfrc;
  if (b->diag) { P.diag_qacc = b->d_diag_qacc; P.diag_force = b->d_diag_force; P.diag_contact = b->d_diag_contact; }
  if (b->contact_readout) { P.contact_force = b->d_contact_force; P.body_contact = b->d_body_contact; }
  P.cfrc_ncon = b->D.dm.ncon_max;
  if (b->body_acc_readout) { P.body_acc = b->d_body_acc; P.body_acc_park = b->d_body_acc_park; }
  P.n_env = b->n_env;
  P.integrate = 1;
  if (b->schedule && b->order_mode) { P.order = b->d_order; P.order2 = staged_on(b) ? b->d_order2.get() : nullptr; }
  P.blk0 = 0; P.nblk = b->n_env;
  P.dr = b->d_dr; P.dr_stride = b->dr_stride;
  P.stamps = b->d_stamps;
#ifdef HB_STAMPS
  if (const char* sp = getenv("HB_STOP_PHASE")) P.stop_phase = atoi(sp);
#endif
  P.stage = staged(b);
  P.duo = b->tune[HB_TUNE_DUO];
  const bool sized_on = b->tune[HB_TUNE_SIZED] != 0;
  P.lean_ok = (b->D.dm.disableflags == 0 && b->tune[HB_TUNE_LEAN] ? 1 : 0) | (b->D.sized_h27 && sized_on ? 2 : 0) | (b->D.sized_team && sized_on ? 4 : 0);
  if (b->diag) P.stage.dm_fast = nullptr;  // the diagnostic buffers are laid out for the kernel of the model's own variant
  if (b->xfrc_std > 0.f && b->d_xfrc) {
    const double rate = b->xfrc_rate > 0.f ? std::exp(-b->model->m.timestep / b->xfrc_rate) : 0.0;  // trajectory.cc:149-150
    P.xfrc_rate = (float)rate; P.xfrc_scale = (float)(b->xfrc_std * std::sqrt(1.0 - rate * rate));
    P.xfrc_seed = b->xfrc_seed; P.xfrc_call = b->xfrc_calls++;
  }
  return P;
}


// order `stream` behind every pipe (no-op unless steps are in flight on the pipes)
void join_pipes(hb_batch* b) {
  if (b->forked) b->main_dirty = true;  // the batch's stream now carries the join: the next fork must carry it to the pipes
  if (!b->forked) return;
  for (int c = 0; c < b->npipe; c++) {
    if (hipEventRecord(b->ev_pipe[c], b->pipe[c]) != hipSuccess || hipStreamWaitEvent(b->stream, b->ev_pipe[c], 0) != hipSuccess) b->join_error = 1;
  }
  b->forked = false;
}
// the batch's stream, ordered behind all enqueued steps: every use of the stream outside launch_steps goes through here
hipStream_t main_stream(hb_batch* b) {
  if (b->fold_n && flush_steps(b) != HB_OK) b->join_error = 1;  // (hb_batch_sync reports it)
  join_pipes(b);
  b->main_dirty = true;  // the caller is about to enqueue something the next step's launches must follow
  return b->stream;
}

// heavy-first re-sort every N-th step call (HB_REORDER_PERIOD overrides, for experiments)
int reorder_period(const hb_batch* b) { return b->tune[HB_TUNE_REORDER_PERIOD] < 1 ? 1 : b->tune[HB_TUNE_REORDER_PERIOD]; }
// number of segments the next step call is cut into (1: one launch on the batch's stream)
int segment_count(const hb_batch* b) { return (b->npipe > 1 && !b->time_steps && b->n_env >= 64 * b->npipe) ? b->npipe : 1; }
Segment segment(hb_batch* b, int c, int nseg) {
  if (nseg == 1) return {0, b->n_env, b->stream};
  return {(int)((long long)b->n_env * c / nseg), (int)((long long)b->n_env * (c + 1) / nseg), b->pipe[c]};
}
// fork: the pipes see everything enqueued on the batch's stream so far (controls written there, resets, ...)
int fork_pipes(hb_batch* b, int nseg) {
  // (step calls held back - fold_steps - come first whoever launches next; flush_steps itself gets here with nothing held any more)
  if (b->fold_n) { const int rc = flush_steps(b); if (rc != HB_OK) return rc; }
  if (nseg == 1) { join_pipes(b); return HB_OK; }
  // (nothing enqueued on the batch's stream since the last fork: the pipes already follow all of it, and a marker on a stream that
  // shares a hardware queue with a busy one would wait behind that one's work)
  if (b->main_dirty) {
    HB_HIP(hipEventRecord(b->ev_fork, b->stream));
    for (int c = 0; c < nseg; c++) HB_HIP(hipStreamWaitEvent(b->pipe[c], b->ev_fork, 0));
    b->main_dirty = false;
  }
  b->forked = true;
  return HB_OK;
}
// the batch's model through launch_step; the launched kernel's name stays with the batch (hb_last_kernel)
hipError_t launch_batch_step(hb_batch* b, const BatchPtrs& P, int nsteps, hipStream_t stream) {
  return launch_step(b->D.d_dm, b->D.dm, P, nsteps, stream, &b->last_kernel);
}
// one segment's launch of the step kernel, then (heavy-first scheduling, every 4th call) the tiny kernel that
// orders the segment's next launch by the cost of this one; costs change slowly, and the sort sits on the
// critical path of its stream
int launch_segment(hb_batch* b, BatchPtrs P, int nsteps, const Segment& sg, int nseg, bool reorder) {
  P.blk0 = sg.lo; P.nblk = sg.hi - sg.lo;
  // a whole-batch permutation would mix segments: a segment only uses the order of its own envs
  P.order = (b->schedule && (nseg == 1 ? b->order_mode != 0 : b->order_mode == 2)) ? b->d_order.get() : nullptr;
  P.order2 = (P.order && staged_on(b)) ? b->d_order2.get() : nullptr;
  HB_HIP(launch_batch_step(b, P, nsteps, sg.st));
  // (the key of the counting sort is 8 bits of the cost: of a single step's rows x sweeps - up to ~ 1600 - the bits above the lowest three; of the
  // AVERAGE over a launch of several steps, which the two-envs-per-wave kernel leaves behind and pairs its envs by - 180 .. 700 -, one bit more)
  if (reorder) HB_HIP(launch_order(b->d_counts, b->d_order, b->n_env, sg.lo, sg.hi - sg.lo, sg.st, /*slot=*/3, /*shift=*/(nsteps >= 8 && b->D.dm.variant == 0) ? 2 : 3));
  if (reorder && staged_on(b)) HB_HIP(launch_order(b->d_counts, b->d_order2, b->n_env, sg.lo, sg.hi - sg.lo, sg.st, /*slot=*/7, /*shift=*/0));
  return HB_OK;
}
// `refreshed`: the launch rewrote the permutations itself (launch_step's in-rollout refresh of a staged multi-step launch sorts the slots
// of each launch: the whole batch when there is one segment, each segment's own envs otherwise)
void steps_enqueued(hb_batch* b, int nseg, bool reorder, bool refreshed) {
  if (reorder || refreshed) b->order_mode = nseg == 1 ? 1 : 2;
  b->launch_count++;
}

static int launch_steps_now(hb_batch* b, BatchPtrs& P, int nsteps, int ncalls = 1) {
  // a launch of several steps has no batch-wide barrier between its steps: nothing for segments to overlap, and three launches that each
  // bring their own rounds of waves fill the chip worse than one (4096 envs, 64 steps: 103 us per step against 71, profiles/r04_fold_sizes.txt)
  const int nseg = (b->D.dm.variant == 0 && nsteps >= 5) ? 1 : segment_count(b);
  const bool sample = nseg == 1 && b->time_steps && (b->launch_count % 8 == 0) && b->tev_used + 2 <= (int)b->tev.size();
  // (a launch of several steps is followed by its re-sort every time: it pairs its envs by the order, and one sort is nothing beside it)
  const bool reorder = b->schedule && (ncalls >= reorder_period(b) || nsteps >= 8 || b->launch_count % reorder_period(b) == 0);
  int rc = fork_pipes(b, nseg);
  if (rc != HB_OK) return rc;
  if (sample) HB_HIP(hipEventRecord(b->tev[b->tev_used], b->stream));
  for (int c = 0; c < nseg; c++) {
    rc = launch_segment(b, P, nsteps, segment(b, c, nseg), nseg, reorder);
    if (rc != HB_OK) return rc;
  }
  if (sample) { HB_HIP(hipEventRecord(b->tev[b->tev_used + 1], b->stream)); b->tev_used += 2; }
  // (the condition of launch_step's refresh: staged, ordered, at least one (t & 7) == 7 with a step behind it)
  const bool refreshed = staged_on(b) && b->D.dm.variant != 0 && b->schedule && nsteps > 8 && (nseg == 1 ? b->order_mode != 0 : b->order_mode == 2);
  steps_enqueued(b, nseg, reorder, refreshed);
  return HB_OK;
}

// Step calls enqueued back to back run as ONE launch.  hb_step_dev is asynchronous: until the caller synchronises, reads something or
// enqueues other work (all of which pass main_stream), nobody can tell K launches of one step from one launch of K steps - except the clock:
// a launch of one step lasts as long as its slowest env and the next one waits for it, a launch of K steps lets every wave run on into
// its envs' next step (the rollout kernels: no batch-wide barrier).  That pays when the launch's waves are all on the chip at once
// (hb_step.hip: fold_pays - up to 2048 envs, 4096 for the models with the two-envs-per-wave kernel).  Such a step call is held back (its
// launch parameters and its control pointer) until one
// of: kFoldMax steps are held, a call with other parameters arrives, anything touches the batch's stream.  The held calls then run as
// one multi-step launch whose step t reads the controls of call t (BatchPtrs::ctrl_tab, ctrl_mode 3).  Results are bit-identical to
// the unfolded launches (tests/test_gpu_fold.py); HB_TUNE_FOLD = 1 switches it off.
// Only for a PIPELINED batch: its caller has already taken on the one obligation this adds - hb_batch_join (or fetching the stream again)
// before enqueueing work of its own on the batch's stream behind step calls (include/hb.h: hb_batch_pipeline).  An unpipelined batch
// keeps its plain stream semantics: every call is launched when it is made.
int flush_steps(hb_batch* b) {
  if (!b->fold_n) return HB_OK;
  BatchPtrs P = b->fold_P;
  const int n = b->fold_n;
  b->fold_n = 0;  // (first: the launch below passes fork_pipes / join_pipes, never main_stream, but nothing may re-enter with steps held)
  HB_HIP(hipSetDevice(b->device));
  bool same = true;
  for (int t = 1; t < n; t++) same = same && b->fold_ctrl[t] == b->fold_ctrl[0];
  if (same) { P.ctrl = b->fold_ctrl[0]; P.ctrl_mode = 0; }  // (one call, with or without substeps: exactly the launch it always was)
  else { P.ctrl = nullptr; P.ctrl_mode = 3; for (int t = 0; t < n; t++) P.ctrl_tab[t] = b->fold_ctrl[t]; }
  return launch_steps_now(b, P, n, n);
}
int launch_steps(hb_batch* b, BatchPtrs& P, int nsteps, bool foldable) {
  const int cap = std::min(b->tune[HB_TUNE_FOLD], kFoldMax);
#ifdef HB_STAMPS
  foldable = false;  // (the diagnostic build samples single launches)
#endif
  foldable = foldable && b->npipe > 1 && cap > 1 && nsteps <= cap && P.ctrl_mode == 0 && !b->time_steps && !b->diag && !P.stamps && P.xfrc_scale == 0.f &&
             fold_pays(b->D.dm, P);
  if (!foldable) {
    const int rc = flush_steps(b);
    return rc != HB_OK ? rc : launch_steps_now(b, P, nsteps);
  }
  BatchPtrs key = P;
  key.ctrl = nullptr;
  if (b->fold_n && (memcmp(&key, &b->fold_P, sizeof key) != 0 || b->fold_n + nsteps > cap)) {
    const int rc = flush_steps(b);
    if (rc != HB_OK) return rc;
  }
  if (!b->fold_n) b->fold_P = key;
  for (int t = 0; t < nsteps; t++) b->fold_ctrl[b->fold_n++] = P.ctrl;
  return b->fold_n >= cap ? flush_steps(b) : HB_OK;
}

// hb_rollout*'s shared opening: the control tape of T steps on the device, and room for the qpos trace when the caller wants one
int rollout_open(hb_batch* b, const float* ctrl, int T, bool want_qpos) {
  const size_t n = (size_t)T * b->n_env * b->D.dm.nu;
  const int rc = ensure_ctrl(b, std::max<size_t>(n, 1));
  if (rc != HB_OK) return rc;
  if (n) HB_HIP(hipMemcpyAsync(ctrl_for_write(b), ctrl, n * sizeof(float), hipMemcpyHostToDevice, main_stream(b)));
  return want_qpos ? b->d_qpos_out.reserve((size_t)T * b->n_env * b->D.dm.nq) : HB_OK;
}
// the batch's xfrc_applied exists, and was zeroed when it was created
int ensure_xfrc(hb_batch* b) { return b->d_xfrc.alloc((size_t)b->n_env * 6 * b->D.dm.nbody, /*zero=*/true); }
// the two buffers of the contact-force read-out: both there or neither
int alloc_contact_readout(hb_batch* b) {
  const size_t n = b->n_env;
  if (b->d_contact_force.alloc(n * b->D.dm.ncon_max * 6, true) != HB_OK || b->d_body_contact.alloc(n * b->D.dm.nbody * 6, true) != HB_OK) {
    reset_all(b->d_contact_force, b->d_body_contact);
    return HB_ENOMEM;
  }
  return HB_OK;
}

// the read-out and the scratch of the body-acceleration read-out: both there or neither
int alloc_body_acc_readout(hb_batch* b) {
  const size_t n = (size_t)b->n_env * b->D.dm.nbody;
  if (b->d_body_acc.alloc(n * 6, true) != HB_OK || b->d_body_acc_park.alloc(n * kAccPark, true) != HB_OK) {
    reset_all(b->d_body_acc, b->d_body_acc_park);
    return HB_ENOMEM;
  }
  return HB_OK;
}

int reset_impl(hb_batch* b, const uint8_t* mask, int keyframe, float perturb_scale, int env_offset) {
  if (!b) return HB_EINVAL;
  const Model& m = b->model->m;
  if (keyframe >= m.nkey) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  const uint8_t* dmask = nullptr;
  if (mask) {
    if (b->d_mask.alloc(b->n_env) != HB_OK) return HB_ENOMEM;
    HB_HIP(hipMemcpyAsync(b->d_mask, mask, b->n_env, hipMemcpyHostToDevice, main_stream(b)));
    dmask = b->d_mask;
  }
  b->env_offset = env_offset;
  const float* src = b->D.d_qpos_src + (keyframe < 0 ? 0 : (size_t)(1 + keyframe) * m.nq);
  HB_HIP(launch_reset(b->D.dm, b->d_state, b->d_status, dmask, src, nullptr, b->n_env, perturb_scale, env_offset, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

static int spec_size(const Model& m, unsigned spec) {
  int n = 0;
  if (spec & HB_STATE_TIME) n += 1;
  if (spec & HB_STATE_QPOS) n += m.nq;
  if (spec & HB_STATE_QVEL) n += m.nv;
  if (spec & HB_STATE_WARMSTART) n += m.nv;
  if (spec & HB_STATE_XFRC_APPLIED) n += 6 * m.nbody;
  return n;
}
static const unsigned kSupportedSpec = HB_STATE_TIME | HB_STATE_QPOS | HB_STATE_QVEL | HB_STATE_WARMSTART | HB_STATE_XFRC_APPLIED;

template <class T>
int get_state_impl(hb_batch* b, unsigned spec, T* out) {
  if (!b || !out || (spec & ~kSupportedSpec) || !spec) return HB_EINVAL;
  const Model& m = b->model->m;
  int ns = b->D.dm.nstate, n = b->n_env, w = spec_size(m, spec);
  std::vector<float> host((size_t)n * ns), xf;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  HB_HIP(hipMemcpy(host.data(), b->d_state, host.size() * sizeof(float), hipMemcpyDeviceToHost));
  if (spec & HB_STATE_XFRC_APPLIED) {
    xf.assign((size_t)n * 6 * m.nbody, 0.f);
    if (b->d_xfrc) HB_HIP(hipMemcpy(xf.data(), b->d_xfrc, xf.size() * sizeof(float), hipMemcpyDeviceToHost));
  }
  for (int e = 0; e < n; e++) {
    const float* s = &host[(size_t)e * ns];
    T* o = out + (size_t)e * w;
    if (spec & HB_STATE_TIME) *o++ = (T)s[0];
    if (spec & HB_STATE_QPOS) for (int i = 0; i < m.nq; i++) *o++ = (T)s[1 + i];
    if (spec & HB_STATE_QVEL) for (int i = 0; i < m.nv; i++) *o++ = (T)s[1 + m.nq + i];
    if (spec & HB_STATE_WARMSTART) for (int i = 0; i < m.nv; i++) *o++ = (T)s[1 + m.nq + m.nv + i];
    if (spec & HB_STATE_XFRC_APPLIED) for (int i = 0; i < 6 * m.nbody; i++) *o++ = (T)xf[(size_t)e * 6 * m.nbody + i];
  }
  return HB_OK;
}

template <class T>
int set_state_impl(hb_batch* b, unsigned spec, const T* in) {
  if (!b || !in || (spec & ~kSupportedSpec) || !spec) return HB_EINVAL;
  const Model& m = b->model->m;
  int ns = b->D.dm.nstate, n = b->n_env, w = spec_size(m, spec);
  std::vector<float> host((size_t)n * ns);
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  HB_HIP(hipMemcpy(host.data(), b->d_state, host.size() * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<float> xf;
  if (spec & HB_STATE_XFRC_APPLIED) xf.assign((size_t)n * 6 * m.nbody, 0.f);
  for (int e = 0; e < n; e++) {
    float* s = &host[(size_t)e * ns];
    const T* o = in + (size_t)e * w;
    if (spec & HB_STATE_TIME) s[0] = (float)*o++;
    if (spec & HB_STATE_QPOS) for (int i = 0; i < m.nq; i++) s[1 + i] = (float)*o++;
    if (spec & HB_STATE_QVEL) for (int i = 0; i < m.nv; i++) s[1 + m.nq + i] = (float)*o++;
    if (spec & HB_STATE_WARMSTART) for (int i = 0; i < m.nv; i++) s[1 + m.nq + m.nv + i] = (float)*o++;
    if (spec & HB_STATE_XFRC_APPLIED) for (int i = 0; i < 6 * m.nbody; i++) xf[(size_t)e * 6 * m.nbody + i] = (float)*o++;
  }
  HB_HIP(hipMemcpy(b->d_state, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  if (spec & HB_STATE_XFRC_APPLIED) {
    const int rc = ensure_xfrc(b);
    if (rc != HB_OK) return rc;
    HB_HIP(hipMemcpy(b->d_xfrc, xf.data(), xf.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  return HB_OK;
}

template <class T>
int set_state_broadcast_impl(hb_batch* b, unsigned spec, const T* one) {
  if (!b || !one) return HB_EINVAL;
  if ((spec & ~kSupportedSpec) || !spec) return HB_EINVAL;
  const int w = spec_size(b->model->m, spec);
  std::vector<T> all((size_t)b->n_env * w);
  for (int e = 0; e < b->n_env; e++) memcpy(&all[(size_t)e * w], one, (size_t)w * sizeof(T));
  return set_state_impl<T>(b, spec, all.data());
}


}  // namespace hb

extern "C" {

int hb_set_state_broadcast(hb_batch* b, unsigned spec, const float* state) { return set_state_broadcast_impl<float>(b, spec, state); }
int hb_set_state_broadcast_f64(hb_batch* b, unsigned spec, const double* state) { return set_state_broadcast_impl<double>(b, spec, state); }

int hb_state_size(const hb_batch* b, unsigned spec) {
  if (!b || (spec & ~kSupportedSpec)) return HB_EINVAL;
  return spec_size(b->model->m, spec);
}
int hb_get_state(hb_batch* b, unsigned spec, float* out) { return get_state_impl<float>(b, spec, out); }
int hb_set_state(hb_batch* b, unsigned spec, const float* in) { return set_state_impl<float>(b, spec, in); }
int hb_get_state_f64(hb_batch* b, unsigned spec, double* out) { return get_state_impl<double>(b, spec, out); }
int hb_set_state_f64(hb_batch* b, unsigned spec, const double* in) { return set_state_impl<double>(b, spec, in); }

}  // extern "C"
