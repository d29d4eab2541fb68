// hb_api_policy.cpp — the C-ABI of libhb.so (include/hb.h), the policy MLP: hb_policy_set_mlp, hb_policy_eval and the closed loop
// hb_rollout_policy.  The policy is a DevMlp (hb_batch.hpp), as the actor and the critic are (hb_api_collect.cpp).
#include "hb_batch.hpp"

extern "C" {

int hb_policy_set_mlp(hb_batch* b, int n_layers, const int* sizes, const float* const* weights, const float* const* biases) {
  if (!b || !mlp_args_ok(n_layers, sizes, weights, biases)) return HB_EINVAL;
  if (sizes[0] != b->D.dm.nobs || sizes[n_layers] != b->D.dm.nu) return HB_EINVAL;
  bool fused = true;  // one-launch policy kernel: every width fits its LDS tiles
  int maxh = 1;
  for (int l = 0; l <= n_layers; l++) {
    if (sizes[l] > 512) return HB_EINVAL;
    fused = fused && sizes[l] <= 256;
    if (l > 0 && l < n_layers) maxh = std::max(maxh, sizes[l]);
  }
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));  // (a call still in flight reads the buffers that are replaced below)
  // (every argument check is behind us: from here on only the device can fail, and then no policy is installed)
  for (int l = 0; l < 4; l++) b->d_mlp_w[l].reset();
  reset_all(b->d_mlp_h[0], b->d_mlp_h[1], b->d_mlp_act);
  rc = b->policy.install(n_layers, sizes, weights, biases);
  if (rc == HB_OK && fused) rc = b->d_mlp_act.alloc(((size_t)(b->n_env + 15) / 16 + hb_batch::kPipes) * 32 * b->policy.desc().ldx, /*zero=*/true);
  for (int l = 0; l < n_layers && rc == HB_OK && !fused; l++) {  // the layer-by-layer path reads the weights as they are given
    const size_t nw = (size_t)sizes[l] * sizes[l + 1];
    rc = b->d_mlp_w[l].alloc(nw);
    if (rc == HB_OK && hipMemcpy(b->d_mlp_w[l], weights[l], nw * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = HB_ENODEVICE;
  }
  for (int i = 0; i < 2 && rc == HB_OK && !fused; i++) rc = b->d_mlp_h[i].alloc((size_t)b->n_env * maxh);
  if (rc != HB_OK) b->policy.clear();
  b->mlp_fused = fused;
  return rc;
}

// obs -> MLP -> ctrl for envs [lo, hi) on `st`
// (seg >= 0: env segment `seg` of a pipelined closed loop: the LDS-free kernel, which the GPU places beside the running step kernels)
static int policy_forward(hb_batch* b, int lo, int hi, hipStream_t st, int seg = -1) {
  const DevMlp& net = b->policy;
  if (net.layers < 1) return HB_EINVAL;
  const DevModel& dm = b->D.dm;
  if (b->mlp_fused) {
    const PolicyDesc pd = net.desc();
    const bool lean_ok = b->tune[HB_TUNE_POLICY_LEAN] != 0;
    const bool lean_all = b->tune[HB_TUNE_POLICY_LEAN] == 2;
    if (lean_all && seg < 0) seg = 0;
    if (seg >= 0 && lean_ok && b->d_mlp_act)
      HB_HIP(launch_policy_lean(dm, pd, b->d_state + (size_t)lo * dm.nstate, ctrl_for_write(b) + (size_t)lo * dm.nu,
                                b->d_mlp_act + ((size_t)(lo + 15) / 16 + seg) * 32 * pd.ldx, hi - lo, st));
    else
      HB_HIP(launch_policy(dm, pd, b->d_state + (size_t)lo * dm.nstate, ctrl_for_write(b) + (size_t)lo * dm.nu, hi - lo, st));
    return HB_OK;
  }
  // wide layers: one launch per layer, activations through HBM
  HB_HIP(launch_obs(dm, b->d_state + (size_t)lo * dm.nstate, b->d_obs + (size_t)lo * net.sizes[0], hi - lo, st));
  const float* x = b->d_obs + (size_t)lo * net.sizes[0];
  for (int l = 0; l < net.layers; l++) {
    float* y = ((l + 1 == net.layers) ? ctrl_for_write(b) : b->d_mlp_h[l & 1]) + (size_t)lo * net.sizes[l + 1];
    HB_HIP(launch_mlp_layer(x, b->d_mlp_w[l], net.b[l], y, hi - lo, net.sizes[l], net.sizes[l + 1], 1 + (l + 1 == net.layers ? kActTanh : net.act), st));
    x = y;
  }
  return HB_OK;
}

int hb_policy_eval(hb_batch* b, float* ctrl_out) {
  if (!b) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  int rc = policy_forward(b, 0, b->n_env, main_stream(b));
  if (rc != HB_OK) return rc;
  if (ctrl_out) HB_HIP(hipMemcpyAsync(ctrl_out, b->d_ctrl, (size_t)b->n_env * b->D.dm.nu * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

int hb_rollout_policy(hb_batch* b, int T, float* qpos_out_dev) {
  if (!b || T < 1) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  // every segment is its own obs -> MLP -> mj_step chain: with pipelining on, the chains run side by side
  const int nseg = segment_count(b);
  int rc = fork_pipes(b, nseg);
  if (rc != HB_OK) return rc;
  for (int t = 0; t < T; t++) {
    const bool reorder = b->schedule && (b->launch_count % reorder_period(b) == 0);
    BatchPtrs P = make_ptrs(b);
    P.qfrc_out = nullptr;  // (the env adapter's read-out: nothing in this loop reads it, and without it the step launches are the lean kernels)
    P.ctrl = b->d_ctrl; P.ctrl_mode = 0;
    P.qpos_out = qpos_out_dev ? qpos_out_dev + (size_t)t * b->n_env * b->D.dm.nq : nullptr;
    for (int c = 0; c < nseg; c++) {
      const Segment sg = segment(b, c, nseg);
      rc = policy_forward(b, sg.lo, sg.hi, sg.st, nseg > 1 ? c : -1);
      if (rc == HB_OK) rc = launch_segment(b, P, 1, sg, nseg, reorder);
      if (rc != HB_OK) return rc;
    }
    steps_enqueued(b, nseg, reorder);
  }
  return HB_OK;
}

}  // extern "C"
