// hb_api_env.cpp — the C-ABI of libhb.so (include/hb.h), the env adapter: observations, rewards and resets, the realism layer and
// domain randomisation, the policy MLP, the sampling actor with its rollout collection, the critic with the PPO buffer over the tapes, and
// the running observation / reward normaliser with its episode statistics.  The policy, the actor and the critic are each a DevMlp
// (hb_batch.hpp): one owner packs, uploads and describes an installed network, and one check (mlp_args_ok) covers the arrays of the three
// hb_*_set_mlp entry points; their kernels share one layer loop (hb_mlp_layers.inl).
#include "hb_batch.hpp"

extern "C" {

static int env_alloc(hb_batch* b) {
  if (b->env_ready) return HB_OK;
  const DevModel& dm = b->D.dm;
  size_t n = b->n_env;
  HB_HIP(hipSetDevice(b->device));
  const size_t nu = std::max(1, dm.nu);
  // one record [obs n x nobs | reward n | terminated n | truncated n]: a host that keeps its four buffers in the same order and
  // back to back (engine.py does) gets them in one transfer instead of four
  // (nobs: the adapter's row, the model's observation and what hb_env_obs_extend appends)
  int rc = b->d_record.alloc(n * b->env_nobs * sizeof(float) + n * sizeof(float) + 2 * n);
  if (rc == HB_OK) rc = b->d_prev.alloc(n * nu, /*zero=*/true);
  if (rc == HB_OK) rc = b->d_latest.alloc(n * nu, /*zero=*/true);
  if (rc == HB_OK) rc = b->d_action.alloc(n * nu);
  if (rc == HB_OK) rc = b->d_qfrc.alloc(n * dm.nv, /*zero=*/true);
  if (rc == HB_OK) rc = b->d_episode.alloc(n, /*zero=*/true);
  if (rc == HB_OK) rc = b->d_seen.alloc(n, /*zero=*/true);
  if (rc != HB_OK) { reset_all(b->d_record, b->d_prev, b->d_latest, b->d_action, b->d_qfrc, b->d_episode, b->d_seen); return rc; }
  b->d_obs = reinterpret_cast<float*>(b->d_record.get());
  b->d_reward = b->d_obs + n * b->env_nobs;
  b->d_term = reinterpret_cast<uint8_t*>(b->d_reward + n);
  b->d_trunc = b->d_term + n;
  hb_env_config def;
  hb_env_default_config(b->model, &def);
  static_assert(sizeof(hb_env_config) == sizeof(EnvConfig), "hb_env_config and EnvConfig must have the same layout");
  memcpy(&b->env_cfg, &def, sizeof def);
  b->env_ready = true;
  return HB_OK;
}

// reward / termination / observation of every env (or those of `mask`).  observe: push the observation through the
// realism layer's noise and delay lines (a step of the episode) instead of returning the true one.
static int env_eval(hb_batch* b, bool allow_reset, bool observe, const uint8_t* mask, float* d_obs, float* d_reward, uint8_t* d_term, uint8_t* d_trunc) {
  EnvConfig cfg = b->env_cfg;
  if (!allow_reset) cfg.auto_reset = 0;
  const Model& m = b->model->m;
  const float* src = b->D.d_qpos_src + (cfg.reset_keyframe < 0 || cfg.reset_keyframe >= m.nkey ? 0 : (size_t)(1 + cfg.reset_keyframe) * m.nq);
  EnvRandState S = b->rs;
  if (!b->rand_on) memset(&S, 0, sizeof S);
  // velocity commands: the env kernel is handed the envs' records; only a step may redraw inside an episode (allow_reset: hb_env_step*,
  // hb_env_collect*; not hb_get_obs, not the settle step or the final observation of hb_env_reset)
  CmdArgs K;
  memset(&K, 0, sizeof K);
  if (b->d_cmd) { K.cmd = b->d_cmd; K.C = b->cmd_cfg; K.resample = allow_reset ? 1 : 0; K.obs_col = b->cmd_cfg.observe ? b->env_nobs - 3 : -1; }
  // foot-contact terms: the read-out of the last substep and the envs' records; only a step writes the records (the same switch)
  FeetArgs A;
  memset(&A, 0, sizeof A);
  if (b->d_feet) {
    A.body_contact = b->d_body_contact; A.rec = b->d_feet; A.F = b->feet_cfg; A.update = allow_reset ? 1 : 0;
    A.obs_col = b->feet_cfg.observe ? b->env_nobs - (b->d_cmd && b->cmd_cfg.observe ? 3 : 0) - b->feet_cfg.n_feet : -1;
  }
  if (b->env_nobs != b->D.dm.nobs) {
    // the extended row: the scan is cast here, at the state the step left (an episode that ends below ends in it, over the elevations
    // it was run on); the env kernel appends the last action and the scan to the rows it writes; the envs it resets get the scan of
    // their new state, over their new elevations, from a second cast masked to them
    const bool scan = b->obs_ext.height_scan != 0;
    ObsExtArgs X;
    memset(&X, 0, sizeof X);
    X.stride = b->env_nobs; X.n_act = b->obs_ext.prev_action ? b->D.dm.nu : 0; X.n_scan = scan ? b->n_ray : 0;
    X.scan = b->d_ext_scan; X.reset_flag = scan && cfg.auto_reset ? b->d_ext_reset.get() : nullptr;
    int rc = scan ? rays_scan_launch(b, nullptr, b->d_ext_scan, b->n_ray, 0) : HB_OK;
    if (rc != HB_OK) return rc;
    HB_HIP(launch_env(b->D.dm, cfg, b->env_rand, S, b->d_state, b->d_qfrc, b->d_counts, b->d_prev, b->d_latest, src, b->d_episode, b->d_status, d_obs, d_reward,
                      d_term, d_trunc, mask, observe ? 1 : 0, b->dom_rand, b->d_dr, b->dr_stride, b->n_env, b->env_offset, main_stream(b), observe ? b->d_term_obs.get() : nullptr, b->d_seen, &X, &K, &A));
    if (X.reset_flag) return rays_scan_launch(b, X.reset_flag, d_obs, b->env_nobs, b->D.dm.nobs + X.n_act);
    return HB_OK;
  }
  HB_HIP(launch_env(b->D.dm, cfg, b->env_rand, S, b->d_state, b->d_qfrc, b->d_counts, b->d_prev, b->d_latest, src, b->d_episode, b->d_status, d_obs, d_reward,
                    d_term, d_trunc, mask, observe ? 1 : 0, b->dom_rand, b->d_dr, b->dr_stride, b->n_env, b->env_offset, main_stream(b), observe ? b->d_term_obs.get() : nullptr, b->d_seen, nullptr, &K, &A));
  return HB_OK;
}

int hb_get_obs(hb_batch* b, float* obs, float* reward, uint8_t* terminated, uint8_t* truncated) {
  if (!b || !obs) return HB_EINVAL;
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  int n = b->n_env, nobs = b->env_nobs;
  if (reward || terminated || truncated || nobs != b->D.dm.nobs) {  // (an extended row is the env kernel's: hb_obs_kernel writes the base alone)
    rc = env_eval(b, false, false, nullptr, b->d_obs, b->d_reward, b->d_term, b->d_trunc);  // pure evaluation: no reset, no bookkeeping, true observation
    if (rc != HB_OK) return rc;
  } else {
    HB_HIP(launch_obs(b->D.dm, b->d_state, b->d_obs, n, main_stream(b)));
  }
  HB_HIP(hipMemcpyAsync(obs, b->d_obs, (size_t)n * nobs * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  if (reward) HB_HIP(hipMemcpyAsync(reward, b->d_reward, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  if (terminated) HB_HIP(hipMemcpyAsync(terminated, b->d_term, n, hipMemcpyDeviceToHost, main_stream(b)));
  if (truncated) HB_HIP(hipMemcpyAsync(truncated, b->d_trunc, n, hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

int hb_env_default_config(const hb_model* h, hb_env_config* c) {
  if (!h || !c) return HB_EINVAL;
  const Model& m = h->m;
  memset(c, 0, sizeof *c);
  double z0 = 1.0;
  for (int j = 0; j < m.njnt; j++) if (m.jnt_type[j] == JNT_FREE) { z0 = m.qpos0[m.jnt_qposadr[j] + 2]; break; }
  c->target_z = (float)(0.94 * z0);  // the reference targets its standing height (Z_INITIAL_POS); 6 % slack for the soft stance
  c->min_z = (float)(0.3 * z0);
  c->max_time = 10.f;                 // MAX_SIM_TIME_STANDUP
  double gear = 0;
  for (int a = 0; a < m.nu; a++) gear += std::fabs(m.actuator_gear[a]);
  c->safe_torque = (float)(m.nu ? 0.05 * gear / m.nu : 1.0);  // reference: 1.0 N m = 5 % of its 20 N m motors
  c->control_frequency = (float)(1.0 / m.timestep);
  c->action_scale = 1.5707963267948966f;
  c->w_hvel = 5.f; c->w_upright = 10.f; c->w_height = 15.f; c->w_torque = 2.5f; c->w_ctrl_change = 2.f; c->w_ctrl_reg = 0.5f; c->w_symmetry = 1.f;
  c->self_collision_penalty = -20.f; c->terminal_reward = -100.f; c->upright_tol = 0.7f;
  // symmetry pairs: actuators named <x>_right / <x>_left (mirrored joint axes in the model => equal controls)
  for (int a = 0; a < m.nu && c->n_equal < HB_ENV_MAX_PAIRS; a++) {
    const std::string& n = m.actuator_name[a];
    const std::string suf = "_right";
    if (n.size() > suf.size() && n.compare(n.size() - suf.size(), suf.size(), suf) == 0) {
      std::string other = n.substr(0, n.size() - suf.size()) + "_left";
      for (int k = 0; k < m.nu; k++) if (m.actuator_name[k] == other) { c->equal_pairs[c->n_equal][0] = k; c->equal_pairs[c->n_equal][1] = a; c->n_equal++; break; }
    }
  }
  c->auto_reset = 1; c->reset_keyframe = -1; c->reset_perturb = 1.f;
  c->reward_kind = 0; c->w_vvel = 0.f;
  c->min_z_grounded = (float)(0.25 * z0);  // the reference's MIN_Z_BEFORE_GROUNDED sits a quarter of the way up its robot
  c->reset_collision_mode = 0;
  return HB_OK;
}

int hb_env_team_config(const hb_model* h, hb_env_config* c) {
  if (!h || !c) return HB_EINVAL;
  const Model& m = h->m;
  int rc = hb_env_default_config(h, c);
  if (rc != HB_OK) return rc;
  auto act = [&](const char* name) { for (int a = 0; a < m.nu; a++) if (m.actuator_name[a] == name) return a; return -1; };
  // reward_functions.py:289-339 (standupReward) and simulation_parameters.py:51-77
  c->target_z = -0.375f;            // TARGET_Z_POS = Z_INITIAL_POS
  c->min_z = -0.6f;                 // MIN_Z_POS_FOR_REWARD
  c->max_time = 10.f;               // MAX_SIM_TIME_STANDUP
  c->safe_torque = 1.0f;            // MAX__SAFE_JOINT_TORQUE
  c->control_frequency = 500.f;     // CONTROL_FREQUENCY
  c->n_equal = c->n_opposite = 0;
  const char* eq[][2] = {{"left_elbow", "right_elbow"}};
  const char* op[][2] = {{"left_hip_roll", "right_hip_roll"}, {"left_hip_pitch", "right_hip_pitch"}, {"left_knee", "right_knee"},
                         {"left_shoulder_pitch", "right_shoulder_pitch"}, {"left_shoulder_roll", "right_shoulder_roll"}};
  for (auto& pr : eq) { const int a = act(pr[0]), b2 = act(pr[1]); if (a < 0 || b2 < 0) return HB_EINVAL; c->equal_pairs[c->n_equal][0] = a; c->equal_pairs[c->n_equal][1] = b2; c->n_equal++; }
  for (auto& pr : op) { const int a = act(pr[0]), b2 = act(pr[1]); if (a < 0 || b2 < 0) return HB_EINVAL; c->opposite_pairs[c->n_opposite][0] = a; c->opposite_pairs[c->n_opposite][1] = b2; c->n_opposite++; }
  c->reset_keyframe = -1;
  for (int k = 0; k < m.nkey; k++) if (m.key_name[k] == "standup_reset") c->reset_keyframe = k;
  c->reset_perturb = 1.f;
  c->reset_quat_perturb = 0.1f;     // QUAT_INITIAL_OFFSET_MAX
  c->obs_actuator_order = 1;        // JOINT_NAMES order = the <motor> order of the reference's humanoid.xml
  c->min_z_grounded = -0.6f;
  c->reset_collision_mode = 1;      // CPUEnv.reset starts over while anything is in contact (cpu_env.py:411-414)
  return HB_OK;
}

int hb_env_configure(hb_batch* b, const hb_env_config* cfg) {
  if (!b || !cfg) return HB_EINVAL;
  if (cfg->n_equal < 0 || cfg->n_equal > HB_ENV_MAX_PAIRS || cfg->n_opposite < 0 || cfg->n_opposite > HB_ENV_MAX_PAIRS || !(cfg->action_scale > 0)) return HB_EINVAL;
  int nu = b->D.dm.nu;
  for (int k = 0; k < cfg->n_equal; k++) for (int t = 0; t < 2; t++) if (cfg->equal_pairs[k][t] < 0 || cfg->equal_pairs[k][t] >= nu) return HB_EINVAL;
  for (int k = 0; k < cfg->n_opposite; k++) for (int t = 0; t < 2; t++) if (cfg->opposite_pairs[k][t] < 0 || cfg->opposite_pairs[k][t] >= nu) return HB_EINVAL;
  if (cfg->reset_keyframe >= b->model->m.nkey) return HB_EINVAL;
  if (cfg->reward_kind < 0 || cfg->reward_kind > 1 || cfg->reset_collision_mode < 0 || cfg->reset_collision_mode > 2) return HB_EINVAL;
  if (!(cfg->reset_quat_perturb >= 0.f) || (cfg->obs_actuator_order != 0 && cfg->obs_actuator_order != 1)) return HB_EINVAL;
  if (cfg->obs_actuator_order && !b->D.has_act_order) return HB_EINVAL;  // needs exactly one actuator per scalar joint
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  memcpy(&b->env_cfg, cfg, sizeof *cfg);
  // the env / observation / policy kernels take the DevModel by value from this host copy: point it at the chosen order
  b->D.dm.obs_jnt = cfg->obs_actuator_order ? b->D.obs_jnt_act : b->D.obs_jnt_joint;
  b->D.dm.obs_src = cfg->obs_actuator_order ? b->D.obs_src_act : b->D.obs_src_joint;
  return HB_OK;
}

int hb_env_default_randomization(const hb_model* h, hb_env_randomization* r) {
  if (!h || !r) return HB_EINVAL;
  memset(r, 0, sizeof *r);
  const float deg = 0.017453292519943295f;
  r->factor = 1.f; r->seed = 0; r->control_timestep = (float)h->m.timestep;
  r->joint_angle_noise = 2.f * deg;     // JOINT_ANGLE_NOISE_STDDEV     (simulation_parameters.py:39-45)
  r->joint_velocity_noise = 5.f * deg;  // JOINT_VELOCITY_NOISE_STDDEV
  r->gyro_noise = 2.f * deg;            // GYRO_NOISE_STDDEV
  r->imu_noise = 5.f * deg;             // IMU_NOISE_STDDEV
  r->action_noise = 0.5f * deg;         // JOINT_ACTION_NOISE_STDDEV
  r->min_delay = 0.01f; r->max_delay = 0.05f;  // MIN_DELAY, MAX_DELAY
  r->frozen_noise = 0;
  r->push_enabled = 1;                  // *_EXTERNAL_FORCE_* (simulation_parameters.py:14-20)
  r->push_min_interval = 1.f; r->push_max_interval = 3.f; r->push_min_duration = 0.05f; r->push_max_duration = 0.15f;
  r->push_min_force = 5.f; r->push_max_force = 15.f;
  return HB_OK;
}

// releases the realism layer's device arrays: the layer is off
static void envrand_free(hb_batch* b) {
  reset_all(b->d_rs_k_act, b->d_rs_k_obs, b->d_rs_delay, b->d_rs_fifo_act, b->d_rs_fifo_joint, b->d_rs_fifo_gyro, b->d_rs_fifo_grav, b->d_rs_push);
  memset(&b->rs, 0, sizeof b->rs);
  b->rand_on = false;
}
int hb_env_randomize(hb_batch* b, const hb_env_randomization* cfg) {
  if (!b) return HB_EINVAL;
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  if (!cfg || !(cfg->factor > 0.f)) { envrand_free(b); return HB_OK; }
  const DevModel& dm = b->D.dm;
  const float dt = cfg->control_timestep > 0.f ? cfg->control_timestep : dm.timestep;
  if (!(cfg->max_delay >= cfg->min_delay) || cfg->min_delay < 0.f || cfg->max_delay * cfg->factor / dt > (float)(kDelaySlots - 1)) return HB_EINVAL;
  if (cfg->push_enabled && (!(cfg->push_max_interval >= cfg->push_min_interval) || !(cfg->push_max_duration >= cfg->push_min_duration) ||
                            !(cfg->push_max_force >= cfg->push_min_force) || dm.nbody < 2)) return HB_EINVAL;
  static_assert(sizeof(hb_env_randomization) == sizeof(EnvRand), "hb_env_randomization and EnvRand must have the same layout");
  const size_t n = b->n_env, nu = std::max(1, dm.nu), nj2 = std::max(2, dm.nobs - 6);
  if (!b->rs.k_act) {
    rc = b->d_rs_k_act.alloc(n);
    if (rc == HB_OK) rc = b->d_rs_k_obs.alloc(n);
    if (rc == HB_OK) rc = b->d_rs_delay.alloc(n * 4);
    if (rc == HB_OK) rc = b->d_rs_fifo_act.alloc(n * kDelaySlots * nu);
    if (rc == HB_OK) rc = b->d_rs_fifo_joint.alloc(n * kDelaySlots * nj2);
    if (rc == HB_OK) rc = b->d_rs_fifo_gyro.alloc(n * kDelaySlots * 3);
    if (rc == HB_OK) rc = b->d_rs_fifo_grav.alloc(n * kDelaySlots * 3);
    if (rc == HB_OK) rc = b->d_rs_push.alloc(n * 8, /*zero=*/true);
    if (rc != HB_OK) { envrand_free(b); return rc; }
    b->rs.k_act = b->d_rs_k_act; b->rs.k_obs = b->d_rs_k_obs; b->rs.delay = b->d_rs_delay; b->rs.fifo_act = b->d_rs_fifo_act;
    b->rs.fifo_joint = b->d_rs_fifo_joint; b->rs.fifo_gyro = b->d_rs_fifo_gyro; b->rs.fifo_grav = b->d_rs_fifo_grav; b->rs.push = b->d_rs_push;
  }
  if (cfg->push_enabled && (rc = ensure_xfrc(b)) != HB_OK) return rc;
  memcpy(&b->env_rand, cfg, sizeof *cfg);
  b->rs.xfrc = cfg->push_enabled ? b->d_xfrc.get() : nullptr;
  b->rand_on = true;
  // a consistent episode state until the caller resets: delays drawn, rings empty
  HB_HIP(launch_envrand_reset(dm, b->env_rand, b->rs, b->d_episode, nullptr, b->n_env, b->env_offset, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

int hb_env_default_domain_randomization(const hb_model* h, hb_domain_randomization* d) {
  if (!h || !d) return HB_EINVAL;
  memset(d, 0, sizeof *d);
  d->factor = 1.f; d->seed = 0;
  d->friction_min_mult = 0.5f; d->friction_max_mult = 1.f;   // FLOOR_FRICTION_*_MULTIPLIER (simulation_parameters.py:5-7)
  d->max_mass_change = 0.05f; d->max_external_mass = 0.2f;   // MAX_MASS_CHANGE_PER_LIMB, MAX_EXTERNAL_MASS_ADDED
  d->armature_max_change = 0.0005f; d->stiffness_max_change = 0.f; d->margin_max_change = 0.05f; d->range_max_change = 0.1f;  // JOINT_*_MAX_CHANGE
  d->kp_nominal = 0.f; d->kp_max_change = 0.5f;              // JOINT_P_GAIN(_MAX_CHANGE); nominal 0: keep the model's gains
  d->force_limit_max_change = 0.05f;                         // JOINT_FORCE_LIMIT_MAX_CHANGE
  d->floor_bump_min = 0.f; d->floor_bump_max = h->m.nhfield > 0 ? 0.1f : 0.f;  // MIN/MAX_FLOOR_BUMP_HEIGHT (simulation_parameters.py:47-48); only with a height field
  return HB_OK;
}

int hb_env_domain_randomize(hb_batch* b, const hb_domain_randomization* cfg) {
  if (!b) return HB_EINVAL;
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  if (!cfg || !(cfg->factor > 0.f)) {
    b->d_dr.reset();
    b->dr_stride = 0;
    return HB_OK;
  }
  if (!(cfg->friction_max_mult >= cfg->friction_min_mult) || cfg->friction_min_mult < 0.f || cfg->max_mass_change < 0.f || cfg->max_external_mass < 0.f ||
      cfg->armature_max_change < 0.f || cfg->stiffness_max_change < 0.f || cfg->margin_max_change < 0.f || cfg->range_max_change < 0.f || cfg->kp_max_change < 0.f ||
      cfg->force_limit_max_change < 0.f || cfg->floor_bump_min < 0.f || cfg->floor_bump_max < 0.f) return HB_EINVAL;
  static_assert(sizeof(hb_domain_randomization) == sizeof(DomainRand), "hb_domain_randomization and DomainRand must have the same layout");
  const DevModel& dm = b->D.dm;
  const DomainLayout L = domain_layout(dm.nbody, dm.nv, dm.nlimcand, dm.nu, dm.nhfielddata);
  if (b->d_dr.alloc((size_t)b->n_env * L.stride) != HB_OK) return HB_ENOMEM;
  b->dr_stride = L.stride;
  memcpy(&b->dom_rand, cfg, sizeof *cfg);
  // valid parameters at once (the draw of episode 0); hb_env_reset draws again for the episode numbers it assigns
  HB_HIP(launch_domain_rand(dm, b->dom_rand, b->d_dr, b->dr_stride, b->d_episode, nullptr, b->n_env, b->env_offset, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

int hb_env_get_domain_params(hb_batch* b, float* out) {
  if (!b) return HB_EINVAL;
  if (!b->d_dr) return 0;
  if (out) {
    HB_HIP(hipSetDevice(b->device));
    HB_HIP(hipStreamSynchronize(main_stream(b)));
    HB_HIP(hipMemcpy(out, b->d_dr, (size_t)b->n_env * b->dr_stride * sizeof(float), hipMemcpyDeviceToHost));
  }
  return b->dr_stride;
}

// ---- observation extension: the last action and the configured height scan behind the model's observation

int hb_env_nobs(hb_batch* b) { return b ? b->env_nobs : HB_EINVAL; }

// the record and the terminal-observation table with rows of `total` floats (the stream is idle); a failure leaves the batch as it was
static int env_rows_resize(hb_batch* b, int total) {
  if (total == b->env_nobs) return HB_OK;
  const bool had_record = b->env_ready, had_term = (bool)b->d_term_obs;
  DevBuf<uint8_t> record;
  DevBuf<float> term;
  const size_t n = b->n_env;
  if (had_record && record.alloc(n * total * sizeof(float) + n * sizeof(float) + 2 * n) != HB_OK) return HB_ENOMEM;
  if (had_term && term.alloc(n * total, /*zero=*/true) != HB_OK) return HB_ENOMEM;
  if (had_record) {
    b->d_record.swap(record);
    b->d_obs = reinterpret_cast<float*>(b->d_record.get());
    b->d_reward = b->d_obs + n * total;
    b->d_term = reinterpret_cast<uint8_t*>(b->d_reward + n);
    b->d_trunc = b->d_term + n;
  }
  if (had_term) b->d_term_obs.swap(term);
  b->env_nobs = total;
  return HB_OK;
}
// the width of a row: [ base | extension (n_ext) | foot-contact flags | command ]
static int env_row_width(const hb_batch* b, int n_ext, bool cmd_observed, int n_feet_observed) {
  return b->D.dm.nobs + n_ext + n_feet_observed + (cmd_observed ? 3 : 0);
}
static int feet_observed(const hb_batch* b) { return b->d_feet && b->feet_cfg.observe ? b->feet_cfg.n_feet : 0; }
static bool obs_consumers_exist(const hb_batch* b) {
  return b->actor.layers >= 1 || b->critic.layers >= 1 || b->q[0].layers >= 1 || b->q[1].layers >= 1 || b->norm_on || b->learner.on || b->sac.on;
}

int hb_env_obs_extend(hb_batch* b, const hb_obs_ext* ext) {
  if (!b) return HB_EINVAL;
  // everything sized by the observation comes after this call
  if (obs_consumers_exist(b)) return HB_EINVAL;
  hb_obs_ext x;
  memset(&x, 0, sizeof x);
  if (ext) {
    if (!std::isfinite(ext->scan_offset) || !std::isfinite(ext->scan_scale) || !std::isfinite(ext->scan_lo) || !std::isfinite(ext->scan_hi)) return HB_EINVAL;
    x.prev_action = ext->prev_action != 0;
    x.height_scan = ext->height_scan != 0;
    if (x.height_scan) {
      if (b->n_ray < 1 || !(b->ray_spec.cutoff > 0.f) || ext->scan_lo > ext->scan_hi) return HB_EINVAL;
      x.scan_offset = ext->scan_offset; x.scan_scale = ext->scan_scale; x.scan_lo = ext->scan_lo; x.scan_hi = ext->scan_hi;
    }
  }
  const int n_ext = (x.prev_action ? b->D.dm.nu : 0) + (x.height_scan ? b->n_ray : 0);
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));  // (a step still in flight writes the buffers that are replaced below)
  // the scan's scratch first: a failure here leaves the batch as it was
  DevBuf<float> scan;
  DevBuf<uint8_t> flag;
  if (x.height_scan && (scan.alloc((size_t)b->n_env * b->n_ray) != HB_OK || flag.alloc((size_t)b->n_env, /*zero=*/true) != HB_OK)) return HB_ENOMEM;
  // the record and the terminal-observation table have rows of the new width (observed commands stay the last three columns)
  const int rc = env_rows_resize(b, env_row_width(b, n_ext, b->d_cmd && b->cmd_cfg.observe, feet_observed(b)));
  if (rc != HB_OK) return rc;
  b->d_ext_scan.swap(scan);
  b->d_ext_reset.swap(flag);
  b->obs_ext = x; b->n_ext = n_ext;
  return HB_OK;
}

// ---- velocity commands (include/hb.h: hb_env_commands)

static thread_local const char* g_cmd_error = "";
static int cmd_refuse(const char* why) { g_cmd_error = why; return HB_EINVAL; }
const char* hb_error(void) { return g_cmd_error; }
extern "C++" int hb::refuse_with(const char* why) { return cmd_refuse(why); }
extern "C++" void hb::refuse_clear() { g_cmd_error = ""; }

int hb_env_default_commands(const hb_model* m, hb_env_commands* out) {
  g_cmd_error = "";
  if (!m || !out) return cmd_refuse("hb_env_default_commands: NULL argument");
  memset(out, 0, sizeof *out);
  out->seed = 0;
  out->vx_min = -1.f; out->vx_max = 1.f; out->vy_min = -0.5f; out->vy_max = 0.5f; out->yaw_min = -1.f; out->yaw_max = 1.f;
  out->resample_time = 5.f; out->zero_fraction = 0.1f;
  out->w_yaw = 2.5f;  // half of hb_env_default_config's w_hvel
  out->frame = 1; out->observe = 1;
  return HB_OK;
}

int hb_env_commands_check(const hb_model* m, const hb_env_commands* c) {
  g_cmd_error = "";
  if (!m || !c) return cmd_refuse("commands: NULL argument");
  const float f[] = {c->vx_min, c->vx_max, c->vy_min, c->vy_max, c->yaw_min, c->yaw_max, c->resample_time, c->zero_fraction, c->w_yaw};
  for (float x : f) if (!std::isfinite(x)) return cmd_refuse("commands: a field is not finite");
  if (c->vx_min > c->vx_max || c->vy_min > c->vy_max || c->yaw_min > c->yaw_max) return cmd_refuse("commands: a range has min > max");
  if (c->zero_fraction < 0.f || c->zero_fraction > 1.f) return cmd_refuse("commands: zero_fraction is outside [0, 1]");
  if (c->frame != 0 && c->frame != 1) return cmd_refuse("commands: frame is neither 0 (world) nor 1 (heading)");
  if (c->observe != 0 && c->observe != 1) return cmd_refuse("commands: observe is neither 0 nor 1");
  bool free_root = false;  // (what the device model's obs_root_dofadr >= 0 says: hb_tables.cpp)
  for (int j = 0; j < m->m.njnt; j++) free_root = free_root || m->m.jnt_type[j] == JNT_FREE;
  if (!free_root) return cmd_refuse("commands: the model's observation has no free root");
  return HB_OK;
}

int hb_env_commands_configure(hb_batch* b, const hb_env_commands* cfg) {
  g_cmd_error = "";
  if (!b) return cmd_refuse("hb_env_commands_configure: NULL batch");
  if (cfg && hb_env_commands_check(b->model, cfg) != HB_OK) return HB_EINVAL;
  static_assert(sizeof(hb_env_commands) == sizeof(EnvCommands), "hb_env_commands and EnvCommands must have the same layout");
  const bool was = b->d_cmd && b->cmd_cfg.observe, now = cfg && cfg->observe;
  if (was != now && obs_consumers_exist(b))
    return cmd_refuse("commands: the observation width would change while an actor, critic, Q network, normaliser or learner exists");
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));  // (a step still in flight reads the buffers that are replaced below)
  DevBuf<float4> rec;
  const bool fresh = cfg && !b->d_cmd;
  if (fresh && rec.alloc((size_t)b->n_env, /*zero=*/true) != HB_OK) return HB_ENOMEM;
  if ((rc = env_rows_resize(b, env_row_width(b, b->n_ext, now, feet_observed(b)))) != HB_OK) return rc;
  if (!cfg) {
    b->d_cmd.reset();
    memset(&b->cmd_cfg, 0, sizeof b->cmd_cfg);
    return HB_OK;
  }
  memcpy(&b->cmd_cfg, cfg, sizeof *cfg);
  if (fresh) {
    // valid commands at once: draw 0 of every env's current episode; hb_env_reset draws again for the episode numbers it assigns
    b->d_cmd.swap(rec);
    HB_HIP(launch_command_reset(b->cmd_cfg, b->d_cmd, b->d_episode, nullptr, b->n_env, b->env_offset, main_stream(b)));
    HB_HIP(hipStreamSynchronize(main_stream(b)));
  }
  return HB_OK;
}

int hb_env_get_commands(hb_batch* b, float* out) {
  g_cmd_error = "";
  if (!b || !out) return cmd_refuse("hb_env_get_commands: NULL argument");
  if (!b->d_cmd) return cmd_refuse("hb_env_get_commands: no command configuration is installed");
  HB_HIP(hipSetDevice(b->device));
  std::vector<float> rec((size_t)b->n_env * 4);
  HB_HIP(hipMemcpyAsync(rec.data(), b->d_cmd, rec.size() * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  for (int e = 0; e < b->n_env; e++) for (int c = 0; c < 3; c++) out[3 * (size_t)e + c] = rec[4 * (size_t)e + c];
  return HB_OK;
}

int hb_env_set_commands(hb_batch* b, const float* cmd, const uint8_t* mask) {
  g_cmd_error = "";
  if (!b || !cmd) return cmd_refuse("hb_env_set_commands: NULL argument");
  if (!b->d_cmd) return cmd_refuse("hb_env_set_commands: no command configuration is installed");
  for (int e = 0; e < b->n_env; e++)
    if (!mask || mask[e]) for (int c = 0; c < 3; c++) if (!std::isfinite(cmd[3 * (size_t)e + c])) return cmd_refuse("hb_env_set_commands: a command is not finite");
  HB_HIP(hipSetDevice(b->device));
  // the records through the host, behind the enqueued work: the chosen envs' commands change, every draw count stays
  std::vector<float> rec((size_t)b->n_env * 4);
  HB_HIP(hipMemcpyAsync(rec.data(), b->d_cmd, rec.size() * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  for (int e = 0; e < b->n_env; e++)
    if (!mask || mask[e]) for (int c = 0; c < 3; c++) rec[4 * (size_t)e + c] = cmd[3 * (size_t)e + c];
  HB_HIP(hipMemcpy(b->d_cmd, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice));
  return HB_OK;
}

// ---- foot-contact terms (include/hb.h: hb_env_feet)

int hb_env_default_feet(const hb_model* m, hb_env_feet* out) {
  g_cmd_error = "";
  if (!m || !out) return cmd_refuse("hb_env_default_feet: NULL argument");
  memset(out, 0, sizeof *out);
  out->contact_threshold = 1.f;
  out->w_air_time = 1.f; out->air_time_target = 0.5f;
  out->air_gate = 1; out->air_cmd_min = 0.1f;
  double mass = 0.0;
  for (int i = 0; i < m->m.nbody; i++) mass += m->m.body_mass[i];
  const double* g = m->m.gravity;
  out->w_force = -0.01f; out->force_max = (float)(2.0 * mass * std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]));
  out->w_stumble = -1.f; out->stumble_ratio = 5.f;
  out->w_collision = -1.f;
  return HB_OK;
}

int hb_env_feet_check(const hb_model* m, const hb_env_feet* c) {
  g_cmd_error = "";
  if (!m || !c) return cmd_refuse("feet: NULL argument");
  if (c->n_feet < 1 || c->n_feet > HB_ENV_MAX_FEET) return cmd_refuse("feet: n_feet is outside 1..4");
  if (c->n_penalised < 0 || c->n_penalised > HB_ENV_MAX_CONTACT_BODIES) return cmd_refuse("feet: n_penalised is outside 0..8");
  if (c->n_terminal < 0 || c->n_terminal > HB_ENV_MAX_CONTACT_BODIES) return cmd_refuse("feet: n_terminal is outside 0..8");
  const int nbody = m->m.nbody;
  auto body_ok = [&](int id) { return id >= 1 && id < nbody; };
  for (int i = 0; i < c->n_feet; i++) if (!body_ok(c->foot_body[i])) return cmd_refuse("feet: a foot body id is outside 1..nbody-1");
  for (int i = 0; i < c->n_penalised; i++) if (!body_ok(c->penalised_body[i])) return cmd_refuse("feet: a penalised body id is outside 1..nbody-1");
  for (int i = 0; i < c->n_terminal; i++) if (!body_ok(c->terminal_body[i])) return cmd_refuse("feet: a terminal body id is outside 1..nbody-1");
  for (int i = 0; i < c->n_feet; i++)
    for (int j = 0; j < i; j++) if (c->foot_body[i] == c->foot_body[j]) return cmd_refuse("feet: a body is named twice in foot_body");
  const float f[] = {c->contact_threshold, c->w_air_time, c->air_time_target, c->air_cmd_min, c->w_force, c->force_max, c->w_stumble, c->stumble_ratio, c->w_collision};
  for (float x : f) if (!std::isfinite(x)) return cmd_refuse("feet: a field is not finite");
  if (c->contact_threshold <= 0.f) return cmd_refuse("feet: contact_threshold is not above 0");
  if (c->air_cmd_min < 0.f) return cmd_refuse("feet: air_cmd_min is below 0");
  if (c->stumble_ratio < 0.f) return cmd_refuse("feet: stumble_ratio is below 0");
  if (c->air_gate != 0 && c->air_gate != 1) return cmd_refuse("feet: air_gate is neither 0 nor 1");
  if (c->observe != 0 && c->observe != 1) return cmd_refuse("feet: observe is neither 0 nor 1");
  return HB_OK;
}

int hb_env_feet_configure(hb_batch* b, const hb_env_feet* cfg) {
  g_cmd_error = "";
  if (!b) return cmd_refuse("hb_env_feet_configure: NULL batch");
  if (cfg && hb_env_feet_check(b->model, cfg) != HB_OK) return HB_EINVAL;
  static_assert(sizeof(hb_env_feet) == sizeof(EnvFeet), "hb_env_feet and EnvFeet must have the same layout");
  static_assert(HB_ENV_MAX_FEET == kMaxFeet && HB_ENV_MAX_CONTACT_BODIES == kMaxContactBodies, "hb.h and hb_device.hpp must agree on the list lengths");
  const int was = feet_observed(b), now = cfg && cfg->observe ? cfg->n_feet : 0;
  if (was != now && obs_consumers_exist(b))
    return cmd_refuse("feet: the observation width would change while an actor, critic, Q network, normaliser or learner exists");
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));  // (a step still in flight reads the buffers that are replaced below)
  if (!cfg) {
    if ((rc = env_rows_resize(b, env_row_width(b, b->n_ext, b->d_cmd && b->cmd_cfg.observe, 0))) != HB_OK) return rc;
    b->d_feet.reset();
    memset(&b->feet_cfg, 0, sizeof b->feet_cfg);
    return HB_OK;
  }
  DevBuf<FeetRec> rec;
  const bool fresh = !b->d_feet;
  if (fresh && rec.alloc((size_t)b->n_env, /*zero=*/true) != HB_OK) return HB_ENOMEM;
  // the terms read the per-body read-out: switched on here, and its error passed on with nothing changed
  const bool readout_was = b->contact_readout;
  if (!readout_was && (rc = hb_contact_readout(b, 1)) != HB_OK) return rc;
  if ((rc = env_rows_resize(b, env_row_width(b, b->n_ext, b->d_cmd && b->cmd_cfg.observe, now))) != HB_OK) {
    if (!readout_was) hb_contact_readout(b, 0);
    return rc;
  }
  memcpy(&b->feet_cfg, cfg, sizeof *cfg);
  if (fresh) b->d_feet.swap(rec);
  // an episode start for every env at once: the feet down at the time each env has now
  HB_HIP(launch_feet_reset(b->d_feet, b->d_state, b->D.dm.nstate, b->feet_cfg.n_feet, nullptr, b->n_env, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

int hb_env_feet_count(hb_batch* b) { return b && b->d_feet ? b->feet_cfg.n_feet : 0; }

int hb_env_get_feet(hb_batch* b, float* t_last, uint8_t* contact) {
  g_cmd_error = "";
  if (!b) return cmd_refuse("hb_env_get_feet: NULL batch");
  if (!b->d_feet) return cmd_refuse("hb_env_get_feet: no feet configuration is installed");
  HB_HIP(hipSetDevice(b->device));
  std::vector<FeetRec> rec((size_t)b->n_env);
  HB_HIP(hipMemcpyAsync(rec.data(), b->d_feet, rec.size() * sizeof(FeetRec), hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  const int nf = b->feet_cfg.n_feet;
  for (int e = 0; e < b->n_env; e++)
    for (int f = 0; f < nf; f++) {
      if (t_last) t_last[(size_t)e * nf + f] = rec[e].t_last[f];
      if (contact) contact[(size_t)e * nf + f] = (rec[e].mask >> f) & 1u;
    }
  return HB_OK;
}

// CPUEnv._apply_action (+ pushes) -> n_substeps x mj_step -> reward / termination / observation, for every env or those of `mask`
static int env_step_impl(hb_batch* b, const float* action_dev, int n_substeps, const uint8_t* mask, bool allow_reset, float* obs_dev, float* reward_dev,
                         uint8_t* terminated_dev, uint8_t* truncated_dev) {
  const int n = b->n_env * b->D.dm.nu;
  if (b->rand_on) {
    HB_HIP(launch_action_env(b->D.dm, b->env_rand, b->rs, action_dev, b->d_prev, b->d_latest, ctrl_for_write(b), b->d_episode, b->d_state, mask, b->n_env, b->env_offset,
                             main_stream(b)));
  } else if (n && action_dev) {
    HB_HIP(launch_action(action_dev, b->d_prev, b->d_latest, ctrl_for_write(b), n, main_stream(b)));
  }
  BatchPtrs P = make_ptrs(b);
  P.ctrl = b->d_ctrl; P.ctrl_mode = 0; P.env_mask = mask;
  int rc = launch_steps(b, P, n_substeps);
  if (rc != HB_OK) return rc;
  return env_eval(b, allow_reset, true, mask, obs_dev, reward_dev, terminated_dev, truncated_dev);
}

int hb_env_reset(hb_batch* b, float* obs) {
  if (!b || !obs) return HB_EINVAL;
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  const EnvConfig& c = b->env_cfg;
  const Model& m = b->model->m;
  const size_t n = b->n_env, nu = std::max(1, b->D.dm.nu);
  HB_HIP(hipMemsetAsync(b->d_prev, 0, n * nu * sizeof(float), main_stream(b)));
  HB_HIP(hipMemsetAsync(b->d_latest, 0, n * nu * sizeof(float), main_stream(b)));
  HB_HIP(hipMemsetAsync(b->d_episode, 0, n * sizeof(int), main_stream(b)));
  if (b->d_ctrl) HB_HIP(hipMemsetAsync(ctrl_for_write(b), 0, n * nu * sizeof(float), main_stream(b)));
  if (c.reset_collision_mode == 0) {
    rc = reset_impl(b, nullptr, c.reset_keyframe, c.reset_perturb, b->env_offset);
    if (rc != HB_OK) return rc;
    if (b->rand_on) HB_HIP(launch_envrand_reset(b->D.dm, b->env_rand, b->rs, b->d_episode, nullptr, b->n_env, b->env_offset, main_stream(b)));
    if (b->d_dr) HB_HIP(launch_domain_rand(b->D.dm, b->dom_rand, b->d_dr, b->dr_stride, b->d_episode, nullptr, b->n_env, b->env_offset, main_stream(b)));
  } else {
    // The reference's protocol (cpu_env.py:374-416): randomise, take one step with the current (zero) controls, and
    // start over with a new draw while that step ends in a collision or in a terminal state.  Pending envs carry
    // a mask; everything (reset, realism layer, physics, evaluation) runs masked, at most eight draws.
    if (b->d_rmask.alloc(n) != HB_OK || b->d_pending.alloc(1) != HB_OK) return HB_ENOMEM;
    HB_HIP(hipMemsetAsync(b->d_rmask, 1, n, main_stream(b)));
    const float* src = b->D.d_qpos_src + (c.reset_keyframe < 0 ? 0 : (size_t)(1 + c.reset_keyframe) * m.nq);
    const float dtc = b->rand_on && b->env_rand.control_timestep > 0.f ? b->env_rand.control_timestep : (float)m.timestep;
    const int substeps = std::max(1, (int)std::lround(dtc / m.timestep));
    for (int attempt = 0; attempt < 8; attempt++) {
      HB_HIP(launch_reset(b->D.dm, b->d_state, b->d_status, b->d_rmask, src, b->d_episode, b->n_env, c.reset_perturb, b->env_offset, main_stream(b), c.reset_quat_perturb));
      if (b->rand_on) HB_HIP(launch_envrand_reset(b->D.dm, b->env_rand, b->rs, b->d_episode, b->d_rmask, b->n_env, b->env_offset, main_stream(b)));
      if (b->d_dr) HB_HIP(launch_domain_rand(b->D.dm, b->dom_rand, b->d_dr, b->dr_stride, b->d_episode, b->d_rmask, b->n_env, b->env_offset, main_stream(b)));
      rc = env_step_impl(b, nullptr, substeps, b->d_rmask, false, b->d_obs, b->d_reward, b->d_term, b->d_trunc);
      if (rc != HB_OK) return rc;
      HB_HIP(hipMemsetAsync(b->d_pending, 0, sizeof(int), main_stream(b)));
      HB_HIP(launch_reset_check(b->d_counts, b->d_term, b->d_trunc, b->d_rmask, b->d_episode, b->d_pending, c.reset_collision_mode, b->n_env, main_stream(b)));
      int pending = 0;
      HB_HIP(hipMemcpyAsync(&pending, b->d_pending, sizeof(int), hipMemcpyDeviceToHost, main_stream(b)));
      HB_HIP(hipStreamSynchronize(main_stream(b)));
      if (pending == 0) break;
    }
  }
  // draw 0 of every env's command, with the episode numbers the envs ended up with
  if (b->d_cmd) HB_HIP(launch_command_reset(b->cmd_cfg, b->d_cmd, b->d_episode, nullptr, b->n_env, b->env_offset, main_stream(b)));
  // the feet records of the episodes that begin: after the last settle step, with the time each env has then
  if (b->d_feet) HB_HIP(launch_feet_reset(b->d_feet, b->d_state, b->D.dm.nstate, b->feet_cfg.n_feet, nullptr, b->n_env, main_stream(b)));
  // the observation the reference returns from reset(): one more pass through the noise and delay lines
  rc = env_eval(b, false, true, nullptr, b->d_obs, b->d_reward, b->d_term, b->d_trunc);
  if (rc != HB_OK) return rc;
  HB_HIP(hipMemcpyAsync(obs, b->d_obs, n * b->env_nobs * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

int hb_env_step_dev(hb_batch* b, const float* action_dev, int n_substeps, float* obs_dev, float* reward_dev, uint8_t* terminated_dev, uint8_t* truncated_dev) {
  if (!b || !action_dev || n_substeps < 1 || !obs_dev || !reward_dev || !terminated_dev || !truncated_dev) return HB_EINVAL;
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  return env_step_impl(b, action_dev, n_substeps, nullptr, true, obs_dev, reward_dev, terminated_dev, truncated_dev);
}

static int env_step_host(hb_batch* b, const float* action, int n_substeps, float* obs, float* reward, uint8_t* terminated, uint8_t* truncated, bool wait) {
  if (!b || !action || !obs || !reward || !terminated || !truncated) return HB_EINVAL;
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  int n = b->n_env, nu = b->D.dm.nu, nobs = b->env_nobs;
  if (nu) HB_HIP(hipMemcpyAsync(b->d_action, action, (size_t)n * nu * sizeof(float), hipMemcpyHostToDevice, main_stream(b)));
  rc = hb_env_step_dev(b, b->d_action, n_substeps, b->d_obs, b->d_reward, b->d_term, b->d_trunc);
  if (rc != HB_OK) return rc;
  const size_t ob = (size_t)n * nobs * sizeof(float), rb = (size_t)n * sizeof(float);
  if (reinterpret_cast<const uint8_t*>(reward) == reinterpret_cast<const uint8_t*>(obs) + ob && terminated == reinterpret_cast<const uint8_t*>(reward) + rb && truncated == terminated + n) {
    HB_HIP(hipMemcpyAsync(obs, b->d_obs, ob + rb + 2 * (size_t)n, hipMemcpyDeviceToHost, main_stream(b)));  // the caller's buffers are one record too
  } else {
    HB_HIP(hipMemcpyAsync(obs, b->d_obs, ob, hipMemcpyDeviceToHost, main_stream(b)));
    HB_HIP(hipMemcpyAsync(reward, b->d_reward, rb, hipMemcpyDeviceToHost, main_stream(b)));
    HB_HIP(hipMemcpyAsync(terminated, b->d_term, n, hipMemcpyDeviceToHost, main_stream(b)));
    HB_HIP(hipMemcpyAsync(truncated, b->d_trunc, n, hipMemcpyDeviceToHost, main_stream(b)));
  }
  if (wait) HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}
int hb_env_terminal_obs(hb_batch* b, float* terminal_obs) {
  if (!b) return HB_EINVAL;
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipSetDevice(b->device));
  const size_t bytes = (size_t)b->n_env * b->env_nobs * sizeof(float);
  if (!b->d_term_obs) {  // first call: from the next hb_env_step on the env kernel records them
    if (b->d_term_obs.alloc((size_t)b->n_env * b->env_nobs) != HB_OK) return HB_ENOMEM;
    HB_HIP(hipMemsetAsync(b->d_term_obs, 0, bytes, main_stream(b)));
  }
  if (terminal_obs) {
    HB_HIP(hipMemcpyAsync(terminal_obs, b->d_term_obs, bytes, hipMemcpyDeviceToHost, main_stream(b)));
    HB_HIP(hipStreamSynchronize(main_stream(b)));
  }
  return HB_OK;
}
int hb_env_step(hb_batch* b, const float* action, int n_substeps, float* obs, float* reward, uint8_t* terminated, uint8_t* truncated) {
  return env_step_host(b, action, n_substeps, obs, reward, terminated, truncated, true);
}
int hb_env_step_async(hb_batch* b, const float* action, int n_substeps, float* obs, float* reward, uint8_t* terminated, uint8_t* truncated) {
  return env_step_host(b, action, n_substeps, obs, reward, terminated, truncated, false);
}

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
  if (sizes[0] != b->env_nobs || sizes[n_layers] != (cfg->head == HB_ACTOR_SQUASHED ? 2 * nu : nu)) return HB_EINVAL;
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
  const size_t n = b->n_env, nu = dm.nu, nobs = b->env_nobs;
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
  if (sizes[0] != b->env_nobs || sizes[n_layers] != 1) return HB_EINVAL;
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
  const int nobs = b->env_nobs;
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
  const int nobs = b->env_nobs;
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  HB_HIP(hipMemcpy(out, b->d_norm_rec + (size_t)b->norm_k * norm_rec_doubles(nobs), (size_t)(2 * nobs + 4) * sizeof(double), hipMemcpyDeviceToHost));
  return HB_OK;
}

int hb_norm_set_stats(hb_batch* b, const double* in) {
  if (!b || !in || !b->norm_on) return HB_EINVAL;
  const int nobs = b->env_nobs;
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
  const int nobs = b->env_nobs;
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  HB_HIP(hipMemcpy(out, b->d_norm_rec + (size_t)b->norm_k * norm_rec_doubles(nobs) + 2 * nobs + 4, 4 * sizeof(double), hipMemcpyDeviceToHost));
  return HB_OK;
}

// the fields every launch of the normaliser shares
static NormDesc norm_desc(hb_batch* b) {
  const hb_norm_config& c = b->norm_cfg;
  NormDesc d;
  memset(&d, 0, sizeof d);
  d.nobs = b->env_nobs;
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

int hb_env_warnings(hb_batch* b, int* warnings) {
  if (!b || !warnings) return HB_EINVAL;
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipSetDevice(b->device));
  hipStream_t st = main_stream(b);
  std::vector<int> seen((size_t)b->n_env);
  HB_HIP(hipMemcpyAsync(warnings, b->d_status, seen.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  HB_HIP(hipMemcpyAsync(seen.data(), b->d_seen, seen.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  HB_HIP(hipMemsetAsync(b->d_seen, 0, seen.size() * sizeof(int), st));
  HB_HIP(hipStreamSynchronize(st));
  for (size_t e = 0; e < seen.size(); e++) warnings[e] |= seen[e];
  return HB_OK;
}

int hb_env_joint_torques(hb_batch* b, float* qfrc) {
  if (!b || !qfrc) return HB_EINVAL;
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipSetDevice(b->device));
  hipStream_t st = main_stream(b);
  HB_HIP(hipMemcpyAsync(qfrc, b->d_qfrc, (size_t)b->n_env * b->D.dm.nv * sizeof(float), hipMemcpyDeviceToHost, st));
  HB_HIP(hipStreamSynchronize(st));
  return HB_OK;
}

}  // extern "C"
