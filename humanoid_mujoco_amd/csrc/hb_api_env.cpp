// hb_api_env.cpp — the C-ABI of libhb.so (include/hb.h), the env adapter: observations, rewards and resets, the row layout, the realism
// layer and domain randomisation, the observation extension, velocity commands, foot-contact terms, and the env step.
#include "hb_batch.hpp"

namespace hb {

int env_alloc(hb_batch* b) {
  if (b->env_ready) return HB_OK;
  const DevModel& dm = b->D.dm;
  size_t n = b->n_env;
  HB_HIP(hipSetDevice(b->device));
  const size_t nu = std::max(1, dm.nu);
  // one record [obs n x nobs | reward n | terminated n | truncated n]: a host that keeps its four buffers in the same order and
  // back to back (engine.py does) gets them in one transfer instead of four
  // (nobs: the adapter's row, the model's observation and what hb_env_obs_extend appends)
  int rc = b->d_record.alloc(n * b->row.width * sizeof(float) + n * sizeof(float) + 2 * n);
  if (rc == HB_OK) rc = b->d_prev.alloc(n * nu, /*zero=*/true);
  if (rc == HB_OK) rc = b->d_latest.alloc(n * nu, /*zero=*/true);
  if (rc == HB_OK) rc = b->d_action.alloc(n * nu);
  if (rc == HB_OK) rc = b->d_qfrc.alloc(n * dm.nv, /*zero=*/true);
  if (rc == HB_OK) rc = b->d_episode.alloc(n, /*zero=*/true);
  if (rc == HB_OK) rc = b->d_seen.alloc(n, /*zero=*/true);
  if (rc != HB_OK) { reset_all(b->d_record, b->d_prev, b->d_latest, b->d_action, b->d_qfrc, b->d_episode, b->d_seen); return rc; }
  b->d_obs = reinterpret_cast<float*>(b->d_record.get());
  b->d_reward = b->d_obs + n * b->row.width;
  b->d_term = reinterpret_cast<uint8_t*>(b->d_reward + n);
  b->d_trunc = b->d_term + n;
  hb_env_config def;
  hb_env_default_config(b->model, &def);
  static_assert(sizeof(hb_env_config) == sizeof(EnvConfig), "hb_env_config and EnvConfig must have the same layout");
  memcpy(&b->env_cfg, &def, sizeof def);
  b->env_ready = true;
  return HB_OK;
}

// reward / termination / observation of every env (or those of `mask`).  step: a step of the episode (hb_env_step*, hb_env_collect*): it
// may reset an env in place, redraw a command inside an episode and write the feet records; not hb_get_obs, not the settle step or the
// final observation of hb_env_reset.  observe: push the observation through the realism layer's noise and delay lines instead of
// returning the true one.
int env_eval(hb_batch* b, bool step, bool observe, const uint8_t* mask, float* d_obs, float* d_reward, uint8_t* d_term, uint8_t* d_trunc) {
  const Model& m = b->model->m;
  EnvArgs G;
  memset(&G, 0, sizeof G);
  G.cfg = b->env_cfg;
  if (!step) G.cfg.auto_reset = 0;
  G.R = b->env_rand;
  if (b->rand_on) G.S = b->rs;
  G.D = b->dom_rand;
  G.state = b->d_state; G.qfrc = b->d_qfrc; G.counts = b->d_counts; G.prev = b->d_prev; G.latest = b->d_latest;
  G.qpos_src = b->D.d_qpos_src + (G.cfg.reset_keyframe < 0 || G.cfg.reset_keyframe >= m.nkey ? 0 : (size_t)(1 + G.cfg.reset_keyframe) * m.nq);
  G.episode = b->d_episode; G.status = b->d_status;
  G.obs = d_obs; G.reward = d_reward; G.terminated = d_term; G.truncated = d_trunc;
  G.mask = mask; G.observe = observe ? 1 : 0; G.step = step ? 1 : 0;
  G.dr = b->d_dr; G.dr_stride = b->dr_stride; G.n_env = b->n_env; G.env_offset = b->env_offset;
  G.term_obs = observe ? b->d_term_obs.get() : nullptr; G.seen = b->d_seen;
  G.row = b->row;
  if (b->d_cmd) { G.cmd = b->d_cmd; G.C = b->cmd_cfg; }
  if (b->d_feet) { G.feet = b->d_feet; G.body_contact = b->d_body_contact; G.F = b->feet_cfg; }
  // the scan is cast here, at the state the step left (an episode that ends below ends in it, over the elevations it was run on); the
  // env kernel copies it into the rows it writes; the envs it resets get the scan of their new state, over their new elevations, from a
  // second cast masked to them
  if (b->row.n_scan) {
    G.scan = b->d_ext_scan; G.reset_flag = G.cfg.auto_reset ? b->d_ext_reset.get() : nullptr;
    const int rc = rays_scan_launch(b, nullptr, nullptr);
    if (rc != HB_OK) return rc;
  }
  HB_HIP(launch_env(b->D.dm, G, main_stream(b)));
  return G.reset_flag ? rays_scan_launch(b, G.reset_flag, d_obs) : HB_OK;
}

bool obs_consumers_exist(const hb_batch* b) {
  return b->actor.layers >= 1 || b->critic.layers >= 1 || b->q[0].layers >= 1 || b->q[1].layers >= 1 || b->norm_on || b->learner.on || b->sac.on;
}

// CPUEnv._apply_action (+ pushes) -> n_substeps x mj_step -> reward / termination / observation, for every env or those of `mask`
int env_step_impl(hb_batch* b, const float* action_dev, int n_substeps, const uint8_t* mask, bool step, float* obs_dev, float* reward_dev,
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
  return env_eval(b, step, true, mask, obs_dev, reward_dev, terminated_dev, truncated_dev);
}

}  // namespace hb

extern "C" {

int hb_get_obs(hb_batch* b, float* obs, float* reward, uint8_t* terminated, uint8_t* truncated) {
  if (!b || !obs) return HB_EINVAL;
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  int n = b->n_env, nobs = b->row.width;
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

int hb_env_nobs(hb_batch* b) { return b ? b->row.width : HB_EINVAL; }

int hb_env_row(hb_batch* b, struct hb_env_row* out) {
  if (!b || !out) return HB_EINVAL;
  static_assert(sizeof(struct hb_env_row) == sizeof(EnvRow), "hb_env_row and EnvRow must have the same layout");
  memcpy(out, &b->row, sizeof *out);
  return HB_OK;
}

// the batch's rows laid out as `row` (env_row() of what the caller proposes): the record and the terminal-observation table get rows of
// its width (the stream is idle); a failure leaves the batch as it was
static int env_relayout(hb_batch* b, const EnvRow& row) {
  const int total = row.width;
  if (total != b->row.width) {
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
  }
  b->row = row;
  return HB_OK;
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
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));  // (a step still in flight writes the buffers that are replaced below)
  // the scan's scratch first: a failure here leaves the batch as it was
  DevBuf<float> scan;
  DevBuf<uint8_t> flag;
  if (x.height_scan && (scan.alloc((size_t)b->n_env * b->n_ray) != HB_OK || flag.alloc((size_t)b->n_env, /*zero=*/true) != HB_OK)) return HB_ENOMEM;
  const EnvRow& W = b->row;
  const int rc = env_relayout(b, env_row(W.base, x.prev_action ? b->D.dm.nu : 0, x.height_scan ? b->n_ray : 0, W.n_foot_contact, W.n_command != 0));
  if (rc != HB_OK) return rc;
  b->d_ext_scan.swap(scan);
  b->d_ext_reset.swap(flag);
  b->obs_ext = x;
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
  const EnvRow& W = b->row;
  const bool was = W.n_command != 0, now = cfg && cfg->observe;
  if (was != now && obs_consumers_exist(b))
    return cmd_refuse("commands: the observation width would change while an actor, critic, Q network, normaliser or learner exists");
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));  // (a step still in flight reads the buffers that are replaced below)
  DevBuf<float4> rec;
  const bool fresh = cfg && !b->d_cmd;
  if (fresh && rec.alloc((size_t)b->n_env, /*zero=*/true) != HB_OK) return HB_ENOMEM;
  if ((rc = env_relayout(b, env_row(W.base, W.n_prev_action, W.n_scan, W.n_foot_contact, now))) != HB_OK) return rc;
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
  const EnvRow& W = b->row;
  const int was = W.n_foot_contact, now = cfg && cfg->observe ? cfg->n_feet : 0;
  if (was != now && obs_consumers_exist(b))
    return cmd_refuse("feet: the observation width would change while an actor, critic, Q network, normaliser or learner exists");
  int rc = env_alloc(b);
  if (rc != HB_OK) return rc;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));  // (a step still in flight reads the buffers that are replaced below)
  if (!cfg) {
    if ((rc = env_relayout(b, env_row(W.base, W.n_prev_action, W.n_scan, 0, W.n_command != 0))) != HB_OK) return rc;
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
  if ((rc = env_relayout(b, env_row(W.base, W.n_prev_action, W.n_scan, now, W.n_command != 0))) != HB_OK) {
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

// Episodes begin outside the env kernel, for every env or those of `mask`, with the episode numbers in d_episode: with `src` the state first
// (the reset pose there, perturbed), then the realism layer's episode state and the episode's model parameters
static int env_begin_episodes(hb_batch* b, const uint8_t* mask, const float* src) {
  const EnvConfig& c = b->env_cfg;
  if (src) HB_HIP(launch_reset(b->D.dm, b->d_state, b->d_status, mask, src, b->d_episode, b->n_env, c.reset_perturb, b->env_offset, main_stream(b), c.reset_quat_perturb));
  if (b->rand_on) HB_HIP(launch_envrand_reset(b->D.dm, b->env_rand, b->rs, b->d_episode, mask, b->n_env, b->env_offset, main_stream(b)));
  if (b->d_dr) HB_HIP(launch_domain_rand(b->D.dm, b->dom_rand, b->d_dr, b->dr_stride, b->d_episode, mask, b->n_env, b->env_offset, main_stream(b)));
  return HB_OK;
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
    if ((rc = env_begin_episodes(b, nullptr, nullptr)) != HB_OK) return rc;
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
      if ((rc = env_begin_episodes(b, b->d_rmask, src)) != HB_OK) return rc;
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
  HB_HIP(hipMemcpyAsync(obs, b->d_obs, n * b->row.width * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
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
  int n = b->n_env, nu = b->D.dm.nu, nobs = b->row.width;
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
  const size_t bytes = (size_t)b->n_env * b->row.width * sizeof(float);
  if (!b->d_term_obs) {  // first call: from the next hb_env_step on the env kernel records them
    if (b->d_term_obs.alloc((size_t)b->n_env * b->row.width) != HB_OK) return HB_ENOMEM;
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
