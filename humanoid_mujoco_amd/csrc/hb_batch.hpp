// hb_batch.hpp — internal to libhb.so: the model and batch handles behind include/hb.h, the owner of their device memory, and the
// launch plumbing (hb_batch.cpp) the C-ABI translation units (hb_api.cpp, hb_api_rollout.cpp, hb_api_env.cpp, hb_api_policy.cpp,
// hb_api_collect.cpp, hb_api_dyn.cpp, hb_api_ppo.cpp, hb_api_sac.cpp) share.
#pragma once
#include "../../include/hb.h"
#include "hb_device.hpp"
#include "hb_launch.hpp"
#include "hb_learn_host.hpp"
#include "hb_model.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace hb;

struct hb_model {
  Model m;
};

namespace hb {

int refuse_with(const char* why);  // HB_EINVAL, with `why` (a string literal) left for hb_error() (hb_api_env.cpp)
void refuse_clear();               // hb_error() reads "" again: at the entry of every function that may call refuse_with
inline void set_err(char* err, int err_sz, const std::string& s) {
  if (err && err_sz > 0) { snprintf(err, err_sz, "%s", s.c_str()); }
}

// HB_DEBUG=1 in the environment names the failing HIP call on stderr
inline bool hb_debug() { static const bool on = getenv("HB_DEBUG") != nullptr; return on; }
// a call whose failure is not fatal (teardown paths): still named under HB_DEBUG, and never left behind as the
// thread's sticky last error for an unrelated launch to trip over
#define HB_IGN(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    if (hb_debug()) fprintf(stderr, "[hb] %s:%d: %s -> %s (ignored)\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
    (void)hipGetLastError(); } } while (0)
#define HB_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    if (hb_debug()) fprintf(stderr, "[hb] %s:%d: %s -> %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
    return HB_ENODEVICE; } } while (0)

// The owner of one device allocation of T (or of none: a null pointer, which call sites read as "this feature is off").  All device
// memory of a DeviceModel and of an hb_batch is held through these, so whatever is allocated is released with its owner.
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t capacity() const { return cap_; }
  void reset() {
    if (p_) HB_IGN(hipFree(p_));
    p_ = nullptr; cap_ = 0;
  }
  // first use allocates exactly n elements (zero: and fills them with zero bytes); nothing when the buffer is there already
  int alloc(size_t n, bool zero = false) {
    if (p_) return HB_OK;
    if (hipMalloc((void**)&p_, n * sizeof(T)) != hipSuccess) { p_ = nullptr; return HB_ENOMEM; }
    cap_ = n;
    if (zero) {
      // (the fill runs on the null stream, which a batch's non-blocking stream does not wait for: it is complete before anyone launches)
      HB_HIP(hipMemset(p_, 0, n * sizeof(T)));
      HB_HIP(hipStreamSynchronize(nullptr));
    }
    return HB_OK;
  }
  // grow only: room for n elements; a buffer that has to grow loses its contents, and is empty when that fails
  int reserve(size_t n) {
    if (n <= cap_) return HB_OK;
    reset();
    return alloc(n);
  }
  // trades allocations with another owner: a replacement is built aside and swapped in once nothing can fail any more
  void swap(DevBuf& o) { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;  // elements
};
// buffers that are allocated together are all there or all released
template <class... B>
void reset_all(B&... bufs) { (bufs.reset(), ...); }

// The owner of one installed MLP as the 16-row fused kernels read it (hb_mlp_layers.inl): per layer the weights W[K][N] (row-major) in
// the B-operand order of v_mfma_f32_16x16x4_f32 and the bias, and the activation behind the hidden layers (HB_ACT_*: every installation
// starts with tanh; hb_mlp_set_activation changes it).  layers 0: none installed.
struct DevMlp {
  short layers = 0;          // (two shorts in the place of the one int this held: the batch handle keeps its layout)
  short act = HB_ACT_TANH;
  int sizes[5] = {0, 0, 0, 0, 0};
  DevBuf<float> wp[4], b[4];

  // wp[tile][k/4][lane] = W[4(k/4) + lane/16][16 tile + lane%16], zero padded: one coalesced 256-byte wave load per MFMA
  static std::vector<float> pack_mfma_b(const float* W, int K, int N) {
    const int KK = (K + 3) / 4, ntile = (N + 15) / 16;
    std::vector<float> out((size_t)ntile * KK * 64, 0.f);
    for (int nt = 0; nt < ntile; nt++)
      for (int kk = 0; kk < KK; kk++)
        for (int ln = 0; ln < 64; ln++) {
          const int k = 4 * kk + (ln >> 4), n = 16 * nt + (ln & 15);
          if (k < K && n < N) out[((size_t)nt * KK + kk) * 64 + ln] = W[(size_t)k * N + n];
        }
    return out;
  }
  // its inverse: W[K][N] from the packed operand (the learners read the installed networks back)
  static std::vector<float> unpack_mfma_b(const std::vector<float>& packed, int K, int N) {
    std::vector<float> W((size_t)K * N);
    for (int k = 0; k < K; k++)
      for (int n = 0; n < N; n++) W[(size_t)k * N + n] = packed[packed_b_index(k, n, K)];
    return W;
  }
  void clear() {
    layers = 0;
    act = HB_ACT_TANH;
    for (int l = 0; l < 4; l++) reset_all(wp[l], b[l]);
  }
  // Replaces the network (arguments checked by the caller: mlp_args_ok; nothing on the device still reads the old one).  Only the device
  // can fail here, and then no network is installed.
  int install(int n_layers, const int* sz, const float* const* weights, const float* const* biases) {
    clear();
    for (int l = 0; l < n_layers; l++) {
      const std::vector<float> packed = pack_mfma_b(weights[l], sz[l], sz[l + 1]);
      if (wp[l].alloc(packed.size()) != HB_OK || b[l].alloc(sz[l + 1]) != HB_OK) { clear(); return HB_ENOMEM; }
      if (hipMemcpy(wp[l], packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(b[l], biases[l], sz[l + 1] * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { clear(); return HB_ENODEVICE; }
    }
    for (int l = 0; l <= n_layers; l++) sizes[l] = sz[l];
    layers = (short)n_layers;
    return HB_OK;
  }
  PolicyDesc desc() const {
    PolicyDesc pd;
    memset(&pd, 0, sizeof pd);
    pd.nl = layers;
    int widest = 1;
    for (int l = 0; l <= layers; l++) { pd.sizes[l] = sizes[l]; widest = std::max(widest, sizes[l]); }
    for (int l = 0; l < layers; l++) { pd.w[l] = wp[l]; pd.b[l] = b[l]; }
    pd.ldx = widest + 4;  // + the K pad columns (K is swept four at a time); 16-row tiles
    pd.act = act;
    return pd;
  }
};
// what every hb_*_set_mlp checks of its arrays before it touches the batch; the widths' upper limit and the end widths are the caller's
inline bool mlp_args_ok(int n_layers, const int* sizes, const float* const* weights, const float* const* biases) {
  if (!sizes || !weights || !biases || n_layers < 1 || n_layers > 4) return false;
  for (int l = 0; l <= n_layers; l++) if (sizes[l] < 1) return false;
  for (int l = 0; l < n_layers; l++) if (!weights[l] || !biases[l]) return false;
  return true;
}

// What the learners of a batch share (hb_learn_host.cpp): the trainable parameters of up to three networks as ONE flat record (per
// network its layers W | b; what else the record holds is the learner's), the gradient and the Adam moments in the same layout, the
// packed transposes of the weights the backward pass multiplies by (LearnNet: which layers have one), and the scratch of a minibatch.
// The forward operands stay where they are: in the batch's networks (DevMlp), which the Adam kernels refresh entry by entry.
struct LearnNets {
  int n;
  const DevMlp* net[3];  // in the order of the record
  int k0[3];             // LearnNet::k0 of each
};
struct LearnerCore {
  bool on = false;
  int P = 0;
  int off_w[3][4] = {}, off_b[3][4] = {};
  DevBuf<float> d_param, d_grad, d_m, d_v, d_zero, d_wt[3][4];
  DevBuf<float> d_scratch;     // activations, dZ, outputs and the by-row terms of a minibatch: grows with mb
  DevBuf<float> d_part;        // [64][P] chunk partials of the gradient
  DevBuf<double> d_dbl;        // the learner's fp64 partials
  void clear() {
    on = false; P = 0;
    reset_all(d_param, d_grad, d_m, d_v, d_zero, d_scratch, d_part);
    d_dbl.reset();
    for (int k = 0; k < 3; k++) for (int l = 0; l < 4; l++) d_wt[k][l].reset();
  }
  // network k as plain data (hb_learn_host.hpp); with_t false: without the transposes (a target network, which has none)
  LearnNet view(const LearnNets& ns, int k, bool with_t = true) const;
  // the layers of network k from entry o of the record on; returns the entry behind them
  int layout(const LearnNets& ns, int k, int o) { return learn_layout(ns.net[k]->layers, ns.net[k]->sizes, o, off_w[k], off_b[k]); }
  // the record of P entries, its gradient, moments (zero) and the zero bias of the reversed networks; d_dbl with ndbl zeros
  int alloc_record(size_t ndbl);
  // the flat record of what is installed: the networks' packed operands read back from the device; every other entry 0
  int read_installed(const LearnNets& ns, std::vector<float>& flat) const;
  // the flat record to the device: the master copy and every operand the kernels read (forward: only with `forward`; the packed
  // transposes always).  The stream is idle.
  int write_params(const LearnNets& ns, const float* flat, bool forward);
  // room for `need` floats of scratch and nchunk chunk partials (a call still in flight uses the buffers that are replaced: the
  // stream is synchronised before they grow)
  int reserve_scratch(size_t need, int nchunk, hipStream_t st);
  // count == P entries of a device record to the host, behind whatever is in flight on the batch's stream; HB_EINVAL: no learner, or another count
  int download(hb_batch* b, const float* dev, float* out, long long count) const;
  // the record and the moments, P entries each (get: behind whatever is in flight; set_moments: the stream is idle)
  int get_record(hb_batch* b, float* params, float* m, float* v) const;
  int set_moments(const float* m, const float* v);
};

// The PPO learner of a batch (hb_learner_*, hb_api_ppo.cpp): the record is the actor's layers, log_std, the critic's layers
// (include/hb.h); layer 0 needs no transpose.
struct Learner : LearnerCore {
  hb_ppo_config cfg = {};
  int off_log_std = 0;
  long long calls = 0;         // Adam calls since t was last set; t = calls - the device's count of skipped steps
  bool log_std_dirty = false;  // the device's log_std is newer than actor_cfg.log_std
  DevBuf<int> d_nskip;         // (d_dbl: advpart [64][2] | statpart [64][8] | normpart)
  void clear() {
    LearnerCore::clear();
    calls = 0; log_std_dirty = false;
    d_nskip.reset();
  }
};

// The SAC learner of a batch (hb_sac_*, hb_api_sac.cpp): the record is the actor's layers, Q1's, Q2's, log_ent_coef (include/hb.h);
// the targets (their record, Q1' then Q2', and the packed operands their forward pass reads); wt[net][0] of a Q network is the
// transpose of layer 0's action rows.
struct SacLearner : LearnerCore {
  hb_sac_config cfg = {};
  int PT = 0, off_q = 0;       // off_q: where Q1's stretch begins; the targets' record mirrors [off_q, P - 1)
  long long t = 0;
  DevMlp tq[2];
  DevBuf<float> d_target, d_alpha;  // (d_dbl: statpart [64][kSacSrow])
  void clear() {
    LearnerCore::clear();
    PT = off_q = 0; t = 0;
    tq[0].clear(); tq[1].clear();
    reset_all(d_target, d_alpha);
  }
};

// One block of the device copies of a host call's arrays: count floats (none: the block is not there, and dev stays null), filled from
// `up` before the launch where that is given and copied to `down` behind it where that is given.
struct StageBlock {
  size_t count;
  const float* up;
  float* down;
  float* dev;
};
// The host form of a read-out: carves the blocks out of buf, each 16-byte aligned (buf grows on demand; it is idle: the host form before
// this one ended synchronised), uploads, runs launch() - which takes the blocks' device pointers -, downloads and ends synchronised.
template <class Launch>
int staged_call(DevBuf<float>& buf, StageBlock* blk, int nblk, hipStream_t stream, Launch&& launch) {
  auto r4 = [](size_t x) { return (x + 3) & ~(size_t)3; };
  size_t total = 4;  // (never an empty allocation)
  for (int i = 0; i < nblk; i++) total += r4(blk[i].count);
  if (buf.reserve(total) != HB_OK) return HB_ENOMEM;
  float* p = buf;
  for (int i = 0; i < nblk; i++) {
    blk[i].dev = blk[i].count ? p : nullptr;
    p += r4(blk[i].count);
    if (blk[i].count && blk[i].up) HB_HIP(hipMemcpyAsync(blk[i].dev, blk[i].up, blk[i].count * sizeof(float), hipMemcpyHostToDevice, stream));
  }
  const int rc = launch();
  if (rc != HB_OK) return rc;
  for (int i = 0; i < nblk; i++)
    if (blk[i].count && blk[i].down) HB_HIP(hipMemcpyAsync(blk[i].down, blk[i].dev, blk[i].count * sizeof(float), hipMemcpyDeviceToHost, stream));
  HB_HIP(hipStreamSynchronize(stream));
  return HB_OK;
}

struct DeviceModel {
  DevModel dm;
  DevBuf<int> d_int;
  DevBuf<float> d_flt;
  DevBuf<unsigned long long> d_u64;
  DevBuf<float> d_qpos_src;  // qpos0 followed by keyframes, fp32
  DevBuf<DevModel> d_dm;     // device copy of dm (the step kernel reads the tables through it)
  DevBuf<DevModel> d_dm_fast;  // variant 2 only: the same model with the variant-1 LDS layout (fast step kernel of the staged step)
  int fast_lds_floats = 0;
  bool sized_h27 = false;  // sizes and LDS layout equal kSizedHumanoid27's: the size-specialised step kernel applies
  bool sized_team = false; // the fast layout equals kSizedTeamV1's
  // observation order tables (device pointers): joint order and, when it exists, actuator order (hb_env_config.obs_actuator_order)
  const int *obs_jnt_joint = nullptr, *obs_src_joint = nullptr, *obs_jnt_act = nullptr, *obs_src_act = nullptr;
  bool has_act_order = false;
};

}  // namespace hb

struct hb_batch {
  const hb_model* model = nullptr;
  DeviceModel D;
  int n_env = 0, device = 0;
  hipStream_t stream = nullptr;
  // device memory: every buffer is a DevBuf member (null until the feature that needs it allocates it), released when the batch is deleted
  DevBuf<float> d_state, d_ctrl, d_xfrc, d_diag_qacc, d_diag_force, d_diag_contact;
  DevBuf<uint8_t> d_record;  // the env adapter's outputs as one block: obs [n_env][nobs] | reward [n_env] | terminated [n_env] | truncated [n_env]
  float *d_obs = nullptr, *d_reward = nullptr;  // (its parts)
  uint8_t *d_term = nullptr, *d_trunc = nullptr;
  DevBuf<int> d_seen;        // [n_env] warning bits of episodes that ended since the last hb_env_warnings
  DevBuf<float> d_term_obs;  // [n_env][nobs] observations of the states episodes ended in (hb_env_terminal_obs), null until asked for
  DevBuf<uint8_t> d_mask;
  DevBuf<int> d_status, d_counts;
  DevBuf<float> d_qpos_out, d_qvel_out;
  DevBuf<float> d_task_out;  // task returns and stage costs
  float xfrc_std = 0.f, xfrc_rate = 0.f;  // rollout noise (hb_rollout_noise)
  int tape_steps = 0;                      // steps of the action tape hb_ctrl_tape_splines left in d_ctrl (0: none)
  DevBuf<float> d_knots;                   // spline nodes and node times staged for it
  unsigned xfrc_seed = 0, xfrc_calls = 0;
  DevBuf<float> d_sensor_out;
  bool diag = false;
  // contact-force read-out (hb_contact_readout): [n_env][ncon_max][6] and [n_env][nbody][6]; a sensor spec with touch / contact-force
  // entries allocates them as well and hands them to its own launches only
  DevBuf<float> d_contact_force, d_body_contact;
  bool contact_readout = false;
  // body-acceleration read-out (hb_body_acc_readout): [n_env][nbody][6], and the scratch the step kernel parks a body's kinematics in
  // across the solver, [n_env][nbody][kAccPark]; a sensor spec with accelerometer / frame-acceleration entries allocates them as well
  DevBuf<float> d_body_acc, d_body_acc_park;
  bool body_acc_readout = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  DevBuf<unsigned long long> d_stamps;
  // staged step of the general variants: the buffers, and the kernel argument that points into them (all null: fused)
  DevBuf<float> d_stage_geom;
  DevBuf<int4> d_stage_item;
  DevBuf<int> d_stage_nsearch, d_stage_nwork, d_stage_defer;  // defer: flags | list | counters
  DevBuf<float4> d_stage_result;
  StageBufs stage = {};
  // env adapter (hb_env_*)
  EnvConfig env_cfg = {};
  bool env_ready = false;
  DevBuf<float> d_prev, d_latest, d_qfrc, d_action;
  DevBuf<float> d_inv;  // hb_inverse's device copies: qacc [n_env][nv] | qfrc_inverse [n_env][nv] | warnings [n_env] (allocated by its first call)
  DevBuf<int> d_inv_scratch;  // hb_inverse_dev: the counts [n_env][kCountStride] | status [n_env] its launches write instead of the batch's
  DevBuf<float> d_kin;     // hb_kinematics / hb_kinematics_states: device copies of their host arrays (outputs | qpos | qvel), grown on demand
  DevBuf<float> d_dyn;     // hb_dynamics / hb_dynamics_states: device copies of their host arrays (outputs | qpos | qvel), grown on demand
  // ray read-out (hb_ray_configure, hb_rays*): the installed rays, pnt [n_ray][3] | vec [n_ray][3], and the eligible geoms in ascending order;
  // the scratch hb_rays* runs the kinematics read-out into, body poses [n_env][nbody][10] | geom poses [n_env][ngeom][7] (allocated only for
  // a configuration that needs either); the device copies of hb_rays' host arrays, dist [n_env][n_ray] | geomid [n_env][n_ray]
  DevBuf<float> d_ray, d_ray_kin, d_ray_out;
  DevBuf<int> d_ray_geoms;
  hb_ray_spec ray_spec = {};
  int n_ray = 0, ray_ngeom = 0;                  // n_ray 0: nothing configured
  bool ray_moving = false, ray_hfield = false;   // a geom of a moving body / a height field is among the eligible geoms
  // the layout of every row the adapter produces (hb_device.hpp: EnvRow): every consumer of them is sized by row.width (hb_env_nobs);
  // row.base is D.dm.nobs, which the policy kernels and compute_obs keep
  EnvRow row = {};
  // observation extension (hb_env_obs_extend): the scan cast before the env kernel, [n_env][n_ray], and the envs the env kernel reset,
  // [n_env], for the masked second cast; both null without a scan
  hb_obs_ext obs_ext = {};
  DevBuf<float> d_ext_scan;
  DevBuf<uint8_t> d_ext_reset;
  // velocity commands (hb_env_commands_configure): the configuration and every env's record (cx, cy, cyaw, draw count), null while
  // none is installed
  EnvCommands cmd_cfg = {};
  DevBuf<float4> d_cmd;
  // foot-contact terms (hb_env_feet_configure): the configuration and every env's record, null while none is installed
  EnvFeet feet_cfg = {};
  DevBuf<FeetRec> d_feet;
  DevBuf<int> d_episode;
  int env_offset = 0;
  // realism layer (hb_env_randomize)
  EnvRand env_rand = {};
  DevBuf<int> d_rs_k_act, d_rs_k_obs, d_rs_delay;
  DevBuf<float> d_rs_fifo_act, d_rs_fifo_joint, d_rs_fifo_gyro, d_rs_fifo_grav, d_rs_push;
  EnvRandState rs = {};     // the kernel argument that points into them; all null while off
  bool rand_on = false;
  DomainRand dom_rand = {};    // hb_env_domain_randomize
  DevBuf<float> d_dr;          // [n_env][dr_stride] per-env model parameters, null while off
  int dr_stride = 0;
  DevBuf<uint8_t> d_rmask;     // hb_env_reset's pending-envs mask
  DevBuf<int> d_pending;
  // policy MLP (hb_policy_*): the installed network; for a network with a width above 256, which takes one launch per layer instead of
  // hb_policy_kernel, also the unpacked weights and the hidden activations (ping-pong), null otherwise
  DevMlp policy;
  bool mlp_fused = false;
  DevBuf<float> d_mlp_w[4];
  DevBuf<float> d_mlp_h[2];
  DevBuf<float> d_mlp_act;   // activation scratch of the LDS-free policy kernel: [n_env / 16 + kPipes][2][16][widest + 4]
  // sampling actor (hb_actor_set_mlp, hb_env_collect_dev): the network of hb_actor_kernel, the head, and the number of steps collected
  // since the actor was installed (the step counter of its random draws)
  DevMlp actor;
  hb_actor_config actor_cfg = {};
  unsigned actor_draw0 = 0;
  // critic (hb_critic_set_mlp, hb_collect_gae_dev): the network of hb_value_kernel, and the scratch the value and terminal-value tapes go
  // to when the caller gives none, [2 T + 1][n_env], grown on demand
  DevMlp critic;
  DevBuf<float> d_gae;
  // PPO learner (hb_learner_create): off until created
  Learner learner;
  // Q networks (hb_q_set_mlp, hb_q_values_dev) over obs | action, and the SAC learner (hb_sac_create): off until created
  DevMlp q[2];
  SacLearner sac;
  // normaliser (hb_norm_*): the double-buffered statistics record (slot norm_k is current; hb_device.hpp: NormDesc), the per-env
  // accumulators ret | ep_ret [2][n_env] and ep_len [n_env], and the chunk partials of a step; all null while none is configured
  bool norm_on = false;
  hb_norm_config norm_cfg = {};
  int norm_k = 0;
  DevBuf<double> d_norm_rec, d_norm_env, d_norm_part;
  DevBuf<int> d_norm_len;
  // optional per-kernel timing of the step kernel (hb_step_timing)
  bool time_steps = false;
  std::vector<hipEvent_t> tev;  // pairs
  int tev_used = 0;
  long long launch_count = 0;
  const char* last_kernel = "";  // hb_last_kernel
  // run-time choices between kernels / schedules that give the same results (hb_batch_tune, include/hb.h: HB_TUNE_*), indexed by knob
  int tune[HB_TUNE_COUNT] = {getenv("HB_DUO") ? atoi(getenv("HB_DUO")) : 1, 1, 1, 1, 1, 1, 1, 4, 1, kFoldMax, 1};
  // hb_step_dev calls not launched yet (fold_steps): the launch parameters they share, and the controls of each
  BatchPtrs fold_P;
  const float* fold_ctrl[kFoldMax] = {};
  int fold_n = 0;
  DevBuf<int> d_order;      // heavy-first dispatch order (hb_order_kernel), valid once a step has run
  DevBuf<int> d_order2;     // the same for the narrowphase launch of a staged step
  int order_mode = 0;       // 0: none yet, 1: one permutation of the whole batch, 2: one permutation per pipe segment
  bool schedule = true;  // heavy-first dispatch order (HB_TUNE_SCHEDULE)
  // Pipelined stepping (hb_batch_pipeline): the batch is cut into npipe fixed env segments, each stepped by
  // its own launch on its own stream.  Envs are independent, so segment c of step t+1 only has to follow
  // segment c of step t: the tail of one step (its slowest envs) overlaps the head of the next.  `stream`
  // stays the batch's ordering point: pipes fork from it at every step call and are joined back into it
  // before anything else is enqueued on it.
  static constexpr int kPipes = 8;  // most segments; npipe of them in use (streams are created when first asked for)
  int npipe = 0;                    // 0: unpipelined
  int probed_segments = 0;          // what hb_batch_pipeline(b, 1)'s probe of the segment streams found (0: not probed yet); the streams are kept, so is the answer
  bool forked = false;
  hipStream_t pipe[kPipes] = {};
  hipEvent_t ev_fork = nullptr, ev_pipe[kPipes] = {};
  int join_error = 0;
  bool main_dirty = true;  // work was enqueued on `stream` since the pipes last forked from it
};

// ---- launch plumbing (hb_batch.cpp); internal to the library
#pragma GCC visibility push(hidden)
namespace hb {
bool build_device_model(const Model& m, DeviceModel& D, std::string& err);
// the batch's control buffer for WRITING: whatever hb_ctrl_tape_splines left there is gone afterwards, so a later
// HB_CTRL_TAPE rollout must fail (HB_EINVAL) instead of rolling out stale controls
inline float* ctrl_for_write(hb_batch* b) { b->tape_steps = 0; return b->d_ctrl; }
int ensure_ctrl(hb_batch* b, size_t floats);
int ensure_xfrc(hb_batch* b);
int alloc_contact_readout(hb_batch* b);
int alloc_body_acc_readout(hb_batch* b);
int reset_impl(hb_batch* b, const uint8_t* mask, int keyframe, float perturb_scale, int env_offset);
bool staged_on(const hb_batch* b);
BatchPtrs make_ptrs(hb_batch* b);
int sensor_args(const Model& m, const DevModel& dm, const hb_sensor_spec* spec, int tail, SensorArgs& S);  // (hb_api_rollout.cpp)
void join_pipes(hb_batch* b);
int flush_steps(hb_batch* b);
hipStream_t main_stream(hb_batch* b);
int reorder_period(const hb_batch* b);
int segment_count(const hb_batch* b);
struct Segment { int lo, hi; hipStream_t st; };
Segment segment(hb_batch* b, int c, int nseg);
int fork_pipes(hb_batch* b, int nseg);
hipError_t launch_batch_step(hb_batch* b, const BatchPtrs& P, int nsteps, hipStream_t stream);
int launch_segment(hb_batch* b, BatchPtrs P, int nsteps, const Segment& sg, int nseg, bool reorder);
void steps_enqueued(hb_batch* b, int nseg, bool reorder, bool refreshed = false);
int launch_steps(hb_batch* b, BatchPtrs& P, int nsteps, bool foldable = false);
int rollout_open(hb_batch* b, const float* ctrl, int T, bool want_qpos);
// the learner's hooks in the calls that read or replace what it trains (hb_api_ppo.cpp): before a descriptor with log_std is built;
// behind hb_actor_set_mlp / hb_critic_set_mlp (net 0 / 1) once the new network is installed, shapes_same telling whether the sizes stayed
int learner_sync_log_std(hb_batch* b);
int learner_net_replaced(hb_batch* b, int net, bool shapes_same);
// behind a change of the actor's or the critic's hidden activation: the learner is destroyed, the actor keeps the log_std it trained
int learner_activation_changed(hb_batch* b);
// both learners (hb_learn_host.cpp): the batch's device current and nothing in flight on its stream
int learner_idle(hb_batch* b);
// the installed rays as the scan of the observation extension (hb_api.cpp): the poses they need, then the ray kernel with the extension's
// transform, for every env or those of `mask`, into the scan columns of `rows` (rows of the batch's layout), or with rows null into
// d_ext_scan [n_env][n_ray]; hb_last_kernel stays what it was
int rays_scan_launch(hb_batch* b, const uint8_t* mask, float* rows);
// the env adapter (hb_api_env.cpp) as the policy and the collection loop use it: the adapter's buffers on first use; reward / termination /
// observation of every env (or those of `mask`); one env step; whether anything sized by the observation exists
int env_alloc(hb_batch* b);
int env_eval(hb_batch* b, bool step, bool observe, const uint8_t* mask, float* d_obs, float* d_reward, uint8_t* d_term, uint8_t* d_trunc);
int env_step_impl(hb_batch* b, const float* action_dev, int n_substeps, const uint8_t* mask, bool step, float* obs_dev, float* reward_dev,
                  uint8_t* terminated_dev, uint8_t* truncated_dev);
bool obs_consumers_exist(const hb_batch* b);
}  // namespace hb
#pragma GCC visibility pop
