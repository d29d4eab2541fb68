// hb_device.hpp — device-side model tables and batch buffers (fp32), shared by the host
// runtime (hb_tables.cpp, hb_batch.cpp) and the kernel translation units (hb_step.hip, hb_step_duo.hip, hb_narrow.hip, hb_env.hip, hb_rollout.hip, hb_policy.hip, hb_kin.hip, hb_ray.hip, hb_dyn.hip).
//
// The model is replicated read-only per device as two flat arrays (int, float); DevModel holds
// typed pointers into them plus the per-env LDS layout.  All tables are small (a few KB) and
// identical for every env, so lane-indexed reads hit L1/L2 and uniform reads go through the
// scalar cache.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

// Model tables are immutable for the lifetime of a batch: device code addresses them through the
// constant address space so that wave-uniform reads become scalar (s_load) instructions served by
// the scalar cache, even though the kernel also writes global memory.
#if defined(__HIP_DEVICE_COMPILE__)
#define HB_CONST __attribute__((address_space(4)))
#else
#define HB_CONST
#endif

namespace hb {

constexpr int kGroup = 64;      // lanes cooperating on one env (one wavefront)
constexpr int kNconMax = 24;    // contact capacity per env (overflow -> HB_WARN_CONTACTFULL)
constexpr int kNefcMax = 63;    // constraint-row capacity per env (overflow -> HB_WARN_CNSTRFULL); lane 63 / row 63 of C carries the extra right-hand side
// the general instantiations (mesh hulls, height-field prisms, condim 4 / 6: the reference's own robot) with the Newton solver hold
// their rows in kBigGroups groups of 64 (lane l owns rows l, l + 64, ...): 256 rows, 48 contacts
constexpr int kBigGroups = 4;
constexpr int kBigNefcMax = 64 * kBigGroups;
constexpr int kBigNconMax = 48;
// ... and with PGS in kPgsGroups groups with the row-by-row matrix AR in LDS (a condim 4 / 6 model solved by PGS: variant 3): 128 rows
constexpr int kPgsGroups = 2;
constexpr int kPgsNefcMax = 64 * kPgsGroups;
constexpr int kListMax = 128;   // general collision: pairs that survive the broadphase per step (more: HB_WARN_CONTACTFULL)
constexpr int kWorkMax = 256;   // general collision: narrowphase work items (pair or pair x prism) per step
constexpr int kConStride = 20;  // floats per contact record in LDS
constexpr int kDiagConStride = 16;
constexpr int kMetaStride = 4;  // floats per row in the general variants' row meta
constexpr int kMeshChunk = 8;   // neighbour records per climb round's load batch (DevModel::mesh_nbr)
constexpr int kMeshStart = 96;  // start records per mesh: cube map, 6 faces x 4 x 4 (DevModel::mesh_start)
constexpr int kCountStride = 8;  // ints per env in BatchPtrs::counts: ncon, nefc, niter, cost, self-collision flag, spare
constexpr int kBrecQuads = 18;  // float4s per level-ordered body record (see build_model_tables)

// contact record layout in LDS (floats)
enum { C_DIST = 0, C_POS = 1, C_FRAME = 4, C_PAIR = 13, C_ROW = 14, C_DIM = 15, C_FRIC = 16 };

struct DevModel {
  // sizes
  int nq, nv, nu, nbody, njnt, ngeom, ntendon, nM, npair, nlevel, ntree, nlimcand, nhfielddata;
  int nstate;   // floats per env in the global state record: time, qpos, qvel, qacc_warmstart
  int nobs;
  // which instantiation of the step kernel runs this model: 0 classic (plane / sphere / capsule, condim 1 / 3), 1 general collision
  // (mesh hulls and height-field prisms through MPR, condim 1 / 3 / 4 / 6) with the 63-row solvers, 2 general collision + Newton on
  // kBigNefcMax rows, 3 general collision + PGS on kPgsNefcMax rows (a PGS model with condim 4 / 6 pairs)
  int variant, ncon_max, nefc_max;
  int mpr_iterations;
  float mpr_tolerance;
  // options
  float timestep, gravity[3], inv_sqrt_impratio, tolerance, pgs_scale;
  int iterations, disableflags;
  int solver, ls_iterations;  // mjtSolver (0 PGS, 2 Newton); Newton line-search evaluation cap
  float ls_tolerance;
  // bodies.  Level-ordered records, kBrecQuads float4 each (slot 0 = world, slot s = lane s-1 of the tree passes):
  // [0] b,parent,jntnum,jntadr  [1] depth,treeid,mass,childnum  [2] pos  [3] quat  [4] ipos  [5] iquat  [6] inertia
  // [7..8] children[8]  [9+3j] joint j: (type,qposadr,dofadr,qpos0) (axis) (pos)
  const float4 HB_CONST* brec;
  const int HB_CONST* body_treeid;
  const float HB_CONST *body_invweight0, *tree_invmass;
  const unsigned long long HB_CONST* body_dofmask;  // bit d set: dof d moves this body
  // joints
  const int HB_CONST *jnt_type, *jnt_qposadr, *jnt_dofadr;
  const float HB_CONST* qpos0;
  // dofs
  const float4 HB_CONST* drec;   // per dof: (jntid,bodyid,type,k) (treeid,armature,damping,stiffness) (qposadr,qpos_spring,-,-)
  const int HB_CONST *dof_jntid, *dof_Madr;
  const float HB_CONST* dof_damping;
  // sparse mass matrix (ancestor-chain layout of mjModel.dof_Madr)
  const int HB_CONST* mrec;      // per entry: i | j << 8 | body(i) << 16
  const float2 HB_CONST* mdiag;  // per entry: (armature, damping) on the diagonal, 0 elsewhere
  // dense view of the sparse mass matrix (both solvers eliminate it on the matrix cores): [32 columns j][32 rows i] -> index of the {M, H} pair holding
  // M(i, j) (nM: the zero pad pair, nM + 1: the one pad pair = identity beyond nv)
  const int HB_CONST* mdense;
  const int HB_CONST* mdense_c;  // the same view in the MFMA accumulator layout: [16 registers][64 lanes]
  // geoms
  const int HB_CONST *geom_type, *geom_bodyid;
  const float HB_CONST *geom_size, *geom_pos, *geom_quat, *geom_rbound;
  const float HB_CONST* geom_half;  // [ngeom][3] half extents of the geom's bounding box in its own frame
  int box_cull;                     // 1: oriented-box test behind the bounding spheres of a portal-search pair (HB_BOX_CULL=0 switches it off: tests)
  int has_box;                      // 1: a candidate pair has a box geom - the model steps in the kernels that carry the box colliders (COLL 2)
  // meshes: hull vertices as 16-byte records (x, y, z, link) and per geom the first record / the count (0 for other geom types);
  // link = first neighbour record << 8 | number of kMeshChunk-record chunks; mesh_nbr: one record per (vertex, neighbour): (x, y, z
  // of the neighbour, the neighbour's own link): the hull's edge graph with the coordinates inlined, every vertex's list padded to
  // whole chunks with copies of the vertex itself (never an improvement), so that a climb round is one batch of independent
  // 16-byte loads (hb_mpr.hpp: ccd_support).  mesh_start: per mesh a cube map of kMeshStart records (6 faces x 4 x 4 cells): the
  // hull's support vertex for the cell's centre direction, where the first climb of a test starts.
  const float4 HB_CONST* mesh_vert;
  const float4 HB_CONST* mesh_nbr;
  const float4 HB_CONST* mesh_start;
  const int HB_CONST *geom_meshadr, *geom_meshnum;
  // height fields (static terrain on the world body): per geom the field id (-1 otherwise)
  const int HB_CONST *geom_dataid, *hfield_nrow, *hfield_ncol, *hfield_adr;
  const float HB_CONST *hfield_size, *hfield_data;
  // collision candidates with pre-mixed contact parameters
  const int HB_CONST *pair_geom1, *pair_geom2, *pair_dim, *pair_self;
  // per pair, 5 float4: [0] body1,body2,tree1,tree2 [1] dofmask1 (lo,hi), dofmask2 (lo,hi) [2] margin-gap, solref[2], invweight0 sum
  // [3] solimp[0..3] [4] solimp[4], condim
  const float4 HB_CONST* prec;
  // per pair, 3 float4 for mj_collision: [0] geom1, geom2, type1 | type2 << 8, margin [1] rbound1, rbound2, size1[0..1] [2] size2[0..1]
  const float4 HB_CONST* crec;
  const float4 HB_CONST* arec;  // per actuator: 4 quads (hb_tables.cpp)
  const float4 HB_CONST* lrec;  // per limit candidate: 4 quads (hb_tables.cpp)
  const float HB_CONST* pair_fricab;  // per pair: (sliding friction of the floor geom if it is in the pair, else 0; the other geom's / the mixed one)
  const float HB_CONST *pair_friction, *pair_solref, *pair_solimp, *pair_margin, *pair_gap;
  // limit candidates: 2 per limited joint/tendon in constraint order (lower, upper)
  const int HB_CONST *lim_kind, *lim_id, *lim_side;  // kind 0 = joint, 1 = tendon
  const float HB_CONST *lim_range, *lim_margin, *lim_solref, *lim_solimp, *lim_invweight;
  // tendons (fixed)
  const int HB_CONST *tendon_adr, *tendon_num, *wrap_dofadr, *wrap_qposadr;
  const float HB_CONST* wrap_prm;
  const float4 HB_CONST* trec;  // per tendon, 3 float4: coefficients, qpos addresses, dof addresses of its first four wraps
  // actuators
  const int HB_CONST *act_qposadr, *act_dofadr, *act_ctrllimited, *act_forcelimited;
  const float HB_CONST *act_gear, *act_ctrlrange, *act_forcerange, *act_gain, *act_bias;
  // env adapter
  int obs_root_body, obs_root_dofadr, obs_root_qadr;
  const int HB_CONST* obs_src;  // [nobs - 3]: state-record offset each copied observation entry comes from (-1: zero)
  const int HB_CONST* obs_jnt;  // [(nobs - 6) / 2]: the scalar joints in observation order (joint order, or actuator order: hb_env_config)
  // LDS layout (float offsets per env) — persistent region
  int o_gquat;  // general collision only: world orientation of every geom (4 floats each)
  int o_meta;   // general variants: per-row (R, K imp (pos - margin), B, -) written by makeConstraint
  int o_AR;     // variant 3 (PGS on kPgsNefcMax rows): the matrix AR, [kPgsNefcMax][kPgsNefcMax]
  int o_qpos, o_qvel, o_warm, o_ctrl, o_gpos, o_gaxis, o_scom, o_cdof, o_qLD, o_smooth, o_vec0, o_vec1, o_vec2, o_tenlen;
  // region A (dynamics scratch)
  int o_xpos, o_xmat, o_xipos, o_xanchor, o_xaxis, o_cinert, o_crb, o_cvel;
  // region B (constraints), aliases region A: contacts, C rows, row meta (later W), forces
  int o_con, o_C, o_efc, o_force;
  int lds_floats;  // total floats per env
  int cstride;     // row stride of C (odd: conflict-free lane-strided access; the last column is zero padding)
  // mjtIntegrator (0 Euler, 1 RK4) and, RK4 only, the stage block behind both regions: q0[nq] | v0[nv] | sum b V [nv] | sum b F [nv]
  int integrator, o_rk;
  // friction loss: the rows in front of the limit rows, one per dof with dof_frictionloss > 0 (0: an ordinary model, or disabled by the
  // options), and per row (dof, frictionloss, R, B) as build_model_tables works them out.  Read by step_body's FRIC instantiations only.
  int nfric;
  const float4 HB_CONST* frec;
  // equality constraints: the rows in front of the friction rows, one per active joint coupling and three per active connect (0: a model
  // without them, or disabled by the options), and per row a kErecQuads record (hb_tables.cpp).  Read by step_body's FRIC == 2 instantiations only.
  int neq_rows;
  // the box - box manifold (Model::box_manifold and a box - box candidate pair): box - box pairs are four analytic work items of two contacts
  // (hb_mpr.hpp: box_box) in place of one portal search.  Read by the host only: it selects the BOX = 2 kernels (hb_pose_boxm_kernel, hb_boxm_*).  It sits in the four bytes of padding
  // between neq_rows and the pointer behind it: no field moves and the structure keeps its size (some kernels take it by value, and
  // a longer one would move their other arguments).
  int box_manifold;
  const float4 HB_CONST* erec;
};
static_assert(sizeof(DevModel) % 8 == 0 && offsetof(DevModel, erec) == offsetof(DevModel, neq_rows) + 8, "box_manifold fills the padding behind neq_rows");
constexpr int kErecQuads = 7;

typedef const DevModel HB_CONST& DevModelRef;

// device copy of hb_env_config (include/hb.h), same field order
constexpr int kEnvMaxPairs = 16;
struct EnvConfig {
  float target_velocity[2];
  float target_z, min_z, max_time, safe_torque, control_frequency, action_scale;
  float w_hvel, w_upright, w_height, w_torque, w_ctrl_change, w_ctrl_reg, w_symmetry;
  float self_collision_penalty, terminal_reward, upright_tol;
  int n_equal, n_opposite;
  int equal_pairs[kEnvMaxPairs][2];
  int opposite_pairs[kEnvMaxPairs][2];
  int auto_reset, reset_keyframe;
  float reset_perturb;
  int reward_kind;
  float w_vvel, min_z_grounded;
  int reset_collision_mode;
  float reset_quat_perturb;
  int obs_actuator_order;
};

// hb_env_randomization (include/hb.h), same layout
struct EnvRand {
  float factor;
  unsigned seed;
  float control_timestep;
  float joint_angle_noise, joint_velocity_noise, gyro_noise, imu_noise, action_noise;
  float min_delay, max_delay;
  int frozen_noise, push_enabled;
  float push_min_interval, push_max_interval, push_min_duration, push_max_duration, push_min_force, push_max_force;
};
// hb_domain_randomization (include/hb.h), same layout
struct DomainRand {
  float factor;
  unsigned seed;
  float friction_min_mult, friction_max_mult, max_mass_change, max_external_mass;
  float armature_max_change, stiffness_max_change, margin_max_change, range_max_change;
  float kp_nominal, kp_max_change, force_limit_max_change;
  float floor_bump_min, floor_bump_max;  // height-field elevations in [0, min + factor (max - min)] (cpu_env.py:267-280); max 0: the model's own data
};
// per-env model parameters [n_env][stride]: mass[nbody] | armature[nv] | stiffness[nv] | lim_margin[nlimcand] |
// lim_range[nlimcand] | act_gain[nu] | act_bias1[nu] | act_forcerange[2 nu] | floor friction scale | hfield_data[nhfielddata]
struct DomainLayout {
  int o_mass, o_arm, o_stiff, o_lmargin, o_lrange, o_gain, o_bias1, o_frc, o_fric, o_hfield, stride;
};
__host__ __device__ inline DomainLayout domain_layout(int nbody, int nv, int nlimcand, int nu, int nhfielddata) {
  DomainLayout L;
  L.o_mass = 0; L.o_arm = nbody; L.o_stiff = L.o_arm + nv; L.o_lmargin = L.o_stiff + nv; L.o_lrange = L.o_lmargin + nlimcand;
  L.o_gain = L.o_lrange + nlimcand; L.o_bias1 = L.o_gain + nu; L.o_frc = L.o_bias1 + nu; L.o_fric = L.o_frc + 2 * nu; L.o_hfield = L.o_fric + 1; L.stride = L.o_hfield + nhfielddata;
  return L;
}
constexpr int kDelaySlots = 64;  // ring size of the delay FIFOs (delays <= 63 control steps)
// per-env state of the realism layer, all [n_env]-major device arrays (null when hb_env_randomize is off)
struct EnvRandState {
  int* k_act;      // actions pushed this episode
  int* k_obs;      // observations pushed this episode
  int* delay;      // [n][4]: action, joints, gyro, gravity (control steps)
  float* fifo_act;   // [n][kDelaySlots][nu]
  float* fifo_joint; // [n][kDelaySlots][2 nscalar]
  float* fifo_gyro;  // [n][kDelaySlots][3]
  float* fifo_grav;  // [n][kDelaySlots][3]
  float* push;     // [n][8]: start, duration, magnitude, dir x, dir y, body, event count, -
  float* xfrc;     // [n][nbody][6] (the batch's xfrc_applied)
};

// fused policy kernel (hb_policy_kernel): layer sizes, host-packed weights (MFMA B-operand order) and biases
// MJPC "Humanoid Stand" cost (tasks/humanoid/stand/stand.cc:41-104): layout of the read-out row and the cost terms
struct StandTask {
  int n_feet, o_head, o_feet, o_com, o_vel, o_qvel, o_ctrl, nv, nu, stride;
  float height_goal, risk;
  int norm[5];
  float weight[5], p[5], q[5];
};

// MJPC "Humanoid Walk" cost (tasks/humanoid/walk/walk.cc:44-163): read-out row offsets and the cost terms (dims as the
// task's user sensors declare them, applied to the residual vector in order)
struct WalkTask {
  int o_torso, o_foot_r, o_foot_l, o_pelvis, o_com, o_vel, o_axes, o_linvel, o_sub, o_qpos, o_ctrl, nq, nu, stride;
  float height_goal, speed_goal, risk;
  int nterm, dim[8], norm[8];
  float weight[8], p[8], q[8];
};

// hb_task_cost: cost terms over consecutive slices of a residual vector (task.cc:71-110)
struct CostSpec {
  int nterm, dim[8], norm[8];
  float weight[8], p[8], q[8], risk;
};

enum { kActTanh = 0, kActRelu = 1, kActElu = 2 };  // the activation behind the hidden layers = HB_ACT_* (include/hb.h)
struct PolicyDesc {
  int nl;
  int sizes[5];
  const float* w[4];
  const float* b[4];
  int ldx;  // LDS row stride of an activation tile: widest layer + 4 (K is swept four columns at a time: zero pad columns)
  int act;  // kAct*: behind every hidden layer (the last layer belongs to the kernel that runs the network)
};

// fused actor kernel (hb_actor_kernel, hb_actor.hip): the same network description, the sampling head (hb_actor_config, include/hb.h)
// and the tapes of one step, each [n_env][nu]; action is always there, the others may be null
constexpr int kActorMaxNu = 32;
enum { kActorDeterministic = 0, kActorGaussian = 1, kActorSquashed = 2 };  // ActorDesc::head = HB_ACTOR_* (include/hb.h)
constexpr unsigned RS_ACTOR = 32;  // random-number stream of the actor's draws (hb_kcommon.hpp: RS_*, 1..8; hb_env.hip: RS_DR_*, 16..25)
struct ActorDesc {
  PolicyDesc net;
  int head, deterministic, nu;
  unsigned seed;
  float log_std[kActorMaxNu];
};
struct ActorTapes {
  float *action, *mean, *log_std, *eps;
};

// hb_collect_gae_dev (hb_gae.hip): the scan's tapes, each [T][n_env] (value: [T + 1][n_env]); term_value null: no bootstrap of truncated
// envs; gl = gamma lam rounded to fp32 once; advantage or returns may be null
struct GaeScan {
  const float *reward, *value, *term_value;
  const uint8_t *terminated, *truncated;
  float *advantage, *returns;
  float gamma, gl;
  int T, n_env;
};
// the log-probability pass: the actor's head (kActorGaussian: log_std[]; kActorSquashed: the mean and log_std tapes), tapes [rows][nu], out [rows]
struct LogProbDesc {
  int head, nu;
  float log_std[kActorMaxNu];
  const float *eps, *mean, *ls;
  float* out;
};

// hb_norm_* (hb_norm.hip).  The rows are reduced in chunks of kNormChunk consecutive envs, chunk c = envs [64 c, 64 c + 64).
// rec: the double-buffered record, slot s at rec + s norm_rec_doubles(nobs): obs_mean[nobs] | obs_var[nobs] | obs_count | ret_mean |
// ret_var | ret_count (the flat record of hb_norm_get_stats) | the four episode totals.  part: one partial per chunk,
// norm_part_doubles(nobs) doubles: n | the chunk's four episode-total terms | (mean, biased variance) of every obs column and of
// the ret column.
constexpr int kNormChunk = 64;
constexpr int kNormMaxObs = 240;  // (a chunk of rows in LDS: 64 x 240 floats = 60 KB)
__host__ __device__ inline int norm_rec_doubles(int nobs) { return 2 * nobs + 8; }
__host__ __device__ inline int norm_part_doubles(int nobs) { return 5 + 2 * (nobs + 1); }
struct NormDesc {
  int nobs;
  long long n_rows;                // rows of this call (n_env for a step or a reset)
  int nchunk;                      // partials to merge (0: none - hb_norm_obs_dev)
  int upd_obs, upd_ret;            // form and merge the partials of obs_rms / ret_rms (training && norm_obs, training)
  int reset;                       // moments: set ret, ep_ret, ep_len to 0 instead of advancing them
  int norm_obs, norm_reward;
  int store;                       // apply: block 0 writes the record to slot k ^ 1 (a step or a reset; not hb_norm_obs_dev)
  int k;                           // the slot that is read
  float clip_obs, clip_reward;
  double gamma, epsilon;
  double *rec, *part;
  double *ret, *ep_ret;            // [n_env]
  int* ep_len;                     // [n_env]
  const float *obs_in, *reward_in, *tobs_in;
  const uint8_t *term, *trunc;
  float *obs_out, *reward_out, *tobs_out, *ep_return_out;
  int* ep_length_out;
};

// hb_ppo_* (hb_ppo.hip): the learner.  Every reduction over the minibatch rows - dW, db, dlog_std, the advantage moments, the loss
// statistics - goes over chunks of ppo_row_chunk(mb) consecutive minibatch rows, chunk c = rows [c chunk, (c + 1) chunk), whose partials
// are merged in chunk order: 64 rows up to 4096, beyond that mb / 64 rounded up to whole 16-row tiles (never more than 64 chunks, which
// bounds the partial gradients at 64 P floats).  The gradient norm goes over chunks of kPpoNormChunk entries of the flat record.
constexpr int kPpoNormChunk = 4096;
__host__ __device__ inline int ppo_row_chunk(int mb) { return mb <= 4096 ? 64 : ((mb + 63) / 64 + 15) / 16 * 16; }
// LDS row stride of a 16-row operand tile of the wgrad kernels (learn_wgrad_chunk): whole 16-column tiles, and 16 mod 32 so that the four rows a wave
// reads in one MFMA operand fall on different banks
__host__ __device__ inline int ppo_ld(int w) { const int p = (w + 15) / 16 * 16; return p % 32 == 0 ? p + 16 : p; }
struct PpoNet {
  PolicyDesc fwd;   // the packed operands the forward kernels read (DevMlp)
  PolicyDesc bwd;   // dA = dZ W^T as the same layer loop: nl = L - 1, the widths in reverse, w[j] = the packed transpose of layer L - 1 - j, b = zeros
  float* act[4];    // act[l] [mb][sizes[l]]: the input of layer l (act[0]: the gathered observations, shared by both networks)
  float* dz[4];     // dz[l] [mb][sizes[l + 1]]: dloss / d(pre-activation of layer l)
  float* out;       // [mb][sizes[L]]: the last layer's output (mean, value)
  int off_w[4], off_b[4];  // where W_l and b_l stand in the flat record
};
struct PpoDesc {
  PpoNet net[2];    // actor, critic
  const float *obs, *action, *old_log_prob, *advantage, *returns;
  const int* index; // null: rows first .. first + mb - 1
  long long first;
  int mb, nobs, nu, chunk, nchunk, P, off_log_std, normalize;
  float clip_range, ent_coef, vf_coef;
  const float* param;  // the flat record (log_std is read from it)
  float* gls;          // [mb][nu] dloss / dlog_std by row
  float* srow;         // [mb][5] by row: the terms of policy_loss, value_loss, approx_kl, clip_fraction, and the ratio
  double* advpart;     // [nchunk][2] sum and sum of squares of the chunk's advantages
  double* statpart;    // [nchunk][8] the chunk's sums of srow (the ratio: its maximum)
  float* part;         // [nchunk][P] the chunk's gradients
  float* grad;         // [P]
  float* stats;        // [16] or null
};
// Both learners (hb_ppo.hip, hb_sac.hip; their shared kernel bodies: hb_learn_core.hpp).  A tensor of a flat parameter record and the
// packed operands that follow it: whoever writes entry i of the record - Adam, the Polyak step - passes the value to learn_refresh.
constexpr int kLearnMaxSeg = 17;  // tensors one Adam or Polyak launch covers: 2 x 4 x (W, b) + log_std or log_ent_coef
struct ParamSeg {
  int start, K, N, k0;   // flat offset; W[K][N], or K = 0: a vector of N; rows k >= k0 have an entry in dst_t, at row k - k0
  float* dst;            // W: the packed B operand of the forward pass; vector: its copy (null: none)
  float* dst_t;          // W: the packed B operand of the transpose of rows k0 .. (null: none)
};
// where W[k][n] of W[K][N] stands in its packed B operand (DevMlp::pack_mfma_b)
__host__ __device__ inline size_t packed_b_index(int k, int n, int K) { return ((size_t)(n >> 4) * ((K + 3) / 4) + (k >> 2)) * 64 + (k & 3) * 16 + (n & 15); }
// entry i of the record took the value pf: the segment it belongs to (seg[0 .. nseg) by ascending start, seg[0].start <= i), and its
// copy into the packed operands.  Pad entries of those are never written, so they stay zero.
__host__ __device__ inline void learn_refresh(const ParamSeg* seg, int nseg, int i, float pf) {
  int sgi = 0;
  while (sgi + 1 < nseg && i >= seg[sgi + 1].start) sgi++;
  const ParamSeg& sg = seg[sgi];
  const int j = i - sg.start;
  if (sg.K == 0) {
    if (sg.dst) sg.dst[j] = pf;
    return;
  }
  const int k = j / sg.N, n = j - k * sg.N;
  if (sg.dst) sg.dst[packed_b_index(k, n, sg.K)] = pf;
  if (sg.dst_t && k >= sg.k0) sg.dst_t[packed_b_index(n, k - sg.k0, sg.N)] = pf;
}
struct PpoAdamDesc {
  int P, nseg, nnorm;
  ParamSeg seg[kLearnMaxSeg];
  float *param, *m, *v;
  const float* grad;
  double* normpart;    // [nnorm]
  int* nskip;          // skipped steps since t was last set
  long long calls;     // t = calls - *nskip (this step included)
  float lr, beta1, beta2, eps, max_grad_norm;
  float* stats;
};

// hb_sac_* (hb_sac.hip): the SAC learner.  The launches of one gradient step are described job by job: a forward pass, a reversed
// (back-propagating) pass and a dW pass each run a list of jobs side by side (grid y), so the same three kernels serve the actor, the two
// Q networks and the two targets.  Row reductions go over the PPO learner's chunks (ppo_row_chunk); the Adam and Polyak launches cover
// ParamSeg segments (above), as the PPO learner's Adam launch does.
constexpr unsigned RS_SAC_PI = 33, RS_SAC_NEXT = 34;  // random-number streams of eps_pi and eps_next (RS_ACTOR is 32)
constexpr int kSacSrow = 8;      // by-row terms of a phase
struct SacFwdJob {
  PolicyDesc net;
  const float *x0, *x1;  // the input row is x0's n0 columns | x1's n1 columns (n1 0: none)
  int n0, n1;
  int gather0, gather1;  // 1: minibatch row r is row index[r] (or first + r) of the array; 0: row r
  float* in_store;       // [mb][n0 + n1] or null: the gathered input rows (act[0] of the dW pass)
  float* act[4];         // act[l] [mb][sizes[l]], l = 1 .. L - 1: the hidden activations' outputs; act[1] null: nothing is stored
  float* out;            // [mb][sizes[L]] the last layer's (linear) output
};
struct SacFwdDesc {
  SacFwdJob job[4];
  const int* index;
  long long first;
  int mb;
};
struct SacBwdJob {
  PolicyDesc net;        // the reversed network: the widths from the top down, w[j] = the packed transpose of layer L - 1 - j, b = zeros;
                         // nl = L - 1 stops at dZ_0; nl = L goes one step further, into the Q network's action inputs
  int L;                 // layers of the forward network
  int unit_top;          // 1: the top gradient is 1 for every row (dQ / da); 0: read from top
  const float* top;      // [mb][sizes[L]]
  int activation;        // kAct* of the forward network: its derivative is formed from the kept outputs
  const float* act[4];   // the hidden activations' outputs the forward pass kept
  float* dz[4];          // dz[l] [mb][sizes[l + 1]], l = 0 .. L - 2, written; dz[0] null: not stored (no dW follows)
  float* da;             // [mb][nu]: dloss / d(action inputs), the nl = L step
};
struct SacBwdDesc {
  SacBwdJob job[2];
  int mb;
};
struct SacWgJob {
  const float *A, *Z;    // dW = A^T Z: A [mb][K], Z [mb][N]
  int K, N, off_w, off_b;
};
struct SacWgDesc {
  SacWgJob job[8];
  int njob, mb, chunk, nchunk, P, ncol;
  float* part;           // [nchunk][P]
  const float* srow;     // [mb][kSacSrow] by-row terms, the first ncol of them summed by the block behind the jobs
  double* statpart;      // [nchunk][kSacSrow]
};
struct SacHeadDesc {
  int mb, nu, eps_given;
  unsigned seed, t;
  const int* index;
  long long first;
  float gamma, target_entropy;
  const float* param;    // the flat record (log_ent_coef is its last entry)
  int P;
  float* alpha;          // [1] exp(log_ent_coef) at the start of the step
  const float *reward;
  const uint8_t* done;
  float *eps_pi, *eps_next;        // the caller's [mb][nu], nullable
  float *eps;                      // [mb][nu] scratch: the draws of the pi branch
  const float *pi_out, *nx_out;    // [mb][2 nu] the actor on obs / next_obs
  float *a_pi, *a_nx, *lp_pi, *lp_nx;
  const float *q[2], *qt[2], *qpi[2];  // [mb] Q(obs, action), Q'(next_obs, a'), Q(obs, a_pi)
  const float* da[2];              // [mb][nu] dQk / da at a_pi
  float *dzq[2];                   // [mb] the Q networks' top dZ
  float *dza;                      // [mb][2 nu] the actor's top dZ
  float* srow;                     // [mb][kSacSrow]
};
struct SacReduceDesc {
  int lo, hi, P, nchunk, mb, phase;  // entries [lo, hi) of the flat record; phase 0: critics and log_ent_coef, 1: actor
  float target_entropy;
  const float *part, *param, *alpha;
  const double* statpart;
  float *grad, *stats;
};
struct SacAdamDesc {
  int lo, hi, nseg, ent_index;   // entries [lo, hi); ent_index: log_ent_coef (its own learning rate), -1: not in this launch
  ParamSeg seg[kLearnMaxSeg];
  float *param, *m, *v;
  const float* grad;
  long long t;           // this step included
  float lr, lr_ent, beta1, beta2, eps;
};
struct SacPolyakDesc {
  int n, nseg;
  ParamSeg seg[kLearnMaxSeg];  // starts relative to the targets' record
  const float* src;      // the live Q networks' stretch of the flat record
  float* target;
  float tau;
};

// Buffers of the STAGED step of the general variants (launch_step): hb_pose_kernel writes every geom's world pose and the env's
// narrowphase work items, hb_narrow_kernel evaluates the items (one per lane, at the occupancy of a small kernel: the MPR climbs are
// chains of dependent loads), the step kernel appends the results in item order.  All null: the step kernel does all of it itself.
struct StageBufs {
  float* geom;     // [n_env][10 ngeom]: world positions[3 ngeom] | z axes[3 ngeom] | orientation quaternions[4 ngeom]
  int4* item;      // [n_env][kWorkMax]: the env's items that need a portal search: prisms of height-field pairs from the front, pairs
                   // of geoms from the back, each in item order:
                   // env, pair | item index << 16, sub-item | ncols << 16, rmin | cmin << 16 (sub-grid of a height-field pair)
  int* nsearch;    // [n_env][2] how many of each kind
  int* nwork;      // [n_env] work items of the env (clamped to kWorkMax)
  float4* result;  // [n_env][kWorkMax][4]: dist0, pos0 | normal0, n | dist1, pos1 | normal1, pair
  int nq, nv, nu, pose_lds;  // host-side copies for the per-step pointer arithmetic and the pose kernel's LDS bytes
  // Variant 2 (Newton, 256 rows in four register groups, one wave per SIMD): the step kernel proper is first the ONE-group
  // instantiation on the variant-1 layout (dm_fast; 63 rows, 24 contacts, two waves per SIMD); an env whose step needs more
  // raises defer[env] and leaves its state alone, and the four-group kernel then steps exactly those envs (rerun = 1).
  const DevModel* dm_fast;  // null: no fast pass (not variant 2, or diagnostics on: their buffers have the big kernel's strides)
  int fast_lds;             // its dynamic LDS bytes
  int has_box;              // DevModel::has_box: the pose / narrowphase launches are the *_box_kernel ones; 2 (DevModel::box_manifold): the pose launch is hb_pose_boxm_kernel
  int* defer;               // [n_env]
  // the deferred envs of a launch as a list, so that the second pass is a handful of waves that loop over it instead of one wave per env
  // that looks at its flag and leaves (4096 waves of the four-group kernel, one per SIMD: 18 us): defer_list[blk0 + k], k < defer_count[blk0]
  // (blk0: the launch's first slot - every env segment has its own stretch and counter).  hb_pose_kernel zeroes the counter.
  int* defer_list;
  int* defer_count;
  int rerun;                // set by launch_step for the second pass
  int no_mesh;              // the model has no mesh geoms: the narrowphase launch is hb_narrow_prim_kernel
};

// ---- The per-env LDS layout of the step kernels: every o_* offset of DevModel, the row stride of C, the RK4 stage block and the total,
// as a function of the model's shape.  This is the one place that computes it: build_model_tables copies the result into the DevModel
// (and, for variants 2 and 3, into the one-group fast model), and the size-specialised kernels below take it as compile-time constants.
enum { kLdsOk = 0, kLdsNoEulerRoom, kLdsTooLarge };  // LdsLayout::fail
struct LdsLayout {
  int o_gquat, o_meta, o_AR;
  int o_qpos, o_qvel, o_warm, o_ctrl, o_gpos, o_gaxis, o_scom, o_cdof, o_qLD, o_smooth, o_vec0, o_vec1, o_vec2, o_tenlen;
  int o_xpos, o_xmat, o_xipos, o_xanchor, o_xaxis, o_cinert, o_crb, o_cvel;
  int o_con, o_C, o_efc, o_force;
  int lds_floats, cstride, o_rk;
  int fail;  // kLdsOk, or why no kernel can run the model: no room for the Euler solve's W_H pair, more LDS than a CU has
};
// variant, solver, integrator, ncon_max, nefc_max: DevModel's (mjtSolver 0 PGS / 2 Newton, mjtIntegrator 0 Euler / 1 RK4)
constexpr LdsLayout lds_layout(int nq, int nv, int nu, int nbody, int njnt, int ngeom, int ntendon, int nM, int ntree, int variant, int solver, int integrator, int ncon_max,
                               int nefc_max) {
  LdsLayout L{};
  int off = 0;
  auto take = [&off](int n) { int o = off; off += (n + 3) & ~3; return o; };
  auto imax = [](int a, int b) { return a > b ? a : b; };
  // row stride of C: 33 (K = 32 for the matrix cores plus a pad column); the big Newton layout stores J rows only as wide as its dense
  // order (NDENSE + 1: 21 for the reference's 18-dof robot, else 29): 256 rows of 33 floats would be 34 KB per env
  // (variant 1 with the Newton solver is the fast layout of a variant-2 model: its one-group Newton kernel reads J rows like the big one)
  L.cstride = (variant == 2 || (variant == 1 && solver == 2)) ? (nv <= 20 ? 21 : 29) : 33;
  // persistent region
  L.o_gquat = variant ? take(4 * ngeom) : 0;
  L.o_qpos = take(nq); L.o_qvel = take(nv); L.o_warm = take(nv); L.o_ctrl = take(imax(1, nu));
  L.o_gpos = take(3 * ngeom); L.o_gaxis = take(3 * ngeom); L.o_scom = take(3 * imax(1, ntree)); L.o_cdof = take(12 * nv);  // angular[3], -, linear[3], -, pad[4] per dof (kCdofStride: conflict-free b128 reads)
  L.o_qLD = take(2 * nM + 4); L.o_smooth = take(nv);  // qLD: {M, H} pairs + the zero and one pad pairs of the dense views
  L.o_vec0 = take(32); L.o_vec1 = take(32); L.o_vec2 = take(32);  /* read 32 wide */ L.o_tenlen = take(imax(1, ntendon));
  const int region = off;
  // region A (dynamics scratch)
  L.o_xpos = take(12 * nbody);  /* xpos[3], -, xquat[4], pad[4] records (kXpqStride) */ L.o_xmat = take(9 * nbody); L.o_xipos = take(3 * nbody);
  L.o_xanchor = take(3 * njnt); L.o_xaxis = take(3 * njnt); L.o_cinert = take(10 * nbody); L.o_crb = take(20 * nbody);  // crb: inertia[10] | cfrc[6] | pad[4] records (kIfStride)
  L.o_cvel = take(12 * nbody);  // cvel[6] | cacc[6] records
  const int endA = off;
  // region B (constraints) aliases region A
  off = region;
  if (variant == 2) {
    // Newton on kBigNefcMax rows: contacts, J rows, the dense M ([32][33], where the classic layout keeps the row meta), the
    // compact row meta, one D / force word per row
    L.o_con = take(ncon_max * kConStride);
    L.o_C = take(imax(nefc_max * L.cstride + 64, kListMax * 5 + kWorkMax));  // (the collision pass borrows the head of C for its lists)
    L.o_efc = take(32 * 36);
    L.o_meta = take(nefc_max * kMetaStride);
  } else if (variant == 3) {
    // PGS on kPgsNefcMax rows: contacts, J / C rows (+ the qfrc_smooth row), W, the compact row meta, the matrix AR
    L.o_con = take(ncon_max * kConStride);
    L.o_C = take(imax((nefc_max + 1) * L.cstride + 64, kListMax * 5 + kWorkMax));
    L.o_efc = take(32 * 36);
    L.o_meta = take(nefc_max * kMetaStride);
    L.o_AR = take(nefc_max * nefc_max);
  } else {
    L.o_con = take(kNconMax * kConStride); L.o_C = take((kNefcMax + 1) * L.cstride);
    // per-row meta (13 slots x kNefcMax) is dead once the row quantities are in registers; W = L^-1 D^-1/2
    // ([32][33]) is built over it before the J W product and lives until the dual finish
    L.o_efc = take(imax(13 * kNefcMax, 32 * 36));
    // mj_Euler builds W_H and its transpose (2 x [32][36]) from the start of C, running on into the row-meta area
    if (L.o_efc != L.o_C + (((kNefcMax + 1) * L.cstride + 3) & ~3) || L.o_efc + imax(13 * kNefcMax, 32 * 36) - L.o_C < 2 * 32 * 36) { L.fail = kLdsNoEulerRoom; return L; }
    if (variant == 1) L.o_meta = take(64 * kMetaStride);
  }
  L.o_force = take(imax(kGroup, nefc_max));
  // xipos and scom/cdof are read while region B is being written (xfrc, Jacobians): keep xipos out of the alias
  L.lds_floats = imax(endA, off);
  // RK4: the stage block (start state and the two running sums) behind both regions, so that an RK4 model's layout is the Euler layout
  // plus a tail and no offset moves
  if (integrator == 1) { off = L.lds_floats; L.o_rk = take(nq + 3 * nv); L.lds_floats = off; }
  if (L.lds_floats * 4 > 160 * 1024) L.fail = kLdsTooLarge;
  return L;
}

// ---- Size-specialised instantiation of the classic PGS step kernel (step_body's SIZED) ---------------------------------------------
// Every loop bound and every LDS offset of the step kernel is a function of the model's sizes.  For the size signature of the
// reference's 27-dof humanoid (simulation/mujoco/model/humanoid/humanoid.xml) they are compile-time constants in one
// more instantiation: addresses fold into the instructions' offset fields and 40 SGPRs spill instead of 84.  Any model with this
// signature takes it (the host compares its sizes, and the layout lds_layout gave it against the constant's: build_model_tables);
// every other model takes the generic kernels.
struct SizedModel : LdsLayout {
  int nq, nv, nu, nbody, njnt, ngeom, ntendon, nM, ntree, npair, nlevel, nlimcand, nstate;
};
// (full capacity, Euler: the layout of variant 0 or 1 as lds_layout computes it for these sizes)
constexpr SizedModel sized_for(int nq, int nv, int nu, int nbody, int njnt, int ngeom, int ntendon, int nM, int ntree, int npair, int nlevel, int nlimcand, int variant, int solver) {
  return {lds_layout(nq, nv, nu, nbody, njnt, ngeom, ntendon, nM, ntree, variant, solver, /*integrator*/ 0, kNconMax, kNefcMax),
          nq, nv, nu, nbody, njnt, ngeom, ntendon, nM, ntree, npair, nlevel, nlimcand, 1 + nq + 2 * nv};
}
constexpr SizedModel kSizedHumanoid27 = sized_for(28, 27, 21, 17, 22, 20, 2, 243, 1, 159, /*tree levels*/ 7, /*limit candidates*/ 46, /*variant*/ 0, /*PGS or Newton: the same layout*/ 0);
// the same humanoid on a height field (configs[4]; general collision, PGS: the variant-1 layout of the staged step's fast kernel)
constexpr SizedModel kSizedHumanoid27V1 = sized_for(28, 27, 21, 17, 22, 20, 2, 243, 1, 159, 7, 46, /*variant*/ 1, /*PGS*/ 0);
// the reference's own robot (simulation/assets/world.xml + humanoid.xml: 18 dofs, 13 geoms) on the variant-1 layout of its fast Newton kernel
// (J row stride 21: a Newton kernel of dense order 20)
constexpr SizedModel kSizedTeamV1 = sized_for(19, 18, 12, 15, 13, 13, 0, 117, 1, 37, /*tree levels*/ 5, /*limit candidates*/ 24, /*variant*/ 1, /*Newton*/ 2);
static_assert(!kSizedHumanoid27.fail && !kSizedHumanoid27V1.fail && !kSizedTeamV1.fail, "the size-specialised kernels' layouts must be valid");

// LDS of hb_pose_kernel in floats: qpos | body poses (12 floats each, kXpqStride) | geom position, z axis, quaternion | the work lists
__host__ __device__ inline int pose_lds_floats(int nq, int nb, int ngeom) {
  return ((nq + 3) & ~3) + 12 * nb + 2 * ((3 * ngeom + 3) & ~3) + 4 * ngeom + kListMax * 5 + kWorkMax;
}

// The layout of a row of the step kernel's sensor read-out, stated once:
//   [ framepos (3 each) | subtreecom, subtreelinvel of one tree (6) | frame axes (3 each) | framelinvel (3 each) | subtreelinvel (3 each)
//     | touch (1 each) | contact force (3 each) | accelerometer, gyro (6 each) | frameangacc, framelinacc (6 each) | qpos? | qvel? | ctrl? ]
// Offsets in floats; n_*: a sensor part's entries (hb_sensor_spec's counts; n_subtree 1 or 0), a tail part's floats (nq, nv, nu or 0).
// A part that is off has count 0 (its offset is then where it would begin).  `width` is what hb_sensor_size returns, `stride` the distance
// between two rows.  sensor_row() computes it from the few facts that determine it; the step kernel, the host, the task rollouts,
// hb_sensor_row (include/hb.h: the same layout up to `width`) and Batch.sensor_layout read it.
struct SensorRow {
  int framepos, n_framepos, subtree, n_subtree, axis, n_axis, linvel, n_linvel, sub, n_sub;  // offset, count of each part; framepos at 0
  int touch, n_touch, cfrc, n_cfrc, imu, n_imu, facc, n_facc;
  int width;
  int qpos, n_qpos, qvel, n_qvel, ctrl, n_ctrl;
  int stride;
};
constexpr int kSensorQvel = 1, kSensorCtrl = 2, kSensorQpos = 4;  // the tail parts a caller asks for
__host__ __device__ inline SensorRow sensor_row(int n_framepos, bool tree, int n_axis, int n_linvel, int n_sub, int n_touch, int n_cfrc, int n_imu, int n_facc,
                                                int tail, int nq, int nv, int nu) {
  SensorRow r;
  r.framepos = 0; r.n_framepos = n_framepos;
  r.subtree = r.framepos + 3 * r.n_framepos; r.n_subtree = tree ? 1 : 0;
  r.axis = r.subtree + 6 * r.n_subtree; r.n_axis = n_axis;
  r.linvel = r.axis + 3 * r.n_axis; r.n_linvel = n_linvel;
  r.sub = r.linvel + 3 * r.n_linvel; r.n_sub = n_sub;
  r.touch = r.sub + 3 * r.n_sub; r.n_touch = n_touch;
  r.cfrc = r.touch + r.n_touch; r.n_cfrc = n_cfrc;
  r.imu = r.cfrc + 3 * r.n_cfrc; r.n_imu = n_imu;
  r.facc = r.imu + 6 * r.n_imu; r.n_facc = n_facc;
  r.width = r.facc + 6 * r.n_facc;
  r.qpos = r.width; r.n_qpos = (tail & kSensorQpos) ? nq : 0;
  r.qvel = r.qpos + r.n_qpos; r.n_qvel = (tail & kSensorQvel) ? nv : 0;
  r.ctrl = r.qvel + r.n_qvel; r.n_ctrl = (tail & kSensorCtrl) ? nu : 0;
  r.stride = r.ctrl + r.n_ctrl;
  return r;
}
// The same row from its counts alone.  The step kernel addresses a row this way: it reads every second word of the record, one scalar
// register each, where neighbouring words would be fetched as 8- and 16-register tuples that leave spill slots in the kernel's frame.
__host__ __device__ inline SensorRow sensor_row(const SensorRow& c) {
  return sensor_row(c.n_framepos, c.n_subtree != 0, c.n_axis, c.n_linvel, c.n_sub, c.n_touch, c.n_cfrc, c.n_imu, c.n_facc,
                    (c.n_qpos ? kSensorQpos : 0) | (c.n_qvel ? kSensorQvel : 0) | (c.n_ctrl ? kSensorCtrl : 0), c.n_qpos, c.n_qvel, c.n_ctrl);
}
// N body ids, four to a word: a body is a lane of the step kernel, so an id fits a byte (whole words: the kernel reads an entry of a
// table in its arguments with one scalar load)
template <int N> struct BodyIds {
  unsigned w[(N + 3) / 4];
  __host__ __device__ int operator[](int k) const { return (w[k >> 2] >> (8 * (k & 3))) & 0xff; }
  void set(int k, int id) { w[k >> 2] |= (unsigned)id << (8 * (k & 3)); }  // (of a zeroed table)
};
// The sensor read-out of a launch (hb_rollout_sensors, hb_sensors, the task rollouts), by value in BatchPtrs: where the rows go, their
// layout and the table of every part (filled by sensor_args, hb_api_rollout.cpp).  out null: no read-out, and nothing else of it is
// read.  (BatchPtrs is compared byte for byte: filled in zeroed memory, as the rest of it.)
struct SensorArgs {
  float* out;                     // [T][n_env][row.stride]
  unsigned long long submask[4];  // subtreelinvel entry k: bit b = body b belongs to that subtree ...
  SensorRow row;
  int tree;                       // the tree whose subtreecom / subtreelinvel are read (when row.n_subtree)
  float subinv[4];                // ... and 1 / the subtree's mass
  float off[16][3];               // framepos of a site: offset in the body frame (zero: the body frame itself)
  float imu_off[4][3];            // accelerometer / gyro: the site's offset in the body frame
  int body[16];                   // framepos
  int axis_body[8];               // framexaxis / framezaxis of a body frame (objtype xbody) ...
  unsigned axis_which;            // ... two bits per entry: 0 the x axis, 2 the z axis
  int linvel_body[8];             // framelinvel, objtype body: velocity of the inertial frame origin, world axes
  BodyIds<8> touch_body;            // the normal-force sum of a body's contacts
  BodyIds<4> cfrc_body;             // the force part of a body's contact wrench
  BodyIds<4> imu_body;              // accelerometer[3] | gyro[3] at body frame + offset, in the body's axes
  BodyIds<4> facc_body;             // frameangacc[3] | framelinacc[3] of a body: its row of body_acc
};
static_assert(__is_trivially_copyable(SensorArgs), "BatchPtrs is copied and compared byte for byte");

// most step calls one launch executes (the calls the host enqueued back to back, hb_batch.cpp fold_steps)
constexpr int kFoldMax = 256;
struct BatchPtrs {
  float* state;        // [n_env][nstate]
  const float* ctrl;   // [n_env][nu] or [T][n_env][nu]
  float* qpos_out;     // nullable, [T][n_env][nq]
  float* qvel_out;     // nullable, [T][n_env][nv]: with qpos_out the recorded states of a trajectory (trajectory.cc:175-190)
  float* xfrc;         // nullable, [n_env][nbody][6]
  float xfrc_rate, xfrc_scale;  // rollout noise (hb_rollout_noise): xfrc <- rate * xfrc + scale * N(0, 1) before every step; scale 0: off
  unsigned xfrc_seed, xfrc_call;
  int* status;         // [n_env] accumulated HB_WARN_* bits
  int* counts;         // [n_env][kCountStride]
  float* qfrc_out;     // nullable [n_env][nv]: qfrc_smooth + qfrc_constraint of the last step (env adapter's joint torques)
  float* diag_qacc;    // nullable [n_env][nv]
  float* diag_force;   // nullable [n_env][kNefcMax]
  float* diag_contact; // nullable [n_env][kNconMax][kDiagConStride]
  int n_env;
  int blk0, nblk;      // this launch covers dispatch slots blk0 .. blk0+nblk-1 (one block each) of the batch
  int ctrl_mode;       // 0: ctrl[e][nu] held for all steps; 1: ctrl[t][e][nu]; 2: on-device Halton; 3: ctrl_tab[t][e][nu]
  int t0, env_offset;  // Halton indexing
  int integrate;       // 1: mj_step, 0: mj_forward only
  // heavy-first block scheduling (nullable): slot s takes env = order[s], a permutation sorted by
  // the cost of each env's previous step (counts[4*e+3]) so the most expensive envs are dispatched first
  const int* order;    // [n_env]
  const int* order2;   // [n_env] nullable: the same for the narrowphase launch of a staged step, by the cost of its waves (counts[..][7])
  const float* dr;     // nullable [n_env][dr_stride]: per-env model parameters (DomainLayout)
  int dr_stride;
  SensorArgs sensor;  // the sensor read-out (sensor.out nullable)
  const unsigned char* env_mask;  // nullable [n_env]: envs with a zero byte are skipped by this launch
  unsigned long long* stamps;  // diagnostic builds (-DHB_STAMPS) only: [n_env][16] s_memtime stamps of the last step
  int lean_ok;                // bit 0: the model's options allow the lean instantiations (mjOption.disableflags == 0); bit 1: its sizes and LDS
                              // layout are kSizedHumanoid27's (the size-specialised instantiations); bit 2: its fast layout is kSizedTeamV1's
  int stop_phase;             // diagnostic builds only: 0 = off (HB_STOP_PHASE in the environment, read at every launch)
  const float* ctrl_tab[kFoldMax];  // ctrl_mode 3: step t of this launch is the step call whose [n_env][nu] controls these are (hb_batch.cpp: fold_steps)
  int duo;                    // host side only (launch_step): two envs per wave 0 never, 1 where it pays, 2 always (hb_batch_duo)
  StageBufs stage;
  // inverse dynamics (launch_inverse, the INV instantiations only): qacc [n_env][nv] in, qfrc_inverse [n_env][nv] out, the per-env
  // HB_WARN_CONTACTFULL / HB_WARN_CNSTRFULL bits out (nullable), HB_INV_* flags; counts and status point at scratch in such a launch
  const float* inv_qacc;
  float* inv_out;
  int* inv_warn;
  int inv_flags;
  // contact-force read-out (hb_contact_readout), both null or both set: mj_contactForce of every contact, [n_env][cfrc_ncon][6] in the
  // contact frame (cfrc_ncon: the MODEL's contact capacity, whichever kernel of a staged step writes the env), and the bodies' contact
  // wrenches, [n_env][nbody][6] = force | torque about the body's xipos, world axes.  A launch that carries them takes a full kernel.
  float* contact_force;
  float* body_contact;
  int cfrc_ncon;
  // body-acceleration read-out (hb_body_acc_readout), both null or both set: [n_env][nbody][6] = angular | linear acceleration of the
  // body's xipos, world axes, gravity pseudo-acceleration included; and the scratch the step kernel parks what the read-out needs of the
  // kinematics in, [n_env][nbody][kAccPark]: bias cacc[6] | cvel[6] | xipos - subtree_com[3] | xpos - subtree_com[3] | xquat[4] | -.
  // A launch that carries them takes the full kernel's instantiation with the read-out (step_body's ACC, hb_step.hip: the ACC rows of HB_KERNELS).
  float* body_acc;
  float* body_acc_park;
};
// arguments of the kinematics read-out (hb_kin.hip; hb_kinematics*): n states, state k's qpos at qpos + k qpos_stride (the batch's state
// records, or packed rows), qvel likewise (read only when body_vel is asked for); the outputs are nullable, layouts in include/hb.h
struct KinArgs {
  const float* qpos;
  const float* qvel;
  int qpos_stride, qvel_stride;
  long long n;
  float* body_pose;  // [n][nbody][10]
  float* body_vel;   // [n][nbody][6]
  float* geom_pose;  // [n][ngeom][7]
};
// arguments of the dynamics read-out (hb_dyn.hip; hb_dynamics*): n states addressed as in KinArgs (qvel null: zero velocities, for M and
// Jacobians only); dr nullable [n][dr_stride]: state k's own masses, armature and stiffness (DomainLayout); the outputs are nullable,
// layouts in include/hb.h; the Jacobian points are hb_jac_spec's (kind 0: a point fixed in the body's frame, 1: the subtree's centre of mass)
constexpr int kJacMax = 16;
struct DynArgs {
  const float* qpos;
  const float* qvel;
  int qpos_stride, qvel_stride;
  long long n;
  const float* dr;
  int dr_stride;
  float* M;        // [n][nv][nv]
  float* bias;     // [n][nv]
  float* passive;  // [n][nv]
  float* jac;      // [n][njac][6][nv]
  int njac, jkind[kJacMax], jbody[kJacMax];
  float joff[kJacMax][3];
};
// arguments of the ray read-out (hb_ray.hip; hb_rays*): n_ray rays of hb_ray_configure against every env's geoms.  geoms: the eligible
// geoms in ascending order (the host checked the types: plane, height field, sphere, capsule).  A geom of the world body has the model's
// own pose; every other one is read from geom_pose, and the frame body from body_pose (hb_kin.hip's layouts; either null when unused).
constexpr int kRayMax = 4096;       // most rays of a configuration
constexpr int kRayBlock = 256;      // lanes of a block: up to four waves of 64 rays share the env's staged elevations
constexpr int kRayLdsFloats = 8192; // elevations staged in LDS when the model has no more than this many (32 KB), read from memory otherwise
struct RayArgs {
  const float* pnt;        // [n_ray][3]
  const float* vec;        // [n_ray][3], unit
  const int* geoms;        // [n_geom]
  int n_ray, n_geom, n_env;
  int frame, frame_body;   // HB_RAY_FRAME_*
  float cutoff;            // <= 0: none
  const float* body_pose;  // [n_env][nbody][10], null for HB_RAY_FRAME_WORLD
  const float* geom_pose;  // [n_env][ngeom][7], null when no geom of a moving body is eligible
  const float* dr;         // nullable [n_env][dr_stride]: per-env model parameters (DomainLayout: the env's own elevations)
  int dr_stride;
  int has_hfield;          // a height field is among the geoms
  float* dist;             // [n_env][n_ray], nullable
  int* geomid;             // [n_env][n_ray], nullable
  // the scan of the env adapter's observation extension (hb_env_obs_extend); all zero for hb_rays*:
  const uint8_t* env_mask; // nullable [n_env]: only the envs whose byte is set are cast (a block is one env: the others return at once)
  int xform;               // 1: dist receives clamp(x_scale * (x_offset - d), x_lo, x_hi), d = the distance, or cutoff where nothing is hit,
  int out_stride, out_col; //    at dist[env * out_stride + out_col + ray]: straight into a row of a wider table
  float x_offset, x_scale, x_lo, x_hi;
};
// The layout of an observation row of the env adapter, stated once:
//   [ base (the model's nobs) | last action (nu) | scan (n_ray) | foot-contact flags (n_feet) | command (3) ]
// A part that is off has count 0 (its offset is then where it would begin).  env_row() computes it from the few facts that determine it;
// the env kernel, the host (hb_batch::row), hb_env_row and VecEnv read it.  The layout of hb_env_row (include/hb.h).
struct EnvRow {
  int base;                          // the count of the base part, at offset 0
  int prev_action, n_prev_action;    // offset, count
  int scan, n_scan;
  int foot_contact, n_foot_contact;
  int command, n_command;
  int width;
};
__host__ __device__ inline EnvRow env_row(int nobs, int n_prev_action, int n_scan, int n_feet_observed, bool cmd_observed) {
  EnvRow r;
  r.base = nobs;
  r.prev_action = nobs; r.n_prev_action = n_prev_action;
  r.scan = r.prev_action + r.n_prev_action; r.n_scan = n_scan;
  r.foot_contact = r.scan + r.n_scan; r.n_foot_contact = n_feet_observed;
  r.command = r.foot_contact + r.n_foot_contact; r.n_command = cmd_observed ? 3 : 0;
  r.width = r.command + r.n_command;
  return r;
}
// velocity commands (hb_env_commands_configure): the configuration (the layout of hb_env_commands); EnvArgs::cmd holds every env's record
constexpr unsigned RS_COMMAND = 40;  // random-number stream of the command draws (1..8, 16..25 and 32..34 are taken)
struct EnvCommands {
  unsigned seed;
  float vx_min, vx_max, vy_min, vy_max, yaw_min, yaw_max;
  float resample_time, zero_fraction, w_yaw;
  int frame, observe;
};
// foot-contact terms (hb_env_feet_configure): the configuration (the layout of hb_env_feet) and every env's record (EnvArgs::feet)
constexpr int kMaxFeet = 4, kMaxContactBodies = 8;
struct EnvFeet {
  int n_feet, foot_body[kMaxFeet];
  int n_penalised, penalised_body[kMaxContactBodies];
  int n_terminal, terminal_body[kMaxContactBodies];
  float contact_threshold;
  float w_air_time, air_time_target;
  int air_gate;
  float air_cmd_min;
  float w_force, force_max;
  float w_stumble, stumble_ratio;
  float w_collision;
  int observe;
};
struct FeetRec {
  float t_last[kMaxFeet];  // the env time at which foot f was last evaluated in contact
  unsigned mask;           // bit f: foot f was in contact at the last step evaluation
  unsigned pad[3];
};
static_assert(sizeof(FeetRec) == 32, "one 32-byte record per env");
// Everything hb_env_kernel takes besides the model, by value (launch_env; filled by env_eval in hb_api_env.cpp).  A feature that is off is
// a null pointer - S.k_obs: the realism layer, dr: domain randomisation, term_obs, scan, cmd, feet - and nothing else of it is read.
struct EnvArgs {
  EnvConfig cfg;
  EnvRand R;
  EnvRandState S;
  DomainRand D;
  float* state; const float* qfrc; const int* counts;  // the batch's state records, the step's joint forces and counts
  float* prev; float* latest;                          // the adapter's action bookkeeping
  const float* qpos_src; int* episode; int* status;    // the reset pose, the episode numbers, the warning bits
  float* obs; float* reward; uint8_t* terminated; uint8_t* truncated;  // the outputs
  const uint8_t* mask;  // nullable [n_env]: only the envs whose byte is set are evaluated
  int observe;          // the observation goes through the realism layer's noise and delay lines instead of being the true one
  int step;             // this launch is a step of the episode: it may redraw a command inside an episode and it writes the feet records
                        // (not a pure evaluation, a settle step or the final observation of hb_env_reset)
  float* dr;            // [n_env][dr_stride] per-env model parameters
  int dr_stride, n_env, env_offset;
  float* term_obs;      // [n_env][row.width]: the observation of the state an episode ends in
  int* seen;            // nullable [n_env]: the warning bits of the episodes that ended
  EnvRow row;           // the rows of obs and term_obs
  // the scan, [n_env][row.n_scan], cast at the state the env kernel is handed (before any reset): it goes into the terminal row of an env
  // that resets and into the observation row of every other one; the scan columns of an env that resets are left to a second, masked ray
  // launch behind the env kernel, which reads reset_flag [n_env] (1: reset in this launch; nullable)
  const float* scan;
  uint8_t* reset_flag;
  // velocity commands: [n_env] (cx, cy, cyaw, the bits of the draw count k of the episode) - one 16-byte read per env
  float4* cmd;
  EnvCommands C;
  // foot-contact terms: every env's record, and the read-out [n_env][nbody][6] of the last physics substep
  FeetRec* feet;
  const float* body_contact;
  EnvFeet F;
};
constexpr int kAccPark = 24;  // floats per body in BatchPtrs::body_acc_park (six 16-byte moves)

}  // namespace hb
