// hb_launch.hpp — host-callable launchers implemented in the kernel translation units (hb_step.hip, hb_narrow.hip, hb_env.hip, hb_rollout.hip, hb_policy.hip, hb_kin.hip, hb_ray.hip, hb_dyn.hip, ...)
#pragma once
#include <hip/hip_runtime.h>
#include "hb_device.hpp"
namespace hb {
// M: the host's copy of *M_dev, from which every launcher reads the sizes, the variant and the LDS layout it needs
// the step launchers leave the name of the kernel they launched in *kernel (hb_last_kernel; a staged step: its fast-pass kernel)
hipError_t launch_step(const DevModel* M_dev, const DevModel& M, const BatchPtrs& P, int nsteps, hipStream_t stream, const char** kernel);
// inverse dynamics of the launch's envs (hb_inverse_dev; hb_step.hip)
hipError_t launch_inverse(const DevModel* M_dev, const DevModel& M, const BatchPtrs& P, hipStream_t stream, const char** kernel);
// whole-body kinematics of A.n states (hb_kin.hip): pack = 0 one state per wave, 1 as many as fit (HB_TUNE_KIN_PACK)
hipError_t launch_kinematics(const DevModel* M_dev, const DevModel& M, const KinArgs& A, int pack, hipStream_t stream, const char** kernel);
// mass matrix, bias and passive forces and Jacobians of A.n states (hb_dyn.hip; hb_dynamics*): pack as for launch_kinematics
hipError_t launch_dynamics(const DevModel* M_dev, const DevModel& M, const DynArgs& A, int pack, hipStream_t stream, const char** kernel);
// ---- the packed read-out kernels: lane = body, L lanes per state (the smallest of 16 / 32 / 64 that holds the nbody - 1 moving bodies; 64 without
// packing), 64 / L states per wave, every state with an LDS block of its own
inline int packed_lanes(int nbody, int pack) {
  const int lanes = nbody - 1;
  return !pack || lanes > 32 ? 64 : (lanes > 16 ? 32 : 16);
}
// one launch of the kernel of a 16 / 32 / 64 triple that packed_lanes() names, over A.n states of lds_floats floats each
template <class Args>
struct PackedKernel { void (*fn)(const DevModel*, const Args); const char* name; };
template <class Args>
inline hipError_t launch_packed(const PackedKernel<Args> (&triple)[3], const DevModel* M_dev, const DevModel& M, const Args& A, int pack, int lds_floats, hipStream_t stream,
                                const char** kernel) {
  (void)hipGetLastError();
  const int L = packed_lanes(M.nbody, pack);
  const int per = kGroup / L;
  const size_t lds = (size_t)per * lds_floats * sizeof(float);
  const long long blocks = (A.n + per - 1) / per;
  if (blocks < 1 || blocks > 0x7fffffffLL || lds > 64 * 1024) return hipErrorInvalidValue;  // (a block has 64 KB of LDS to ask for)
  const PackedKernel<Args>& K = triple[L == 16 ? 0 : (L == 32 ? 1 : 2)];
  hipLaunchKernelGGL(K.fn, dim3((unsigned)blocks), dim3(kGroup), lds, stream, M_dev, A);
  *kernel = K.name;
  return hipGetLastError();
}
// the configured rays against every env's geoms (hb_ray.hip; hb_rays*, and the scan of hb_env_obs_extend: RayArgs::xform)
hipError_t launch_rays(const DevModel* M_dev, const DevModel& M, const RayArgs& A, hipStream_t stream, const char** kernel);
// two envs per wave: a lean launch of the 27-dof humanoid's PGS kernel (hb_step_duo.hip; chosen by launch_step)
hipError_t launch_step_duo(const DevModel* M_dev, const BatchPtrs& P, int nsteps, hipStream_t stream, const char** kernel);
bool fold_pays(const DevModel& M, const BatchPtrs& P);
// the pose + narrowphase launches of one staged step (hb_narrow.hip)
hipError_t launch_pose_narrow(const DevModel* M_dev, const BatchPtrs& Q, hipStream_t stream);
hipError_t launch_reset(const DevModel& M, float* state, int* status, const uint8_t* mask, const float* qpos_src, const int* episode, int n_env, float perturb,
                        int env_offset, hipStream_t stream, float quat_perturb = 0.f);
hipError_t launch_envrand_reset(const DevModel& M, const EnvRand& R, const EnvRandState& S, const int* episode, const uint8_t* mask, int n_env, int env_offset,
                                hipStream_t stream);
hipError_t launch_action_env(const DevModel& M, const EnvRand& R, const EnvRandState& S, const float* action, float* prev, float* latest, float* ctrl,
                             const int* episode, const float* state, const uint8_t* mask, int n_env, int env_offset, hipStream_t stream);
hipError_t launch_reset_check(const int* counts, const uint8_t* terminated, const uint8_t* truncated, uint8_t* mask, int* episode, int* pending, int mode, int n_env,
                              hipStream_t stream);
hipError_t launch_obs(const DevModel& M, const float* state, float* obs, int n_env, hipStream_t stream);
hipError_t launch_action(const float* action, float* prev, float* latest, float* ctrl, int n, hipStream_t stream);
// reward / termination / auto-reset / observation row of G.n_env envs (hb_env.hip: hb_env_kernel)
hipError_t launch_env(const DevModel& M, const EnvArgs& G, hipStream_t stream);
// the feet records at an episode start outside the env kernel: t_last = the env's state time, every foot's bit set
hipError_t launch_feet_reset(FeetRec* rec, const float* state, int nstate, int n_feet, const uint8_t* mask, int n_env, hipStream_t stream);
// draw 0 of the episodes in `episode` for every env (or those of `mask`): the command state at an episode start outside the env kernel
hipError_t launch_command_reset(const EnvCommands& C, float4* cmd, const int* episode, const uint8_t* mask, int n_env, int env_offset, hipStream_t stream);
hipError_t launch_domain_rand(const DevModel& M, const DomainRand& D, float* dr, int stride, const int* episode, const uint8_t* mask, int n_env, int env_offset,
                              hipStream_t stream);
hipError_t launch_policy(const DevModel& M, const PolicyDesc& pd, const float* state, float* ctrl, int n_env, hipStream_t stream);
hipError_t launch_policy_lean(const DevModel& M, const PolicyDesc& pd, const float* state, float* ctrl, float* act, int n_env, hipStream_t stream);
// the sampling actor on obs [n_env][nobs] (hb_actor.hip; hb_env_collect_dev): env_global0 is the global index of row 0, draw the step counter of the draws
hipError_t launch_actor(const ActorDesc& ad, const float* obs, const ActorTapes& tp, int n_env, unsigned env_global0, unsigned draw, hipStream_t stream);
// the critic over rows [n_rows][nobs] (hb_gae.hip; hb_collect_gae_dev): out[i] = V(rows[i]); term / trunc given: only where trunc[i] && !term[i], the
// other rows are not read and get 0
hipError_t launch_value(const PolicyDesc& pd, const float* rows, const uint8_t* term, const uint8_t* trunc, long long n_rows, float* out, hipStream_t stream);
hipError_t launch_gae_scan(const GaeScan& g, hipStream_t stream);
hipError_t launch_log_prob(const LogProbDesc& d, long long n_rows, hipStream_t stream);
// the normaliser (hb_norm.hip): the chunk partials of a step or reset (and the per-env accumulators), then the merge and the normalisation
hipError_t launch_norm_moments(const NormDesc& d, hipStream_t stream);
hipError_t launch_norm_apply(const NormDesc& d, hipStream_t stream);
// the learner (hb_ppo.hip): the five launches of hb_ppo_grad_dev - forward with kept activations (and the advantage partials), the head
// (loss terms and the top gradients by row), the back-propagation of dZ through the layers, the chunk partials of dW / db / dlog_std
// and the statistics - and their merge; then the two of hb_ppo_adam_dev - the norm partials, and clipping + Adam + operand refresh.
// (What this learner's kernels and the SAC learner's do alike - the dW / db sweep, the merge of the partials, Adam's step, the refresh
// over ParamSeg segments, at most kLearnMaxSeg a launch - is hb_learn_core.hpp's and hb_device.hpp's learn_refresh.)
hipError_t launch_ppo_grad(const PpoDesc& d, hipStream_t stream);
hipError_t launch_ppo_adam(const PpoAdamDesc& d, hipStream_t stream);
// the SAC learner (hb_sac.hip), one launch each: njob forward passes side by side; the head by row (what: 0 the two samples and their
// log-probabilities, 1 the target and the critics' top dZ, 2 the actor's top dZ); njob reversed passes; the chunk partials of dW / db of
// the jobs and of the by-row terms; their merge; Adam over a stretch of the flat record; the Polyak step of the targets
hipError_t launch_sac_forward(const SacFwdDesc& d, int njob, hipStream_t stream);
hipError_t launch_sac_head(const SacHeadDesc& d, int what, hipStream_t stream);
hipError_t launch_sac_backprop(const SacBwdDesc& d, int njob, hipStream_t stream);
hipError_t launch_sac_wgrad(const SacWgDesc& d, hipStream_t stream);
hipError_t launch_sac_reduce(const SacReduceDesc& d, hipStream_t stream);
hipError_t launch_sac_adam(const SacAdamDesc& d, hipStream_t stream);
hipError_t launch_sac_polyak(const SacPolyakDesc& d, hipStream_t stream);
// order: [2 * n_env] ints - the permutation, then the sort keys of the pass (read once from counts)
hipError_t launch_order(const int* counts, int* order, int n_env, int e0, int n, hipStream_t stream, int slot = 3, int shift = 3);
hipError_t launch_mlp_layer(const float* X, const float* W, const float* bias, float* Y, int Mrows, int K, int N, int act, hipStream_t stream);
hipError_t launch_halton_ctrl(float* out, int T, int n_env, int nu, int t0, int env_offset, hipStream_t stream);
hipError_t launch_stand_cost(const float* rows, int H, int n_env, const StandTask& K, const int* status, float* total, float* costs, hipStream_t stream);
hipError_t launch_walk_cost(const float* rows, int H, int n_env, const WalkTask& K, const int* status, float* total, float* costs, hipStream_t stream);
hipError_t launch_cost_terms(const float* residual, int n, int nres, const CostSpec& K, float* terms, float* cost, hipStream_t stream);
hipError_t launch_spline_tape(const DevModel& M, const float* knots, const float* times, int P, int interp, float time0, float dt, int T, int n_env, float* tape, hipStream_t stream);
hipError_t launch_probe_spin(unsigned long long* out, unsigned ticks, hipStream_t stream);
hipError_t set_step_lds_limit(int bytes);
}  // namespace hb
