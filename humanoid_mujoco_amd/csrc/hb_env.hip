// hb_env.hip - the env adapter: reset, the realism layer, domain randomisation, the observation, the action bookkeeping, velocity
// commands, foot-contact terms, the env kernel (rewards, termination, auto-reset, the observation row) - and their launchers.
#include <hip/hip_runtime.h>
#include "hb_kcommon.hpp"
#include "hb_launch.hpp"

namespace hb {

// ------------------------------------------------------------------------------------------
// reset: qpos0/keyframe (+ Halton perturbation), zero velocity/warmstart/time/status
// qpos <- reset pose (+ the Halton perturbation indexed by global env and, for the env adapter, episode), rest zero
// (lane l of nl cooperating lanes writes the entries it owns: the qpos entries of joints l, l + nl, ... - every qpos entry belongs to one
// joint - and a strided share of the velocity and warm-start entries; l = 0, nl = 1: one thread does it all)
__device__ __forceinline__ void reset_state(const DevModel& M, float* s, const float* qpos_src, float perturb, int env_global, int ep, float quat_perturb = 0.f, int l = 0,
                                            int nl = 1) {
  if (l == 0) s[0] = 0.f;
  for (int i = l; i < 2 * M.nv; i += nl) s[1 + M.nq + i] = 0.f;
  const int idx = env_global + 1 + ep * 7919;
  for (int j = l; j < M.njnt; j += nl) {
    const int qa = M.jnt_qposadr[j];
    if (M.jnt_type[j] == 0) {
      for (int i = 0; i < 7; i++) s[1 + qa + i] = qpos_src[qa + i];
      if (perturb > 0.f) {
        s[1 + qa + 2] += perturb * 0.1f * halton(idx, 3);
        // root orientation: every quaternion component +- quat_perturb (cpu_env.py:316-328), left unnormalised as in the reference
        for (int i = 0; i < 4; i++) s[1 + qa + 3 + i] += perturb * quat_perturb * (2.f * halton(idx, 2 + M.njnt + i) - 1.f);
      }
    } else {
      s[1 + qa] = qpos_src[qa];
      if (perturb > 0.f) s[1 + qa] += perturb * 0.2f * (2.f * halton(idx, 2 + j) - 1.f);
    }
  }
}
__global__ void hb_reset_kernel(const DevModel M, float* state, int* status, const uint8_t* mask, const float* qpos_src, const int* episode, int n_env, float perturb,
                                int env_offset, float quat_perturb) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_env) return;
  if (mask && !mask[e]) return;
  reset_state(M, state + (size_t)e * M.nstate, qpos_src, perturb, env_offset + e, episode ? episode[e] : 0, quat_perturb);
  status[e] = 0;
}

// ---- env realism (hb_env_randomization): counter-based random numbers, delay rings, pushes -------------------
// One 32-bit word per (seed, global env, episode, step, stream, element): reproducible, order-free, and the same
// on any split of the batch.  tests/env_ref.py restates these functions in numpy.


// start of an episode: delays drawn (cpu_env.py:135-168), rings logically empty, push schedule cleared
__device__ __forceinline__ void envrand_begin_episode(const DevModel& M, const EnvRand& R, const EnvRandState& S, int e, int env_global, int ep) {
  const float dt = R.control_timestep > 0.f ? R.control_timestep : M.timestep;
  for (int c = 0; c < 4; c++) {
    const float u = rng_uniform(R.seed, env_global, ep, 0, RS_DELAY, c);
    const float d = (R.min_delay + u * (R.max_delay - R.min_delay)) * R.factor;
    S.delay[4 * e + c] = min(kDelaySlots - 1, max(0, (int)rintf(d / dt)));
  }
  S.k_act[e] = 0;
  S.k_obs[e] = 0;
  float* p = S.push + 8 * (size_t)e;
  if (S.xfrc) {
    const int body = (int)p[5];
    if (body > 0 && body < M.nbody) { S.xfrc[((size_t)e * M.nbody + body) * 6] = 0.f; S.xfrc[((size_t)e * M.nbody + body) * 6 + 1] = 0.f; }
  }
  for (int i = 0; i < 8; i++) p[i] = 0.f;
}
__global__ void hb_envrand_reset_kernel(const DevModel M, const EnvRand R, const EnvRandState S, const int* episode, const uint8_t* mask, int n_env, int env_offset) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_env || (mask && !mask[e])) return;
  envrand_begin_episode(M, R, S, e, env_offset + e, episode[e]);
}

// Per-env model parameters of one episode (cpu_env.py:188-264): see hb_domain_randomization in include/hb.h.
enum { RS_DR_MASS = 16, RS_DR_EXTRA, RS_DR_FRIC, RS_DR_ARM, RS_DR_STIFF, RS_DR_MARGIN, RS_DR_RANGE, RS_DR_KP, RS_DR_FRC, RS_DR_FLOOR };
// (NL cooperating lanes, l = this lane's number among them: every table is filled lane-strided; the height map's range is reduced
// over the lanes with shuffles, so NL is 1 or the env kernels' kDrawLanes = 16 consecutive lanes of a wave)
constexpr int kDrawLanes = 16;
template <int NL>
__device__ __forceinline__ void domain_draw(const DevModel& M, const DomainRand& D, float* d, int env_global, int ep, int l = 0) {
  static_assert(NL == 1 || NL == kDrawLanes, "domain_draw: one lane or kDrawLanes");
  const DomainLayout L = domain_layout(M.nbody, M.nv, M.nlimcand, M.nu, M.nhfielddata);
  const float rf = D.factor;
  auto U = [&](int stream, int idx) { return rng_uniform(D.seed, env_global, ep, 0, stream, idx); };
  if (l == 0) d[L.o_mass] = 0.f;
  const int bx = M.nbody > 1 ? 1 + min(M.nbody - 2, (int)(U(RS_DR_EXTRA, 0) * (float)(M.nbody - 1))) : -1;  // the body that carries the extra mass
  for (int sl = 1 + l; sl < M.nbody; sl += NL) {  // brec is level-ordered: slot -> body id, mass
    const float4 q0 = M.brec[(size_t)sl * kBrecQuads], q1 = M.brec[(size_t)sl * kBrecQuads + 1];
    const int b = __float_as_int(q0.x);
    float mass = fmaxf(1e-5f, q1.z + (2.f * U(RS_DR_MASS, b) - 1.f) * D.max_mass_change * rf);
    if (b == bx) mass += U(RS_DR_EXTRA, 1) * D.max_external_mass * rf;
    d[L.o_mass + b] = mass;
  }
  for (int i = l; i < M.nv; i += NL) {
    const float4 dA = M.drec[3 * i], dB = M.drec[3 * i + 1];
    const bool scalar = __float_as_int(dA.z) >= 2;  // hinge / slide
    d[L.o_arm + i] = dB.y + (scalar ? U(RS_DR_ARM, i) * D.armature_max_change * rf : 0.f);
    d[L.o_stiff + i] = dB.w + (scalar ? U(RS_DR_STIFF, i) * D.stiffness_max_change * rf : 0.f);
  }
  for (int c = l; c < M.nlimcand; c += NL) {
    const bool joint = M.lim_kind[c] == 0;
    const int id = M.lim_id[c];
    d[L.o_lmargin + c] = M.lim_margin[c] + (joint ? U(RS_DR_MARGIN, id) * D.margin_max_change * rf : 0.f);  // one margin per joint
    d[L.o_lrange + c] = M.lim_range[c] + (joint ? (2.f * U(RS_DR_RANGE, c) - 1.f) * D.range_max_change * rf : 0.f);
  }
  for (int a = l; a < M.nu; a += NL) {
    float gain = M.act_gain[a], bias1 = M.act_bias[3 * a + 1];
    if (D.kp_nominal > 0.f) {
      gain = D.kp_nominal + (2.f * U(RS_DR_KP, a) - 1.f) * D.kp_max_change * rf;
      if (bias1 != 0.f) bias1 = -gain;
    }
    d[L.o_gain + a] = gain;
    d[L.o_bias1 + a] = bias1;
    d[L.o_frc + 2 * a] = M.act_forcerange[2 * a] + (2.f * U(RS_DR_FRC, 2 * a) - 1.f) * D.force_limit_max_change * rf;
    d[L.o_frc + 2 * a + 1] = M.act_forcerange[2 * a + 1] + (2.f * U(RS_DR_FRC, 2 * a + 1) - 1.f) * D.force_limit_max_change * rf;
  }
  if (l == 0) d[L.o_fric] = (1.f - rf) + (D.friction_min_mult + U(RS_DR_FRIC, 0) * (D.friction_max_mult - D.friction_min_mult)) * rf;
  // floor height maps (CPUEnv._randomize_floor_heightmap, cpu_env.py:267-280: Perlin noise on the grid, shifted and scaled to
  // [0, 1], times MIN + factor (MAX - MIN)).  The reference's noise comes from the third-party perlin_noise package; here:
  // three octaves of smooth value noise from the counter-based generator, normalised the same way.
  const float bump = D.floor_bump_min + rf * (D.floor_bump_max - D.floor_bump_min);
  for (int hf = 0, adr = 0; adr < M.nhfielddata; hf++) {
    const int nr = M.hfield_nrow[hf], nc = M.hfield_ncol[hf], n = nr * nc;
    float* h = d + L.o_hfield + adr;
    if (!(D.floor_bump_max > 0.f)) { for (int i = l; i < n; i += NL) h[i] = M.hfield_data[adr + i]; adr += n; continue; }
    float lo = 3.0e38f, hi = -3.0e38f;
    for (int i = l; i < n; i += NL) {
      const int r = i / nc, c = i - r * nc;
      float v = 0.f, amp = 1.f;
      for (int oct = 0, cells = 2; oct < 3; oct++, cells *= 2, amp *= 0.5f) {  // lattices of 3x3, 5x5, 9x9 nodes over the field
        const float x = (float)c / (float)max(1, nc - 1) * (float)cells, y = (float)r / (float)max(1, nr - 1) * (float)cells;
        const int x0 = min((int)x, cells - 1), y0 = min((int)y, cells - 1);
        float fx = x - (float)x0, fy = y - (float)y0;
        fx = fx * fx * (3.f - 2.f * fx); fy = fy * fy * (3.f - 2.f * fy);  // smoothstep
        auto node = [&](int ix, int iy) { return rng_uniform(D.seed, env_global, ep, hf, RS_DR_FLOOR, (oct * 16 + iy) * 16 + ix); };
        const float a = node(x0, y0), b = node(x0 + 1, y0), cc = node(x0, y0 + 1), dd = node(x0 + 1, y0 + 1);
        v += amp * ((a * (1.f - fx) + b * fx) * (1.f - fy) + (cc * (1.f - fx) + dd * fx) * fy);
      }
      h[i] = v;  // (re-read below by the lane that wrote it)
      lo = fminf(lo, v); hi = fmaxf(hi, v);
    }
    if (NL > 1) {
#pragma unroll
      for (int m = NL / 2; m >= 1; m >>= 1) { lo = fminf(lo, __shfl_xor(lo, m, NL)); hi = fmaxf(hi, __shfl_xor(hi, m, NL)); }
    }
    const float sc = hi > lo ? bump / (hi - lo) : 0.f;
    for (int i = l; i < n; i += NL) h[i] = (h[i] - lo) * sc;
    adr += n;
  }
}
__global__ void hb_domain_rand_kernel(const DevModel M, const DomainRand D, float* dr, int stride, const int* episode, const uint8_t* mask, int n_env, int env_offset) {
  const int e = (blockIdx.x * blockDim.x + threadIdx.x) / kDrawLanes, l = threadIdx.x % kDrawLanes;
  if (e >= n_env || (mask && !mask[e])) return;
  domain_draw<kDrawLanes>(M, D, dr + (size_t)e * stride, env_offset + e, episode[e], l);
}

// value through a delay ring: push x as item k, return item k - d (filler before the ring has d items)
__device__ __forceinline__ float ring_delay(float* ring, int stride, int k, int d, float x, float filler) {
  ring[(size_t)(k % kDelaySlots) * stride] = x;
  if (d == 0) return x;
  return k >= d ? ring[(size_t)((k - d) % kDelaySlots) * stride] : filler;
}

// CPUEnv._apply_action + _apply_external_forces (cpu_env.py:612-674) for one env per thread.
// action == nullptr: the reference's step(None), which re-applies the current controls without noise.
__global__ void hb_action_env_kernel(const DevModel M, const EnvRand R, const EnvRandState S, const float* action, float* prev, float* latest, float* ctrl,
                                     const int* episode, const float* state, const uint8_t* mask, int n_env, int env_offset) {
  // (sixteen lanes per env: the actuators lane-strided, the push schedule on the env's first lane)
  const int e = (blockIdx.x * blockDim.x + threadIdx.x) / 16, l = threadIdx.x % 16;
  if (e >= n_env || (mask && !mask[e])) return;
  const int nu = M.nu, ge = env_offset + e, ep = episode[e];
  const int k = S.k_act[e], d = S.delay[4 * e];
  const unsigned kk = R.frozen_noise ? 0u : (unsigned)k;
  for (int i = l; i < nu; i += 16) {
    const size_t ai = (size_t)e * nu + i;
    float a = action ? action[ai] : ctrl[ai];
    if (action && R.action_noise > 0.f) a += R.factor * R.action_noise * rng_normal(R.seed, ge, ep, kk, RS_ACTION, i);
    const float out = ring_delay(S.fifo_act + ((size_t)e * kDelaySlots) * nu + i, nu, k, d, a, 0.f);
    prev[ai] = latest[ai];
    latest[ai] = out;
    ctrl[ai] = out;
  }
  if (l != 0) return;
  S.k_act[e] = k + 1;
  if (R.push_enabled && S.xfrc) {
    float* p = S.push + 8 * (size_t)e;
    float* xf = S.xfrc + (size_t)e * M.nbody * 6;
    const float time = state[(size_t)e * M.nstate];
    if (time >= p[0] + p[1]) {  // window over (or first step): clear the old force, schedule the next push
      const unsigned ev = (unsigned)p[6];
      int body = (int)p[5];
      if (body > 0 && body < M.nbody) { xf[6 * body] = 0.f; xf[6 * body + 1] = 0.f; }
      p[0] = time + R.push_min_interval + rng_uniform(R.seed, ge, ep, ev, RS_PUSH, 0) * (R.push_max_interval - R.push_min_interval);
      p[1] = R.push_min_duration + rng_uniform(R.seed, ge, ep, ev, RS_PUSH, 1) * (R.push_max_duration - R.push_min_duration);
      p[2] = R.factor * (R.push_min_force + rng_uniform(R.seed, ge, ep, ev, RS_PUSH, 2) * (R.push_max_force - R.push_min_force));
      float dx = 2.f * rng_uniform(R.seed, ge, ep, ev, RS_PUSH, 3) - 1.f, dy = 2.f * rng_uniform(R.seed, ge, ep, ev, RS_PUSH, 4) - 1.f;
      const float n = sqrtf(dx * dx + dy * dy);  // never 0: the uniforms are odd multiples of 2^-24
      p[3] = dx / n; p[4] = dy / n;
      body = 1 + min(M.nbody - 2, (int)(rng_uniform(R.seed, ge, ep, ev, RS_PUSH, 5) * (float)(M.nbody - 1)));
      p[5] = (float)body;
      p[6] = (float)(ev + 1);
    }
    if (time > p[0] && time < p[0] + p[1]) {
      const int body = (int)p[5];
      xf[6 * body] = p[3] * p[2];
      xf[6 * body + 1] = p[4] * p[2];
    }
  }
}

// CPUEnv._get_obs's noise and delay lines (cpu_env.py:465-545) applied in place to the true observation o
// env adapter: observation, the 27-DoF analogue of CPUEnv._get_obs (cpu_env.py:465-571):
// [hinge/slide qpos, hinge/slide qvel, root angular velocity, gravity direction in the root body frame]
// (lane l of nl cooperating lanes writes entries l, l + nl, ... of each part)
__device__ __forceinline__ Q4 obs_root_quat(const DevModel& M, const float* s) {
  const int da = M.obs_root_dofadr;
  return da >= 0 ? ldq(s + 1 + M.jnt_qposadr[M.dof_jntid[da]] + 3) : Q4{1.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ void compute_obs(const DevModel& M, const float* s, float* o, int l = 0, int nl = 1) {
  const float* qpos = s + 1;
  const float* qvel = s + 1 + M.nq;
  const int nj = (M.nobs - 6) / 2;
  for (int i = l; i < nj; i += nl) { o[i] = qpos[M.jnt_qposadr[M.obs_jnt[i]]]; o[nj + i] = qvel[M.jnt_dofadr[M.obs_jnt[i]]]; }
  const int da = M.obs_root_dofadr;
  // gravity direction in the torso frame: R(q)^T (0,0,-1)  (cpu_env.py:510-519)
  float m[9];
  q2mat(m, qnormalize(obs_root_quat(M, s)));
  for (int c = l; c < 3; c += nl) { o[2 * nj + c] = da >= 0 ? qvel[da + 3 + c] : 0.f; o[2 * nj + 3 + c] = -m[6 + c]; }
}

// the same observation through CPUEnv's sensor model (cpu_env.py:465-571): noise on every reading, each group of readings delayed by
// its own number of control steps (rings of kDelaySlots past readings)
__device__ __forceinline__ void envrand_observe(const DevModel& M, const EnvRand& R, const EnvRandState& S, int e, int env_global, int ep, const float* s, float* o, int l = 0,
                                                int nl = 1) {
  const float* qpos = s + 1;
  const float* qvel = s + 1 + M.nq;
  const int k = S.k_obs[e];
  const unsigned kk = R.frozen_noise ? 0u : (unsigned)k;
  const int nj = (M.nobs - 6) / 2;
  const int dj = S.delay[4 * e + 1], dg = S.delay[4 * e + 2], dv = S.delay[4 * e + 3];
  float* rj = S.fifo_joint + ((size_t)e * kDelaySlots) * 2 * nj;
  for (int i = l; i < nj; i += nl) {
    const float a = qpos[M.jnt_qposadr[M.obs_jnt[i]]] + R.factor * R.joint_angle_noise * rng_normal(R.seed, env_global, ep, kk, RS_JOINT_POS, i);
    const float v = qvel[M.jnt_dofadr[M.obs_jnt[i]]] + R.factor * R.joint_velocity_noise * rng_normal(R.seed, env_global, ep, kk, RS_JOINT_VEL, i);
    o[i] = ring_delay(rj + i, 2 * nj, k, dj, a, 0.f);
    o[nj + i] = ring_delay(rj + nj + i, 2 * nj, k, dj, v, 0.f);
  }
  if (l < 3) {  // (the three components of the gyro and of the gravity direction: lanes 0..2, or one lane all three)
    const int da = M.obs_root_dofadr;
    // gravity direction from the noisy, re-normalised torso quaternion (Rotation.from_quat normalises)
    Q4 q = obs_root_quat(M, s);
    q.w += R.factor * R.imu_noise * rng_normal(R.seed, env_global, ep, kk, RS_IMU, 0);
    q.x += R.factor * R.imu_noise * rng_normal(R.seed, env_global, ep, kk, RS_IMU, 1);
    q.y += R.factor * R.imu_noise * rng_normal(R.seed, env_global, ep, kk, RS_IMU, 2);
    q.z += R.factor * R.imu_noise * rng_normal(R.seed, env_global, ep, kk, RS_IMU, 3);
    float m[9];
    q2mat(m, qnormalize(q));
    float* rg = S.fifo_gyro + ((size_t)e * kDelaySlots) * 3;
    float* rv = S.fifo_grav + ((size_t)e * kDelaySlots) * 3;
    for (int c = l; c < 3; c += nl) {
      const float w = (da >= 0 ? qvel[da + 3 + c] : 0.f) + R.factor * R.gyro_noise * rng_normal(R.seed, env_global, ep, kk, RS_GYRO, c);
      o[2 * nj + c] = ring_delay(rg + c, 3, k, dg, w, 0.f);
      o[2 * nj + 3 + c] = ring_delay(rv + c, 3, k, dv, -m[6 + c], c == 2 ? -1.f : 0.f);
    }
  }
  if (l == 0) S.k_obs[e] = k + 1;
}

__global__ void hb_obs_kernel(const DevModel M, const float* state, float* obs, int n_env) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_env) return;
  compute_obs(M, state + (size_t)e * M.nstate, obs + (size_t)e * M.nobs);
}

// CPUEnv._apply_action bookkeeping (cpu_env.py:656-674): previous <- latest, latest <- action, ctrl <- action
__global__ void hb_action_kernel(const float* action, float* prev, float* latest, float* ctrl, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  prev[i] = latest[i];
  float a = action[i];
  latest[i] = a;
  ctrl[i] = a;
}

__device__ __forceinline__ float scaled_exp(float x) { return expf(-x / 0.5f); }  // reward_functions.py:17-19

// ---- velocity commands (hb_env_commands_configure; include/hb.h has the definitions, tests/cmd_ref.py restates them) ----------------
// Draw k of episode ep of global env g, by NL >= 4 cooperating lanes of which l is this one: lane c < 3 returns component c of the
// command, lo_c + u_{c+1} (hi_c - lo_c) as a subtract, a multiply and an add, each rounded once, or 0 where u_0 < zero_fraction (lane 3
// draws u_0 and hands it round); the other lanes return nothing of use.  One hash per lane and one shuffle: no serial loop.
template <int NL>
__device__ __forceinline__ float command_draw(const EnvCommands& C, int env_global, int ep, int k, int l) {
  static_assert(NL >= 4 && (NL & (NL - 1)) == 0, "command_draw: four lanes or more");
  const float u = rng_uniform(C.seed, env_global, ep, k, RS_COMMAND, (l + 1) & 3);
  const float u0 = __shfl(u, 3, NL);
  // (the three ranges applied to this lane's u and the lane's own picked from the results: a pick among the configuration's fields
  // themselves becomes an indexed read of the kernel argument, which costs the env kernel a stack frame)
  const float vx = __fadd_rn(C.vx_min, __fmul_rn(u, __fsub_rn(C.vx_max, C.vx_min)));
  const float vy = __fadd_rn(C.vy_min, __fmul_rn(u, __fsub_rn(C.vy_max, C.vy_min)));
  const float vw = __fadd_rn(C.yaw_min, __fmul_rn(u, __fsub_rn(C.yaw_max, C.yaw_min)));
  return u0 < C.zero_fraction ? 0.f : l == 0 ? vx : l == 1 ? vy : vw;
}
// ... and into the env's record: lanes 0..2 their component, lane 3 the new draw count (four neighbouring words: one transaction)
__device__ __forceinline__ void command_store(float4* rec, int l, float v, int k_next) {
  if (l < 3) reinterpret_cast<float*>(rec)[l] = v;
  else if (l == 3) reinterpret_cast<int*>(rec)[3] = k_next;
}
constexpr int kCmdLanes = 4;
__global__ void hb_command_reset_kernel(const EnvCommands C, float4* cmd, const int* episode, const uint8_t* mask, int n_env, int env_offset) {
  const int e = (blockIdx.x * blockDim.x + threadIdx.x) / kCmdLanes, l = threadIdx.x % kCmdLanes;
  if (e >= n_env || (mask && !mask[e])) return;
  command_store(cmd + e, l, command_draw<kCmdLanes>(C, env_offset + e, episode[e], 0, l), 1);
}

// ---- foot-contact terms (hb_env_feet_configure; include/hb.h has the definitions, tests/feet_ref.py restates them) -------------------
// |F|^2 of a body's read-out row, and the planar and the normal part it is made of: every product and sum rounded once, in the order
// (Fx Fx + Fy Fy) + Fz Fz, so that the contact and stumble decisions are reproducible bit for bit
__device__ __forceinline__ float contact_n2(const float* bc, int body, float& pl, float& zz) {
  const float fx = bc[6 * body], fy = bc[6 * body + 1], fz = bc[6 * body + 2];
  pl = __fadd_rn(__fmul_rn(fx, fx), __fmul_rn(fy, fy));
  zz = __fmul_rn(fz, fz);
  return __fadd_rn(pl, zz);
}
// The body lane l owns in a list of the configuration (-1: none).  The list's entries are compared and selected one by one: an
// indexed read of the kernel argument would cost the env kernel a stack frame (see command_draw).
template <int N>
__device__ __forceinline__ int feet_pick(const int (&list)[N], int n, int l) {
  int b = -1;
#pragma unroll
  for (int i = 0; i < N; i++) b = l == i ? list[i] : b;
  return l < n ? b : -1;
}
// episode start outside the env kernel (hb_env_reset, hb_env_feet_configure): t_last = the env's state time, every foot's bit set
__global__ void hb_feet_reset_kernel(FeetRec* rec, const float* state, int nstate, int n_feet, const uint8_t* mask, int n_env) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_env || (mask && !mask[e])) return;
  const float t = state[(size_t)e * nstate];
  FeetRec r;
  for (int f = 0; f < kMaxFeet; f++) r.t_last[f] = t;
  r.mask = (1u << n_feet) - 1u;
  r.pad[0] = r.pad[1] = r.pad[2] = 0u;
  rec[e] = r;
}

// standupReward (reward_functions.py:247-374) + observation + termination + auto-reset.  kEnvLanes lanes per env, 256 / kEnvLanes
// envs per block (it was one thread per env: 37 us of serial work on 32 CUs for 4096 envs, a fifth of VecEnv.step_torch's GPU time).
// The env's state record is staged in LDS (one coalesced pass instead of a strided read per thread); sums over joints, actuators
// and symmetry pairs are lane-strided partial sums reduced over the env's lanes; an auto-reset writes the new state into the same
// LDS copy (every lane the joints it owns), so that the observation of the new episode is read from it after the block barrier.
constexpr int kEnvLanes = 16;
__device__ __forceinline__ float env_lane_sum(float x) {
#pragma unroll
  for (int m = kEnvLanes / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m, kEnvLanes);
  return x;
}
// What a row holds behind the base observation (EnvRow; no noise, no delay), written by the env's lanes: the env's last action, the scan
// cast before this kernel (with_scan) or nothing in its columns, the feet's contact flags of `feet_mask`, the command of which `cmd_l` is
// this lane's component.  A part that is off has count 0.
__device__ __forceinline__ void env_row_tail(const EnvArgs& G, float* o, int e, int l, int nu, bool with_scan, unsigned feet_mask, float cmd_l) {
  const EnvRow& W = G.row;
  for (int i = l; i < W.n_prev_action; i += kEnvLanes) o[W.prev_action + i] = G.latest[(size_t)e * nu + i];
  if (with_scan) for (int i = l; i < W.n_scan; i += kEnvLanes) o[W.scan + i] = G.scan[(size_t)e * W.n_scan + i];
  if (l < W.n_foot_contact) o[W.foot_contact + l] = (feet_mask >> l) & 1u ? 1.f : 0.f;
  for (int i = l; i < W.n_command; i += kEnvLanes) o[W.command + i] = cmd_l;
}
__global__ __launch_bounds__(256) void hb_env_kernel(const DevModel M, const EnvArgs G) {
  const EnvConfig& cfg = G.cfg;
  const EnvRand& R = G.R;
  const EnvRandState& S = G.S;
  const EnvCommands& C = G.C;
  const EnvFeet& F = G.F;
  extern __shared__ float sh_state[];
  const int grp = threadIdx.x / kEnvLanes, l = threadIdx.x % kEnvLanes;
  const int e = blockIdx.x * (256 / kEnvLanes) + grp;
  const bool active = e < G.n_env && (!G.mask || G.mask[e]);
  const int nsp = (M.nstate + 3) & ~3;
  float* ls = sh_state + grp * nsp;
  float* s = G.state + (size_t)(active ? e : 0) * M.nstate;
  if (active) for (int i = l; i < M.nstate; i += kEnvLanes) ls[i] = s[i];
  __syncthreads();
  bool reset = false;
  float feet_t = 0.f;      // (feet, lane f < n_feet: the time foot f was last in contact, as this evaluation leaves it)
  unsigned feet_mask = 0;  // (feet: the contact bits of this evaluation where it updates the record, else the record's)
  float cmd_l = 0.f;  // (commands: this lane's word of the env's record - lanes 0..2: a component of the command in force during the
                      // step that is rewarded here, lane 3: the draws made so far in the episode)
  if (active) {
    const float* qpos = ls + 1;
    const float* qvel = ls + 1 + M.nq;
    const int da = M.obs_root_dofadr;
    // root height and the gravity direction in the torso frame (every lane)
    Q4 q = {1.f, 0.f, 0.f, 0.f};
    float z = 0.f;
    if (da >= 0) { const int qa = M.jnt_qposadr[M.dof_jntid[da]]; q = qnormalize(ldq(qpos + qa + 3)); z = qpos[qa + 2]; }
    float m[9];
    q2mat(m, q);
    const float g[3] = {-m[6], -m[7], -m[8]};
    float r = 0.f;
    // horizontal velocity
    float vx = da >= 0 ? qvel[da] : 0.f, vy = da >= 0 ? qvel[da + 1] : 0.f;
    float tvx = cfg.target_velocity[0], tvy = cfg.target_velocity[1];
    float4 cmd = {0.f, 0.f, 0.f, 0.f};
    if (G.cmd) {
      cmd = G.cmd[e];
      tvx = cmd.x; tvy = cmd.y;
      cmd_l = l == 0 ? cmd.x : l == 1 ? cmd.y : l == 2 ? cmd.z : cmd.w;
      if (C.frame == 1) {  // the planar velocity in the root's heading frame (m[0], m[3]: the root's x axis in the world)
        float hc, hs;
        heading_cs(m[0], m[3], hc, hs);
        const float wx = vx, wy = vy;
        vx = hc * wx + hs * wy; vy = hc * wy - hs * wx;
      }
    }
    float dvx = vx - tvx, dvy = vy - tvy;
    r += cfg.w_hvel * scaled_exp(dvx * dvx + dvy * dvy);
    if (G.cmd) {  // the yaw rate: the world z component of the root's (body-frame) angular velocity
      const float dw = (da >= 0 ? m[6] * qvel[da + 3] + m[7] * qvel[da + 4] + m[8] * qvel[da + 5] : 0.f) - cmd.z;
      r += C.w_yaw * scaled_exp(dw * dw);
    }
    // upright: |g_local - (0,0,-1)|^2
    r += cfg.w_upright * scaled_exp(g[0] * g[0] + g[1] * g[1] + (g[2] + 1.f) * (g[2] + 1.f));
    // torso height: linear ramp min_z -> target_z, clamped (numpy.interp)
    float t = (z - cfg.min_z) / fmaxf(cfg.target_z - cfg.min_z, 1e-9f);
    r += cfg.w_height * fminf(fmaxf(t, 0.f), 1.f);
    // joint torques on the scalar joints' dofs
    {
      float acc = 0.f, n = 0.f;
      for (int j = l; j < M.njnt; j += kEnvLanes)
        if (M.jnt_type[j] >= 2) {
          float x = fmaxf(fabsf(G.qfrc[(size_t)e * M.nv + M.jnt_dofadr[j]]) - cfg.safe_torque, 0.f);
          acc += scaled_exp(x * x);
          n += 1.f;
        }
      acc = env_lane_sum(acc); n = env_lane_sum(n);
      if (n > 0.f) r += cfg.w_torque * acc / n;
    }
    // control change / regularisation / symmetry on the (scaled) actions
    const float* pa = G.prev + (size_t)e * M.nu;
    const float* la = G.latest + (size_t)e * M.nu;
    const float inv = 1.f / cfg.action_scale;
    if (M.nu > 0) {
      float chg = 0.f, reg = 0.f;
      for (int i = l; i < M.nu; i += kEnvLanes) {
        float d = (la[i] - pa[i]) * inv * cfg.control_frequency;
        chg += scaled_exp(d * d);
        float a = la[i] * inv;
        reg += scaled_exp(a * a);
      }
      chg = env_lane_sum(chg); reg = env_lane_sum(reg);
      r += cfg.w_ctrl_change * chg / (float)M.nu + cfg.w_ctrl_reg * reg / (float)M.nu;
    }
    if (cfg.n_equal + cfg.n_opposite > 0) {
      float sym = 0.f;
      for (int k = l; k < cfg.n_equal + cfg.n_opposite; k += kEnvLanes) {
        const bool eq = k < cfg.n_equal;
        const int a0 = eq ? cfg.equal_pairs[k][0] : cfg.opposite_pairs[k - cfg.n_equal][0], a1 = eq ? cfg.equal_pairs[k][1] : cfg.opposite_pairs[k - cfg.n_equal][1];
        const float d = (eq ? la[a0] - la[a1] : la[a0] + la[a1]) * inv;
        sym += scaled_exp(d * d);
      }
      sym = env_lane_sum(sym);
      r += cfg.w_symmetry * sym / (float)(cfg.n_equal + cfg.n_opposite);
    }
    if (cfg.w_vvel != 0.f) { const float vz = da >= 0 ? qvel[da + 2] : 0.f; r += cfg.w_vvel * scaled_exp(vz * vz); }  // vertical_velocity_penalty
    if (G.counts[kCountStride * e + 4]) r += cfg.self_collision_penalty;
    bool feet_term = false;
    if (G.feet) {
      // lane f < n_feet owns foot f; lanes 0..7 a penalised body each, lanes 8..15 a terminal body each.  The flags travel as one
      // small integer per lane - stumbles, collisions and terminal contacts counted in fields of four bits, the feet's contact bits
      // above them -, exact in fp32, so that three lane sums serve every term.
      const float* bc = G.body_contact + (size_t)e * M.nbody * 6;
      const float thr2 = __fmul_rn(F.contact_threshold, F.contact_threshold);
      const int fb = feet_pick(F.foot_body, F.n_feet, l);
      const int pb = feet_pick(F.penalised_body, F.n_penalised, l);
      const int tb = feet_pick(F.terminal_body, F.n_terminal, l - kMaxContactBodies);
      const unsigned old_mask = G.feet[e].mask;
      float air = 0.f, force = 0.f, pl, zz;
      int flags = 0;
      if (fb >= 0) {
        const float tl = G.feet[e].t_last[l];
        const float n2 = contact_n2(bc, fb, pl, zz);
        const bool c = n2 > thr2;
        if (c && !((old_mask >> l) & 1u)) air = __fsub_rn(ls[0], tl) - F.air_time_target;
        force = fmaxf(sqrtf(n2) - F.force_max, 0.f);
        if (c && pl > __fmul_rn(__fmul_rn(F.stumble_ratio, F.stumble_ratio), zz)) flags += 1;
        if (c) flags += 4096 << l;
        feet_t = c ? ls[0] : tl;
      }
      if (pb >= 0 && contact_n2(bc, pb, pl, zz) > thr2) flags += 16;
      if (tb >= 0 && contact_n2(bc, tb, pl, zz) > thr2) flags += 256;
      air = env_lane_sum(air); force = env_lane_sum(force);
      flags = (int)env_lane_sum((float)flags);
      const bool gate = !F.air_gate || __fadd_rn(__fmul_rn(tvx, tvx), __fmul_rn(tvy, tvy)) > __fmul_rn(F.air_cmd_min, F.air_cmd_min);
      if (gate) r += F.w_air_time * air;
      r += F.w_force * force;
      if (flags & 15) r += F.w_stumble;
      r += F.w_collision * (float)((flags >> 4) & 15);
      feet_term = ((flags >> 8) & 15) != 0;
      feet_mask = G.step ? (unsigned)flags >> 12 : old_mask;
    }
    const bool upright = fmaxf(fabsf(g[0]), fabsf(g[1])) < cfg.upright_tol;
    const bool timeup = cfg.max_time > 0.f && ls[0] >= cfg.max_time;
    bool term, trunc;
    if (cfg.reward_kind == 1) {  // controlInputReward: fall = terminal (with the terminal reward), time limit = truncation
      term = !upright || z < cfg.min_z_grounded;
      trunc = timeup;
    } else {                     // standupReward: time limit = terminal, standing up = truncation ("is_success")
      term = timeup;
      trunc = z >= cfg.target_z && upright;
    }
    term = term || feet_term;
    if (term) r = cfg.terminal_reward;
    if (l == 0) { G.reward[e] = r; G.terminated[e] = term ? 1 : 0; G.truncated[e] = trunc ? 1 : 0; }
    reset = (term || trunc) && cfg.auto_reset;
  }
  const bool rand_on = S.k_obs != nullptr;
  int ep = active ? G.episode[e] : 0;
  // the observation of the state an episode ENDS in, before the env is reset in place: what stable-baselines3's VecEnv hands the learner as
  // infos[i]["terminal_observation"] (DummyVecEnv.step_wait; SAC / PPO bootstrap from it when the episode was truncated) - the same sensor
  // model, noise and delays as any other observation of that episode (CPUEnv.step returns self._get_obs() before anything resets)
  if (reset && G.term_obs) {
    float* to = G.term_obs + (size_t)e * G.row.width;
    if (rand_on && G.observe) envrand_observe(M, R, S, e, G.env_offset + e, ep, ls, to, l, kEnvLanes);
    else compute_obs(M, ls, to, l, kEnvLanes);
    // of the state the episode ends in: the action just applied, the scan before the reset (over the old elevations), the ending state's
    // flags, the old command
    env_row_tail(G, to, e, l, M.nu, true, feet_mask, cmd_l);
  }
  __syncthreads();  // (every lane has read the old state and the old episode number)
  if (reset) {
    // CPUEnv.reset for this env; the perturbation index advances with the episode count
    ep += 1;
    reset_state(M, ls, G.qpos_src, cfg.reset_perturb, G.env_offset + e, ep, cfg.reset_quat_perturb, l, kEnvLanes);
    for (int i = l; i < M.nu; i += kEnvLanes) { G.prev[(size_t)e * M.nu + i] = 0.f; G.latest[(size_t)e * M.nu + i] = 0.f; }
    if (l == 0) {
      G.episode[e] = ep;
      if (G.seen) G.seen[e] |= G.status[e];  // (the warning bits of the episode that ends here stay readable: hb_env_warnings)
      G.status[e] = 0;
      if (rand_on) envrand_begin_episode(M, R, S, e, G.env_offset + e, ep);
    }
    static_assert(kEnvLanes == kDrawLanes, "the env kernel draws an episode's model parameters with all lanes of the env");
    if (G.dr) domain_draw<kDrawLanes>(M, G.D, G.dr + (size_t)e * G.dr_stride, G.env_offset + e, ep, l);
  }
  if (G.cmd && active) {
    // draw 0 of the episode that begins here, or - in a step - draw k of the one that goes on once its time has come: at most one draw
    const int k = reset ? 0 : __float_as_int(__shfl(cmd_l, 3, kEnvLanes));
    if (reset || (G.step && C.resample_time > 0.f && ls[0] >= __fmul_rn((float)k, C.resample_time))) {
      cmd_l = command_draw<kEnvLanes>(C, G.env_offset + e, ep, k, l);
      command_store(G.cmd + e, l, cmd_l, k + 1);
    }
  }
  __threadfence_block();
  __syncthreads();  // the new state (LDS) and the new episode's delays (global, written by lane 0) are visible to the env's lanes
  if (active) {
    if (reset) for (int i = l; i < M.nstate; i += kEnvLanes) s[i] = ls[i];
    float* o = G.obs + (size_t)e * G.row.width;
    if (rand_on && G.observe) envrand_observe(M, R, S, e, G.env_offset + e, ep, ls, o, l, kEnvLanes);
    else compute_obs(M, ls, o, l, kEnvLanes);
    if (G.feet) {
      // an episode that begins here starts with its feet down at the new state's time: a standing start pays nothing
      if (reset) { feet_t = ls[0]; feet_mask = (1u << F.n_feet) - 1u; }
      if (G.step) {
        if (l < F.n_feet) G.feet[e].t_last[l] = feet_t;
        if (l == 0) G.feet[e].mask = feet_mask;
      }
    }
    // the last action - zero in a new episode: this lane cleared these very entries above -, and the scan of an env that goes on; an env
    // that was reset gets its scan from the masked ray launch behind this kernel
    env_row_tail(G, o, e, l, M.nu, !reset, feet_mask, cmd_l);
  }
  if (G.reset_flag && e < G.n_env && l == 0) G.reset_flag[e] = reset ? 1 : 0;
}

// hb_env_reset's collision test (cpu_env.py:411-414): envs of the mask that collide (mode 1: any contact, mode 2:
// self-contact) or ended in their settle step stay in the mask, get a new episode number and are counted
__global__ void hb_reset_check_kernel(const int* counts, const uint8_t* terminated, const uint8_t* truncated, uint8_t* mask, int* episode, int* pending, int mode,
                                      int n_env) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_env || !mask[e]) return;
  const bool hit = mode == 1 ? counts[kCountStride * e] > 0 : counts[kCountStride * e + 4] != 0;
  if (hit || terminated[e] || truncated[e]) { episode[e]++; atomicAdd(pending, 1); }
  else mask[e] = 0;
}

hipError_t launch_reset(const DevModel& M, float* state, int* status, const uint8_t* mask, const float* qpos_src, const int* episode, int n_env, float perturb,
                        int env_offset, hipStream_t stream, float quat_perturb) {
  (void)hipGetLastError();  // the result below must be this launch's, not an older call's sticky error
  hipLaunchKernelGGL(hb_reset_kernel, dim3((n_env + 255) / 256), dim3(256), 0, stream, M, state, status, mask, qpos_src, episode, n_env, perturb, env_offset, quat_perturb);
  return hipGetLastError();
}
hipError_t launch_envrand_reset(const DevModel& M, const EnvRand& R, const EnvRandState& S, const int* episode, const uint8_t* mask, int n_env, int env_offset,
                                hipStream_t stream) {
  (void)hipGetLastError();  // the result below must be this launch's, not an older call's sticky error
  hipLaunchKernelGGL(hb_envrand_reset_kernel, dim3((n_env + 127) / 128), dim3(128), 0, stream, M, R, S, episode, mask, n_env, env_offset);
  return hipGetLastError();
}
hipError_t launch_action_env(const DevModel& M, const EnvRand& R, const EnvRandState& S, const float* action, float* prev, float* latest, float* ctrl,
                             const int* episode, const float* state, const uint8_t* mask, int n_env, int env_offset, hipStream_t stream) {
  (void)hipGetLastError();  // the result below must be this launch's, not an older call's sticky error
  hipLaunchKernelGGL(hb_action_env_kernel, dim3((n_env + 15) / 16), dim3(256), 0, stream, M, R, S, action, prev, latest, ctrl, episode, state, mask, n_env,
                     env_offset);
  return hipGetLastError();
}
hipError_t launch_reset_check(const int* counts, const uint8_t* terminated, const uint8_t* truncated, uint8_t* mask, int* episode, int* pending, int mode, int n_env,
                              hipStream_t stream) {
  (void)hipGetLastError();  // the result below must be this launch's, not an older call's sticky error
  hipLaunchKernelGGL(hb_reset_check_kernel, dim3((n_env + 255) / 256), dim3(256), 0, stream, counts, terminated, truncated, mask, episode, pending, mode, n_env);
  return hipGetLastError();
}
hipError_t launch_obs(const DevModel& M, const float* state, float* obs, int n_env, hipStream_t stream) {
  (void)hipGetLastError();  // the result below must be this launch's, not an older call's sticky error
  hipLaunchKernelGGL(hb_obs_kernel, dim3((n_env + 255) / 256), dim3(256), 0, stream, M, state, obs, n_env);
  return hipGetLastError();
}
hipError_t launch_action(const float* action, float* prev, float* latest, float* ctrl, int n, hipStream_t stream) {
  (void)hipGetLastError();  // the result below must be this launch's, not an older call's sticky error
  hipLaunchKernelGGL(hb_action_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, action, prev, latest, ctrl, n);
  return hipGetLastError();
}
hipError_t launch_env(const DevModel& M, const EnvArgs& G, hipStream_t stream) {
  (void)hipGetLastError();  // the result below must be this launch's, not an older call's sticky error
  const int per_block = 256 / kEnvLanes;
  hipLaunchKernelGGL(hb_env_kernel, dim3((G.n_env + per_block - 1) / per_block), dim3(256), (size_t)per_block * ((M.nstate + 3) & ~3) * sizeof(float), stream, M, G);
  return hipGetLastError();
}
hipError_t launch_feet_reset(FeetRec* rec, const float* state, int nstate, int n_feet, const uint8_t* mask, int n_env, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(hb_feet_reset_kernel, dim3((n_env + 255) / 256), dim3(256), 0, stream, rec, state, nstate, n_feet, mask, n_env);
  return hipGetLastError();
}
hipError_t launch_command_reset(const EnvCommands& C, float4* cmd, const int* episode, const uint8_t* mask, int n_env, int env_offset, hipStream_t stream) {
  (void)hipGetLastError();
  const int per_block = 256 / kCmdLanes;
  hipLaunchKernelGGL(hb_command_reset_kernel, dim3((n_env + per_block - 1) / per_block), dim3(256), 0, stream, C, cmd, episode, mask, n_env, env_offset);
  return hipGetLastError();
}
hipError_t launch_domain_rand(const DevModel& M, const DomainRand& D, float* dr, int stride, const int* episode, const uint8_t* mask, int n_env, int env_offset,
                              hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(hb_domain_rand_kernel, dim3((n_env + 256 / kDrawLanes - 1) / (256 / kDrawLanes)), dim3(256), 0, stream, M, D, dr, stride, episode, mask, n_env, env_offset);
  return hipGetLastError();
}
}  // namespace hb
