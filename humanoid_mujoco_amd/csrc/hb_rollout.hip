// hb_rollout.hip - what the open-loop rollouts and the launch plumbing need besides the step kernels: the MJPC task costs, the spline
// tape, the benchmark controls, the heavy-first dispatch order and the queue probe - and their launchers.
#include <hip/hip_runtime.h>
#include "hb_kcommon.hpp"
#include "hb_launch.hpp"

namespace hb {

// ---- MJPC task cost on the recorded read-out rows --------------------------------------------------------------
// mjpc::Norm (mujoco_mpc/mjpc/norm.cc:50-208), value only
__device__ __forceinline__ float mjpc_norm(int type, const float* x, int n, float p, float q) {
  float y = 0.f;
  switch (type) {
    case 0: for (int i = 0; i < n; i++) y += x[i] * x[i]; return 0.5f * y;                                   // kQuadratic
    case 1: { float c = 0.f; for (int i = 0; i < n; i++) c += x[i] * x[i]; return powf(powf(c, 0.5f * q) + powf(p, q), 1.f / q) - p; }  // kL22
    case 2: { float c = 0.f; for (int i = 0; i < n; i++) c += x[i] * x[i]; return sqrtf(c + p * p) - p; }  // kL2
    case 3: for (int i = 0; i < n; i++) y += p * p * (coshf(x[i] / p) - 1.f); return y;                      // kCosh
    case 5: for (int i = 0; i < n; i++) y += powf(fabsf(x[i]), p); return y;                                   // kPowerLoss
    case 6: for (int i = 0; i < n; i++) y += sqrtf(x[i] * x[i] + p * p) - p; return y;                         // kSmoothAbsLoss
    case 7: for (int i = 0; i < n; i++) y += powf(powf(fabsf(x[i]), q) + powf(p, q), 1.f / q) - p; return y;  // kSmoothAbs2Loss
    case 8: for (int i = 0; i < n; i++) y += p > 0.f ? p * logf(1.f + expf(x[i] / p)) : fmaxf(x[i], 0.f); return y;  // kRectifyLoss
    default: return x[0];                                                                                       // kNull
  }
}

// BaseResidualFn::CostTerms + CostValue (mujoco_mpc/mjpc/task.cc:71-110): term k = weight[k] * Norm(norm[k]) of the next dim[k] residual
// entries; the sum goes through the risk transformation (risk-neutral below kRiskNeutralTolerance = 1e-6).  `terms` nullable.
__device__ __forceinline__ float mjpc_risk(float risk, float c) { return fabsf(risk) >= 1e-6f ? (expf(risk * c) - 1.f) / risk : c; }
__device__ __forceinline__ float mjpc_cost_value(int nterm, const int* dim, const int* norm, const float* weight, const float* p, const float* q, float risk,
                                                 const float* res, float* terms) {
  float cost = 0.f;
  int sh = 0;
  for (int k = 0; k < nterm; k++) {
    const float tk = weight[k] * mjpc_norm(norm[k], res + sh, dim[k], p[k], q[k]);
    if (terms) terms[k] = tk;
    cost += tk;
    sh += dim[k];
  }
  return mjpc_risk(risk, cost);
}

// hb_task_cost: the same cost evaluation for n caller-supplied residual vectors (one thread each)
__global__ void hb_cost_terms_kernel(const float* residual, int n, int nres, const CostSpec K, float* terms, float* cost) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  cost[e] = mjpc_cost_value(K.nterm, K.dim, K.norm, K.weight, K.p, K.q, K.risk, residual + (size_t)e * nres, terms ? terms + (size_t)e * K.nterm : nullptr);
}

// One thread per candidate: Stand::ResidualFn::Residual (tasks/humanoid/stand/stand.cc:41-104) on each of the H rows,
// BaseResidualFn::CostValue (task.cc:71-110), Trajectory::UpdateReturn (trajectory.cc:312-326); a candidate that raised
// a bad-state warning returns kMaxReturnValue (trajectory.cc:29,169-173)
__global__ void hb_stand_cost_kernel(const float* rows, int H, int n_env, const StandTask K, const int* status, float* total, float* costs) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_env) return;
  float sum = 0.f;
  for (int t = 0; t < H; t++) {
    const float* r = rows + ((size_t)t * n_env + e) * K.stride;
    float fz = 0.f, fx = 0.f, fy = 0.f;
    for (int k = 0; k < K.n_feet; k++) { fx += r[K.o_feet + 3 * k]; fy += r[K.o_feet + 3 * k + 1]; fz += r[K.o_feet + 3 * k + 2]; }
    const float inv = 1.f / (float)K.n_feet;
    const float height = r[K.o_head + 2] - fz * inv - K.height_goal;
    const float kFallTime = 0.2f;
    const float dx = fx * inv - (r[K.o_com] + kFallTime * r[K.o_vel]), dy = fy * inv - (r[K.o_com + 1] + kFallTime * r[K.o_vel + 1]);
    const float balance = sqrtf(dx * dx + dy * dy);
    float c = K.weight[0] * mjpc_norm(K.norm[0], &height, 1, K.p[0], K.q[0]);
    c += K.weight[1] * mjpc_norm(K.norm[1], &balance, 1, K.p[1], K.q[1]);
    c += K.weight[2] * mjpc_norm(K.norm[2], r + K.o_vel, 2, K.p[2], K.q[2]);
    c += K.weight[3] * mjpc_norm(K.norm[3], r + K.o_qvel + 6, K.nv - 6, K.p[3], K.q[3]);
    c += K.weight[4] * mjpc_norm(K.norm[4], r + K.o_ctrl, K.nu, K.p[4], K.q[4]);
    c = mjpc_risk(K.risk, c);
    if (costs) costs[(size_t)t * n_env + e] = c;
    sum += c;
  }
  const bool failed = status[e] & ((1 << 4) | (1 << 5) | (1 << 6));
  total[e] = failed ? 1.0e6f : sum / (float)max(H, 1);
}

// Walk::ResidualFn::Residual (tasks/humanoid/walk/walk.cc:44-163) on each of the H rows, then the cost terms in the
// order and with the dimensions the task's user sensors declare (task.cc:71-89), return as in hb_stand_cost_kernel
__global__ void hb_walk_cost_kernel(const float* rows, int H, int n_env, const WalkTask K, const int* status, float* total, float* costs) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_env) return;
  float sum = 0.f;
  for (int t = 0; t < H; t++) {
    const float* r = rows + ((size_t)t * n_env + e) * K.stride;
    float res[96];
    int c = 0;
    const float torso_height = r[K.o_torso + 2];
    res[c++] = torso_height - K.height_goal;
    const float* fr = r + K.o_foot_r;
    const float* fl = r + K.o_foot_l;
    res[c++] = 0.5f * (fl[2] + fr[2]) - r[K.o_pelvis + 2] - 0.2f;
    // balance: capture point against its projection onto the segment between the feet
    float cp[3] = {r[K.o_com] + 0.3f * r[K.o_vel], r[K.o_com + 1] + 0.3f * r[K.o_vel + 1], 1.0e-3f};
    float axis[3] = {fr[0] - fl[0], fr[1] - fl[1], 1.0e-3f};
    float an = sqrtf(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    if (an < 1e-15f) { axis[0] = 1.f; axis[1] = 0.f; axis[2] = 0.f; } else { axis[0] /= an; axis[1] /= an; axis[2] /= an; }  // mju_normalize3
    const float length = 0.5f * an - 0.05f;
    const float center[3] = {0.5f * (fr[0] + fl[0]), 0.5f * (fr[1] + fl[1]), 0.5f * (fr[2] + fl[2])};
    const float vec[3] = {cp[0] - center[0], cp[1] - center[1], cp[2] - center[2]};
    float tt = vec[0] * axis[0] + vec[1] * axis[1] + vec[2] * axis[2];
    tt = fmaxf(-length, fminf(length, tt));
    const float pcp[2] = {axis[0] * tt + center[0], axis[1] * tt + center[1]};
    const float standing = torso_height / sqrtf(torso_height * torso_height + 0.45f * 0.45f) - 0.4f;
    res[c++] = standing * (cp[0] - pcp[0]);
    res[c++] = standing * (cp[1] - pcp[1]);
    // upright: axes are [torso_up, pelvis_up, foot_right_up, foot_left_up, torso_forward, pelvis_forward, foot_right_forward, foot_left_forward]
    const float* ax = r + K.o_axes;
    res[c++] = ax[2] - 1.f;
    res[c++] = 0.3f * (ax[3 + 2] - 1.f);
    for (int f = 0; f < 2; f++) {
      const float* up = ax + 3 * (2 + f);
      res[c++] = 0.1f * standing * up[0]; res[c++] = 0.1f * standing * up[1]; res[c++] = 0.1f * standing * (up[2] - 1.f);
    }
    // posture
    for (int i = 7; i < K.nq; i++) res[c++] = r[K.o_qpos + i];
    // walk
    float fw[2] = {0.f, 0.f};
    for (int k = 4; k < 8; k++) { fw[0] += ax[3 * k]; fw[1] += ax[3 * k + 1]; }
    const float fn = sqrtf(fw[0] * fw[0] + fw[1] * fw[1]);
    if (fn < 1e-15f) { fw[0] = 1.f; fw[1] = 0.f; } else { fw[0] /= fn; fw[1] /= fn; }  // mju_normalize
    const float* tv = r + K.o_linvel;  // torso, foot_right, foot_left
    const float cv[2] = {0.5f * (r[K.o_sub] + tv[0]), 0.5f * (r[K.o_sub + 1] + tv[1])};
    res[c++] = standing * (cv[0] * fw[0] + cv[1] * fw[1] - K.speed_goal);
    // move feet
    res[c++] = standing * (cv[0] - 0.5f * tv[3] - 0.5f * tv[6]);
    res[c++] = standing * (cv[1] - 0.5f * tv[4] - 0.5f * tv[7]);
    // control
    for (int i = 0; i < K.nu; i++) res[c++] = r[K.o_ctrl + i];
    const float cost = mjpc_cost_value(K.nterm, K.dim, K.norm, K.weight, K.p, K.q, K.risk, res, nullptr);
    if (costs) costs[(size_t)t * n_env + e] = cost;
    sum += cost;
  }
  const bool failed = status[e] & ((1 << 4) | (1 << 5) | (1 << 6));
  total[e] = failed ? 1.0e6f : sum / (float)max(H, 1);
}

// ---- SamplingPolicy::Action on the device (mujoco_mpc/mjpc/planners/sampling/policy.cc:50-58): every candidate's
// time spline (mjpc/spline/spline.cc:103-156,240-277: zero-order / linear / cubic Hermite with finite-difference slopes)
// sampled at time0 + t * dt and clamped to ctrlrange, written as the action tape [T][n_env][nu] the rollouts read.
// knots: [n_env][P][nu]; times: [P], increasing, shared by the candidates.
__global__ void hb_spline_tape_kernel(const DevModel M, const float* knots, const float* times, int P, int interp, float time0, float dt, int T, int n_env, float* tape) {
  const int nu = M.nu;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)T * n_env * nu;
  if (idx >= total) return;
  const int i = (int)(idx % nu), e = (int)((idx / nu) % n_env), t = (int)(idx / ((size_t)nu * n_env));
  const float time = time0 + (float)t * dt;
  const float* y = knots + (size_t)e * P * nu + i;  // y[k * nu]: node k
  float v;
  int up = 0;
  while (up < P && times[up] <= time) up++;  // std::upper_bound
  if (P == 0) v = 0.f;
  else if (up == P) v = y[(size_t)(P - 1) * nu];
  else if (up == 0) v = y[0];
  else {
    const int lo = up - 1;
    const float t0 = times[lo], t1 = times[up], x = (time - t0) / (t1 - t0);
    const float p0 = y[(size_t)lo * nu], p1 = y[(size_t)up * nu];
    if (interp == 0) v = p0;
    else if (interp == 1) v = p0 * (1.f - x) + p1 * x;
    else {
      // TimeSpline::Slope: one-sided at the ends, mean of the two one-sided differences inside
      auto slope = [&](int k) {
        if (k == 0) return (y[(size_t)1 * nu] - y[0]) / (times[1] - times[0]);
        const float back = (y[(size_t)k * nu] - y[(size_t)(k - 1) * nu]) / (times[k] - times[k - 1]);
        if (k == P - 1) return back;
        return 0.5f * (y[(size_t)(k + 1) * nu] - y[(size_t)k * nu]) / (times[k + 1] - times[k]) + 0.5f * back;
      };
      const float h = t1 - t0, x2 = x * x, x3 = x2 * x;
      v = (2.f * x3 - 3.f * x2 + 1.f) * p0 + (x3 - 2.f * x2 + x) * h * slope(lo) + (-2.f * x3 + 3.f * x2) * p1 + (x3 - x2) * h * slope(up);
    }
  }
  // Clamp(action, actuator_ctrlrange, nu) (utilities.cc:94-98); an actuator without a control range is left alone
  const float lo_r = M.act_ctrlrange[2 * i], hi_r = M.act_ctrlrange[2 * i + 1];
  if (M.act_ctrllimited[i] || lo_r < hi_r) v = fminf(fmaxf(v, lo_r), hi_r);
  tape[idx] = v;
}

// Probe for hb_batch_pipeline: one wave that idles for `ticks` of the 100 MHz wall clock (bounded by the sleep count as well) and
// records when it began and ended.  Two of these on two streams overlap in time exactly when the streams own different hardware queues.
__global__ __launch_bounds__(64) void hb_probe_spin_kernel(unsigned long long* out, unsigned ticks) {
  const unsigned long long t0 = wall_clock64();
  unsigned long long t = t0;
  for (int guard = 0; guard < 2048 && t - t0 < ticks; guard++) {
    __builtin_amdgcn_s_sleep(64);
    t = wall_clock64();
  }
  if (threadIdx.x == 0) { out[0] = t0; out[1] = t; }
}
// Heavy-first dispatch order for the next launch: counting sort of the envs by the cost proxy of their
// last step (constraint rows x solver sweeps, counts[4e+3]), most expensive first (LPT scheduling of
// the 4096 blocks over the resident slots).  One block; the order inside a cost bin is arbitrary,
// which cannot change results (envs are independent).
__global__ __launch_bounds__(1024) void hb_order_kernel(const int* counts, int* order, int* keys, int e0, int n, int slot, int shift) {
  // sorts envs e0 .. e0+n-1 into order[e0 .. e0+n-1], most expensive first; cost = counts[env][slot] >> shift, 256 bins
  __shared__ int hist[256];
  __shared__ int base[256];
  const int tid = threadIdx.x;
  if (tid < 256) hist[tid] = 0;
  __syncthreads();
  for (int e = e0 + tid; e < e0 + n; e += blockDim.x) {
    int key = min(255, counts[kCountStride * e + slot] >> shift);
    keys[e] = key;  // read ONCE: the slow lane of two-lane stepping may be writing counts beside this kernel, and a key that changed
                    // between the two passes would leave an env out of the permutation
    atomicAdd(&hist[255 - key], 1);  // bin 0 = most expensive
  }
  __syncthreads();
  // exclusive prefix sum of the 256 bins (Hillis-Steele on 256 threads: 8 rounds instead of a 256-step serial loop
  // on one thread, which was most of this kernel's 9 us on the critical path of every fourth step)
  if (tid < 256) base[tid] = hist[tid];
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    int v = 0;
    if (tid < 256 && tid >= o) v = base[tid - o];
    __syncthreads();
    if (tid < 256) base[tid] += v;
    __syncthreads();
  }
  if (tid < 256) base[tid] += e0 - hist[tid];  // inclusive -> exclusive, offset by the segment start
  __syncthreads();
  for (int e = e0 + tid; e < e0 + n; e += blockDim.x) {
    const int key = keys[e];
    order[atomicAdd(&base[255 - key], 1)] = e;
  }
}

// benchmark controls: ctrl[t][e][i] = 2*H(1+t0+t+1000*(env_offset+e), i+2) - 1  (testspeed.cc:64-80)
__global__ void hb_halton_ctrl_kernel(float* out, int T, int n_env, int nu, int t0, int env_offset) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)T * n_env * nu;
  if (idx >= total) return;
  int i = (int)(idx % nu);
  size_t r = idx / nu;
  int e = (int)(r % n_env), t = (int)(r / n_env);
  out[idx] = 2.f * halton(1 + t0 + t + 1000 * (env_offset + e), i + 2) - 1.f;
}

hipError_t launch_probe_spin(unsigned long long* out, unsigned ticks, hipStream_t stream) {
  hipLaunchKernelGGL(hb_probe_spin_kernel, dim3(1), dim3(64), 0, stream, out, ticks);
  return hipGetLastError();
}
hipError_t launch_order(const int* counts, int* order, int n_env, int e0, int n, hipStream_t stream, int slot, int shift) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(hb_order_kernel, dim3(1), dim3(1024), 0, stream, counts, order, order + n_env, e0, n, slot, shift);
  return hipGetLastError();
}
hipError_t launch_halton_ctrl(float* out, int T, int n_env, int nu, int t0, int env_offset, hipStream_t stream) {
  size_t total = (size_t)T * n_env * nu;
  (void)hipGetLastError();  // the result below must be this launch's, not an older call's sticky error
  hipLaunchKernelGGL(hb_halton_ctrl_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, out, T, n_env, nu, t0, env_offset);
  return hipGetLastError();
}
hipError_t launch_stand_cost(const float* rows, int H, int n_env, const StandTask& K, const int* status, float* total, float* costs, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(hb_stand_cost_kernel, dim3((n_env + 127) / 128), dim3(128), 0, stream, rows, H, n_env, K, status, total, costs);
  return hipGetLastError();
}
hipError_t launch_walk_cost(const float* rows, int H, int n_env, const WalkTask& K, const int* status, float* total, float* costs, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(hb_walk_cost_kernel, dim3((n_env + 63) / 64), dim3(64), 0, stream, rows, H, n_env, K, status, total, costs);
  return hipGetLastError();
}
hipError_t launch_cost_terms(const float* residual, int n, int nres, const CostSpec& K, float* terms, float* cost, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(hb_cost_terms_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, residual, n, nres, K, terms, cost);
  return hipGetLastError();
}
hipError_t launch_spline_tape(const DevModel& M, const float* knots, const float* times, int P, int interp, float time0, float dt, int T, int n_env, float* tape, hipStream_t stream) {
  (void)hipGetLastError();
  const size_t total = (size_t)T * n_env * M.nu;
  hipLaunchKernelGGL(hb_spline_tape_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, M, knots, times, P, interp, time0, dt, T, n_env, tape);
  return hipGetLastError();
}
}  // namespace hb
