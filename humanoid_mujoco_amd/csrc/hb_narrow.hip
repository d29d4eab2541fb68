// hb_narrow.hip - the staged step of the general variants: hb_pose_kernel (poses, broadphase, work items) and the narrowphase kernels
// (one work item per lane).  See hb_step.hip for the step kernels that gather their results.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#ifdef HB_STAMPS
// diagnostic build only (tools/gpu_narrow_limits.sh): HB_MPR_LIMIT="a,b" in the environment cuts every portal search off after a support
// calls and every hull climb after b rounds - WRONG contacts, but the launch durations say where the narrowphase's time goes
#define HB_NARROW_DIAG 1
namespace hb { __device__ int g_mpr_limit[2] = {1 << 30, 1 << 30}; }
#endif
#include "hb_kinematics.hpp"
#include "hb_collide.hpp"
#include "hb_launch.hpp"

namespace hb {

// ---- staged step of the general variants: poses + work lists, then the narrowphase, each in a kernel of its own ------------------
// hb_pose_kernel: one wave per env.  The state checks of step_body and the same mj_kinematics (hb_kinematics.hpp; the step kernel
// repeats them: a pose costs less to recompute than to hand over), the geoms' world poses, broadphase and work items.
#define HB_POSE_BOX 0
#include "hb_pose_kernel.inl"
#undef HB_POSE_BOX
#define HB_POSE_BOX 1
#include "hb_pose_kernel.inl"
#undef HB_POSE_BOX
#define HB_POSE_BOX 2
#include "hb_pose_kernel.inl"
#undef HB_POSE_BOX

// hb_narrow_kernel: the portal searches, one wave per env (and per 64 of its searches): lane l runs the env's l-th search, prisms
// first, exactly as the fused step kernel would (eval_work_item).  The waves are mostly empty (an env has about nine searches), but
// there are as many of them as the chip holds at once; packing the searches of all envs densely into waves (a prefix sum over the
// per-env counts, 64 / 16 / 4 searches per wave, one kernel per kind of search) measured slower: a wave's time is set by its
// longest search and the divergence between its lanes, not by how many lanes it has.  Round 4 tried it again on top of the
// four-lane searches and the one-loop portal search (a flat list filled by one atomicAdd per env in hb_pose_kernel, sixteen consecutive
// searches per wave): the narrowphase launch stayed at 85 us - it lasts as long as its longest search, 170-190 k cycles - and the 4096
// atomics on one counter cost the pose kernel 23 us.
// A model with meshes (MESH = 1): FOUR lanes per search (hb_mpr.hpp: climb4 - the four share the rounds of a hull climb), sixteen searches per
// wave; without meshes a lane per search.  Where that came from: the diagnostic build's HB_MPR_LIMIT (tools/gpu_narrow_limits.sh,
// profiles/r04_narrow_limits.txt) showed the launch VALU-bound at 4.6 active lanes, 10 us per support call allowed, 8 of them the climb.
// PAIR = 1: TWO envs per wave (lanes 0..31: one env's searches, 32..63: the other's).  Half the waves, each a little longer: the unpipelined
// step of 4096 robots 267 -> 233 us with one lane per search (profiles/r04_narrow_pairs.txt), and with four lanes per search the launch is
// 84 us in this form (profiles/r04_team_counters.json: 11.7 active lanes per vector instruction).  The launch then is ONE round of waves and
// lasts as long as its slowest; for pipelined segments the two forms measure the same (169 us per step of 4096 robots), and
// launch_pose_narrow takes the pair form for a launch that covers its whole batch.
template <int MESH, int PAIR = 0, int BOX = 0>
__device__ __forceinline__ void narrow_body(const DevModel* Mp, const BatchPtrs& P) {
  DevModelRef M = *(const DevModel HB_CONST*)(uintptr_t)Mp;
  const int lane = threadIdx.x;
  // heavy first (BatchPtrs::order2: the envs of this launch sorted by the time their wave took in an earlier step): the launch ends
  // when its slowest wave does, and a slow wave that starts in the last round ends late
  constexpr int G = MESH ? 4 : 1;  // lanes per search
  constexpr int kPer = (PAIR ? 32 : kGroup) / G;  // searches of an env per chunk
  const int nslot = PAIR ? (P.nblk + 1) >> 1 : P.nblk;
  const int nwaves = (int)gridDim.x / nslot;  // waves per slot: wave c takes chunks c, c + nwaves, ... of its env(s)
  const int pr = (int)blockIdx.x % nslot;
  const int half = PAIR ? lane >> 5 : 0, l = PAIR ? lane & 31 : lane;
  const int slot = P.blk0 + (PAIR ? 2 * pr + half : pr);
  const bool live = !PAIR || 2 * pr + half < P.nblk;
  const int env = live ? (P.order2 ? P.order2[slot] : slot) : 0;
  const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
  const int n1 = live ? P.stage.nsearch[2 * env] : 0, n2 = live ? P.stage.nsearch[2 * env + 1] : 0;
  const bool first = (int)blockIdx.x / nslot == 0;
  if (first && l == 0 && live) P.counts[kCountStride * (size_t)env + 7] = 0;
  const int ng = M.ngeom;
  const DomainLayout DL = domain_layout(M.nbody, M.nv, M.nlimcand, M.nu, M.nhfielddata);
  const float* g = P.stage.geom + (size_t)env * ng * 10;
  const float* hdata = P.dr ? P.dr + (size_t)env * P.dr_stride + DL.o_hfield : (const float*)M.hfield_data;
  auto run_chunk = [&](int chunk) {
    const int j = chunk * kPer + l / G;
    const bool have = j < n1 + n2;
    int4 it = {env, 0, 1 << 16, 0};
    if (have) it = P.stage.item[(size_t)env * kWorkMax + (j < n1 ? j : kWorkMax - 1 - (j - n1))];
    const int p = it.y & 0xffff, w = it.y >> 16;
    ConOut co0, co1;
    int n;
    V3 hint;
    eval_work_item<2, MESH, G, BOX>(M, hdata, have, p, it.z & 0xffff, it.w & 0xffff, it.w >> 16, it.z >> 16, 0.f, g, g + 3 * ng, g + 6 * ng, co0, co1, n, hint);
    if (have && (l & (G - 1)) == 0) {
      float4* R = P.stage.result + ((size_t)env * kWorkMax + w) * 4;
      R[0] = {co0.dist, co0.pos.x, co0.pos.y, co0.pos.z};
      R[1] = {co0.n.x, co0.n.y, co0.n.z, __int_as_float(n)};
      R[2] = {co1.dist, co1.pos.x, co1.pos.y, co1.pos.z};
      R[3] = {co1.n.x, co1.n.y, co1.n.z, __int_as_float(p)};
    }
  };
  if constexpr (G == 1) {  // (a wave per chunk: launch_pose_narrow; a loop here costs the kernel without the hull climb 50 more spilled registers)
    if (__any((int)blockIdx.x / nslot * kPer < n1 + n2)) run_chunk((int)blockIdx.x / nslot);
  } else {
    for (int chunk = (int)blockIdx.x / nslot; __any(chunk * kPer < n1 + n2); chunk += nwaves) run_chunk(chunk);
  }
  // (the cost the heavy-first order of the next launches sorts by: the time of the env's - first - wave)
  if (first && l == 0 && live) P.counts[kCountStride * (size_t)env + 7] = (int)min(255ull, (__builtin_amdgcn_s_memtime() - t_begin) >> 10);
}
__global__ __launch_bounds__(kGroup, 2) void hb_narrow_kernel(const DevModel* Mp, const BatchPtrs P) { narrow_body<1>(Mp, P); }
// a model without mesh geoms (configs[4]: capsules and spheres over the height field's prisms): no hull climb in the kernel
__global__ __launch_bounds__(kGroup, 2) void hb_narrow_prim_kernel(const DevModel* Mp, const BatchPtrs P) { narrow_body<0>(Mp, P); }
// two envs per wave (narrow_body's PAIR): the unpipelined launches
__global__ __launch_bounds__(kGroup, 2) void hb_narrow2_kernel(const DevModel* Mp, const BatchPtrs P) { narrow_body<1, 1>(Mp, P); }
__global__ __launch_bounds__(kGroup, 2) void hb_narrow2_prim_kernel(const DevModel* Mp, const BatchPtrs P) { narrow_body<0, 1>(Mp, P); }
// the same four for a model with box geoms (StageBufs::has_box): the portal search with the box's closed-form support point; without
// meshes (the "prim" pair) a search is capsule - box, box - box or a prism against a box, a lane each
__global__ __launch_bounds__(kGroup, 2) void hb_narrow_box_kernel(const DevModel* Mp, const BatchPtrs P) { narrow_body<1, 0, 1>(Mp, P); }
__global__ __launch_bounds__(kGroup, 2) void hb_narrow_prim_box_kernel(const DevModel* Mp, const BatchPtrs P) { narrow_body<0, 0, 1>(Mp, P); }
__global__ __launch_bounds__(kGroup, 2) void hb_narrow2_box_kernel(const DevModel* Mp, const BatchPtrs P) { narrow_body<1, 1, 1>(Mp, P); }
__global__ __launch_bounds__(kGroup, 2) void hb_narrow2_prim_box_kernel(const DevModel* Mp, const BatchPtrs P) { narrow_body<0, 1, 1>(Mp, P); }

hipError_t launch_pose_narrow(const DevModel* M_dev, const BatchPtrs& Q, hipStream_t stream) {
  (void)hipGetLastError();
#ifdef HB_NARROW_DIAG
  static const bool limits_set = [] {
    if (const char* e = getenv("HB_MPR_LIMIT")) {
      int v[2] = {1 << 30, 1 << 30};
      sscanf(e, "%d,%d", &v[0], &v[1]);
      (void)hipMemcpyToSymbol(HIP_SYMBOL(g_mpr_limit), v, sizeof v);
    }
    return true;
  }();
  (void)limits_set;
#endif
  const bool box = Q.stage.has_box != 0;
  // (has_box 2: the box - box manifold - its pairs are evaluated in the pose kernel and never searched: the narrowphase kernels are the box ones)
  hipLaunchKernelGGL(Q.stage.has_box == 2 ? hb_pose_boxm_kernel : box ? hb_pose_box_kernel : hb_pose_kernel, dim3(Q.nblk), dim3(kGroup), (size_t)Q.stage.pose_lds, stream, M_dev, Q);
  const bool pairs = Q.nblk == Q.n_env && Q.n_env >= 512;  // a launch that covers its whole batch: nothing overlaps its tail anyway
  if (pairs) {
    // (waves per pair of envs: a wave without searches left ends at once.  Meshes: four lanes per search, two waves hold sixteen searches per env -
    // the reference's robot has at most eleven - and loop for more; without meshes a lane per search, a wave per 32 searches of each env)
    const int slots = (Q.nblk + 1) / 2;
    if (Q.stage.no_mesh) hipLaunchKernelGGL(box ? hb_narrow2_prim_box_kernel : hb_narrow2_prim_kernel, dim3(slots * (kWorkMax / 32)), dim3(kGroup), 0, stream, M_dev, Q);
    else hipLaunchKernelGGL(box ? hb_narrow2_box_kernel : hb_narrow2_kernel, dim3(slots * 2), dim3(kGroup), 0, stream, M_dev, Q);
  } else if (Q.stage.no_mesh) hipLaunchKernelGGL(box ? hb_narrow_prim_box_kernel : hb_narrow_prim_kernel, dim3(Q.nblk * (kWorkMax / kGroup)), dim3(kGroup), 0, stream, M_dev, Q);
  else hipLaunchKernelGGL(box ? hb_narrow_box_kernel : hb_narrow_kernel, dim3(Q.nblk * 2), dim3(kGroup), 0, stream, M_dev, Q);
  return hipGetLastError();
}

}  // namespace hb
