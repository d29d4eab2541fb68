// hb_kin.hip - the whole-body kinematics read-out (hb_kinematics*, include/hb.h): mj_kinematics and mj_objectVelocity of any number of
// states, a pure function of (qpos, qvel) and the model.  A kernel of its own: no solver, no collision and no per-env model parameter
// enters, so every model takes it whatever kernels it steps in, and no step kernel carries anything for it.
#include <hip/hip_runtime.h>
#include "hb_kcommon.hpp"
#include "hb_launch.hpp"

namespace hb {

// floats per body of the velocity block beside the pose block (kXpqStride): omega[3], -, v at xpos[3], - (two 16-byte accesses)
constexpr int kKinVelStride = 8;
// LDS floats of one state: qpos | qvel | poses (kXpqStride) | velocities (kKinVelStride)
__host__ __device__ inline int kin_lds_floats(int nq, int nv, int nb) { return ((nq + 3) & ~3) + ((nv + 3) & ~3) + kXpqStride * nb + kKinVelStride * nb; }

// Lane = body, L lanes per state (the smallest of 16 / 32 / 64 that holds the nbody - 1 moving bodies), 64 / L states per wave: the 27-dof
// humanoid (16 bodies) and the reference's robot (14) run four states per wave instead of leaving 47 lanes empty.  Every sub-group of L
// lanes has an LDS block of its own and executes the same instructions on it as a wave that holds one state: a state's result
// depends neither on L nor on its place in the wave, its neighbours or n (tests/test_gpu_kinematics.py holds that bit for bit).
// mj_kinematics as local_pose() and compose_world() of hb_kinematics.hpp do it, statement for statement (level-ordered records, pointer
// jumping over the 1 / 2 / 4 / 8-up ancestors), with the velocities between their statements; the kernel calls none of the header's
// functions (with ancestor_up and geom_world_pose its time on the 15-body robot left the parent's spread: profiles/kinematics_shared_bench.txt).
// The velocities ride along in the same rounds: a body carries (omega, v of its frame origin) RELATIVE to the ancestor it currently
// refers to, in that ancestor's axes, and composing with the ancestor's own record is
//   omega' = W + Q omega,   v' = V + W x (Q p) + Q v        (P, Q, W, V: the ancestor's record; p: the body's position in it)
// so that after the last round both are world quantities.  No mass enters (mj_comVel refers its cvel to the subtree's centre of mass;
// moved to the same point the two agree).  Nothing of the batch is written; a non-finite input makes that state's own rows garbage
// and nothing else: no index depends on data.
template <int L>
__device__ __forceinline__ void kin_body(const DevModel* Mp, const KinArgs& A) {
  DevModelRef M = *(const DevModel HB_CONST*)(uintptr_t)Mp;
  extern __shared__ float lds[];
  constexpr int kPer = kGroup / L;  // states per wave
  const int sub = (int)threadIdx.x / L, l = (int)threadIdx.x % L;
  const long long s = (long long)blockIdx.x * kPer + sub;
  const bool live = s < A.n;
  const int nq = M.nq, nv = M.nv, nb = M.nbody, ng = M.ngeom;
  float* s_qpos = lds + (size_t)sub * kin_lds_floats(nq, nv, nb);
  float* s_qvel = s_qpos + ((nq + 3) & ~3);
  float* s_xpq = s_qvel + ((nv + 3) & ~3);
  float* s_vel = s_xpq + kXpqStride * nb;
  const bool want_vel = A.body_vel != nullptr;
  for (int i = l; i < nq; i += L) s_qpos[i] = live ? A.qpos[(size_t)s * A.qpos_stride + i] : 0.f;
  for (int i = l; i < nv; i += L) s_qvel[i] = live && want_vel ? A.qvel[(size_t)s * A.qvel_stride + i] : 0.f;
  const bool bl = l + 1 < nb;
  float4 q0 = {0.f, 0.f, 0.f, 0.f}, q1 = q0, bp = q0, bq = q0, bi = q0;
  float4 JA[3], JB[3], JC[3];
#pragma unroll
  for (int jj = 0; jj < 3; jj++) { JA[jj] = q0; JB[jj] = q0; JC[jj] = q0; }
  if (bl) {
    const float4 HB_CONST* R = M.brec + (size_t)(l + 1) * kBrecQuads;
    q0 = R[0]; q1 = R[1]; bp = R[2]; bq = R[3]; bi = R[4];
#pragma unroll
    for (int jj = 0; jj < 3; jj++) { JA[jj] = R[9 + 3 * jj]; JB[jj] = R[10 + 3 * jj]; JC[jj] = R[11 + 3 * jj]; }
  }
  if (l == 0) {  // the world
    reinterpret_cast<float4*>(s_xpq)[0] = {0.f, 0.f, 0.f, 0.f};
    reinterpret_cast<float4*>(s_xpq)[1] = {1.f, 0.f, 0.f, 0.f};
    reinterpret_cast<float4*>(s_vel)[0] = {0.f, 0.f, 0.f, 0.f};
    reinterpret_cast<float4*>(s_vel)[1] = {0.f, 0.f, 0.f, 0.f};
  }
  gsync();
  const int myb = __float_as_int(q0.x), myp = __float_as_int(q0.y), myjn = __float_as_int(q0.z);
  const int myanc2 = (__float_as_int(q1.x) >> 8) & 255, myanc4 = (__float_as_int(q1.x) >> 16) & 255, myanc8 = (__float_as_int(q1.x) >> 24) & 255;
  const bool isfree = bl && myjn == 1 && __float_as_int(JA[0].x) == 0;
  // the body in its parent's frame: pose, and (omega, v of the frame origin) relative to the parent
  V3 posl = {bp.x, bp.y, bp.z};
  Q4 quatl = {bq.x, bq.y, bq.z, bq.w};
  V3 myw = {0.f, 0.f, 0.f}, myv = {0.f, 0.f, 0.f};
  if (isfree) {
    const int qa = __float_as_int(JA[0].y), da = __float_as_int(JA[0].z);
    posl = ld3(s_qpos + qa);
    quatl = qnormalize(ldq(s_qpos + qa + 3));
    myv = ld3(s_qvel + da);                    // (the free joint's linear velocity is in world axes, its angular velocity in the body's)
    myw = qrot(quatl, ld3(s_qvel + da + 3));
  } else if (bl) {
    V3 jw[3], janc[3];
#pragma unroll
    for (int jj = 0; jj < 3; jj++) {
      jw[jj] = {0.f, 0.f, 0.f}; janc[jj] = {0.f, 0.f, 0.f};
      if (jj < myjn) {
        const int qa = __float_as_int(JA[jj].y), da = __float_as_int(JA[jj].z);
        const V3 laxis = {JB[jj].x, JB[jj].y, JB[jj].z}, lpos = {JC[jj].x, JC[jj].y, JC[jj].z};
        const V3 axl = qrot(quatl, laxis);
        const V3 ancl = qrot(quatl, lpos) + posl;
        const float dq = s_qpos[qa] - JA[jj].w;
        const float qd = s_qvel[da];
        if (__float_as_int(JA[jj].x) == 2) { posl = posl + axl * dq; myv = myv + axl * qd; }
        else {
          quatl = qmul(quatl, axisangle(laxis, dq));
          posl = ancl - qrot(quatl, lpos);
          jw[jj] = axl * qd; janc[jj] = ancl;
        }
      }
    }
    // a hinge turns the body about its anchor as mj_kinematics placed it (the joints before it applied, the ones behind it not)
#pragma unroll
    for (int jj = 0; jj < 3; jj++) { myw = myw + jw[jj]; myv = myv + cross(jw[jj], posl - janc[jj]); }
  }
  V3 mypos = posl;
  Q4 myquat = quatl;
  if (bl) {
    reinterpret_cast<float4*>(s_xpq + kXpqStride * myb)[0] = {mypos.x, mypos.y, mypos.z, 0.f};
    reinterpret_cast<float4*>(s_xpq + kXpqStride * myb)[1] = {myquat.w, myquat.x, myquat.y, myquat.z};
    reinterpret_cast<float4*>(s_vel + kKinVelStride * myb)[0] = {myw.x, myw.y, myw.z, 0.f};
    reinterpret_cast<float4*>(s_vel + kKinVelStride * myb)[1] = {myv.x, myv.y, myv.z, 0.f};
  }
  gsync();
  for (int r = 0, span = 1; span < M.nlevel - 1 || r == 0; r++, span <<= 1) {
    const int anc = r == 0 ? myp : (r == 1 ? myanc2 : (r == 2 ? myanc4 : myanc8));
    float4 pp4 = {0.f, 0.f, 0.f, 0.f}, pq4 = {1.f, 0.f, 0.f, 0.f}, pw4 = pp4, pv4 = pp4;
    if (bl) {
      const float4* Pp = reinterpret_cast<const float4*>(s_xpq + kXpqStride * anc);
      const float4* Pv = reinterpret_cast<const float4*>(s_vel + kKinVelStride * anc);
      pp4 = Pp[0]; pq4 = Pp[1]; pw4 = Pv[0]; pv4 = Pv[1];
    }
    gsync();
    if (bl && anc != 0) {
      const Q4 pq = {pq4.x, pq4.y, pq4.z, pq4.w};
      const V3 pw = {pw4.x, pw4.y, pw4.z};
      const V3 rp = qrot(pq, mypos);
      myv = V3{pv4.x, pv4.y, pv4.z} + cross(pw, rp) + qrot(pq, myv);
      myw = pw + qrot(pq, myw);
      mypos = V3{pp4.x, pp4.y, pp4.z} + rp;
      myquat = qnormalize(qmul(pq, myquat));
      reinterpret_cast<float4*>(s_xpq + kXpqStride * myb)[0] = {mypos.x, mypos.y, mypos.z, 0.f};
      reinterpret_cast<float4*>(s_xpq + kXpqStride * myb)[1] = {myquat.w, myquat.x, myquat.y, myquat.z};
      reinterpret_cast<float4*>(s_vel + kKinVelStride * myb)[0] = {myw.x, myw.y, myw.z, 0.f};
      reinterpret_cast<float4*>(s_vel + kKinVelStride * myb)[1] = {myv.x, myv.y, myv.z, 0.f};
    }
    gsync();
  }
  if (!live) return;  // (the tail of a part-filled wave: its lanes ran the rounds on zeros, and write nothing)
  // bodies: xpos | xquat | xipos, and omega | v moved from xpos to xipos
  const V3 ioff = qrot(myquat, V3{bi.x, bi.y, bi.z});
  if (A.body_pose) {
    float* o = A.body_pose + (size_t)s * nb * 10;
    if (l == 0) { st3(o, {0.f, 0.f, 0.f}); stq(o + 3, {1.f, 0.f, 0.f, 0.f}); st3(o + 7, {0.f, 0.f, 0.f}); }
    if (bl) { o += 10 * myb; st3(o, mypos); stq(o + 3, myquat); st3(o + 7, mypos + ioff); }
  }
  if (A.body_vel) {
    float* o = A.body_vel + (size_t)s * nb * 6;
    if (l == 0) { st3(o, {0.f, 0.f, 0.f}); st3(o + 3, {0.f, 0.f, 0.f}); }
    if (bl) { o += 6 * myb; st3(o, myw); st3(o + 3, myv + cross(myw, ioff)); }
  }
  // geoms, in rounds of L: world position (the offset rotated with the body's matrix, as the step kernels do) and orientation
  if (A.geom_pose) {
    float* o = A.geom_pose + (size_t)s * ng * 7;
    for (int g = l; g < ng; g += L) {
      const int b = M.geom_bodyid[g];
      const Q4 bqw = ldq(s_xpq + kXpqStride * b + 4);
      float mat[9];
      q2mat(mat, bqw);
      st3(o + 7 * g, ld3(s_xpq + kXpqStride * b) + mrot(mat, ld3(M.geom_pos + 3 * g)));
      stq(o + 7 * g + 3, qmul(bqw, ldq(M.geom_quat + 4 * g)));
    }
  }
}
__global__ __launch_bounds__(kGroup) void hb_kin16_kernel(const DevModel* Mp, const KinArgs A) { kin_body<16>(Mp, A); }
__global__ __launch_bounds__(kGroup) void hb_kin32_kernel(const DevModel* Mp, const KinArgs A) { kin_body<32>(Mp, A); }
__global__ __launch_bounds__(kGroup) void hb_kin64_kernel(const DevModel* Mp, const KinArgs A) { kin_body<64>(Mp, A); }

hipError_t launch_kinematics(const DevModel* M_dev, const DevModel& M, const KinArgs& A, int pack, hipStream_t stream, const char** kernel) {
  static const PackedKernel<KinArgs> triple[3] = {{hb_kin16_kernel, "hb_kin16_kernel"}, {hb_kin32_kernel, "hb_kin32_kernel"}, {hb_kin64_kernel, "hb_kin64_kernel"}};
  return launch_packed(triple, M_dev, M, A, pack, kin_lds_floats(M.nq, M.nv, M.nbody), stream, kernel);
}

}  // namespace hb
