// hb_kinematics.hpp - the parts of mj_kinematics that the kernels computing body poses share (step_body, step_duo, hb_pose_kernel,
// dyn_body), so that the poses of a state are the same bits wherever they are computed: a staged step equals a fused one, the duo kernel the
// one-env kernel, and the read-outs the step.  Each kernel loads and decodes its own body record (DevModel::brec) and passes what a
// function needs; everything is __forceinline__ and written per lane.  kin_body interleaves its velocities with these statements and
// calls none of them (profiles/kinematics_shared_bench.txt).
#pragma once
#include "hb_kcommon.hpp"

namespace hb {

// the ancestor 2^r links up of a body, of its ancestors 1 / 2 / 4 / 8 up (the world is every short chain's fixed point): round r of a
// pointer-jumping pass refers to it
__device__ __forceinline__ int ancestor_up(int r, int up1, int up2, int up4, int up8) { return r == 0 ? up1 : (r == 1 ? up2 : (r == 2 ? up4 : up8)); }

// The pose of a body relative to its parent (body frame bp, bq, then its jntnum joints in order; JA, JB, JC: the record's joint quads (type,
// qposadr, dofadr, qpos0) (axis) (pos)) does not depend on the parent's world pose, so all of it - the sin/cos of every joint included - is
// done for every body at once; the rounds that follow only compose ancestor and local pose (mj_kinematics does the same products in world
// coordinates, body by body).  Out: posl, quatl, and the joint axes and anchors in the parent's frame (a hinge's anchor: the joints before
// it applied, the ones behind it not).
__device__ __forceinline__ void local_pose(bool bl, bool isfree, int jntnum, float4 bp, float4 bq, const float4 (&JA)[3], const float4 (&JB)[3], const float4 (&JC)[3],
                                           const float* s_qpos, V3& posl, Q4& quatl, V3 (&axl)[3], V3 (&ancl)[3]) {
  posl = {bp.x, bp.y, bp.z};
  quatl = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
  for (int jj = 0; jj < 3; jj++) { axl[jj] = {0.f, 0.f, 0.f}; ancl[jj] = {0.f, 0.f, 0.f}; }
  if (isfree) {
    const int qa = __float_as_int(JA[0].y);
    posl = ld3(s_qpos + qa);
    quatl = qnormalize(ldq(s_qpos + qa + 3));
  } else if (bl) {
#pragma unroll
    for (int jj = 0; jj < 3; jj++) {
      if (jj < jntnum) {
        const int qa = __float_as_int(JA[jj].y);
        const V3 laxis = {JB[jj].x, JB[jj].y, JB[jj].z}, lpos = {JC[jj].x, JC[jj].y, JC[jj].z};
        axl[jj] = qrot(quatl, laxis);
        ancl[jj] = qrot(quatl, lpos) + posl;
        const float dq = s_qpos[qa] - JA[jj].w;
        if (__float_as_int(JA[jj].x) == 2) posl = posl + axl[jj] * dq;
        else {
          quatl = qmul(quatl, axisangle(laxis, dq));
          posl = ancl[jj] - qrot(quatl, lpos);
        }
      }
    }
  }
}

// World poses by pointer jumping: every body (b, in the lanes with bl) starts with its pose relative to its parent (in: pos, quat) and, in
// round r, composes it with the (partially composed) pose of its ancestor 2^r links up; after ceil(log2(depth)) rounds it is the world
// pose (out: pos, quat, and s_xpq of every body).  The world's record holds the identity (the caller's store, a gsync before this).
// (mj_kinematics composes the same transforms root to leaf; the association differs, the product does not.)
__device__ __forceinline__ void compose_world(bool bl, int b, int up1, int up2, int up4, int up8, int nlevel, float* s_xpq, V3& pos, Q4& quat) {
  if (bl) {
    reinterpret_cast<float4*>(s_xpq + kXpqStride * b)[0] = {pos.x, pos.y, pos.z, 0.f};
    reinterpret_cast<float4*>(s_xpq + kXpqStride * b)[1] = {quat.w, quat.x, quat.y, quat.z};
  }
  gsync();
  for (int r = 0, span = 1; span < nlevel - 1 || r == 0; r++, span <<= 1) {
    const int anc = ancestor_up(r, up1, up2, up4, up8);
    float4 pp4 = {0.f, 0.f, 0.f, 0.f}, pq4 = {1.f, 0.f, 0.f, 0.f};
    if (bl) { const float4* Pp = reinterpret_cast<const float4*>(s_xpq + kXpqStride * anc); pp4 = Pp[0]; pq4 = Pp[1]; }
    gsync();  // every lane has read its ancestor before anyone overwrites a pose
    if (bl && anc != 0) {
      const Q4 pq = {pq4.x, pq4.y, pq4.z, pq4.w};
      pos = V3{pp4.x, pp4.y, pp4.z} + qrot(pq, pos);
      quat = qnormalize(qmul(pq, quat));
      reinterpret_cast<float4*>(s_xpq + kXpqStride * b)[0] = {pos.x, pos.y, pos.z, 0.f};
      reinterpret_cast<float4*>(s_xpq + kXpqStride * b)[1] = {quat.w, quat.x, quat.y, quat.z};
    }
    gsync();
  }
}

// Everything that hangs off the world poses in the step kernels, all bodies at once (the lanes that hold one): the joints' world axes and
// anchors (xaxis, xanchor; a free joint: the body's origin and the record's axis jaxis0), the body's matrix and the world position ipos of
// its centre of mass.
__device__ __forceinline__ void store_world_frames(bool isfree, int b, int parent, int jntnum, int jntadr, float4 jaxis0, const V3 (&axl)[3], const V3 (&ancl)[3], float4 ipos,
                                                   V3 pos, Q4 quat, const float* s_xpq, float* s_xaxis, float* s_xanchor, float* s_xmat, float* s_xipos) {
  if (isfree) {
    st3(s_xanchor + 3 * jntadr, pos);
    st3(s_xaxis + 3 * jntadr, {jaxis0.x, jaxis0.y, jaxis0.z});
  } else {
    const Q4 pq = ldq(s_xpq + kXpqStride * parent + 4);
    const V3 pp = ld3(s_xpq + kXpqStride * parent);
#pragma unroll
    for (int jj = 0; jj < 3; jj++) {
      if (jj < jntnum) {
        st3(s_xaxis + 3 * (jntadr + jj), qrot(pq, axl[jj]));
        st3(s_xanchor + 3 * (jntadr + jj), qrot(pq, ancl[jj]) + pp);
      }
    }
  }
  float mat[9];
  q2mat(mat, quat);
  for (int i = 0; i < 9; i++) s_xmat[9 * b + i] = mat[i];
  st3(s_xipos + 3 * b, pos + mrot(mat, {ipos.x, ipos.y, ipos.z}));
}

// A geom's world pose from its body's record: the offset rotated with the body's matrix (mat: the caller's own operand - the stored xmat, or
// q2mat of the record's quaternion), the orientation the quaternion product; and the z axis of an orientation.
struct GeomPose { V3 pos; Q4 quat; };
__device__ __forceinline__ GeomPose geom_world_pose(const float* s_xpq, int b, const float* mat, V3 gpos, Q4 gquat) {
  return {ld3(s_xpq + kXpqStride * b) + mrot(mat, gpos), qmul(ldq(s_xpq + kXpqStride * b + 4), gquat)};
}
__device__ __forceinline__ V3 quat_zaxis(Q4 q) { return {2.f * (q.x * q.z + q.w * q.y), 2.f * (q.y * q.z - q.w * q.x), q.w * q.w - q.x * q.x - q.y * q.y + q.z * q.z}; }

}  // namespace hb
