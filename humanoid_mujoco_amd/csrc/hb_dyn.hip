// hb_dyn.hip - the dynamics read-out (hb_dynamics*, include/hb.h): the terms of the equations of motion of any number of states - the dense
// joint-space mass matrix (mj_fullM of mjData.qM), qfrc_bias (mj_rne with zero acceleration), qfrc_passive (joint springs and dampers) and
// the Jacobians of body-fixed points and subtree centres of mass (mj_jac*, mj_jacSubtreeCom) - as a pure function of (qpos, qvel), the model
// and, for the batch's own state, the env's own masses, armature and stiffness.  A kernel of its own: no solver and no collision enters, so
// every model takes it whatever kernels it steps in, and no step kernel carries anything for it.
#include <hip/hip_runtime.h>
#include "hb_kinematics.hpp"
#include "hb_launch.hpp"

namespace hb {

// per dof, three 16-byte quads: axis[3], kind (0: the dof turns the body about `anchor`, 1: it moves it along `axis`) | anchor[3], body |
// the linear half of cdof about the tree's subtree centre of mass [3], - (the angular half is `axis` for kind 0, zero for kind 1)
constexpr int kDynDofStride = 12;
// per body beside the pose record (kXpqStride, whose pad holds the body's ancestor mask): xipos[3], mass
constexpr int kDynXimStride = 4;
constexpr int kDynVaStride = 12;  // cvel[6] | cacc[6]
__host__ __device__ inline int dyn_stage_floats(int nv) { const int a = nv * nv, b = 6 * nv; return ((a > b ? a : b) + 3) & ~3; }
// LDS floats of one state: qpos | qvel | poses | xipos, mass | dof records | cvel, cacc | composite inertia, force | subtree coms | the
// block an output is assembled in before it leaves in 16-byte stores (M [nv][nv], then one Jacobian [6][nv] at a time)
__host__ __device__ inline int dyn_lds_floats(int nq, int nv, int nb, int ntree) {
  return ((nq + 3) & ~3) + ((nv + 3) & ~3) + kXpqStride * nb + kDynXimStride * nb + kDynDofStride * nv + kDynVaStride * nb + kIfStride * nb + 4 * (ntree > 0 ? ntree : 1) +
         dyn_stage_floats(nv);
}

// cnt floats of an LDS block to dst (4-byte aligned), by the L lanes of a state: 16-byte stores over the aligned middle, single floats at
// the ragged ends (at most three each)
template <int L>
__device__ __forceinline__ void dyn_copy_out(float* dst, const float* src, int cnt, int l) {
  int head = (int)((4u - (unsigned)(((uintptr_t)dst >> 2) & 3u)) & 3u);
  if (head > cnt) head = cnt;
  const int nquad = (cnt - head) >> 2;
  if (l < head) dst[l] = src[l];
  for (int k = l; k < nquad; k += L) {
    const float* p = src + head + 4 * k;
    *reinterpret_cast<float4*>(dst + head + 4 * k) = {p[0], p[1], p[2], p[3]};
  }
  const int t0 = head + 4 * nquad;
  if (l < cnt - t0) dst[t0 + l] = src[t0 + l];
}

// Lane = body for the tree passes and lane = dof (in rounds of L) for everything per dof; L lanes per state (packed_lanes()), 64 / L states per
// wave, as in hb_kin.hip: every sub-group of L lanes has an LDS block of its
// own and executes the same instructions on it as a wave that holds one state, so a state's result depends neither on L nor on its place
// in the wave, its neighbours or n.  No atomics: every sum runs in a fixed order.  Nothing of the batch is written; a non-finite input
// makes that state's own rows garbage and nothing else: no index depends on data.
template <int L>
__device__ __forceinline__ void dyn_body(const DevModel* Mp, const DynArgs& A) {
  DevModelRef M = *(const DevModel HB_CONST*)(uintptr_t)Mp;
  extern __shared__ float4 lds4[];  // (16-byte aligned base)
  float* lds = reinterpret_cast<float*>(lds4);
  constexpr int kPer = kGroup / L;  // states per wave
  const int sub = (int)threadIdx.x / L, l = (int)threadIdx.x % L;
  const long long s = (long long)blockIdx.x * kPer + sub;
  const bool live = s < A.n;
  const int nq = M.nq, nv = M.nv, nb = M.nbody, ntree = M.ntree;
  float* s_qpos = lds + (size_t)sub * dyn_lds_floats(nq, nv, nb, ntree);
  float* s_qvel = s_qpos + ((nq + 3) & ~3);
  float* s_xpq = s_qvel + ((nv + 3) & ~3);
  float* s_xim = s_xpq + kXpqStride * nb;
  float* s_dof = s_xim + kDynXimStride * nb;
  float* s_va = s_dof + kDynDofStride * nv;
  float* s_if = s_va + kDynVaStride * nb;
  float* s_scom = s_if + kIfStride * nb;
  float* s_out = s_scom + 4 * (ntree > 0 ? ntree : 1);
  // the env's own parameters (the batch-state forms with domain randomisation installed), or the model's
  const float* dr = (A.dr && live) ? A.dr + (size_t)s * A.dr_stride : nullptr;
  const DomainLayout DL = domain_layout(nb, nv, M.nlimcand, M.nu, M.nhfielddata);
  for (int i = l; i < nq; i += L) s_qpos[i] = live ? A.qpos[(size_t)s * A.qpos_stride + i] : 0.f;
  for (int i = l; i < nv; i += L) s_qvel[i] = live && A.qvel ? A.qvel[(size_t)s * A.qvel_stride + i] : 0.f;
  const bool bl = l + 1 < nb;
  float4 q0 = {0.f, 0.f, 0.f, 0.f}, q1 = q0, bp = q0, bq = q0, bi = q0, biq = q0, bin = q0, ch0 = q0, ch1 = q0;
  float4 JA[3], JB[3], JC[3];
#pragma unroll
  for (int jj = 0; jj < 3; jj++) { JA[jj] = q0; JB[jj] = q0; JC[jj] = q0; }
  if (bl) {
    const float4 HB_CONST* R = M.brec + (size_t)(l + 1) * kBrecQuads;
    q0 = R[0]; q1 = R[1]; bp = R[2]; bq = R[3]; bi = R[4]; biq = R[5]; bin = R[6]; ch0 = R[7]; ch1 = R[8];
#pragma unroll
    for (int jj = 0; jj < 3; jj++) { JA[jj] = R[9 + 3 * jj]; JB[jj] = R[10 + 3 * jj]; JC[jj] = R[11 + 3 * jj]; }
  }
  if (l == 0) {  // the world: at the origin, massless, its own only ancestor
    reinterpret_cast<float4*>(s_xpq)[0] = {0.f, 0.f, 0.f, 0.f};
    reinterpret_cast<float4*>(s_xpq)[1] = {1.f, 0.f, 0.f, 0.f};
    reinterpret_cast<float4*>(s_xpq)[2] = {__int_as_float(1), __int_as_float(0), 0.f, 0.f};
    reinterpret_cast<float4*>(s_xim)[0] = {0.f, 0.f, 0.f, 0.f};
  }
  gsync();
  const int myb = __float_as_int(q0.x), myp = __float_as_int(q0.y), myjn = __float_as_int(q0.z);
  const int mylevel = bl ? (__float_as_int(q1.x) & 255) : -1, mycn = __float_as_int(q1.w), mytree = __float_as_int(q1.y);
  const int myanc2 = (__float_as_int(q1.x) >> 8) & 255, myanc4 = (__float_as_int(q1.x) >> 16) & 255, myanc8 = (__float_as_int(q1.x) >> 24) & 255;
  const float mymass = (dr && bl) ? dr[DL.o_mass + myb] : q1.z;
  const int mych[8] = {__float_as_int(ch0.x), __float_as_int(ch0.y), __float_as_int(ch0.z), __float_as_int(ch0.w),
                       __float_as_int(ch1.x), __float_as_int(ch1.y), __float_as_int(ch1.z), __float_as_int(ch1.w)};
  // ---------------------------------------------------------------- mj_kinematics (hb_kinematics.hpp: the pose in the parent's frame, then pointer jumping)
  const bool isfree = bl && myjn == 1 && __float_as_int(JA[0].x) == 0;
  V3 posl, axl[3], ancl[3];  // the pose, joint axes and anchors in the parent's frame
  Q4 quatl;
  local_pose(bl, isfree, myjn, bp, bq, JA, JB, JC, s_qpos, posl, quatl, axl, ancl);
  V3 mypos = posl;
  Q4 myquat = quatl;
  // bit b of a body's mask: body b is the body itself or one of its ancestors (the subtree test of the centre-of-mass Jacobians); it rides
  // along in the pose records' pad and is composed in the same rounds (compose_world()'s, statement for statement, with the masks between)
  unsigned mylo = bl ? (myb < 32 ? 1u << myb : 0u) | 1u : 0u, myhi = bl && myb >= 32 ? 1u << (myb - 32) : 0u;
  if (bl) {
    reinterpret_cast<float4*>(s_xpq + kXpqStride * myb)[0] = {mypos.x, mypos.y, mypos.z, 0.f};
    reinterpret_cast<float4*>(s_xpq + kXpqStride * myb)[1] = {myquat.w, myquat.x, myquat.y, myquat.z};
    reinterpret_cast<float4*>(s_xpq + kXpqStride * myb)[2] = {__uint_as_float(mylo), __uint_as_float(myhi), 0.f, 0.f};
  }
  gsync();
  for (int r = 0, span = 1; span < M.nlevel - 1 || r == 0; r++, span <<= 1) {
    const int anc = ancestor_up(r, myp, myanc2, myanc4, myanc8);
    float4 pp4 = {0.f, 0.f, 0.f, 0.f}, pq4 = {1.f, 0.f, 0.f, 0.f}, pm4 = pp4;
    if (bl) { const float4* Pp = reinterpret_cast<const float4*>(s_xpq + kXpqStride * anc); pp4 = Pp[0]; pq4 = Pp[1]; pm4 = Pp[2]; }
    gsync();  // every lane has read its ancestor before anyone overwrites a record
    if (bl && anc != 0) {
      const Q4 pq = {pq4.x, pq4.y, pq4.z, pq4.w};
      mypos = V3{pp4.x, pp4.y, pp4.z} + qrot(pq, mypos);
      myquat = qnormalize(qmul(pq, myquat));
      mylo |= __float_as_uint(pm4.x); myhi |= __float_as_uint(pm4.y);
      reinterpret_cast<float4*>(s_xpq + kXpqStride * myb)[0] = {mypos.x, mypos.y, mypos.z, 0.f};
      reinterpret_cast<float4*>(s_xpq + kXpqStride * myb)[1] = {myquat.w, myquat.x, myquat.y, myquat.z};
      reinterpret_cast<float4*>(s_xpq + kXpqStride * myb)[2] = {__uint_as_float(mylo), __uint_as_float(myhi), 0.f, 0.f};
    }
    gsync();
  }
  // what hangs off the world poses: xipos, and per dof of the body's joints the world axis and anchor (xaxis, xanchor).  A free joint's
  // translations run along the world axes, its rotations about the body's own axes through its frame origin (mj_kinematics, mj_comPos).
  float mymat[9];
  q2mat(mymat, myquat);
  const V3 myipos = mypos + mrot(mymat, V3{bi.x, bi.y, bi.z});
  if (bl) {
    reinterpret_cast<float4*>(s_xim + kDynXimStride * myb)[0] = {myipos.x, myipos.y, myipos.z, mymass};
    if (isfree) {
      const int da = __float_as_int(JA[0].z);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        float4* D = reinterpret_cast<float4*>(s_dof + kDynDofStride * (da + k));
        D[0] = {k == 0 ? 1.f : 0.f, k == 1 ? 1.f : 0.f, k == 2 ? 1.f : 0.f, __int_as_float(1)};
        D[1] = {0.f, 0.f, 0.f, __int_as_float(myb)};
        float4* E = reinterpret_cast<float4*>(s_dof + kDynDofStride * (da + 3 + k));
        E[0] = {mymat[k], mymat[3 + k], mymat[6 + k], __int_as_float(0)};
        E[1] = {mypos.x, mypos.y, mypos.z, __int_as_float(myb)};
      }
    } else {
      const Q4 pq = ldq(s_xpq + kXpqStride * myp + 4);
      const V3 pp = ld3(s_xpq + kXpqStride * myp);
#pragma unroll
      for (int jj = 0; jj < 3; jj++) {
        if (jj < myjn) {
          const int da = __float_as_int(JA[jj].z);
          const V3 ax = qrot(pq, axl[jj]), an = qrot(pq, ancl[jj]) + pp;
          float4* D = reinterpret_cast<float4*>(s_dof + kDynDofStride * da);
          D[0] = {ax.x, ax.y, ax.z, __int_as_float(__float_as_int(JA[jj].x) == 2 ? 1 : 0)};
          D[1] = {an.x, an.y, an.z, __int_as_float(myb)};
        }
      }
    }
  }
  gsync();
  // ---------------------------------------------------------------- mj_comPos: the point cinert, cdof, cvel and cfrc refer to
  // lane = tree: the mass-weighted mean of the tree's xipos, bodies in ascending order (with the model's own 1 / mass, as the step kernels
  // take it: under per-env masses the point is not exactly the centre of mass, and need not be - every quantity refers to the same point)
  for (int t = l; t < ntree; t += L) {
    V3 acc = {0.f, 0.f, 0.f};
    for (int b = 1; b < nb; b++) {
      const float4 xm = reinterpret_cast<const float4*>(s_xim + kDynXimStride * b)[0];
      if (M.body_treeid[b] == t) acc = acc + V3{xm.x, xm.y, xm.z} * xm.w;
    }
    const float im = M.tree_invmass[t];
    reinterpret_cast<float4*>(s_scom + 4 * t)[0] = {acc.x * im, acc.y * im, acc.z * im, 0.f};
  }
  gsync();
  for (int d = l; d < nv; d += L) {
    const float4* D = reinterpret_cast<const float4*>(s_dof + kDynDofStride * d);
    const float4 a = D[0], c = D[1];
    const V3 axis = {a.x, a.y, a.z};
    const V3 com = ld3(s_scom + 4 * __float_as_int(M.drec[3 * d + 1].x));
    const V3 lin = __float_as_int(a.w) ? axis : cross(axis, com - V3{c.x, c.y, c.z});
    reinterpret_cast<float4*>(s_dof + kDynDofStride * d)[2] = {lin.x, lin.y, lin.z, 0.f};
  }
  float in[10];
#pragma unroll
  for (int i = 0; i < 10; i++) in[i] = 0.f;
  if (bl) {  // cinert: the body's inertia about that point, world axes (mj_comPos)
    const V3 dif = myipos - ld3(s_scom + 4 * mytree);
    float mat[9], t[9];
    q2mat(mat, qmul(myquat, Q4{biq.x, biq.y, biq.z, biq.w}));
    for (int r = 0; r < 3; r++) { t[3 * r] = mat[3 * r] * bin.x; t[3 * r + 1] = mat[3 * r + 1] * bin.y; t[3 * r + 2] = mat[3 * r + 2] * bin.z; }
    const float mass = mymass;
    in[0] = t[0] * mat[0] + t[1] * mat[1] + t[2] * mat[2] + mass * (dif.y * dif.y + dif.z * dif.z);
    in[1] = t[3] * mat[3] + t[4] * mat[4] + t[5] * mat[5] + mass * (dif.x * dif.x + dif.z * dif.z);
    in[2] = t[6] * mat[6] + t[7] * mat[7] + t[8] * mat[8] + mass * (dif.x * dif.x + dif.y * dif.y);
    in[3] = t[0] * mat[3] + t[1] * mat[4] + t[2] * mat[5] - mass * dif.x * dif.y;
    in[4] = t[0] * mat[6] + t[1] * mat[7] + t[2] * mat[8] - mass * dif.x * dif.z;
    in[5] = t[3] * mat[6] + t[4] * mat[7] + t[5] * mat[8] - mass * dif.y * dif.z;
    in[6] = mass * dif.x; in[7] = mass * dif.y; in[8] = mass * dif.z; in[9] = mass;
  }
  gsync();
  // one dof's motion axis: angular[3], linear[3]
  auto ld_dyn_cdof = [&](int d, float out[6]) {
    const float4* D = reinterpret_cast<const float4*>(s_dof + kDynDofStride * d);
    const float4 a = D[0], c = D[2];
    const bool rot = __float_as_int(a.w) == 0;
    out[0] = rot ? a.x : 0.f; out[1] = rot ? a.y : 0.f; out[2] = rot ? a.z : 0.f; out[3] = c.x; out[4] = c.y; out[5] = c.z;
  };
  // ---------------------------------------------------------------- mj_comVel + the forward pass of mj_rne with qacc = 0
  // a body's own share: lv = sum cdof qvel over its dofs, la = sum (velocity before the dof) x cdof qvel; then chains by pointer jumping,
  // a segment U above a segment L composing as V = V_U + V_L, A = A_U + A_L + V_U x V_L (the motion cross product is bilinear)
  float mycvel[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, mycacc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (bl) {
    float cd[6], t[6];
    if (isfree) {
      const int da = __float_as_int(JA[0].z);
      for (int k = 0; k < 3; k++) {
        const float qv = s_qvel[da + k];
        ld_dyn_cdof(da + k, cd);
        for (int i = 0; i < 6; i++) mycvel[i] += cd[i] * qv;
      }
      // the three rotational dofs all see the velocity after the translational ones (mj_comVel, free joint)
      float rot[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < 3; k++) {
        const float qv = s_qvel[da + 3 + k];
        ld_dyn_cdof(da + 3 + k, cd);
        cross_motion(t, mycvel, cd);
        for (int i = 0; i < 6; i++) { mycacc[i] += t[i] * qv; rot[i] += cd[i] * qv; }
      }
      for (int i = 0; i < 6; i++) mycvel[i] += rot[i];
    } else {
#pragma unroll
      for (int jj = 0; jj < 3; jj++) {
        if (jj < myjn) {
          const int da = __float_as_int(JA[jj].z);
          const float qv = s_qvel[da];
          ld_dyn_cdof(da, cd);
          cross_motion(t, mycvel, cd);
          for (int i = 0; i < 6; i++) { mycacc[i] += t[i] * qv; mycvel[i] += cd[i] * qv; }
        }
      }
    }
    float4* Op = reinterpret_cast<float4*>(s_va + kDynVaStride * myb);
    Op[0] = {mycvel[0], mycvel[1], mycvel[2], mycvel[3]};
    Op[1] = {mycvel[4], mycvel[5], mycacc[0], mycacc[1]};
    Op[2] = {mycacc[2], mycacc[3], mycacc[4], mycacc[5]};
  }
  gsync();
  for (int r = 0, span = 1; span < M.nlevel - 1 || r == 0; r++, span <<= 1) {
    const int anc = ancestor_up(r, myp, myanc2, myanc4, myanc8);
    float4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0;
    if (bl && anc != 0) { const float4* Pp = reinterpret_cast<const float4*>(s_va + kDynVaStride * anc); a0 = Pp[0]; a1 = Pp[1]; a2 = Pp[2]; }
    gsync();
    if (bl && anc != 0) {
      const float uv[6] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y};
      const float ua[6] = {a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
      float t[6];
      cross_motion(t, uv, mycvel);
      for (int i = 0; i < 6; i++) { mycacc[i] += ua[i] + t[i]; mycvel[i] += uv[i]; }
      float4* Op = reinterpret_cast<float4*>(s_va + kDynVaStride * myb);
      Op[0] = {mycvel[0], mycvel[1], mycvel[2], mycvel[3]};
      Op[1] = {mycvel[4], mycvel[5], mycacc[0], mycacc[1]};
      Op[2] = {mycacc[2], mycacc[3], mycacc[4], mycacc[5]};
    }
    gsync();
  }
  if (!(M.disableflags & (1 << 6))) for (int i = 0; i < 3; i++) mycacc[3 + i] -= M.gravity[i];  // the world's cacc (mjDSBL_GRAVITY: none)
  // ---------------------------------------------------------------- mj_crb and the backward pass of mj_rne, one sweep up the tree
  // seeds: the body's own cinert and its force cinert cacc + cvel x* (cinert cvel); then children into parents in pull form, level by level
  if (bl) {
    float f0[6], f1[6], f2[6];
    mul_inert_vec(f0, in, mycacc);
    mul_inert_vec(f1, in, mycvel);
    cross_force(f2, mycvel, f1);
    float4* Op = reinterpret_cast<float4*>(s_if + kIfStride * myb);
    Op[0] = {in[0], in[1], in[2], in[3]};
    Op[1] = {in[4], in[5], in[6], in[7]};
    Op[2] = {in[8], in[9], f0[0] + f2[0], f0[1] + f2[1]};
    Op[3] = {f0[2] + f2[2], f0[3] + f2[3], f0[4] + f2[4], f0[5] + f2[5]};
  }
  if (l < 4) reinterpret_cast<float4*>(s_if)[l] = {0.f, 0.f, 0.f, 0.f};  // the world
  gsync();
  for (int lev = M.nlevel - 2; lev >= 1; lev--) {
    if (mylevel == lev && mycn > 0) {
      float4* Op = reinterpret_cast<float4*>(s_if + kIfStride * myb);
      float4 acc[4] = {Op[0], Op[1], Op[2], Op[3]};
#pragma unroll
      for (int k = 0; k < 8; k++)
        if (k < mycn) {
          const float4* Cp = reinterpret_cast<const float4*>(s_if + kIfStride * mych[k]);
#pragma unroll
          for (int q = 0; q < 4; q++) { const float4 c = Cp[q]; acc[q].x += c.x; acc[q].y += c.y; acc[q].z += c.z; acc[q].w += c.w; }
        }
#pragma unroll
      for (int q = 0; q < 4; q++) Op[q] = acc[q];
    }
    gsync();
  }
  // ---------------------------------------------------------------- M: row i along dof i's ancestor chain, lane = dof
  // M(i, j) = cdof_j . (crb[body(i)] cdof_i) for every dof j at or above i (the entries of mjData.qM, in its own order: mrec), armature on
  // the diagonal, zero off the chains.  Both triangles are written from the one value.
  if (A.M) {
    for (int i = l; i < nv * nv; i += L) s_out[i] = 0.f;
    gsync();
    const int nM = M.nM;
    for (int i = l; i < nv; i += L) {
      const float4 dA = M.drec[3 * i], dB = M.drec[3 * i + 1];
      const int bi_ = __float_as_int(dA.y);
      float cd[6], buf[6], cin[10];
      ld_dyn_cdof(i, cd);
      {
        const float4* Ip = reinterpret_cast<const float4*>(s_if + kIfStride * bi_);
        const float4 i0 = Ip[0], i1 = Ip[1], i2 = Ip[2];
        cin[0] = i0.x; cin[1] = i0.y; cin[2] = i0.z; cin[3] = i0.w; cin[4] = i1.x; cin[5] = i1.y; cin[6] = i1.z; cin[7] = i1.w; cin[8] = i2.x; cin[9] = i2.y;
      }
      mul_inert_vec(buf, cin, cd);
      const float arm = dr ? dr[DL.o_arm + i] : dB.y;
      const int e0 = M.dof_Madr[i];
      int pf_pk = M.mrec[e0];
      for (int e = e0; e < nM; e++) {
        const int pk = pf_pk;
        if ((pk & 255) != i) break;
        if (e + 1 < nM) pf_pk = M.mrec[e + 1];  // the next entry's word, one ahead
        const int j = (pk >> 8) & 255;
        float cj[6];
        ld_dyn_cdof(j, cj);
        float v = 0.f;
        for (int t = 0; t < 6; t++) v += cj[t] * buf[t];
        if (j == i) v += arm;
        s_out[i * nv + j] = v;
        s_out[j * nv + i] = v;
      }
    }
    gsync();
    if (live) dyn_copy_out<L>(A.M + (size_t)s * nv * nv, s_out, nv * nv, l);
    gsync();
  }
  // ---------------------------------------------------------------- qfrc_bias (the backward pass projected onto cdof), qfrc_passive (mj_passive)
  if (A.bias || A.passive) {
    for (int d = l; d < nv; d += L) {
      const float4 dA = M.drec[3 * d], dB = M.drec[3 * d + 1], dC = M.drec[3 * d + 2];
      const int b = __float_as_int(dA.y);
      float cd[6];
      ld_dyn_cdof(d, cd);
      float bias = 0.f;
      for (int t = 0; t < 6; t++) bias += cd[t] * s_if[kIfStride * b + 10 + t];
      float passive = 0.f;
      if (!(M.disableflags & (1 << 5))) {
        if (__float_as_int(dA.z) >= 2) passive -= (dr ? dr[DL.o_stiff + d] : dB.w) * (s_qpos[__float_as_int(dC.x)] - dC.y);
        passive -= dB.z * s_qvel[d];
      }
      if (live && A.bias) A.bias[(size_t)s * nv + d] = bias;
      if (live && A.passive) A.passive[(size_t)s * nv + d] = passive;
    }
  }
  // ---------------------------------------------------------------- Jacobians, one point at a time, lane = dof
  // column d of a point p that dof d moves: jacr = axis, jacp = axis x (p - anchor) for a turning dof; jacp = axis for a sliding one
  if (A.jac) {
    for (int k = 0; k < A.njac; k++) {
      const int jb = A.jbody[k];
      const bool sub_com = A.jkind[k] != 0;
      const V3 pnt = ld3(s_xpq + kXpqStride * jb) + qrot(ldq(s_xpq + kXpqStride * jb + 4), V3{A.joff[k][0], A.joff[k][1], A.joff[k][2]});
      // dof d moves body b when d's own body is b or one of b's ancestors: bit body(d) of b's mask
      const float4 jm = reinterpret_cast<const float4*>(s_xpq + kXpqStride * jb)[2];
      const unsigned long long pmask = (unsigned long long)__float_as_uint(jm.x) | ((unsigned long long)__float_as_uint(jm.y) << 32);
      for (int d = l; d < nv; d += L) {
        const float4* D = reinterpret_cast<const float4*>(s_dof + kDynDofStride * d);
        const float4 a = D[0], c = D[1];
        const V3 axis = {a.x, a.y, a.z}, anchor = {c.x, c.y, c.z};
        const bool slide = __float_as_int(a.w) != 0;
        const int db = __float_as_int(c.w);
        V3 jp = {0.f, 0.f, 0.f}, jr = {0.f, 0.f, 0.f};
        if (!sub_com) {
          if ((pmask >> db) & 1ull) {
            jp = slide ? axis : cross(axis, pnt - anchor);
            if (!slide) jr = axis;
          }
        } else {
          // mj_jacSubtreeCom: the mass-weighted mean of the xipos Jacobians of the subtree's bodies, in ascending order
          float msum = 0.f;
          for (int b = 1; b < nb; b++) {
            const float4 am = reinterpret_cast<const float4*>(s_xpq + kXpqStride * b)[2];
            const unsigned long long anc = (unsigned long long)__float_as_uint(am.x) | ((unsigned long long)__float_as_uint(am.y) << 32);
            if (!((anc >> jb) & 1ull)) continue;
            const float4 xm = reinterpret_cast<const float4*>(s_xim + kDynXimStride * b)[0];
            msum += xm.w;
            if ((anc >> db) & 1ull) jp = jp + (slide ? axis : cross(axis, V3{xm.x, xm.y, xm.z} - anchor)) * xm.w;
          }
          jp = jp * (msum > 0.f ? 1.f / msum : 0.f);
        }
        s_out[d] = jp.x; s_out[nv + d] = jp.y; s_out[2 * nv + d] = jp.z;
        s_out[3 * nv + d] = jr.x; s_out[4 * nv + d] = jr.y; s_out[5 * nv + d] = jr.z;
      }
      gsync();
      if (live) dyn_copy_out<L>(A.jac + ((size_t)s * A.njac + k) * 6 * nv, s_out, 6 * nv, l);
      gsync();
    }
  }
}
__global__ __launch_bounds__(kGroup) void hb_dyn16_kernel(const DevModel* Mp, const DynArgs A) { dyn_body<16>(Mp, A); }
__global__ __launch_bounds__(kGroup) void hb_dyn32_kernel(const DevModel* Mp, const DynArgs A) { dyn_body<32>(Mp, A); }
__global__ __launch_bounds__(kGroup) void hb_dyn64_kernel(const DevModel* Mp, const DynArgs A) { dyn_body<64>(Mp, A); }

hipError_t launch_dynamics(const DevModel* M_dev, const DevModel& M, const DynArgs& A, int pack, hipStream_t stream, const char** kernel) {
  static const PackedKernel<DynArgs> triple[3] = {{hb_dyn16_kernel, "hb_dyn16_kernel"}, {hb_dyn32_kernel, "hb_dyn32_kernel"}, {hb_dyn64_kernel, "hb_dyn64_kernel"}};
  return launch_packed(triple, M_dev, M, A, pack, dyn_lds_floats(M.nq, M.nv, M.nbody, M.ntree), stream, kernel);
}

}  // namespace hb
