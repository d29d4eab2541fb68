// hb_pose_kernel.inl - included three times by hb_narrow.hip (HB_POSE_BOX 0, 1, 2): hb_pose_kernel with the text, registers and instructions it had
// before box geoms, hb_pose_box_kernel, its twin for a model with box geoms (StageBufs::has_box), which alone carries the analytic box
// colliders and the box cases of the work lists, and hb_pose_boxm_kernel (has_box 2: the box - box manifold on), which adds box_box.  Twice the text and not a function template called from two entries: the entry then
// takes its arguments through a reference, and the compiler schedules the kernel's argument loads differently (133 instructions of
// hb_pose_kernel moved when that was tried).
#if HB_POSE_BOX == 2
#define HB_POSE_KERNEL hb_pose_boxm_kernel
#elif HB_POSE_BOX
#define HB_POSE_KERNEL hb_pose_box_kernel
#else
#define HB_POSE_KERNEL hb_pose_kernel
#endif
__global__ __launch_bounds__(kGroup, 4) void HB_POSE_KERNEL(const DevModel* Mp, const BatchPtrs P) {
  DevModelRef M = *(const DevModel HB_CONST*)(uintptr_t)Mp;
  extern __shared__ float lds[];
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= P.nblk) return;
  const int env = P.blk0 + (int)blockIdx.x;
  if (blockIdx.x == 0 && lane == 0 && P.stage.defer_count) P.stage.defer_count[P.blk0] = 0;  // (the list the step's fast pass fills for its second pass)
  if (P.env_mask && !P.env_mask[env]) { if (lane == 0) { P.stage.nwork[env] = 0; P.stage.nsearch[2 * env] = 0; P.stage.nsearch[2 * env + 1] = 0; } return; }
  const int nq = M.nq, nv = M.nv, nb = M.nbody, ng = M.ngeom;
  float* s_qpos = lds;
  float* s_xpq = s_qpos + ((nq + 3) & ~3);
  float* s_gpos = s_xpq + kXpqStride * nb;
  float* s_gaxis = s_gpos + ((3 * ng + 3) & ~3);
  float* s_gquat = s_gaxis + ((3 * ng + 3) & ~3);
  int* s_scratch = reinterpret_cast<int*>(s_gquat + 4 * ng);
  const float* gstate = P.state + (size_t)env * M.nstate;
  // mj_checkPos / mj_checkVel: a bad state is reset before the step, and the step's poses are those of qpos0
  bool badp = false, badv = false;
  for (int i = lane; i < nq; i += kGroup) { const float v = gstate[1 + i]; s_qpos[i] = v; badp |= !(fabsf(v) <= HB_MAXVAL); }
  for (int i = lane; i < nv; i += kGroup) { const float v = gstate[1 + nq + i]; badv |= !(fabsf(v) <= HB_MAXVAL); }
  if (__any(badp) || __any(badv)) for (int i = lane; i < nq; i += kGroup) s_qpos[i] = M.qpos0[i];
  const bool bl = lane + 1 < nb;
  float4 q0 = {0.f, 0.f, 0.f, 0.f}, q1 = q0, bp = q0, bq = q0;
  float4 JA[3], JB[3], JC[3];
#pragma unroll
  for (int jj = 0; jj < 3; jj++) { JA[jj] = q0; JB[jj] = q0; JC[jj] = q0; }
  if (bl) {
    const float4 HB_CONST* R = M.brec + (size_t)(lane + 1) * kBrecQuads;
    q0 = R[0]; q1 = R[1]; bp = R[2]; bq = R[3];
#pragma unroll
    for (int jj = 0; jj < 3; jj++) { JA[jj] = R[9 + 3 * jj]; JB[jj] = R[10 + 3 * jj]; JC[jj] = R[11 + 3 * jj]; }
  }
  int pf_gbody = 0;
  V3 pf_gpos = {0.f, 0.f, 0.f};
  Q4 pf_gquat = {1.f, 0.f, 0.f, 0.f};
  if (lane < ng) { pf_gbody = M.geom_bodyid[lane]; pf_gpos = ld3(M.geom_pos + 3 * lane); pf_gquat = ldq(M.geom_quat + 4 * lane); }
  if (lane == 0) { st3(s_xpq, {0.f, 0.f, 0.f}); stq(s_xpq + 4, {1.f, 0.f, 0.f, 0.f}); }
  gsync();
  const int myb = __float_as_int(q0.x), myp = __float_as_int(q0.y), myjn = __float_as_int(q0.z);
  const int myanc2 = (__float_as_int(q1.x) >> 8) & 255, myanc4 = (__float_as_int(q1.x) >> 16) & 255, myanc8 = (__float_as_int(q1.x) >> 24) & 255;
  const bool isfree = bl && myjn == 1 && __float_as_int(JA[0].x) == 0;
  V3 posl, axl[3], ancl[3];
  Q4 quatl;
  local_pose(bl, isfree, myjn, bp, bq, JA, JB, JC, s_qpos, posl, quatl, axl, ancl);
  V3 mypos = posl;
  Q4 myquat = quatl;
  compose_world(bl, myb, myp, myanc2, myanc4, myanc8, M.nlevel, s_xpq, mypos, myquat);
  // geoms: world position, z axis and orientation (the step kernel rotates the offset with the body's matrix: the same q2mat here)
  if (lane < ng) {
    const int g = lane, b = pf_gbody;
    float mat[9];
    q2mat(mat, ldq(s_xpq + kXpqStride * b + 4));
    const GeomPose G = geom_world_pose(s_xpq, b, mat, pf_gpos, pf_gquat);
    const V3 gp = G.pos, ga = quat_zaxis(G.quat);
    const Q4 q = G.quat;
    st3(s_gpos + 3 * g, gp); st3(s_gaxis + 3 * g, ga); stq(s_gquat + 4 * g, q);
    float* o = P.stage.geom + (size_t)env * ng * 10;  // per env: positions[3 ng] | z axes[3 ng] | quaternions[4 ng]
    st3(o + 3 * g, gp); st3(o + 3 * ng + 3 * g, ga); stq(o + 6 * ng + 4 * g, q);
  }
  gsync();
  int status = 0;
  const int nwork = build_work_list<HB_POSE_BOX>(M, lane, s_gpos, s_gaxis, s_gquat, s_scratch, status);
  const int* s_list = s_scratch;
  const int* s_pinfo = s_scratch + kListMax;
  const int* s_work = s_pinfo + 4 * kListMax;
  // Every item but its portal search (the analytic pairs completely; a prism's height test): results of the items that are done
  // go straight to the step kernel's input, the others are listed for hb_narrow_kernel, which packs them 64 to a wave whatever env
  // they belong to (an env has about nine: one wave per env would run mostly empty).
  const DomainLayout DL = domain_layout(M.nbody, M.nv, M.nlimcand, M.nu, M.nhfielddata);
  const float* hdata = P.dr ? P.dr + (size_t)env * P.dr_stride + DL.o_hfield : (const float*)M.hfield_data;
  float4* R = P.stage.result + (size_t)env * kWorkMax * 4;
  int4* items = P.stage.item + (size_t)env * kWorkMax;
  int nsearch1 = 0, nsearch2 = 0;
  for (int w0 = 0; w0 < nwork; w0 += kGroup) {
    const int w = w0 + lane;
    const bool have = w < nwork;
    const int item = have ? s_work[w] : 0;
    const int idx = item >> 16, sub = item & 0xffff;
    const int p = have ? s_list[idx] : 0;
    const int rmin = s_pinfo[4 * idx], cmin = s_pinfo[4 * idx + 1], ncols = s_pinfo[4 * idx + 2];
    ConOut co0, co1;
    int n;
    V3 hint;
    const int kind = eval_work_item<1, 1, 1, HB_POSE_BOX>(M, hdata, have, p, sub, rmin, cmin, ncols, __int_as_float(s_pinfo[4 * idx + 3]), s_gpos, s_gaxis, s_gquat, co0, co1, n, hint);
    if (have && !kind) {
      R[4 * w] = {co0.dist, co0.pos.x, co0.pos.y, co0.pos.z};
      R[4 * w + 1] = {co0.n.x, co0.n.y, co0.n.z, __int_as_float(n)};
      R[4 * w + 2] = {co1.dist, co1.pos.x, co1.pos.y, co1.pos.z};
      R[4 * w + 3] = {co1.n.x, co1.n.y, co1.n.z, __int_as_float(p)};
    }
    // (the env's own slots: prism searches from the front, pair searches from the back)
    const unsigned long long need1 = __ballot(have && kind == 1), need2 = __ballot(have && kind == 2);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int4 rec = {env, p | (w << 16), sub | (ncols << 16), rmin | (cmin << 16)};
    if (have && kind == 1) items[nsearch1 + __popcll(need1 & below)] = rec;
    if (have && kind == 2) items[kWorkMax - 1 - (nsearch2 + __popcll(need2 & below))] = rec;
    nsearch1 += __popcll(need1); nsearch2 += __popcll(need2);
  }
  if (lane == 0) {
    P.stage.nwork[env] = nwork;
    P.stage.nsearch[2 * env] = nsearch1; P.stage.nsearch[2 * env + 1] = nsearch2;
    int* c = P.counts + kCountStride * (size_t)env;
    c[5] = nwork; c[6] = nsearch1 + nsearch2;
    if (status) atomicOr(P.status + env, status);
  }
}
#undef HB_POSE_KERNEL
