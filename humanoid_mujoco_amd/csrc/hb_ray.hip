// hb_ray.hip - the ray read-out (hb_rays*, include/hb.h): mj_ray of every configured ray against every env's geoms, a pure function of
// the geoms' world poses (the model's own for the world body, hb_kin.hip's read-out for the rest), the model and the env's elevations.
// A kernel of its own: nothing of the batch is written and no step kernel carries anything for it.  The same kernels cast the scan of the
// env adapter's observation extension (hb_env_obs_extend): RayArgs::xform turns the distance into the observation's entry and writes it
// into a row of a wider table, RayArgs::env_mask leaves out the envs that are not asked for.
#include <hip/hip_runtime.h>
#include "hb_kcommon.hpp"
#include "hb_launch.hpp"

namespace hb {

constexpr float kRayNone = 3.0e38f;  // "no hit" while the nearest hit is being looked for

// Roots of |o + t d|^2 = r^2 through the point of closest approach (tc, and the half chord h behind it): r^2 - |o + tc d|^2 has none of the
// cancellation of the textbook discriminant b^2 - a c for a ray that starts far away.  false: the line misses, or d is (numerically) zero.
__device__ __forceinline__ bool ray_roots(V3 o, V3 d, float r, float& t0, float& t1) {
  const float dd = dot(d, d);
  if (!(dd > 1e-12f)) return false;
  const float inv = 1.f / dd;
  const float tc = -dot(o, d) * inv;
  const V3 q = o + d * tc;
  const float disc = r * r - dot(q, q);
  if (!(disc >= 0.f)) return false;
  const float h = sqrtf(disc * inv);
  t0 = tc - h; t1 = tc + h;
  return true;
}
__device__ __forceinline__ void ray_take(float& best, float t, bool ok) {
  if (ok && t >= 0.f && t < best) best = t;
}

// mj_rayGeom's surfaces in the geom's own frame (o, d: the ray there; d unit up to rounding): the distance, or kRayNone
__device__ __forceinline__ float ray_plane(V3 o, V3 d, float sx, float sy) {
  if (d.z == 0.f) return kRayNone;
  const float t = -o.z / d.z;
  const float x = o.x + t * d.x, y = o.y + t * d.y;
  const bool in = (sx <= 0.f || fabsf(x) <= sx) && (sy <= 0.f || fabsf(y) <= sy);
  return in && t >= 0.f ? t : kRayNone;
}
__device__ __forceinline__ float ray_sphere(V3 o, V3 d, float r) {
  float best = kRayNone, t0, t1;
  if (ray_roots(o, d, r, t0, t1)) { ray_take(best, t0, true); ray_take(best, t1, true); }
  return best;
}
// the cylinder wall between the caps, and the outer half of each end sphere
__device__ __forceinline__ float ray_capsule(V3 o, V3 d, float r, float half) {
  float best = kRayNone, t0, t1;
  if (ray_roots({o.x, o.y, 0.f}, {d.x, d.y, 0.f}, r, t0, t1)) {
    ray_take(best, t0, fabsf(o.z + t0 * d.z) <= half);
    ray_take(best, t1, fabsf(o.z + t1 * d.z) <= half);
  }
  if (ray_roots({o.x, o.y, o.z - half}, d, r, t0, t1)) {
    ray_take(best, t0, o.z + t0 * d.z >= half);
    ray_take(best, t1, o.z + t1 * d.z >= half);
  }
  if (ray_roots({o.x, o.y, o.z + half}, d, r, t0, t1)) {
    ray_take(best, t0, o.z + t0 * d.z <= -half);
    ray_take(best, t1, o.z + t1 * d.z <= -half);
  }
  return best;
}
// A box of half extents h: the six faces (the slab test, face by face, as mj_rayGeom walks them).  A face is hit where the ray crosses its
// plane inside the other two extents; the nearest non-negative crossing counts, so a ray from outside gets the face it enters by and one
// that starts inside the face it leaves by, as for the sphere and the capsule.  A ray parallel to a pair of faces cannot cross them.  eps
// widens a face by what the crossing point is known to: a ray through an edge is found from either face and never slips between two.
__device__ __forceinline__ float ray_box(V3 o, V3 d, V3 h) {
  float best = kRayNone;
  const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z}, hh[3] = {h.x, h.y, h.z};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (dd[a] == 0.f) continue;
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    const float inv = 1.f / dd[a];
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const float t = ((s ? hh[a] : -hh[a]) - oo[a]) * inv;
      const float eb = 1e-6f * (hh[b] + fabsf(oo[b])), ec = 1e-6f * (hh[c] + fabsf(oo[c]));
      ray_take(best, t, fabsf(oo[b] + t * dd[b]) <= hh[b] + eb && fabsf(oo[c] + t * dd[c]) <= hh[c] + ec);
    }
  }
  return best;
}

// One triangle of a grid cell, in the cell's coordinates (u along the columns, v along the rows, both 0..1): the surface is
// z = z0 + a u + b v over v <= u (LOWER) or v >= u; the ray is (u0 + t du, v0 + t dv, oz + t dz).  Both faces are hit.  eps widens the
// triangle by what u and v are known to: a ray through an edge or a vertex is found from either side and never falls between two cells.
template <bool LOWER>
__device__ __forceinline__ void ray_cell_tri(float& best, float z0, float a, float b, float u0, float v0, float oz, float du, float dv, float dz, float eps) {
  const float f0 = oz - z0 - a * u0 - b * v0, fd = dz - a * du - b * dv;
  if (fd == 0.f) return;
  const float t = -f0 / fd;
  const float u = u0 + t * du, v = v0 + t * dv;
  const bool in = u >= -eps && u <= 1.f + eps && v >= -eps && v <= 1.f + eps && (LOWER ? v <= u + eps : v >= u - eps);
  ray_take(best, t, in);
}

// The elevation surface of a height field in the field's frame: x in [-sx, sx] over the ncol columns, y in [-sy, sy] over the nrow rows,
// z = data[row][col] sz, cell (r, c) cut along the diagonal (r, c) - (r + 1, c + 1) as the collider cuts it (hb_collide.hpp: the strip
// order of mjc_ConvexHField).  The ray is clipped to the xy extent and walks the cells its projection crosses, nearest first (a 2-D DDA in
// grid units: at most nrow + ncol - 3 cells, and the loop ends after nrow + ncol whatever the data); the first cell with a hit has the
// nearest one.  Side walls and base are not part of the surface.  Every index is clamped into the grid before it is used.
__device__ __forceinline__ float ray_hfield(const float* data, int nrow, int ncol, float sx, float sy, float sz, V3 o, V3 d, float tmax) {
  if (nrow < 2 || ncol < 2) return kRayNone;
  float t0 = 0.f, t1 = tmax;
  if (d.x != 0.f) {
    const float inv = 1.f / d.x, a = (-sx - o.x) * inv, b = (sx - o.x) * inv;
    t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b));
  } else if (!(fabsf(o.x) <= sx)) return kRayNone;
  if (d.y != 0.f) {
    const float inv = 1.f / d.y, a = (-sy - o.y) * inv, b = (sy - o.y) * inv;
    t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b));
  } else if (!(fabsf(o.y) <= sy)) return kRayNone;
  if (!(t0 <= t1)) return kRayNone;
  // grid units: column coordinate gx in [0, ncol - 1], row coordinate gy in [0, nrow - 1]
  const float kx = (float)(ncol - 1) / (2.f * sx), ky = (float)(nrow - 1) / (2.f * sy);
  const float gx0 = (o.x + sx) * kx, gy0 = (o.y + sy) * ky, dgx = d.x * kx, dgy = d.y * ky;
  const float ix = dgx != 0.f ? 1.f / dgx : 0.f, iy = dgy != 0.f ? 1.f / dgy : 0.f;
  // the cell the ray is in at t0: on a grid line, the one it is heading into
  const float px = gx0 + t0 * dgx, py = gy0 + t0 * dgy;
  int c = (int)clampf(dgx < 0.f ? ceilf(px) - 1.f : floorf(px), 0.f, (float)(ncol - 2));
  int r = (int)clampf(dgy < 0.f ? ceilf(py) - 1.f : floorf(py), 0.f, (float)(nrow - 2));
  c = min(max(c, 0), ncol - 2); r = min(max(r, 0), nrow - 2);
  const float eps = 1e-6f * (float)(8 + nrow + ncol);
  float best = kRayNone;
  for (int it = 0; it < nrow + ncol; it++) {
    const float* row = data + r * ncol + c;
    const float h00 = row[0] * sz, h10 = row[1] * sz, h01 = row[ncol] * sz, h11 = row[ncol + 1] * sz;
    const float u0 = gx0 - (float)c, v0 = gy0 - (float)r;
    ray_cell_tri<true>(best, h00, h10 - h00, h11 - h10, u0, v0, o.z, dgx, dgy, d.z, eps);
    ray_cell_tri<false>(best, h00, h11 - h01, h01 - h00, u0, v0, o.z, dgx, dgy, d.z, eps);
    if (best < kRayNone) break;
    // on to the next cell: across the column or the row boundary the ray reaches first
    const float tnx = dgx != 0.f ? ((float)(dgx > 0.f ? c + 1 : c) - gx0) * ix : __builtin_inff();
    const float tny = dgy != 0.f ? ((float)(dgy > 0.f ? r + 1 : r) - gy0) * iy : __builtin_inff();
    if (!(fminf(tnx, tny) <= t1)) break;  // (leaves the extent or passes the cutoff inside this cell; a vertical ray has one cell: no boundary is ever reached)
    if (tnx <= tny) { c += dgx > 0.f ? 1 : -1; if (c < 0 || c > ncol - 2) break; }
    else { r += dgy > 0.f ? 1 : -1; if (r < 0 || r > nrow - 2) break; }
  }
  return best;
}

// Lane = ray: a block is up to four waves of 64 rays of ONE env (blockIdx.x), so that the geom records - type, size, pose - are the same
// in every lane (scalar loads of the model's tables, one address per wave for the poses) and the env's elevations are staged in LDS once
// for all of them (LDS = 1; a model whose fields do not fit reads them from memory, LDS = 0).  The wave walks the eligible geoms in
// ascending order and every lane keeps its nearest hit, a later geom only when it is strictly nearer: ties go to the lowest geom id.
// A lane's result is a function of its ray, the env's poses and the model alone - no cross-lane operation, no atomics - so it has the
// same bits wherever the ray stands in the array and however many envs or rays the launch has.  A non-finite pose makes that env's rows
// garbage and nothing else: the only data-dependent indices are the grid cell's, and those are clamped.
template <int LDS>
__device__ __forceinline__ void ray_body(const DevModel* Mp, const RayArgs& A) {
  const int env = (int)blockIdx.x;
  if (A.env_mask && !A.env_mask[env]) return;  // (the same for every lane of the block: nobody is left waiting at the barrier below)
  DevModelRef M = *(const DevModel HB_CONST*)(uintptr_t)Mp;
  extern __shared__ float lds[];
  const int i = (int)(blockIdx.y * blockDim.x + threadIdx.x);
  const DomainLayout DL = domain_layout(M.nbody, M.nv, M.nlimcand, M.nu, M.nhfielddata);
  const float* hglobal = A.dr ? A.dr + (size_t)env * A.dr_stride + DL.o_hfield : (const float*)M.hfield_data;
  if constexpr (LDS != 0) {
    for (int k = (int)threadIdx.x; k < M.nhfielddata; k += (int)blockDim.x) lds[k] = hglobal[k];
    __syncthreads();
  }
  if (i >= A.n_ray) return;
  // the ray in world coordinates
  V3 o = ld3(A.pnt + 3 * i), d = ld3(A.vec + 3 * i);
  if (A.frame != 0) {
    const float* bp = A.body_pose + ((size_t)env * M.nbody + A.frame_body) * 10;
    const V3 xp = ld3(bp);
    const Q4 xq = ldq(bp + 3);
    if (A.frame == 1) { o = xp + qrot(xq, o); d = qrot(xq, d); }
    else {
      // the heading frame: the body's x axis flattened onto the world xy plane, z up
      const V3 ax = qrot(xq, {1.f, 0.f, 0.f});
      float cx, cy;
      heading_cs(ax.x, ax.y, cx, cy);
      o = {xp.x + cx * o.x - cy * o.y, xp.y + cy * o.x + cx * o.y, xp.z + o.z};
      d = {cx * d.x - cy * d.y, cy * d.x + cx * d.y, d.z};
    }
  }
  const float tmax = A.cutoff > 0.f ? A.cutoff : kRayNone;
  float best = kRayNone;
  int bestg = -1;
  for (int k = 0; k < A.n_geom; k++) {
    const int g = A.geoms[k];
    const int type = M.geom_type[g];
    V3 gp;
    Q4 gq;
    if (M.geom_bodyid[g] == 0) { gp = ld3(M.geom_pos + 3 * g); gq = ldq(M.geom_quat + 4 * g); }
    else { const float* p = A.geom_pose + ((size_t)env * M.ngeom + g) * 7; gp = ld3(p); gq = ldq(p + 3); }
    const Q4 gc = qconj(gq);
    const V3 lo = qrot(gc, o - gp), ld = qrot(gc, d);
    const float s0 = M.geom_size[3 * g], s1 = M.geom_size[3 * g + 1];
    float t = kRayNone;
    if (type == 0) t = ray_plane(lo, ld, s0, s1);
    else if (type == 2) t = ray_sphere(lo, ld, s0);
    else if (type == 3) t = ray_capsule(lo, ld, s0, s1);
    else if (type == 6) t = ray_box(lo, ld, {s0, s1, M.geom_size[3 * g + 2]});
    else if (type == 1) {
      const int hid = M.geom_dataid[g];
      const float* data = (LDS != 0 ? (const float*)lds : hglobal) + M.hfield_adr[hid];
      t = ray_hfield(data, M.hfield_nrow[hid], M.hfield_ncol[hid], M.hfield_size[4 * hid], M.hfield_size[4 * hid + 1], M.hfield_size[4 * hid + 2], lo, ld, tmax);
    }
    if (t < best) { best = t; bestg = g; }
  }
  if (bestg < 0 || !(best <= tmax)) { best = -1.f; bestg = -1; }  // (nothing hit, or only beyond the cutoff; a NaN is no hit)
  if (A.xform) {
    // the observation's scan entry: a subtract, a multiply, a clamp - each rounded on its own (numpy float32 gives the same bits)
    const float d = best < 0.f ? A.cutoff : best;
    const float v = __fmul_rn(A.x_scale, __fsub_rn(A.x_offset, d));
    A.dist[(size_t)env * A.out_stride + A.out_col + i] = fminf(fmaxf(v, A.x_lo), A.x_hi);
    return;
  }
  const size_t at = (size_t)env * A.n_ray + i;
  if (A.dist) A.dist[at] = best;
  if (A.geomid) A.geomid[at] = bestg;
}
__global__ __launch_bounds__(kRayBlock) void hb_ray_kernel(const DevModel* Mp, const RayArgs A) { ray_body<0>(Mp, A); }
__global__ __launch_bounds__(kRayBlock) void hb_ray_lds_kernel(const DevModel* Mp, const RayArgs A) { ray_body<1>(Mp, A); }

hipError_t launch_rays(const DevModel* M_dev, const DevModel& M, const RayArgs& A, hipStream_t stream, const char** kernel) {
  (void)hipGetLastError();
  if (A.n_env < 1 || A.n_ray < 1 || A.n_ray > kRayMax) return hipErrorInvalidValue;
  if (A.xform && (!A.dist || A.out_stride < A.out_col + A.n_ray || A.out_col < 0)) return hipErrorInvalidValue;
  const int threads = min(kRayBlock, (A.n_ray + kGroup - 1) / kGroup * kGroup);
  const dim3 grid((unsigned)A.n_env, (unsigned)((A.n_ray + threads - 1) / threads));  // (y: at most kRayMax / 64 blocks)
  if (A.has_hfield && M.nhfielddata <= kRayLdsFloats) {
    hipLaunchKernelGGL(hb_ray_lds_kernel, grid, dim3(threads), (size_t)M.nhfielddata * sizeof(float), stream, M_dev, A);
    *kernel = "hb_ray_lds_kernel";
  } else {
    hipLaunchKernelGGL(hb_ray_kernel, grid, dim3(threads), 0, stream, M_dev, A);
    *kernel = "hb_ray_kernel";
  }
  return hipGetLastError();
}

}  // namespace hb
