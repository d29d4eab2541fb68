// hb_tables.cpp — builds the device model tables on the host (hb_tables.hpp): validation, topology, the record tables and the LDS
// layout, as named steps in the order their refusals are reported.  build_device_model (hb_batch.cpp) uploads the result; the
// build/hb_tables tool prints it.
#include "hb_tables.hpp"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace hb {

namespace {

// an integer as the bits of a float, as every record keeps its integers
float fi(int v) { float f; memcpy(&f, &v, 4); return f; }
// a 64-bit dof mask as two record words: lo, hi
void put_mask(float* r, unsigned long long mask) { r[0] = fi((int)(mask & 0xffffffffull)); r[1] = fi((int)(mask >> 32)); }

// the flat arrays: an empty table still takes one element, a record table (addraw) starts on a 16-byte boundary
size_t addi(std::vector<int>& iv, const std::vector<int>& v) { size_t o = iv.size(); iv.insert(iv.end(), v.begin(), v.end()); if (v.empty()) iv.push_back(0); return o; }
size_t addf(std::vector<float>& fv, const std::vector<double>& v) { size_t o = fv.size(); for (double x : v) fv.push_back((float)x); if (v.empty()) fv.push_back(0.f); return o; }
size_t addraw(std::vector<float>& fv, const std::vector<float>& v) { while (fv.size() % 4) fv.push_back(0.f); size_t o = fv.size(); fv.insert(fv.end(), v.begin(), v.end()); return o; }
size_t addu(std::vector<unsigned long long>& uv, const std::vector<unsigned long long>& v) { size_t o = uv.size(); uv.insert(uv.end(), v.begin(), v.end()); if (v.empty()) uv.push_back(0); return o; }

// contact dimension of a candidate pair (mj_contactParam: the geom of higher priority decides, else the larger condim)
int pair_condim(const Model& m, int g1, int g2) {
  const int p1 = m.geom_priority[g1], p2 = m.geom_priority[g2];
  return p1 != p2 ? m.geom_condim[p1 > p2 ? g1 : g2] : std::max(m.geom_condim[g1], m.geom_condim[g2]);
}

// contact parameter mixing per candidate pair (mj_contactParam restatement; static per pair)
void mix_pair(const Model& m, int g1, int g2, int& dim, double* fr, double* solref, double* solimp, double& margin, double& gap) {
  dim = pair_condim(m, g1, g2);
  int p1 = m.geom_priority[g1], p2 = m.geom_priority[g2];
  if (p1 != p2) {
    int g = p1 > p2 ? g1 : g2;
    for (int i = 0; i < 3; i++) fr[i] = m.geom_friction[3 * g + i];
    for (int i = 0; i < 2; i++) solref[i] = m.geom_solref[2 * g + i];
    for (int i = 0; i < 5; i++) solimp[i] = m.geom_solimp[5 * g + i];
  } else {
    for (int i = 0; i < 3; i++) fr[i] = std::max(m.geom_friction[3 * g1 + i], m.geom_friction[3 * g2 + i]);
    double s1 = m.geom_solmix[g1], s2 = m.geom_solmix[g2], mix;
    const double MINVAL = 1e-15;
    if (s1 >= MINVAL && s2 >= MINVAL) mix = s1 / (s1 + s2);
    else if (s1 < MINVAL && s2 < MINVAL) mix = 0.5;
    else mix = s1 < MINVAL ? 0.0 : 1.0;
    const double *r1 = &m.geom_solref[2 * g1], *r2 = &m.geom_solref[2 * g2];
    if (r1[0] > 0 && r2[0] > 0) for (int i = 0; i < 2; i++) solref[i] = mix * r1[i] + (1 - mix) * r2[i];
    else for (int i = 0; i < 2; i++) solref[i] = std::min(r1[i], r2[i]);
    for (int i = 0; i < 5; i++) solimp[i] = mix * m.geom_solimp[5 * g1 + i] + (1 - mix) * m.geom_solimp[5 * g2 + i];
  }
  margin = std::max(m.geom_margin[g1], m.geom_margin[g2]);
  gap = std::max(m.geom_gap[g1], m.geom_gap[g2]);
}

// ---- validation: the sizes this build handles, the scalar fields of the DevModel, the step kernel variant and the integrator
bool validate_model(const Model& m, DevModel& dm, std::string& err) {
  if (m.nv > 32) { err = "this build supports nv <= 32 degrees of freedom"; return false; }
  if (m.nbody > 64 || m.ngeom > 64) { err = "this build supports at most 64 bodies and 64 geoms"; return false; }
  for (int g = 0; g < m.ngeom; g++)
    if (m.geom_type[g] == GEOM_HFIELD && m.geom_bodyid[g] != 0) { err = "height fields must be attached to the world body"; return false; }
  for (int j = 0; j < m.njnt; j++)
    if (m.jnt_type[j] == JNT_BALL) { err = "ball joints are not supported"; return false; }
  int nb = m.nbody, nv = m.nv;
  dm.nq = m.nq; dm.nv = nv; dm.nu = m.nu; dm.nbody = nb; dm.njnt = m.njnt; dm.ngeom = m.ngeom; dm.ntendon = m.ntendon; dm.nM = m.nM; dm.npair = m.npair; dm.nhfielddata = m.nhfielddata;
  dm.nstate = 1 + m.nq + 2 * nv;
  dm.timestep = (float)m.timestep;
  for (int i = 0; i < 3; i++) dm.gravity[i] = (float)m.gravity[i];
  dm.inv_sqrt_impratio = (float)(1.0 / std::sqrt(m.impratio));
  dm.tolerance = (float)m.tolerance;
  dm.pgs_scale = (float)(1.0 / (m.meaninertia * std::max(1, nv)));
  dm.iterations = m.iterations;
  dm.disableflags = m.disableflags;
  dm.solver = m.solver; dm.ls_iterations = m.ls_iterations; dm.ls_tolerance = (float)m.ls_tolerance;
  if (!model_variant(m, dm.variant, dm.ncon_max, dm.nefc_max, err)) return false;
  dm.integrator = m.integrator;
  if (m.integrator != INT_EULER && m.integrator != INT_RK4) { err = "integrator " + std::to_string(m.integrator) + " is not implemented (Euler = 0, RK4 = 1)"; return false; }
  if (m.integrator == INT_RK4 && dm.variant != 0) {
    err = "RK4: only models that step in one kernel (plane / sphere / capsule geoms, condim 1 / 3) are implemented; this model steps in stages (mesh hulls, height fields or condim 4 / 6): use the Euler integrator";
    return false;
  }
  dm.mpr_iterations = 50; dm.mpr_tolerance = 1e-6f;  // mjOption.mpr_iterations / mpr_tolerance defaults (mjmodel.h:413,437)
  return true;
}

// ---- always-active rows, friction loss (mj_instantiateFriction): one row per dof with dof_frictionloss > 0, in front of the limit rows,
// unless the options disable it - then the model is an ordinary one.  What a row needs besides its dof and its bound does not depend on the
// state (pos = margin = 0), so it is worked out here, in fp64, with the options as they are now: one record per row, (dof, frictionloss, R, B).
bool friction_rows(const Model& m, DevModel& dm, std::vector<float>& frec, std::string& err) {
  const int nv = m.nv;
  if (!(m.disableflags & (DSBL_CONSTRAINT | DSBL_FRICTIONLOSS))) {
    for (int d = 0; d < nv; d++) {
      const double fl = m.dof_frictionloss[d];
      if (!(fl > 0)) continue;
      static const double def_ref[2] = {0.02, 1}, def_imp[5] = {0.9, 0.95, 0.001, 0.5, 2};
      const double* sr = m.dof_solref_friction.size() == (size_t)2 * nv ? &m.dof_solref_friction[2 * d] : def_ref;
      const double* si = m.dof_solimp_friction.size() == (size_t)5 * nv ? &m.dof_solimp_friction[5 * d] : def_imp;
      const double MINVAL = 1e-15, MINIMP = 0.0001, MAXIMP = 0.9999;
      auto clip = [](double x, double lo, double hi) { return std::min(std::max(x, lo), hi); };
      // impedance(solimp, 0, 0): solimp[0] clipped - or the mean of the two ends in the degenerate cases of getimpedance
      const double d0 = clip(si[0], MINIMP, MAXIMP), d1 = clip(si[1], MINIMP, MAXIMP);
      const double imp = (d0 == d1 || std::max(0.0, si[2]) <= MINVAL) ? 0.5 * (d0 + d1) : d0;
      const double R = std::max(MINVAL, (1 - imp) / imp * m.dof_invweight0[d]);
      double B;  // (kb_from_solref; K multiplies pos - margin = 0)
      if (sr[0] > 0) {
        const double tc = (m.disableflags & DSBL_REFSAFE) ? sr[0] : std::max(sr[0], 2 * m.timestep);
        B = 2 / std::max(MINVAL, d1 * tc);
      } else B = -sr[1] / std::max(MINVAL, d1);
      frec.push_back(fi(d)); frec.push_back((float)fl); frec.push_back((float)R); frec.push_back((float)B);
    }
  }
  dm.nfric = (int)frec.size() / 4;
  if (dm.nfric && dm.variant != 0) {
    err = "friction loss: only models that step in one kernel (plane / sphere / capsule geoms, condim 1 / 3) are implemented; this model steps in stages (mesh hulls, height fields or condim 4 / 6): remove the joints' frictionloss or set <flag frictionloss=\"disable\"/>";
    return false;
  }
  if (dm.nfric && m.integrator == INT_RK4) { err = "friction loss: the RK4 integrator is not implemented for a model with joint frictionloss: use the Euler integrator"; return false; }
  if (frec.empty()) frec.assign(4, 0.f);
  return true;
}

// ---- topology: trees, levels (bodies in level order), children, per body the dofs that move it, the sparse mass matrix's (i, j) per entry
// and its dense views: mdense [32 columns j][32 rows i] -> entry (nM: the zero pad, nM + 1: the one pad on the diagonal), mdense_c the same
// in the MFMA accumulator layout [16 registers][64 lanes]
struct Topology {
  std::vector<int> treeid, level_body, childadr, childnum, child_list, Mi, Mj, mdense, mdense_c;
  std::vector<double> tree_invmass;
  std::vector<unsigned long long> dofmask;
};
bool build_topology(const Model& m, DevModel& dm, Topology& tp, std::string& err) {
  const int nb = m.nbody, nv = m.nv;
  std::vector<int> roots;
  tp.treeid.assign(nb, 0);
  for (int b = 1; b < nb; b++) {
    if (m.body_parentid[b] == 0) { tp.treeid[b] = (int)roots.size(); roots.push_back(b); }
    else tp.treeid[b] = tp.treeid[m.body_parentid[b]];
  }
  dm.ntree = (int)roots.size();
  for (int r : roots) tp.tree_invmass.push_back(m.body_subtreemass[r] > 1e-15 ? 1.0 / m.body_subtreemass[r] : 0.0);
  int maxdepth = 0;
  for (int b = 0; b < nb; b++) maxdepth = std::max(maxdepth, m.body_depth[b]);
  dm.nlevel = maxdepth + 1;
  for (int L = 0; L <= maxdepth; L++)
    for (int b = 0; b < nb; b++) if (m.body_depth[b] == L) tp.level_body.push_back(b);
  tp.childadr.assign(nb, 0); tp.childnum.assign(nb, 0);
  for (int b = 0; b < nb; b++) {
    tp.childadr[b] = (int)tp.child_list.size();
    for (int c = 1; c < nb; c++) if (m.body_parentid[c] == b && c != b) { tp.child_list.push_back(c); tp.childnum[b]++; }
  }
  tp.dofmask.assign(nb, 0);
  for (int b = 1; b < nb; b++)
    for (int a = b; a > 0; a = m.body_parentid[a])
      for (int k = 0; k < m.body_dofnum[a]; k++) tp.dofmask[b] |= 1ull << (m.body_dofadr[a] + k);
  // dof ancestry
  tp.Mi.assign(m.nM, 0); tp.Mj.assign(m.nM, 0);
  for (int i = 0; i < nv; i++) {
    int adr = m.dof_Madr[i];
    for (int j = i; j >= 0; j = m.dof_parentid[j]) { tp.Mi[adr] = i; tp.Mj[adr] = j; adr++; }
  }
  if (m.nM > 1023) { err = "sparse mass matrix too large for the packed index tables"; return false; }
  tp.mdense.assign((size_t)32 * 32, m.nM);
  for (int i = 0; i < 32; i++) tp.mdense[(size_t)i * 32 + i] = m.nM + 1;
  for (int e = 0; e < m.nM; e++) { tp.mdense[(size_t)tp.Mj[e] * 32 + tp.Mi[e]] = e; tp.mdense[(size_t)tp.Mi[e] * 32 + tp.Mj[e]] = e; }
  tp.mdense_c.resize((size_t)16 * 64);
  for (int r = 0; r < 16; r++)
    for (int ln = 0; ln < 64; ln++) tp.mdense_c[(size_t)r * 64 + ln] = tp.mdense[(size_t)(ln & 31) * 32 + ((r & 3) + 8 * (r >> 2) + 4 * (ln >> 5))];
  return true;
}

// ---- LDS layout (hb_device.hpp: lds_layout - a function of the variant: a variant-2 / -3 model also gets the variant-1 layout for its fast
// step kernel); hands the layout back for the comparison with the size-specialised kernels'
bool layout_for(const Model& m, DevModel& dm, LdsLayout& L, std::string& err) {
  L = lds_layout(m.nq, m.nv, m.nu, m.nbody, m.njnt, m.ngeom, m.ntendon, m.nM, dm.ntree, dm.variant, dm.solver, dm.integrator, dm.ncon_max, dm.nefc_max);
  if (L.fail == kLdsNoEulerRoom) { err = "internal: LDS layout leaves no room for the Euler solve's W_H pair"; return false; }
  if (L.fail == kLdsTooLarge) { err = "model needs more LDS than one CU has"; return false; }
  set_layout(dm, L);
  return true;
}
// a model takes a size-specialised kernel when its sizes are the constant's and its layout is, every field, the constant's layout
static_assert(std::has_unique_object_representations_v<LdsLayout>, "layouts are compared as bytes");
bool sized_as(const Model& m, const DevModel& dm, const SizedModel& z, const LdsLayout& L) {
  return m.nq == z.nq && m.nv == z.nv && m.nu == z.nu && m.nbody == z.nbody && m.njnt == z.njnt && m.ngeom == z.ngeom && m.ntendon == z.ntendon && m.nM == z.nM && dm.ntree == z.ntree &&
         m.npair == z.npair && dm.nlevel == z.nlevel && dm.nlimcand == z.nlimcand && dm.nstate == z.nstate && memcmp(&L, static_cast<const LdsLayout*>(&z), sizeof(LdsLayout)) == 0;
}

// ---- collision, per candidate pair: the mixed contact parameters; fricab: (sliding friction of the floor - the first plane geom - if it
// takes part, else 0; the other geom's coefficient / the mixed one), what domain randomisation scales; self: both geoms on the robot
struct Pairs {
  std::vector<int> dim, self;
  std::vector<double> fr, solref, solimp, margin, gap, fricab;
};
bool mix_pairs(const Model& m, Pairs& P, std::string& err) {
  for (int p = 0; p < m.npair; p++) {
    int dim; double fr[3], sr[2], si[5], mg, gp;
    mix_pair(m, m.pair_geom1[p], m.pair_geom2[p], dim, fr, sr, si, mg, gp);
    if (dim != 1 && dim != 3 && dim != 4 && dim != 6) { err = "contact dimension " + std::to_string(dim) + " does not exist (condim 1, 3, 4, 6)"; return false; }
    P.dim.push_back(dim);
    for (double v : fr) P.fr.push_back(v);
    for (double v : sr) P.solref.push_back(v);
    for (double v : si) P.solimp.push_back(v);
    P.margin.push_back(mg); P.gap.push_back(gp);
  }
  int floor_geom = -1;
  for (int g = 0; g < m.ngeom && floor_geom < 0; g++) if (m.geom_type[g] == GEOM_PLANE) floor_geom = g;
  for (int p = 0; p < m.npair; p++) {
    const int g1 = m.pair_geom1[p], g2 = m.pair_geom2[p];
    if (g1 == floor_geom || g2 == floor_geom) {
      const int other = g1 == floor_geom ? g2 : g1;
      P.fricab.push_back(m.geom_friction[3 * floor_geom]); P.fricab.push_back(m.geom_friction[3 * other]);
    } else { P.fricab.push_back(0.0); P.fricab.push_back(P.fr[3 * p]); }
  }
  if (P.fricab.empty()) { P.fricab.push_back(0.0); P.fricab.push_back(0.0); }
  for (int p = 0; p < m.npair; p++) P.self.push_back(m.geom_bodyid[m.pair_geom1[p]] != 0);
  return true;
}
// per collision pair, everything mj_makeConstraint needs of it in one 5-quad record (one scalar fetch per contact):
// [0] body1, body2, tree1, tree2   [1] dof mask of body1 (lo, hi), of body2 (lo, hi)
// [2] margin - gap, solref[2], invweight0 sum   [3] solimp[0..3]   [4] solimp[4], condim, -, -
std::vector<float> pair_records(const Model& m, const Topology& tp, const Pairs& P) {
  std::vector<float> prec((size_t)std::max(1, m.npair) * 20, 0.f);
  for (int p = 0; p < m.npair; p++) {
    float* r = &prec[(size_t)p * 20];
    const int b1 = m.geom_bodyid[m.pair_geom1[p]], b2 = m.geom_bodyid[m.pair_geom2[p]];
    r[0] = fi(b1); r[1] = fi(b2); r[2] = fi(tp.treeid[b1]); r[3] = fi(tp.treeid[b2]);
    put_mask(r + 4, tp.dofmask[b1]); put_mask(r + 6, tp.dofmask[b2]);
    r[8] = (float)(P.margin[p] - P.gap[p]); r[9] = (float)P.solref[2 * p]; r[10] = (float)P.solref[2 * p + 1];
    r[11] = (float)(m.body_invweight0[2 * b1] + m.body_invweight0[2 * b2]);
    for (int i = 0; i < 4; i++) r[12 + i] = (float)P.solimp[5 * p + i];
    r[16] = (float)P.solimp[5 * p + 4]; r[17] = fi(P.dim[p]);
  }
  return prec;
}
// per collision pair, what mj_collision needs of it in one 3-quad record (one vector fetch per lane and round):
// [0] geom1, geom2, type1 | type2 << 8, margin   [1] rbound1, rbound2, size1[0], size1[1]   [2] size2[0], size2[1], -, -
std::vector<float> collision_records(const Model& m, const Pairs& P) {
  std::vector<float> crec((size_t)(std::max(1, m.npair) + 64) * 12, 0.f);  // + one round of padding for the prefetch
  for (int p = 0; p < m.npair; p++) {
    float* r = &crec[(size_t)p * 12];
    const int g1 = m.pair_geom1[p], g2 = m.pair_geom2[p];
    r[0] = fi(g1); r[1] = fi(g2); r[2] = fi(m.geom_type[g1] | (m.geom_type[g2] << 8)); r[3] = (float)P.margin[p];
    r[4] = (float)m.geom_rbound[g1]; r[5] = (float)m.geom_rbound[g2]; r[6] = (float)m.geom_size[3 * g1]; r[7] = (float)m.geom_size[3 * g1 + 1];
    r[8] = (float)m.geom_size[3 * g2]; r[9] = (float)m.geom_size[3 * g2 + 1];
  }
  return crec;
}
// half extents of every geom's bounding box in its own frame (the oriented boxes the broadphase of the general path tests before a
// pair of geoms is handed to the portal search): the hull's coordinate range for a mesh, the obvious for spheres and capsules
std::vector<double> geom_half_extents(const Model& m) {
  std::vector<double> geom_half((size_t)std::max(1, m.ngeom) * 3, 0.0);
  for (int g = 0; g < m.ngeom; g++) {
    double* h = &geom_half[3 * (size_t)g];
    h[0] = h[1] = h[2] = m.geom_rbound[g];
    if (m.geom_type[g] == GEOM_SPHERE) h[0] = h[1] = h[2] = m.geom_size[3 * g];
    else if (m.geom_type[g] == GEOM_CAPSULE) { h[0] = h[1] = m.geom_size[3 * g]; h[2] = m.geom_size[3 * g] + m.geom_size[3 * g + 1]; }
    else if (m.geom_type[g] == GEOM_BOX) { for (int c = 0; c < 3; c++) h[c] = m.geom_size[3 * g + c]; }  // the box itself: its colliders read their three sizes here
    else if (m.geom_type[g] == GEOM_MESH && m.geom_dataid[g] >= 0) {
      const int k = m.geom_dataid[g];
      h[0] = h[1] = h[2] = 0.0;
      for (int v = 0; v < m.mesh_vertnum[k]; v++)
        for (int c = 0; c < 3; c++) h[c] = std::max(h[c], std::fabs((double)(float)m.mesh_vert[3 * (size_t)(m.mesh_vertadr[k] + v) + c]));
    }
  }
  return geom_half;
}
// hull vertices as 16-byte records (x, y, z, link) and the edge graph with inlined coordinates, each vertex's neighbour list padded
// to whole chunks of kMeshChunk records with copies of the vertex itself (hb_device.hpp); per mesh the cube map of start vertices
struct MeshTables { std::vector<float> vert, nbr, start; };
bool mesh_tables(const Model& m, MeshTables& M, std::string& err) {
  std::vector<int> padadr(std::max(1, m.nmeshvert), 0), padchunks(std::max(1, m.nmeshvert), 0);
  int npad = 0;
  for (int g = 0; g < m.nmeshvert; g++) {
    padadr[g] = npad;
    padchunks[g] = (m.mesh_nbrnum[g] + kMeshChunk - 1) / kMeshChunk;
    npad += padchunks[g] * kMeshChunk;
    if (padchunks[g] > 255 || padadr[g] >= (1 << 23)) { err = "mesh edge graph too large for the packed link words"; return false; }
  }
  std::vector<float>&meshv = M.vert, &meshn = M.nbr, &meshs = M.start;
  meshv.assign((size_t)std::max(1, m.nmeshvert) * 4, 0.f); meshn.assign((size_t)std::max(1, npad) * 4, 0.f); meshs.assign((size_t)std::max(1, m.nmesh) * kMeshStart * 4, 0.f);
  auto link_of = [&](int g) { return fi((padadr[g] << 8) | padchunks[g]); };
  for (int k = 0; k < m.nmesh; k++) {
    for (int v = 0; v < m.mesh_vertnum[k]; v++) {
      const int g = m.mesh_vertadr[k] + v;
      for (int i = 0; i < 3; i++) meshv[(size_t)4 * g + i] = (float)m.mesh_vert[3 * g + i];
      meshv[(size_t)4 * g + 3] = link_of(g);
      for (int i = 0; i < padchunks[g] * kMeshChunk; i++) {
        const int w = i < m.mesh_nbrnum[g] ? m.mesh_vertadr[k] + m.mesh_nbr[m.mesh_nbradr[g] + i] : g;
        const size_t r = (size_t)padadr[g] + i;
        for (int c = 0; c < 3; c++) meshn[4 * r + c] = (float)m.mesh_vert[3 * w + c];
        meshn[4 * r + 3] = link_of(w);
      }
    }
    // cube map: face f = 2 * axis + (negative ? 1 : 0), cell (iu, iv) over the other two axes in cyclic order, u, v in [-1, 1]
    for (int f = 0; f < 6; f++)
      for (int iu = 0; iu < 4; iu++)
        for (int iv = 0; iv < 4; iv++) {
          const int ax = f >> 1;
          double d[3];
          d[ax] = (f & 1) ? -1.0 : 1.0; d[(ax + 1) % 3] = -0.75 + 0.5 * iu; d[(ax + 2) % 3] = -0.75 + 0.5 * iv;
          int best = m.mesh_vertadr[k];
          double bd = -1e300;
          for (int v = 0; v < m.mesh_vertnum[k]; v++) {
            const int g = m.mesh_vertadr[k] + v;
            // (the float-rounded coordinates the device climbs on)
            const double val = (double)(float)m.mesh_vert[3 * g] * d[0] + (double)(float)m.mesh_vert[3 * g + 1] * d[1] + (double)(float)m.mesh_vert[3 * g + 2] * d[2];
            if (val > bd) { bd = val; best = g; }
          }
          float* rec = &meshs[((size_t)k * kMeshStart + f * 16 + iu * 4 + iv) * 4];
          for (int c = 0; c < 3; c++) rec[c] = (float)m.mesh_vert[3 * best + c];
          rec[3] = link_of(best);
        }
  }
  return true;
}

// ---- limit candidates: two (lower, upper) per limited hinge / slide joint, then per limited tendon, in constraint order; and per candidate
// everything mj_instantiateLimit needs of it in one 4-quad record (one round trip instead of the dependent walk candidate -> joint -> addresses):
// [0] kind, id, side, qpos address (joints)   [1] margin, range, solref[2]   [2] solimp[0..3]   [3] solimp[4], invweight, dof address (joints), -
struct Limits {
  std::vector<int> kind, id, side;
  std::vector<double> range, margin, solref, solimp, invw;
  std::vector<float> lrec;
};
void build_limits(const Model& m, DevModel& dm, Limits& L) {
  auto add = [&](int kind, int id, const double* range, double margin, const double* solref, const double* solimp, double invw) {
    for (int side = -1; side <= 1; side += 2) {
      L.kind.push_back(kind); L.id.push_back(id); L.side.push_back(side);
      L.range.push_back(range[(side + 1) / 2]); L.margin.push_back(margin);
      for (int i = 0; i < 2; i++) L.solref.push_back(solref[i]);
      for (int i = 0; i < 5; i++) L.solimp.push_back(solimp[i]);
      L.invw.push_back(invw);
    }
  };
  for (int j = 0; j < m.njnt; j++)
    if (m.jnt_limited[j] && is_scalar_joint(m, j)) add(0, j, &m.jnt_range[2 * j], m.jnt_margin[j], &m.jnt_solref[2 * j], &m.jnt_solimp[5 * j], m.dof_invweight0[m.jnt_dofadr[j]]);
  for (int t = 0; t < m.ntendon; t++)
    if (m.tendon_limited[t]) add(1, t, &m.tendon_range[2 * t], m.tendon_margin[t], &m.tendon_solref_lim[2 * t], &m.tendon_solimp_lim[5 * t], m.tendon_invweight0[t]);
  dm.nlimcand = (int)L.kind.size();
  L.lrec.assign((size_t)std::max(1, dm.nlimcand) * 16, 0.f);
  for (int c = 0; c < dm.nlimcand; c++) {
    float* r = &L.lrec[(size_t)c * 16];
    const bool joint = L.kind[c] == 0;
    r[0] = fi(L.kind[c]); r[1] = fi(L.id[c]); r[2] = fi(L.side[c]); r[3] = fi(joint ? m.jnt_qposadr[L.id[c]] : 0);
    r[4] = (float)L.margin[c]; r[5] = (float)L.range[c]; r[6] = (float)L.solref[2 * c]; r[7] = (float)L.solref[2 * c + 1];
    for (int i = 0; i < 5; i++) r[8 + i] = (float)L.solimp[5 * c + i];
    r[13] = (float)L.invw[c]; r[14] = fi(joint ? m.jnt_dofadr[L.id[c]] : 0);
  }
}

// ---- observation tables of the env adapter.  A gather table: state-record offsets of the listed joints' qpos and qvel, then the root's
// angular velocity (3) - the first nobs - 3 observation entries are plain copies out of the state record.  The scalar joints in
// observation order: joint order, and - when every scalar joint has exactly one actuator - actuator order (the reference's JOINT_NAMES
// order, hb_env_config.obs_actuator_order)
struct ObsTables {
  std::vector<int> jnt, src, jnt_act, src_act;
  bool has_act_order = false;
};
void build_obs(const Model& m, DevModel& dm, ObsTables& O) {
  dm.obs_root_body = -1; dm.obs_root_dofadr = -1; dm.obs_root_qadr = -1;
  for (int j = 0; j < m.njnt; j++)
    if (m.jnt_type[j] == JNT_FREE) { dm.obs_root_dofadr = m.jnt_dofadr[j]; dm.obs_root_body = m.jnt_bodyid[j]; dm.obs_root_qadr = m.jnt_qposadr[j]; break; }
  dm.nobs = model_nobs(m);
  auto gather = [&](const std::vector<int>& joints) {
    std::vector<int> src;
    for (int j : joints) src.push_back(1 + m.jnt_qposadr[j]);
    for (int j : joints) src.push_back(1 + m.nq + m.jnt_dofadr[j]);
    for (int i = 0; i < 3; i++) src.push_back(dm.obs_root_dofadr >= 0 ? 1 + m.nq + dm.obs_root_dofadr + 3 + i : -1);
    return src;
  };
  for (int j = 0; j < m.njnt; j++) if (is_scalar_joint(m, j)) O.jnt.push_back(j);
  O.src = gather(O.jnt);
  std::vector<int> seen(m.njnt, 0);
  bool ok = m.nu == (int)O.jnt.size();
  for (int a = 0; a < m.nu && ok; a++) { if (seen[m.actuator_trnid[a]]++) ok = false; O.jnt_act.push_back(m.actuator_trnid[a]); }
  if (!ok) O.jnt_act.clear();
  O.has_act_order = ok;
  O.src_act = gather(O.jnt_act);
}

// ---- level-ordered body records, dof records, packed M entries (layouts in hb_device.hpp)
bool body_records(const Model& m, const Topology& tp, std::vector<float>& brec, std::string& err) {
  const int nb = m.nbody;
  brec.assign((size_t)nb * kBrecQuads * 4, 0.f);
  for (int sl = 0; sl < nb; sl++) {
    int b = tp.level_body[sl];
    float* r = &brec[(size_t)sl * kBrecQuads * 4];
    if (m.body_jntnum[b] > 3) { err = "at most 3 joints per body are supported (body '" + m.body_name[b] + "')"; return false; }
    if (tp.childnum[b] > 8) { err = "at most 8 child bodies per body are supported (body '" + m.body_name[b] + "')"; return false; }
    r[0] = fi(b); r[1] = fi(m.body_parentid[b]); r[2] = fi(m.body_jntnum[b]); r[3] = fi(m.body_jntadr[b]);
    {  // depth, and the ancestors 2, 4 and 8 links up (the world once the chain ends): the kinematics pass composes
       // poses by pointer jumping, log2(depth) rounds instead of one per level
      auto up = [&](int x, int k) { while (k-- > 0 && x > 0) x = m.body_parentid[x]; return x; };
      if (m.body_depth[b] > 16) { err = "kinematic trees deeper than 16 bodies are not supported"; return false; }
      r[4] = fi(m.body_depth[b] | (up(b, 2) << 8) | (up(b, 4) << 16) | (up(b, 8) << 24));
    }
    r[5] = fi(tp.treeid[b]); r[6] = (float)m.body_mass[b]; r[7] = fi(tp.childnum[b]);
    for (int i = 0; i < 3; i++) { r[8 + i] = (float)m.body_pos[3 * b + i]; r[16 + i] = (float)m.body_ipos[3 * b + i]; r[24 + i] = (float)m.body_inertia[3 * b + i]; }
    for (int i = 0; i < 4; i++) { r[12 + i] = (float)m.body_quat[4 * b + i]; r[20 + i] = (float)m.body_iquat[4 * b + i]; }
    for (int c = 0; c < 8; c++) r[28 + c] = fi(c < tp.childnum[b] ? tp.child_list[tp.childadr[b] + c] : 0);
    for (int jj = 0; jj < m.body_jntnum[b]; jj++) {
      int j = m.body_jntadr[b] + jj;
      float* q = r + 36 + 12 * jj;
      q[0] = fi(m.jnt_type[j]); q[1] = fi(m.jnt_qposadr[j]); q[2] = fi(m.jnt_dofadr[j]); q[3] = (float)m.qpos0[m.jnt_qposadr[j]];
      for (int i = 0; i < 3; i++) { q[4 + i] = (float)m.jnt_axis[3 * j + i]; q[8 + i] = (float)m.jnt_pos[3 * j + i]; }
    }
  }
  return true;
}
struct DofTables { std::vector<float> drec, mdiag; std::vector<int> mrec; };
void dof_records(const Model& m, const Topology& tp, DofTables& D) {
  const int nv = m.nv;
  D.drec.assign((size_t)nv * 12, 0.f);
  for (int d = 0; d < nv; d++) {
    int j = m.dof_jntid[d], b = m.dof_bodyid[d];
    float* r = &D.drec[(size_t)d * 12];
    r[0] = fi(j); r[1] = fi(b); r[2] = fi(m.jnt_type[j]); r[3] = fi(d - m.jnt_dofadr[j]);
    r[4] = fi(tp.treeid[b]); r[5] = (float)m.dof_armature[d]; r[6] = (float)m.dof_damping[d]; r[7] = (float)m.jnt_stiffness[j];
    r[8] = fi(m.jnt_qposadr[j]); r[9] = (float)m.qpos_spring[m.jnt_qposadr[j]];
  }
  D.mrec.assign(m.nM, 0);
  D.mdiag.assign((size_t)m.nM * 2, 0.f);
  for (int e = 0; e < m.nM; e++) {
    D.mrec[e] = tp.Mi[e] | (tp.Mj[e] << 8) | (m.dof_bodyid[tp.Mi[e]] << 16);
    if (tp.Mi[e] == tp.Mj[e]) { D.mdiag[2 * e] = (float)m.dof_armature[tp.Mi[e]]; D.mdiag[2 * e + 1] = (float)m.dof_damping[tp.Mi[e]]; }
  }
}
// per actuator its joint's addresses and one 4-quad record: [0] ctrllimited, forcelimited, qpos address, dof address   [1] ctrlrange[2], gear, gain
// [2] biasprm[0..2], -   [3] forcerange[2], -, -;  per wrap its joint's addresses, and per fixed tendon its first four wraps in one 3-quad
// record (a tendon with more falls back to the wrap tables): [0] coefficients   [1] qpos addresses   [2] dof addresses; unused slots have
// coefficient 0 and address 0
struct ActTendonTables {
  std::vector<int> wrap_dofadr, wrap_qposadr, act_qposadr, act_dofadr;
  std::vector<float> arec, trec;
};
void actuator_tendon_records(const Model& m, ActTendonTables& A) {
  for (int w = 0; w < m.nwrap; w++) { A.wrap_dofadr.push_back(m.jnt_dofadr[m.wrap_objid[w]]); A.wrap_qposadr.push_back(m.jnt_qposadr[m.wrap_objid[w]]); }
  for (int a = 0; a < m.nu; a++) { A.act_qposadr.push_back(m.jnt_qposadr[m.actuator_trnid[a]]); A.act_dofadr.push_back(m.jnt_dofadr[m.actuator_trnid[a]]); }
  A.trec.assign((size_t)std::max(1, m.ntendon) * 12, 0.f);
  for (int t = 0; t < m.ntendon; t++)
    for (int w = 0; w < std::min(4, m.tendon_num[t]); w++) {
      const int a = m.tendon_adr[t] + w;
      A.trec[(size_t)t * 12 + w] = (float)m.wrap_prm[a];
      A.trec[(size_t)t * 12 + 4 + w] = fi(A.wrap_qposadr[a]);
      A.trec[(size_t)t * 12 + 8 + w] = fi(A.wrap_dofadr[a]);
    }
  A.arec.assign((size_t)std::max(1, m.nu) * 16, 0.f);
  for (int a = 0; a < m.nu; a++) {
    float* r = &A.arec[(size_t)a * 16];
    r[0] = fi(m.actuator_ctrllimited[a]); r[1] = fi(m.actuator_forcelimited[a]); r[2] = fi(A.act_qposadr[a]); r[3] = fi(A.act_dofadr[a]);
    r[4] = (float)m.actuator_ctrlrange[2 * a]; r[5] = (float)m.actuator_ctrlrange[2 * a + 1]; r[6] = (float)m.actuator_gear[a]; r[7] = (float)m.actuator_gainprm[a];
    for (int i = 0; i < 3; i++) r[8 + i] = (float)m.actuator_biasprm[3 * a + i];
    r[12] = (float)m.actuator_forcerange[2 * a]; r[13] = (float)m.actuator_forcerange[2 * a + 1];
  }
}

// ---- always-active rows, equalities (mj_instantiateEquality): the rows in front of the friction rows, in the order of the model's
// equalities - one per active joint coupling, three (world x, y, z) per active connect - unless the options disable them: then the model
// is an ordinary one.  Per row a 7-quad record (kErecQuads):
//   joint:    [0] 0, -, qposadr1, qposadr2 (-1: none)   [1] dof1, dof2, qpos0 of joint1, of joint2   [2] polycoef[0..3]   [3] polycoef[4]
//   connect:  [0] 1, axis, body1, body2   [1] tree1, tree2   [2] dof mask of body1 (lo, hi), of body2 (lo, hi)   [3] anchor in body1's frame
//             [4].xyz anchor in body2's frame
//   both:     [4].w diagApprox   [5] solref[2], solimp[0..1]   [6] solimp[2..4]
bool equality_rows(const Model& m, const Topology& tp, DevModel& dm, std::vector<float>& erec, std::string& err) {
  if (!(m.disableflags & (DSBL_CONSTRAINT | DSBL_EQUALITY))) {
    for (int e = 0; e < m.neq(); e++) {
      if (!m.eq_active0[e]) continue;
      const double* d = &m.eq_data[(size_t)kEqData * e];
      const int o1 = m.eq_obj1id[e], o2 = m.eq_obj2id[e];
      const int nrow = m.eq_type[e] == EQ_JOINT ? 1 : 3;
      for (int a = 0; a < nrow; a++) {
        float r[4 * kErecQuads] = {0};
        if (m.eq_type[e] == EQ_JOINT) {
          const int q1 = m.jnt_qposadr[o1], q2 = o2 >= 0 ? m.jnt_qposadr[o2] : -1;
          r[0] = fi(0); r[2] = fi(q1); r[3] = fi(q2);
          r[4] = fi(m.jnt_dofadr[o1]); r[5] = fi(o2 >= 0 ? m.jnt_dofadr[o2] : 0); r[6] = (float)m.qpos0[q1]; r[7] = o2 >= 0 ? (float)m.qpos0[q2] : 0.f;
          for (int i = 0; i < 5; i++) r[8 + i] = (float)d[i];
          r[19] = (float)(m.dof_invweight0[m.jnt_dofadr[o1]] + (o2 >= 0 ? m.dof_invweight0[m.jnt_dofadr[o2]] : 0.0));
        } else {
          r[0] = fi(1); r[1] = fi(a); r[2] = fi(o1); r[3] = fi(o2);
          r[4] = fi(tp.treeid[o1]); r[5] = fi(tp.treeid[o2]);
          put_mask(r + 8, tp.dofmask[o1]); put_mask(r + 10, tp.dofmask[o2]);
          for (int i = 0; i < 3; i++) { r[12 + i] = (float)d[i]; r[16 + i] = (float)d[3 + i]; }
          r[19] = (float)(m.body_invweight0[2 * o1] + m.body_invweight0[2 * o2]);
        }
        r[20] = (float)m.eq_solref[2 * e]; r[21] = (float)m.eq_solref[2 * e + 1];
        for (int i = 0; i < 5; i++) r[22 + i] = (float)m.eq_solimp[5 * e + i];
        erec.insert(erec.end(), r, r + 4 * kErecQuads);
      }
    }
  }
  dm.neq_rows = (int)erec.size() / (4 * kErecQuads);
  if (dm.neq_rows && dm.variant != 0) {
    err = "equality constraints: only models that step in one kernel (plane / sphere / capsule geoms, condim 1 / 3) are implemented; this model steps in stages (mesh hulls, height fields or condim 4 / 6): remove the <equality> section or set <flag equality=\"disable\"/>";
    return false;
  }
  if (dm.neq_rows && m.integrator == INT_RK4) { err = "equality constraints: the RK4 integrator is not implemented for a model with equality rows: use the Euler integrator"; return false; }
  if (dm.neq_rows && dm.neq_rows + dm.nfric > 32) {
    err = "equality constraints: " + std::to_string(dm.neq_rows) + " equality rows and " + std::to_string(dm.nfric) + " friction-loss rows: a model may have at most 32 always-active rows";
    return false;
  }
  if (erec.empty()) erec.assign(4 * kErecQuads, 0.f);
  return true;
}

}  // namespace

void set_layout(DevModel& dm, const LdsLayout& L) {
  dm.o_gquat = L.o_gquat; dm.o_meta = L.o_meta; dm.o_AR = L.o_AR;
  dm.o_qpos = L.o_qpos; dm.o_qvel = L.o_qvel; dm.o_warm = L.o_warm; dm.o_ctrl = L.o_ctrl; dm.o_gpos = L.o_gpos; dm.o_gaxis = L.o_gaxis; dm.o_scom = L.o_scom;
  dm.o_cdof = L.o_cdof; dm.o_qLD = L.o_qLD; dm.o_smooth = L.o_smooth; dm.o_vec0 = L.o_vec0; dm.o_vec1 = L.o_vec1; dm.o_vec2 = L.o_vec2; dm.o_tenlen = L.o_tenlen;
  dm.o_xpos = L.o_xpos; dm.o_xmat = L.o_xmat; dm.o_xipos = L.o_xipos; dm.o_xanchor = L.o_xanchor; dm.o_xaxis = L.o_xaxis; dm.o_cinert = L.o_cinert; dm.o_crb = L.o_crb;
  dm.o_cvel = L.o_cvel; dm.o_con = L.o_con; dm.o_C = L.o_C; dm.o_efc = L.o_efc; dm.o_force = L.o_force;
  dm.lds_floats = L.lds_floats; dm.cstride = L.cstride; dm.o_rk = L.o_rk;
}

bool model_variant(const Model& m, int& variant, int& ncon_max, int& nefc_max, std::string& err) {
  bool general = false, wide = false;  // wide: a pair of contact dimension 4 / 6 (six / ten pyramid rows per contact)
  for (int p = 0; p < m.npair; p++) {
    const int g1 = m.pair_geom1[p], g2 = m.pair_geom2[p];
    const int t1 = m.geom_type[g1], t2 = m.geom_type[g2];
    if (t1 == GEOM_MESH || t2 == GEOM_MESH || t1 == GEOM_HFIELD || t2 == GEOM_HFIELD || t1 == GEOM_BOX || t2 == GEOM_BOX) general = true;
    const int dim = pair_condim(m, g1, g2);
    if (dim != 1 && dim != 3) { general = true; wide = true; }
  }
  variant = 0; ncon_max = kNconMax; nefc_max = kNefcMax;
  if (!general) return true;
  if (m.nv > 28) { err = "models with mesh geoms, height fields or condim 4 / 6 support at most 28 degrees of freedom in this build"; return false; }
  if (m.npair > 65535) { err = "general collision: more than 65535 candidate pairs"; return false; }  // (packed work-item words, hb_pose_kernel)
  for (int h = 0; h < m.nhfield; h++)
    if (m.hfield_nrow[h] > 32767 || m.hfield_ncol[h] > 32767) { err = "height fields larger than 32767 x 32767 are not supported"; return false; }
  if (m.solver == SOL_NEWTON) { variant = 2; ncon_max = kBigNconMax; nefc_max = kBigNefcMax; }
  else if (wide) { variant = 3; ncon_max = kBigNconMax; nefc_max = kPgsNefcMax; }  // PGS with six / ten rows per contact: kPgsNefcMax rows, AR in LDS
  else variant = 1;
  return true;
}

int model_nobs(const Model& m) {
  int nscalar = 0;
  for (int j = 0; j < m.njnt; j++) if (is_scalar_joint(m, j)) nscalar++;
  return 2 * nscalar + 6;
}

bool build_model_tables(const Model& m, HostTables& H, std::string& err) {
  H = HostTables{};
  DevModel& dm = H.dm;
  // the steps in the order their refusals are reported: a model that breaks two rules gets the message of the first
  std::vector<float> frec, erec, brec;
  Topology tp; Pairs P; Limits L; ObsTables O; DofTables D; ActTendonTables A; MeshTables M;
  if (!validate_model(m, dm, err) || !friction_rows(m, dm, frec, err) || !build_topology(m, dm, tp, err) || !layout_for(m, dm, H.lay, err) || !mix_pairs(m, P, err)) return false;
  build_limits(m, dm, L);
  actuator_tendon_records(m, A);
  build_obs(m, dm, O);
  if (!body_records(m, tp, brec, err)) return false;
  dof_records(m, tp, D);

  // ---- the flat tables: every array goes in here, and every pointer field of DevModel gets its fix-up here
#define TAB(field, array, add, to, vec) do { const auto& v_ = (vec); H.fix.push_back({offsetof(DevModel, field), array, add(to, v_), #field, v_.size()}); } while (0)
#define TI(field, vec) TAB(field, kTabInt, addi, H.iv, vec)
#define TF(field, vec) TAB(field, kTabFloat, addf, H.fv, vec)
#define TR(field, vec) TAB(field, kTabFloat, addraw, H.fv, vec)
  TI(body_treeid, tp.treeid); TF(body_invweight0, m.body_invweight0); TF(tree_invmass, tp.tree_invmass);
  TI(jnt_type, m.jnt_type); TI(jnt_qposadr, m.jnt_qposadr); TI(jnt_dofadr, m.jnt_dofadr); TF(qpos0, m.qpos0); TI(dof_jntid, m.dof_jntid); TI(dof_Madr, m.dof_Madr); TF(dof_damping, m.dof_damping); TI(mrec, D.mrec);
  TI(mdense, tp.mdense); TI(mdense_c, tp.mdense_c);
  TI(geom_type, m.geom_type); TI(geom_bodyid, m.geom_bodyid); TI(geom_dataid, m.geom_dataid);
  std::vector<int> geom_meshadr(m.ngeom, 0), geom_meshnum(m.ngeom, 0);
  for (int g = 0; g < m.ngeom; g++)
    if (m.geom_type[g] == GEOM_MESH) { geom_meshadr[g] = m.mesh_vertadr[m.geom_dataid[g]]; geom_meshnum[g] = m.mesh_vertnum[m.geom_dataid[g]]; }
  TI(geom_meshadr, geom_meshadr); TI(geom_meshnum, geom_meshnum);
  TI(hfield_nrow, m.hfield_nrow); TI(hfield_ncol, m.hfield_ncol); TI(hfield_adr, m.hfield_adr); TF(hfield_size, m.hfield_size); TF(hfield_data, m.hfield_data);
  TF(geom_size, m.geom_size); TF(geom_pos, m.geom_pos); TF(geom_quat, m.geom_quat); TF(geom_rbound, m.geom_rbound);
  TF(geom_half, geom_half_extents(m));
  dm.box_cull = !(getenv("HB_BOX_CULL") && atoi(getenv("HB_BOX_CULL")) == 0);
  dm.has_box = 0;
  for (int p = 0; p < m.npair; p++) if (m.geom_type[m.pair_geom1[p]] == GEOM_BOX || m.geom_type[m.pair_geom2[p]] == GEOM_BOX) dm.has_box = 1;
  // (the mode counts only where it changes something: a model without a box - box candidate pair builds the tables it built before)
  dm.box_manifold = 0;
  if (m.box_manifold) for (int p = 0; p < m.npair; p++) if (m.geom_type[m.pair_geom1[p]] == GEOM_BOX && m.geom_type[m.pair_geom2[p]] == GEOM_BOX) dm.box_manifold = 1;
  TI(pair_geom1, m.pair_geom1); TI(pair_geom2, m.pair_geom2); TI(pair_dim, P.dim); TI(pair_self, P.self);
  TF(pair_fricab, P.fricab);
  TF(pair_friction, P.fr); TF(pair_solref, P.solref); TF(pair_solimp, P.solimp); TF(pair_margin, P.margin); TF(pair_gap, P.gap);
  TI(lim_kind, L.kind); TI(lim_id, L.id); TI(lim_side, L.side);
  TF(lim_range, L.range); TF(lim_margin, L.margin); TF(lim_solref, L.solref); TF(lim_solimp, L.solimp); TF(lim_invweight, L.invw);
  TI(obs_src, O.src); TI(obs_jnt, O.jnt);
  H.has_act_order = O.has_act_order;
  H.o_obs_jnt_act = addi(H.iv, O.jnt_act.empty() ? std::vector<int>{0} : O.jnt_act); H.o_obs_src_act = addi(H.iv, O.src_act.empty() ? std::vector<int>{0} : O.src_act);
  TI(tendon_adr, m.tendon_adr); TI(tendon_num, m.tendon_num); TI(wrap_dofadr, A.wrap_dofadr); TI(wrap_qposadr, A.wrap_qposadr);
  TF(wrap_prm, m.wrap_prm);
  TI(act_qposadr, A.act_qposadr); TI(act_dofadr, A.act_dofadr); TI(act_ctrllimited, m.actuator_ctrllimited); TI(act_forcelimited, m.actuator_forcelimited);
  TF(act_gear, m.actuator_gear); TF(act_ctrlrange, m.actuator_ctrlrange); TF(act_forcerange, m.actuator_forcerange); TF(act_gain, m.actuator_gainprm);
  TF(act_bias, m.actuator_biasprm);
  TAB(body_dofmask, kTabU64, addu, H.uv, tp.dofmask);
  if (!equality_rows(m, tp, dm, erec, err) || !mesh_tables(m, M, err)) return false;
  TR(mesh_vert, M.vert); TR(mesh_nbr, M.nbr); TR(mesh_start, M.start);
  TR(arec, A.arec);
  TR(brec, brec); TR(drec, D.drec); TR(mdiag, D.mdiag); TR(prec, pair_records(m, tp, P)); TR(crec, collision_records(m, P)); TR(trec, A.trec);
  TR(lrec, L.lrec); TR(frec, frec); TR(erec, erec);
#undef TI
#undef TF
#undef TR
#undef TAB

  for (double v : m.qpos0) H.qsrc.push_back((float)v);
  for (double v : m.key_qpos) H.qsrc.push_back((float)v);
  // the size-specialised kernels (hb_step_h27_kernel and its kin): the model's sizes and the layout computed above against the constant's
  H.sized_h27 = (dm.variant == 0 || (dm.variant == 1 && dm.solver == 0)) && sized_as(m, dm, dm.variant == 1 ? kSizedHumanoid27V1 : kSizedHumanoid27, H.lay);
  // A variant-2 model (Newton on 256 rows in four register groups: one wave per SIMD) almost always has at most 63 rows and 24
  // contacts in a step: its staged step first runs the one-group Newton instantiation (two waves per SIMD) on the variant-1 LDS
  // layout and falls back to the four-group kernel for the envs that overflow (launch_step).  Same tables, other offsets.
  if (dm.variant == 2 || dm.variant == 3) {
    DevModel fm = dm;
    fm.variant = 1; fm.ncon_max = kNconMax; fm.nefc_max = kNefcMax;
    if (!layout_for(m, fm, H.fast_lay, err)) return false;
    H.fast_lds_floats = fm.lds_floats;
    H.sized_team = dm.variant == 2 && sized_as(m, dm, kSizedTeamV1, H.fast_lay);  // (the robot's fast layout: hb_step_newton_gen20_team_kernel)
  }
  return true;
}

}  // namespace hb
