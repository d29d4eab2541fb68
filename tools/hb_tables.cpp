// hb_tables — build the device model tables of a model on the host and print them (no GPU needed).
// usage: hb_tables in.xml|in.hbm [--solver PGS|Newton] [--integrator N] [--pair-order geom|body] [--dump FILE]
// (the options override the model after loading, as hb_options_set / hb_model_pair_order do)
// Prints one line per scalar field of DevModel ("name value"), per flat array ("array NAME length") and per table
// ("table NAME ARRAY offset count fnv1a64-of-its-bytes"), then the flags; exit 0.  A model the engine refuses: "refused: <message>", exit 1.
// --dump FILE writes the whole HostTables, little endian, every count and offset as u64:
//   "HBTABLE1" | sizeof(DevModel), its bytes (pointers null) | n, int[n] | n, float[n] | n, u64[n]
//   | n, n x (field offset, array, element offset) sorted by field offset | n, float[n] qpos sources
//   | has_act_order, o_obs_jnt_act, o_obs_src_act | sizeof(LdsLayout), the layout's bytes | the fast layout's bytes (zero: none), fast_lds_floats
//   | sized_h27, sized_team
#include "../humanoid_mujoco_amd/csrc/hb_tables.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace hb;

static unsigned long long fnv1a(const void* p, size_t n) {
  unsigned long long h = 1469598103934665603ull;
  for (size_t i = 0; i < n; i++) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; }
  return h;
}

static bool dump(const HostTables& H, const char* path) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  auto u64 = [&](unsigned long long v) { fwrite(&v, 8, 1, f); };
  auto raw = [&](const void* p, size_t n) { if (n) fwrite(p, 1, n, f); };
  raw("HBTABLE1", 8);
  u64(sizeof(DevModel)); raw(&H.dm, sizeof(DevModel));
  u64(H.iv.size()); raw(H.iv.data(), H.iv.size() * 4);
  u64(H.fv.size()); raw(H.fv.data(), H.fv.size() * 4);
  u64(H.uv.size()); raw(H.uv.data(), H.uv.size() * 8);
  std::vector<TableFixup> fix = H.fix;
  std::sort(fix.begin(), fix.end(), [](const TableFixup& a, const TableFixup& b) { return a.field < b.field; });
  u64(fix.size());
  for (const TableFixup& x : fix) { u64(x.field); u64(x.array); u64(x.off); }
  u64(H.qsrc.size()); raw(H.qsrc.data(), H.qsrc.size() * 4);
  u64(H.has_act_order); u64(H.o_obs_jnt_act); u64(H.o_obs_src_act);
  u64(sizeof(LdsLayout)); raw(&H.lay, sizeof(LdsLayout)); raw(&H.fast_lay, sizeof(LdsLayout)); u64(H.fast_lds_floats);
  u64(H.sized_h27); u64(H.sized_team);
  return fclose(f) == 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s in.xml|in.hbm [--solver PGS|Newton] [--integrator N] [--pair-order geom|body] [--dump FILE]\n", argv[0]); return 2; }
  Model m;
  std::string err, in = argv[1];
  const char* dump_path = nullptr;
  bool ok = in.size() > 4 && in.substr(in.size() - 4) == ".hbm" ? load_hbm(in, m, err) : compile_mjcf_file(in, m, err);
  if (!ok) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
  for (int i = 2; i + 1 < argc; i += 2) {
    if (!strcmp(argv[i], "--solver")) {
      if (!strcmp(argv[i + 1], "PGS")) m.solver = SOL_PGS;
      else if (!strcmp(argv[i + 1], "Newton")) m.solver = SOL_NEWTON;
      else { fprintf(stderr, "error: unknown solver %s\n", argv[i + 1]); return 2; }
    } else if (!strcmp(argv[i], "--integrator")) m.integrator = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--pair-order")) sort_pairs(m, !strcmp(argv[i + 1], "geom") ? 0 : 1);
    else if (!strcmp(argv[i], "--dump")) dump_path = argv[i + 1];
    else { fprintf(stderr, "error: unknown option %s\n", argv[i]); return 2; }
  }
  HostTables H;
  if (!build_model_tables(m, H, err)) { printf("refused: %s\n", err.c_str()); return 1; }
  const DevModel& dm = H.dm;
#define I(f) printf(#f " %d\n", dm.f);
#define F(f) printf(#f " %.9g\n", (double)dm.f);
  I(nq) I(nv) I(nu) I(nbody) I(njnt) I(ngeom) I(ntendon) I(nM) I(npair) I(nlevel) I(ntree) I(nlimcand) I(nhfielddata) I(nstate) I(nobs)
  I(variant) I(ncon_max) I(nefc_max) I(mpr_iterations) F(mpr_tolerance)
  F(timestep) F(gravity[0]) F(gravity[1]) F(gravity[2]) F(inv_sqrt_impratio) F(tolerance) F(pgs_scale)
  I(iterations) I(disableflags) I(solver) I(ls_iterations) F(ls_tolerance) I(box_cull) I(has_box) I(obs_root_body) I(obs_root_dofadr) I(obs_root_qadr)
  I(o_gquat) I(o_meta) I(o_AR) I(o_qpos) I(o_qvel) I(o_warm) I(o_ctrl) I(o_gpos) I(o_gaxis) I(o_scom) I(o_cdof) I(o_qLD) I(o_smooth) I(o_vec0) I(o_vec1) I(o_vec2) I(o_tenlen)
  I(o_xpos) I(o_xmat) I(o_xipos) I(o_xanchor) I(o_xaxis) I(o_cinert) I(o_crb) I(o_cvel) I(o_con) I(o_C) I(o_efc) I(o_force)
  I(lds_floats) I(cstride) I(integrator) I(o_rk) I(nfric) I(neq_rows) I(box_manifold)
#undef I
#undef F
  printf("array int %zu\narray float %zu\narray u64 %zu\n", H.iv.size(), H.fv.size(), H.uv.size());
  static const char* const array_name[3] = {"int", "float", "u64"};
  auto table = [&](const char* name, int array, size_t off, size_t count) {
    const void* p = array == kTabInt ? (const void*)(H.iv.data() + off) : array == kTabFloat ? (const void*)(H.fv.data() + off) : (const void*)(H.uv.data() + off);
    printf("table %s %s %zu %zu %016llx\n", name, array_name[array], off, count, fnv1a(p, count * (array == kTabU64 ? 8 : 4)));
  };
  for (const TableFixup& x : H.fix) table(x.name, x.array, x.off, x.count);
  const size_t nact = H.has_act_order ? (size_t)(dm.nobs - 6) / 2 : 0;
  table("obs_jnt_act", kTabInt, H.o_obs_jnt_act, nact);
  table("obs_src_act", kTabInt, H.o_obs_src_act, 2 * nact + 3);
  printf("qpos_src %zu %016llx\n", H.qsrc.size(), fnv1a(H.qsrc.data(), H.qsrc.size() * 4));
  printf("fast_lds_floats %d\nhas_act_order %d\nsized_h27 %d\nsized_team %d\n", H.fast_lds_floats, (int)H.has_act_order, (int)H.sized_h27, (int)H.sized_team);
  if (dump_path && !dump(H, dump_path)) { fprintf(stderr, "error: cannot write %s\n", dump_path); return 2; }
  return 0;
}
