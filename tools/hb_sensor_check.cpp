// hb_sensor_check - sensor_args (humanoid_mujoco_amd/csrc/hb_api_rollout.cpp: a spec checked, its row laid out, its tables filled) run on
// the host for a model file (no GPU: the function needs no batch; unreferenced code of its unit is dropped at link time).  Meant to be
// built with -fsanitize=address,undefined as well: make build/hb_sensor_check_san.
// usage: hb_sensor_check humanoid27.hbm
// It checks that
//   - the rows of the walk and stand tasks' specs with their tails have the offsets those tasks wrote as literals before the layout was
//     stated once (walk: 0 3 6 9 | 12 15 | 18 | 42 | 51 | qpos 54 | ctrl 54 + nq; stand: 0 3 | 15 18 | qvel 21 | ctrl 21 + nv);
//   - the tables hold the spec's bodies, offsets and axes, the tree's index and the subtree's bodies and mass;
//   - two records built from equal inputs are equal byte for byte, whatever the memory held before;
//   - every spec the function refuses is refused with its code, counts before the unsupported read-out before bodies.
// Prints "ok <case>" per case; exit 0, or 1 at the first failure.
#include "../humanoid_mujoco_amd/csrc/hb_batch.hpp"
#include "../humanoid_mujoco_amd/csrc/hb_tables.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace hb;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s fails (%s)\n", __FILE__, __LINE__, #c, what); exit(1); } } while (0)
static const char* what = "";

static int body(const Model& m, const char* name) {
  for (int b = 0; b < m.nbody; b++) if (m.body_name[b] == name) return b;
  fprintf(stderr, "no body %s\n", name);
  exit(1);
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s model.hbm\n", argv[0]); return 2; }
  Model m;
  std::string err;
  if (!load_hbm(argv[1], m, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
  HostTables H;
  if (!build_model_tables(m, H, err)) { fprintf(stderr, "refused: %s\n", err.c_str()); return 2; }
  const DevModel& dm = H.dm;
  const int nq = dm.nq, nv = dm.nv, nu = dm.nu;
  const int torso = body(m, "torso"), pelvis = body(m, "pelvis"), foot_r = body(m, "foot_right"), foot_l = body(m, "foot_left"), waist = body(m, "waist_lower"),
            head = body(m, "head");
  // two records in memory that held different bytes before
  SensorArgs A, B;
  memset(&A, 0x5a, sizeof A); memset(&B, 0xa5, sizeof B);

  what = "walk";  // hb_rollout_task_walk's spec: 4 framepos, the torso's tree, 8 axes, 3 linvel, 1 subtreelinvel, qpos | ctrl
  hb_sensor_spec walk;
  memset(&walk, 0, sizeof walk);
  const int fp[4] = {torso, foot_r, foot_l, pelvis}, axb[4] = {torso, pelvis, foot_r, foot_l};
  walk.n_framepos = 4;
  for (int k = 0; k < 4; k++) { walk.framepos_body[k] = fp[k]; for (int i = 0; i < 3; i++) walk.framepos_offset[k][i] = (float)m.body_ipos[3 * fp[k] + i]; }
  walk.subtree_body = torso;
  walk.n_frameaxis = 8;
  for (int k = 0; k < 4; k++) { walk.frameaxis_body[k] = axb[k]; walk.frameaxis_which[k] = 2; walk.frameaxis_body[4 + k] = axb[k]; walk.frameaxis_which[4 + k] = 0; }
  walk.n_framelinvel = 3;
  walk.framelinvel_body[0] = torso; walk.framelinvel_body[1] = foot_r; walk.framelinvel_body[2] = foot_l;
  walk.n_subtreelinvel = 1;
  walk.subtreelinvel_body[0] = waist;
  CHECK(sensor_args(m, dm, &walk, kSensorQpos | kSensorCtrl, A) == HB_OK);
  {
    const SensorRow& R = A.row;
    CHECK(R.framepos == 0 && R.subtree == 12);
    CHECK(R.axis == 18 && R.linvel == 42 && R.sub == 51 && R.width == 54 && hb_sensor_size(&walk) == 54);
    CHECK(R.qpos == 54 && R.n_qpos == nq && R.n_qvel == 0 && R.ctrl == 54 + nq && R.n_ctrl == nu && R.stride == 54 + nq + nu);
    CHECK(R.n_framepos == 4 && R.n_subtree == 1 && R.n_axis == 8 && R.n_linvel == 3 && R.n_sub == 1 && R.n_touch + R.n_cfrc + R.n_imu + R.n_facc == 0);
    CHECK(R.touch == 54 && R.cfrc == 54 && R.imu == 54 && R.facc == 54);  // (parts that are off: where they would begin)
    CHECK(A.out == nullptr && A.tree == 0);
    for (int k = 0; k < 4; k++) {
      CHECK(A.body[k] == fp[k] && A.axis_body[k] == axb[k] && (A.axis_which >> (2 * k) & 3) == 2 && A.axis_body[4 + k] == axb[k] && (A.axis_which >> (2 * (4 + k)) & 3) == 0);
      for (int i = 0; i < 3; i++) CHECK(A.off[k][i] == (float)m.body_ipos[3 * fp[k] + i]);
    }
    CHECK(A.linvel_body[0] == torso && A.linvel_body[1] == foot_r && A.linvel_body[2] == foot_l);
    unsigned long long mask = 0;
    double mass = 0;
    for (int b = 1; b < m.nbody; b++) {
      int a = b;
      while (a > 0 && a != waist) a = m.body_parentid[a];
      if (a == waist) { mask |= 1ull << b; mass += m.body_mass[b]; }
    }
    CHECK(A.submask[0] == mask && (mask >> waist & 1) && !(mask >> torso & 1) && A.subinv[0] == (float)(1.0 / mass));
  }
  CHECK(sensor_args(m, dm, &walk, kSensorQpos | kSensorCtrl, B) == HB_OK && memcmp(&A, &B, sizeof A) == 0);
  puts("ok walk");

  what = "stand";  // hb_rollout_task_stand's spec: head and four foot sites, the torso's tree, qvel | ctrl
  hb_sensor_spec stand;
  memset(&stand, 0, sizeof stand);
  stand.n_framepos = 5;
  stand.framepos_body[0] = head;
  for (int k = 0; k < 4; k++) { stand.framepos_body[1 + k] = k < 2 ? foot_l : foot_r; stand.framepos_offset[1 + k][0] = k % 2 ? 0.14f : -0.07f; }
  stand.subtree_body = torso;
  CHECK(sensor_args(m, dm, &stand, kSensorQvel | kSensorCtrl, A) == HB_OK);
  {
    const SensorRow& R = A.row;
    CHECK(R.framepos == 0 && R.subtree == 15 && R.width == 21 && hb_sensor_size(&stand) == 21);
    CHECK(R.n_qpos == 0 && R.qvel == 21 && R.n_qvel == nv && R.ctrl == 21 + nv && R.n_ctrl == nu && R.stride == 21 + nv + nu);
    CHECK(A.body[0] == head && A.body[2] == foot_l && A.body[3] == foot_r && A.off[2][0] == 0.14f && A.off[3][0] == -0.07f && A.off[3][1] == 0.f);
  }
  CHECK(sensor_args(m, dm, &stand, kSensorQvel | kSensorCtrl, B) == HB_OK && memcmp(&A, &B, sizeof A) == 0);
  CHECK(sensor_args(m, dm, &stand, 0, B) == HB_OK && B.row.stride == 21 && B.row.qpos == 21 && B.row.qvel == 21 && B.row.ctrl == 21);
  puts("ok stand");

  what = "contact and acceleration parts";
  hb_sensor_spec full = stand;
  full.n_touch = 2; full.touch_body[0] = foot_r; full.touch_body[1] = foot_l;
  full.n_contactforce = 1; full.contactforce_body[0] = torso;
  full.n_imu = 2; full.imu_body[0] = torso; full.imu_body[1] = head; full.imu_offset[1][2] = 0.1f;
  full.n_frameacc = 1; full.frameacc_body[0] = pelvis;
  CHECK(sensor_args(m, dm, &full, 0, A) == HB_OK);
  CHECK(A.row.touch == 21 && A.row.cfrc == 23 && A.row.imu == 26 && A.row.facc == 38 && A.row.width == 44 && A.row.stride == 44);
  CHECK(A.touch_body[1] == foot_l && A.cfrc_body[0] == torso && A.imu_body[1] == head && A.imu_off[1][2] == 0.1f && A.imu_off[0][2] == 0.f && A.facc_body[0] == pelvis);
  puts("ok contact and acceleration parts");

  what = "refusals";
  const auto rc = [&](const hb_sensor_spec& s, const DevModel& d) { return sensor_args(m, d, &s, 0, B); };
  hb_sensor_spec s;
  CHECK(sensor_args(m, dm, nullptr, 0, B) == HB_EINVAL);
  memset(&s, 0, sizeof s); s.subtree_body = -1;
  CHECK(rc(s, dm) == HB_EINVAL);  // nothing to read
  // counts
  s = full; s.n_framepos = 17; CHECK(rc(s, dm) == HB_EINVAL);
  s = full; s.n_framepos = -1; CHECK(rc(s, dm) == HB_EINVAL);
  s = full; s.n_frameaxis = 9; CHECK(rc(s, dm) == HB_EINVAL);
  s = full; s.n_framelinvel = 9; CHECK(rc(s, dm) == HB_EINVAL);
  s = full; s.n_subtreelinvel = 5; CHECK(rc(s, dm) == HB_EINVAL);
  s = full; s.n_touch = 9; CHECK(rc(s, dm) == HB_EINVAL);
  s = full; s.n_contactforce = 5; CHECK(rc(s, dm) == HB_EINVAL);
  s = full; s.n_imu = 5; CHECK(rc(s, dm) == HB_EINVAL);
  s = full; s.n_frameacc = 5; CHECK(rc(s, dm) == HB_EINVAL);
  // body ranges (framelinvel and subtreelinvel: not the world either)
  s = full; s.framepos_body[4] = m.nbody; CHECK(rc(s, dm) == HB_EINVAL);
  s = full; s.framepos_body[0] = -1; CHECK(rc(s, dm) == HB_EINVAL);
  s = walk; s.frameaxis_body[7] = m.nbody; CHECK(rc(s, dm) == HB_EINVAL);
  s = walk; s.framelinvel_body[2] = 0; CHECK(rc(s, dm) == HB_EINVAL);
  s = walk; s.framelinvel_body[0] = m.nbody; CHECK(rc(s, dm) == HB_EINVAL);
  s = walk; s.subtreelinvel_body[0] = 0; CHECK(rc(s, dm) == HB_EINVAL);
  s = walk; s.subtreelinvel_body[0] = m.nbody; CHECK(rc(s, dm) == HB_EINVAL);
  s = full; s.touch_body[1] = m.nbody; CHECK(rc(s, dm) == HB_EINVAL);
  s = full; s.contactforce_body[0] = -1; CHECK(rc(s, dm) == HB_EINVAL);
  s = full; s.imu_body[1] = m.nbody; CHECK(rc(s, dm) == HB_EINVAL);
  s = full; s.frameacc_body[0] = m.nbody; CHECK(rc(s, dm) == HB_EINVAL);
  // a body that is no tree root, the world, a body past the end; the `which` of an axis
  s = full; s.subtree_body = pelvis; CHECK(m.body_parentid[pelvis] != 0 && rc(s, dm) == HB_EINVAL);
  s = full; s.subtree_body = 0; CHECK(rc(s, dm) == HB_EINVAL);
  s = full; s.subtree_body = m.nbody; CHECK(rc(s, dm) == HB_EINVAL);
  s = walk; s.frameaxis_which[3] = 1; CHECK(rc(s, dm) == HB_EINVAL);
  s = walk; s.frameaxis_which[3] = 3; CHECK(rc(s, dm) == HB_EINVAL);
  // accelerometer / frame-acceleration entries on a model with friction-loss or equality rows; without them such a model is served
  DevModel fric = dm, eq = dm;
  fric.nfric = 1; eq.neq_rows = 3;
  CHECK(rc(full, fric) == HB_EUNSUPPORTED && rc(full, eq) == HB_EUNSUPPORTED && rc(stand, fric) == HB_OK && rc(walk, eq) == HB_OK);
  s = full; s.n_imu = 0; CHECK(rc(s, fric) == HB_EUNSUPPORTED);
  s = full; s.n_imu = 0; s.n_frameacc = 0; CHECK(rc(s, eq) == HB_OK);
  // several faults: counts, then the unsupported read-out, then bodies
  s = full; s.n_touch = 9; s.framepos_body[0] = -1; CHECK(rc(s, fric) == HB_EINVAL);
  s = full; s.framepos_body[0] = -1; s.subtree_body = pelvis; CHECK(rc(s, fric) == HB_EUNSUPPORTED && rc(s, dm) == HB_EINVAL);
  puts("ok refusals");
  return 0;
}
