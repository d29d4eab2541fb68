// hb_tables.hpp — the device model tables as the host builds them: everything build_device_model (hb_batch.cpp) uploads, worked out
// from a Model without a GPU.  Plain C++: no HIP runtime call on this side of the upload.
#pragma once
#include "hb_device.hpp"
#include "hb_model.hpp"
#include <string>
#include <vector>

namespace hb {

// One pointer field of DevModel: where the field sits in the struct, which flat array it points into and at which element.
enum { kTabInt = 0, kTabFloat = 1, kTabU64 = 2 };
struct TableFixup {
  size_t field;  // byte offset of the pointer in DevModel
  int array;     // kTabInt / kTabFloat / kTabU64
  size_t off;    // element offset into that array
  const char* name;  // the field's name, and how many elements the table has (an empty one still takes one element of the array)
  size_t count;
};

struct HostTables {
  DevModel dm;  // every pointer field null: the upload sets them from `fix`
  std::vector<int> iv;
  std::vector<float> fv;
  std::vector<unsigned long long> uv;
  std::vector<TableFixup> fix;
  std::vector<float> qsrc;  // qpos0 followed by keyframes, fp32
  // observation order tables: dm.obs_jnt / dm.obs_src are the joint order; when every scalar joint has exactly one actuator, the actuator
  // order (hb_env_config.obs_actuator_order) sits at these offsets of iv
  bool has_act_order = false;
  size_t o_obs_jnt_act = 0, o_obs_src_act = 0;
  LdsLayout lay;  // the layout that went into dm
  // variants 2 / 3: the variant-1 layout of the fast step kernel (the fast DevModel is dm with variant 1, kNconMax, kNefcMax and these offsets)
  LdsLayout fast_lay;
  int fast_lds_floats = 0;  // 0: no fast model
  bool sized_h27 = false;   // sizes and LDS layout equal kSizedHumanoid27's: the size-specialised step kernel applies
  bool sized_team = false;  // the fast layout equals kSizedTeamV1's
};

// a layout into a DevModel's o_* fields (the one place that does it)
void set_layout(DevModel& dm, const LdsLayout& L);

// false: the model is refused, err says why
bool build_model_tables(const Model& m, HostTables& H, std::string& err);

// Which instantiation of the step kernel a model needs (DevModel::variant): the classic one handles plane / sphere / capsule pairs
// with condim 1 / 3; a mesh geom, a height field or a condim 4 / 6 pair takes the general collision + constraint assembly, with PGS on
// 63 rows or Newton on kBigNefcMax rows.  false: no instantiation fits.
bool model_variant(const Model& m, int& variant, int& ncon_max, int& nefc_max, std::string& err);

// hinge or slide: one qpos, one dof, two observation entries
inline bool is_scalar_joint(const Model& m, int j) { return m.jnt_type[j] == JNT_HINGE || m.jnt_type[j] == JNT_SLIDE; }
// observation width of the env adapter: qpos and qvel of the scalar joints, the root's angular velocity and projected gravity
int model_nobs(const Model& m);

}  // namespace hb
