// hb_api_dyn.cpp — the C-ABI of libhb.so (include/hb.h), the dynamics read-out: mass matrix, bias and passive forces and Jacobians of the
// batch's state or of given states (the kernel is hb_dyn.hip).
#include "hb_batch.hpp"

namespace {

struct DynOut { float *M, *bias, *passive, *jac; };

// what every form checks: some output, jac and spec together and the spec's entries in range, velocities where an output needs them
bool dyn_args_ok(const hb_batch* b, const DynOut& o, const hb_jac_spec* spec, bool have_qvel) {
  if (!b || (!o.M && !o.bias && !o.passive && !o.jac) || (o.jac != nullptr) != (spec != nullptr)) return false;
  if ((o.bias || o.passive) && !have_qvel) return false;
  if (spec) {
    if (spec->n < 1 || spec->n > HB_MAX_JAC) return false;
    for (int k = 0; k < spec->n; k++)
      if (spec->body[k] < 0 || spec->body[k] >= b->D.dm.nbody || (spec->kind[k] != HB_JAC_POINT && spec->kind[k] != HB_JAC_SUBTREE_COM)) return false;
  }
  return true;
}

// one launch on `stream`; dr: the per-env parameters of the batch's own state, null for given states
int dynamics_launch(hb_batch* b, const float* qpos, const float* qvel, int qpos_stride, int qvel_stride, long long n, const float* dr, const DynOut& o,
                    const hb_jac_spec* spec, hipStream_t stream) {
  static_assert(HB_MAX_JAC == kJacMax, "hb_jac_spec and DynArgs hold the same number of points");
  DynArgs A;
  memset(&A, 0, sizeof A);
  A.qpos = qpos; A.qvel = qvel; A.qpos_stride = qpos_stride; A.qvel_stride = qvel_stride; A.n = n;
  A.dr = dr; A.dr_stride = dr ? b->dr_stride : 0;
  A.M = o.M; A.bias = o.bias; A.passive = o.passive; A.jac = o.jac;
  if (spec) {
    A.njac = spec->n;
    for (int k = 0; k < spec->n; k++) {
      A.jkind[k] = spec->kind[k]; A.jbody[k] = spec->body[k];
      for (int i = 0; i < 3; i++) A.joff[k][i] = spec->kind[k] == HB_JAC_POINT ? spec->offset[k][i] : 0.f;
    }
  }
  HB_HIP(launch_dynamics(b->D.d_dm, b->D.dm, A, b->tune[HB_TUNE_KIN_PACK], stream, &b->last_kernel));
  return HB_OK;
}

// host form: the outputs asked for (and qpos / qvel when given) staged in d_dyn, one launch, copied back
int dynamics_host(hb_batch* b, const float* qpos, const float* qvel, long long n, const DynOut& o, const hb_jac_spec* spec) {
  const DevModel& dm = b->D.dm;
  const size_t sn = (size_t)n;
  StageBlock blk[6] = {{o.M ? sn * dm.nv * dm.nv : 0, nullptr, o.M}, {o.bias ? sn * dm.nv : 0, nullptr, o.bias}, {o.passive ? sn * dm.nv : 0, nullptr, o.passive},
                       {o.jac ? sn * spec->n * 6 * dm.nv : 0, nullptr, o.jac}, {qpos ? sn * dm.nq : 0, qpos, nullptr}, {qpos && qvel ? sn * dm.nv : 0, qvel, nullptr}};
  const hipStream_t stream = main_stream(b);  // (held step calls launched, pipes joined)
  return staged_call(b->d_dyn, blk, 6, stream, [&] {
    const DynOut dev = {blk[0].dev, blk[1].dev, blk[2].dev, blk[3].dev};
    if (qpos) return dynamics_launch(b, blk[4].dev, blk[5].dev, dm.nq, dm.nv, n, nullptr, dev, spec, stream);
    return dynamics_launch(b, b->d_state + 1, b->d_state + 1 + dm.nq, dm.nstate, dm.nstate, n, b->d_dr, dev, spec, stream);
  });
}

}  // namespace

extern "C" {

int hb_dynamics_dev(hb_batch* b, float* M_dev, float* qfrc_bias_dev, float* qfrc_passive_dev, const hb_jac_spec* spec, float* jac_dev) {
  const DynOut o = {M_dev, qfrc_bias_dev, qfrc_passive_dev, jac_dev};
  if (!dyn_args_ok(b, o, spec, true)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  const hipStream_t stream = main_stream(b);  // (held step calls launched, pipes joined: the read-out sees the state they leave)
  const DevModel& dm = b->D.dm;
  return dynamics_launch(b, b->d_state + 1, b->d_state + 1 + dm.nq, dm.nstate, dm.nstate, b->n_env, b->d_dr, o, spec, stream);
}

int hb_dynamics(hb_batch* b, float* M, float* qfrc_bias, float* qfrc_passive, const hb_jac_spec* spec, float* jac) {
  const DynOut o = {M, qfrc_bias, qfrc_passive, jac};
  if (!dyn_args_ok(b, o, spec, true)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  return dynamics_host(b, nullptr, nullptr, b->n_env, o, spec);
}

int hb_dynamics_states_dev(hb_batch* b, const float* qpos_dev, const float* qvel_dev, int n, float* M_dev, float* qfrc_bias_dev, float* qfrc_passive_dev,
                           const hb_jac_spec* spec, float* jac_dev) {
  const DynOut o = {M_dev, qfrc_bias_dev, qfrc_passive_dev, jac_dev};
  if (!qpos_dev || n <= 0 || !dyn_args_ok(b, o, spec, qvel_dev != nullptr)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  const hipStream_t stream = main_stream(b);
  return dynamics_launch(b, qpos_dev, qvel_dev, b->D.dm.nq, b->D.dm.nv, n, nullptr, o, spec, stream);
}

int hb_dynamics_states(hb_batch* b, const float* qpos, const float* qvel, int n, float* M, float* qfrc_bias, float* qfrc_passive, const hb_jac_spec* spec, float* jac) {
  const DynOut o = {M, qfrc_bias, qfrc_passive, jac};
  if (!qpos || n <= 0 || !dyn_args_ok(b, o, spec, qvel != nullptr)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  return dynamics_host(b, qpos, qvel, n, o, spec);
}

}  // extern "C"
