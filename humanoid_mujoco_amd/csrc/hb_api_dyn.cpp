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
  auto r4 = [](size_t x) { return (x + 3) & ~(size_t)3; };  // (every block starts 16-byte aligned)
  const size_t nM = o.M ? (size_t)n * dm.nv * dm.nv : 0, nb = o.bias ? (size_t)n * dm.nv : 0, np = o.passive ? (size_t)n * dm.nv : 0;
  const size_t nj = o.jac ? (size_t)n * spec->n * 6 * dm.nv : 0;
  const size_t nqp = qpos ? (size_t)n * dm.nq : 0, nqv = qpos && qvel ? (size_t)n * dm.nv : 0;
  const hipStream_t stream = main_stream(b);  // (held step calls launched, pipes joined; d_dyn is idle: the host form before this one ended synchronised)
  if (b->d_dyn.reserve(r4(nM) + r4(nb) + r4(np) + r4(nj) + r4(nqp) + r4(nqv) + 4) != HB_OK) return HB_ENOMEM;
  DynOut d;
  d.M = b->d_dyn;
  d.bias = d.M + r4(nM);
  d.passive = d.bias + r4(nb);
  d.jac = d.passive + r4(np);
  float* d_qpos = d.jac + r4(nj);
  float* d_qvel = d_qpos + r4(nqp);
  if (nqp) HB_HIP(hipMemcpyAsync(d_qpos, qpos, nqp * sizeof(float), hipMemcpyHostToDevice, stream));
  if (nqv) HB_HIP(hipMemcpyAsync(d_qvel, qvel, nqv * sizeof(float), hipMemcpyHostToDevice, stream));
  const DynOut dev = {nM ? d.M : nullptr, nb ? d.bias : nullptr, np ? d.passive : nullptr, nj ? d.jac : nullptr};
  int rc;
  if (qpos) rc = dynamics_launch(b, d_qpos, nqv ? d_qvel : nullptr, dm.nq, dm.nv, n, nullptr, dev, spec, stream);
  else rc = dynamics_launch(b, b->d_state + 1, b->d_state + 1 + dm.nq, dm.nstate, dm.nstate, n, b->d_dr, dev, spec, stream);
  if (rc != HB_OK) return rc;
  if (nM) HB_HIP(hipMemcpyAsync(o.M, d.M, nM * sizeof(float), hipMemcpyDeviceToHost, stream));
  if (nb) HB_HIP(hipMemcpyAsync(o.bias, d.bias, nb * sizeof(float), hipMemcpyDeviceToHost, stream));
  if (np) HB_HIP(hipMemcpyAsync(o.passive, d.passive, np * sizeof(float), hipMemcpyDeviceToHost, stream));
  if (nj) HB_HIP(hipMemcpyAsync(o.jac, d.jac, nj * sizeof(float), hipMemcpyDeviceToHost, stream));
  HB_HIP(hipStreamSynchronize(stream));
  return HB_OK;
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
