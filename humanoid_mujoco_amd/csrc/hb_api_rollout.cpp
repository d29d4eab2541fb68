// hb_api_rollout.cpp — the C-ABI of libhb.so (include/hb.h), rollouts: open-loop rollouts, the control tape, cost terms, noise,
// trajectories, hb_transition_fd, the proto wire format of a state, sensors, the walk / stand tasks and the Halton controls.
#include "hb_batch.hpp"

extern "C" {

int hb_rollout_dev(hb_batch* b, const float* ctrl_dev, int T, float* qpos_out_dev) {
  if (!b || T < 1 || (!ctrl_dev && b->D.dm.nu > 0)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  BatchPtrs P = make_ptrs(b);
  P.ctrl = ctrl_dev; P.ctrl_mode = 1; P.qpos_out = qpos_out_dev;
  return launch_steps(b, P, T);
}

int hb_rollout(hb_batch* b, const float* ctrl, int T, float* qpos_out) {
  if (!b || T < 1 || (!ctrl && b->D.dm.nu > 0)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  int rc = rollout_open(b, ctrl, T, qpos_out != nullptr);
  if (rc != HB_OK) return rc;
  const size_t nq_out = (size_t)T * b->n_env * b->D.dm.nq;
  rc = hb_rollout_dev(b, b->d_ctrl, T, qpos_out ? b->d_qpos_out.get() : nullptr);
  if (rc != HB_OK) return rc;
  if (qpos_out) HB_HIP(hipMemcpyAsync(qpos_out, b->d_qpos_out, nq_out * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

// ---- mjd_transitionFD over a batch ------------------------------------------------------------------------------
namespace {
// mj_integratePos (mujoco.h:466) with dt = 1 on one state: qpos <- qpos (+) dq, dq in R^nv
void integrate_pos(const Model& m, double* qpos, const double* dq) {
  for (int j = 0; j < m.njnt; j++) {
    const int qa = m.jnt_qposadr[j], da = m.jnt_dofadr[j];
    if (m.jnt_type[j] == JNT_FREE) {
      for (int i = 0; i < 3; i++) qpos[qa + i] += dq[da + i];
      double v[3] = {dq[da + 3], dq[da + 4], dq[da + 5]};
      const double ang = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      if (ang > 1e-15) {
        const double s = std::sin(0.5 * ang) / ang, c = std::cos(0.5 * ang);
        const double r[4] = {c, v[0] * s, v[1] * s, v[2] * s};
        double* q = qpos + qa + 3;
        const double o[4] = {q[0] * r[0] - q[1] * r[1] - q[2] * r[2] - q[3] * r[3], q[0] * r[1] + q[1] * r[0] + q[2] * r[3] - q[3] * r[2],
                             q[0] * r[2] - q[1] * r[3] + q[2] * r[0] + q[3] * r[1], q[0] * r[3] + q[1] * r[2] - q[2] * r[1] + q[3] * r[0]};
        const double n = std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]);
        for (int i = 0; i < 4; i++) q[i] = o[i] / n;
      }
    } else qpos[qa] += dq[da];
  }
}
// mj_differentiatePos (mujoco.h:463) with dt = 1: dq = q2 (-) q1 in R^nv
void differentiate_pos(const Model& m, double* dq, const double* q1, const double* q2) {
  for (int j = 0; j < m.njnt; j++) {
    const int qa = m.jnt_qposadr[j], da = m.jnt_dofadr[j];
    if (m.jnt_type[j] == JNT_FREE) {
      for (int i = 0; i < 3; i++) dq[da + i] = q2[qa + i] - q1[qa + i];
      // rotation taking q1 to q2, in q1's frame: conj(q1) * q2, as a rotation vector (mju_subQuat)
      const double* a = q1 + qa + 3;
      const double* c = q2 + qa + 3;
      double d[4] = {a[0] * c[0] + a[1] * c[1] + a[2] * c[2] + a[3] * c[3], a[0] * c[1] - a[1] * c[0] - a[2] * c[3] + a[3] * c[2],
                     a[0] * c[2] + a[1] * c[3] - a[2] * c[0] - a[3] * c[1], a[0] * c[3] - a[1] * c[2] + a[2] * c[1] - a[3] * c[0]};
      const double sn = std::sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
      double ang = 2 * std::atan2(sn, d[0]);
      if (ang > M_PI) ang -= 2 * M_PI;
      const double k = sn > 1e-15 ? ang / sn : 0.0;
      for (int i = 0; i < 3; i++) dq[da + 3 + i] = d[1 + i] * k;
    } else dq[da] = q2[qa] - q1[qa];
  }
}
}  // namespace

static int transition_fd_impl(hb_batch* b, const double* x, const double* u, const double* warm, int T, double eps, int centered, const hb_sensor_spec* spec,
                              double* A, double* B, double* C, double* D) {
  if (!b || !x || T < 1 || !(eps > 0) || (!u && b->D.dm.nu > 0) || (!A && !B && !C && !D) || ((C || D) && !spec)) return HB_EINVAL;
  const Model& m = b->model->m;
  const int nq = m.nq, nv = m.nv, nu = m.nu, nx = 2 * nv, ncol = nx + nu, k = centered ? 2 : 1, per = 1 + k * ncol;
  if ((long long)T * per > b->n_env) return HB_EINVAL;
  const int N = b->n_env, rec = 1 + nq + 2 * nv;
  std::vector<double> st((size_t)N * rec, 0.0), step_of((size_t)T * per, 0.0);
  std::vector<float> ctrl((size_t)N * std::max(1, nu), 0.f);
  // unused envs: a valid rest state (they step along and are ignored)
  for (int e = T * per; e < N; e++) for (int i = 0; i < nq; i++) st[(size_t)e * rec + 1 + i] = m.qpos0[i];
  std::vector<double> dq(nv);
  for (int t = 0; t < T; t++) {
    const double* xt = x + (size_t)t * (nq + nv);
    for (int c = 0; c < per; c++) {
      const int e = t * per + c;
      double* s = st.data() + (size_t)e * rec;
      for (int i = 0; i < nq; i++) s[1 + i] = xt[i];
      for (int i = 0; i < nv; i++) s[1 + nq + i] = xt[nq + i];
      if (warm) for (int i = 0; i < nv; i++) s[1 + nq + nv + i] = warm[(size_t)t * nv + i];
      for (int i = 0; i < nu; i++) ctrl[(size_t)e * nu + i] = (float)u[(size_t)t * nu + i];
      if (c == 0) continue;
      const int col = (c - 1) % ncol;
      const double sign = (c - 1) / ncol == 0 ? 1.0 : -1.0;  // second block: the minus side of a centered difference
      double h = sign * eps;
      if (col < nv) {  // position, in the tangent space
        std::fill(dq.begin(), dq.end(), 0.0);
        dq[col] = h;
        integrate_pos(m, s + 1, dq.data());
      } else if (col < nx) s[1 + nq + (col - nv)] += h;
      else {
        const int a = col - nx;
        double v = u[(size_t)t * nu + a] + h;
        if (m.actuator_ctrllimited[a]) v = std::min(std::max(v, m.actuator_ctrlrange[2 * a]), m.actuator_ctrlrange[2 * a + 1]);  // nudge inside the range
        ctrl[(size_t)e * nu + a] = (float)v;
        h = v - u[(size_t)t * nu + a];
      }
      step_of[e] = h;  // the step actually taken
    }
  }
  int rc = hb_set_state_f64(b, HB_STATE_INTEGRATION, st.data());
  if (rc != HB_OK) return rc;
  std::vector<float> rows;
  int ns = 0;
  if (C || D) {
    // one step with the read-out row of every env (evaluated in the forward pass, before the integration)
    ns = hb_sensor_size(spec);
    if (ns <= 0) return HB_EINVAL;
    rows.resize((size_t)N * ns);
    rc = hb_rollout_sensors(b, ctrl.data(), 1, spec, rows.data(), nullptr);
  } else rc = hb_step(b, ctrl.data(), 1);
  if (rc != HB_OK) return rc;
  rc = hb_get_state_f64(b, HB_STATE_INTEGRATION, st.data());
  if (rc != HB_OK) return rc;
  std::vector<double> dp(nx), dm(nx);
  auto diff = [&](int e_ref, int e, double* out) {  // x'(e) (-) x'(e_ref) in tangent coordinates
    const double* r = st.data() + (size_t)e_ref * rec;
    const double* s = st.data() + (size_t)e * rec;
    differentiate_pos(m, out, r + 1, s + 1);
    for (int i = 0; i < nv; i++) out[nv + i] = s[1 + nq + i] - r[1 + nq + i];
  };
  for (int t = 0; t < T; t++) {
    const int e0 = t * per;
    for (int col = 0; col < ncol; col++) {
      const int ep = e0 + 1 + col, em = centered ? e0 + 1 + ncol + col : e0;
      const double hp = step_of[ep], hm = centered ? step_of[em] : 0.0;
      std::vector<double> d(nx, 0.0);
      if (hp - hm != 0.0) {
        diff(e0, ep, dp.data());
        if (centered) diff(e0, em, dm.data()); else std::fill(dm.begin(), dm.end(), 0.0);
        for (int i = 0; i < nx; i++) d[i] = (dp[i] - dm[i]) / (hp - hm);
      }
      if (col < nx) { if (A) for (int i = 0; i < nx; i++) A[((size_t)t * nx + i) * nx + col] = d[i]; }
      else if (B) for (int i = 0; i < nx; i++) B[((size_t)t * nx + i) * nu + (col - nx)] = d[i];
      if (C || D) {
        const float* rp = rows.data() + (size_t)ep * ns;
        const float* rm = rows.data() + (size_t)em * ns;
        for (int i = 0; i < ns; i++) {
          const double g = hp - hm != 0.0 ? ((double)rp[i] - (double)rm[i]) / (hp - hm) : 0.0;
          if (col < nx) { if (C) C[((size_t)t * ns + i) * nx + col] = g; }
          else if (D) D[((size_t)t * ns + i) * nu + (col - nx)] = g;
        }
      }
    }
  }
  return HB_OK;
}

int hb_transition_fd(hb_batch* b, const double* x, const double* u, const double* warm, int T, double eps, int centered, double* A, double* B) {
  if (!A && !B) return HB_EINVAL;
  return transition_fd_impl(b, x, u, warm, T, eps, centered, nullptr, A, B, nullptr, nullptr);
}
int hb_transition_fd_sensors(hb_batch* b, const double* x, const double* u, const double* warm, int T, double eps, int centered, const hb_sensor_spec* spec,
                             double* A, double* B, double* C, double* D) {
  return transition_fd_impl(b, x, u, warm, T, eps, centered, spec, A, B, C, D);
}

int hb_ctrl_tape_splines(hb_batch* b, const float* knots, const float* times, int n_points, int interpolation, double time0, int T) {
  // an empty spline samples as zeros and a one-node spline as its node, whatever the interpolation (spline.cc:103-118; spline_test.cc:41-64)
  if (!b || n_points < 0 || n_points > 64 || (n_points > 0 && (!knots || !times)) || interpolation < 0 || interpolation > 2 || T < 1 || b->D.dm.nu < 1) return HB_EINVAL;
  for (int k = 1; k < n_points; k++) if (!(times[k] > times[k - 1])) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  const int N = b->n_env, nu = b->D.dm.nu;
  const size_t nk = (size_t)N * n_points * nu;
  int rc = b->d_knots.reserve(nk + 64);
  if (rc != HB_OK) return rc;
  rc = ensure_ctrl(b, (size_t)T * N * nu);
  if (rc != HB_OK) return rc;
  if (n_points > 0) {
    HB_HIP(hipMemcpyAsync(b->d_knots, knots, nk * sizeof(float), hipMemcpyHostToDevice, main_stream(b)));
    HB_HIP(hipMemcpyAsync(b->d_knots + nk, times, (size_t)n_points * sizeof(float), hipMemcpyHostToDevice, main_stream(b)));
  }
  HB_HIP(launch_spline_tape(b->D.dm, b->d_knots, b->d_knots + nk, n_points, interpolation, (float)time0, (float)b->model->m.timestep, T, N, b->d_ctrl, main_stream(b)));
  b->tape_steps = T;
  return HB_OK;
}

int hb_ctrl_tape_read(hb_batch* b, int T, float* out) {
  if (!b || !out || T < 1 || T > b->tape_steps) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipMemcpyAsync(out, b->d_ctrl, (size_t)T * b->n_env * b->D.dm.nu * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

int hb_task_cost(hb_batch* b, const float* residual, int n, int n_residual, const hb_cost_spec* spec, float* terms, float* cost) {
  if (!b || !residual || !spec || !cost || n < 1 || n_residual < 1 || spec->n_term < 1 || spec->n_term > 8) return HB_EINVAL;
  CostSpec K;
  memset(&K, 0, sizeof K);
  int total_dim = 0;
  for (int k = 0; k < spec->n_term; k++) {
    if (spec->dim[k] < 1 || spec->norm[k] < -1 || spec->norm[k] > 8 || spec->norm[k] == 4) return HB_EINVAL;  // kJunction (4) has no value-only form here
    K.dim[k] = spec->dim[k]; K.norm[k] = spec->norm[k]; K.weight[k] = spec->weight[k]; K.p[k] = spec->norm_p[k][0]; K.q[k] = spec->norm_p[k][1];
    total_dim += spec->dim[k];
  }
  if (total_dim != n_residual) return HB_EINVAL;  // "mismatch between total user-sensor dimension and actual length of residual"
  K.nterm = spec->n_term; K.risk = spec->risk;
  HB_HIP(hipSetDevice(b->device));
  const size_t nr = (size_t)n * n_residual, nt = (size_t)n * spec->n_term;
  int rc = b->d_sensor_out.reserve(nr);
  if (rc != HB_OK) return rc;
  if ((rc = b->d_task_out.reserve(nt + n)) != HB_OK) return rc;
  HB_HIP(hipMemcpyAsync(b->d_sensor_out, residual, nr * sizeof(float), hipMemcpyHostToDevice, main_stream(b)));
  HB_HIP(launch_cost_terms(b->d_sensor_out, n, n_residual, K, terms ? b->d_task_out + n : nullptr, b->d_task_out, main_stream(b)));
  HB_HIP(hipMemcpyAsync(cost, b->d_task_out, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  if (terms) HB_HIP(hipMemcpyAsync(terms, b->d_task_out + n, nt * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

int hb_rollout_noise(hb_batch* b, float xfrc_std, float xfrc_rate, unsigned seed) {
  if (!b || !(xfrc_std >= 0.f) || !(xfrc_rate >= 0.f)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  if (xfrc_std > 0.f) {
    const int rc = ensure_xfrc(b);
    if (rc != HB_OK) return rc;
  }
  b->xfrc_std = xfrc_std; b->xfrc_rate = xfrc_rate; b->xfrc_seed = seed; b->xfrc_calls = 0;
  return HB_OK;
}

int hb_rollout_trajectory(hb_batch* b, const float* ctrl, int T, float* qpos_out, float* qvel_out, int* failed) {
  if (!b || T < 1 || (!ctrl && b->D.dm.nu > 0)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  int rc = rollout_open(b, ctrl, T, qpos_out != nullptr);
  if (rc != HB_OK) return rc;
  const size_t nq_out = (size_t)T * b->n_env * b->D.dm.nq, nv_out = (size_t)T * b->n_env * b->D.dm.nv;
  if (qvel_out && (rc = b->d_qvel_out.reserve(nv_out)) != HB_OK) return rc;
  BatchPtrs P = make_ptrs(b);
  P.ctrl = b->d_ctrl; P.ctrl_mode = 1;
  P.qpos_out = qpos_out ? b->d_qpos_out.get() : nullptr;
  P.qvel_out = qvel_out ? b->d_qvel_out.get() : nullptr;
  rc = launch_steps(b, P, T);
  if (rc != HB_OK) return rc;
  if (qpos_out) HB_HIP(hipMemcpyAsync(qpos_out, b->d_qpos_out, nq_out * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  if (qvel_out) HB_HIP(hipMemcpyAsync(qvel_out, b->d_qvel_out, nv_out * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  if (failed) {
    // CheckWarnings (mujoco_mpc/mjpc/utilities.cc:787-799): a trajectory that raised a bad-state warning is a failure
    std::vector<int> st(b->n_env);
    rc = hb_get_status(b, st.data());
    if (rc != HB_OK) return rc;
    for (int e = 0; e < b->n_env; e++) failed[e] = (st[e] & (HB_WARN_BADQPOS | HB_WARN_BADQVEL | HB_WARN_BADQACC)) ? 1 : 0;
  }
  return HB_OK;
}

// ---- agent.proto State <-> one env's state record (protobuf wire format, no protobuf dependency) ----
namespace {
size_t pb_varint(unsigned long long v, unsigned char* out) {
  size_t n = 0;
  do { unsigned char c = v & 0x7f; v >>= 7; if (v) c |= 0x80; if (out) out[n] = c; n++; } while (v);
  return n;
}
// appends `tag`, and for packed doubles the byte length, then the little-endian doubles; counts when out == nullptr
size_t pb_doubles(int field, const double* v, int n, bool packed, unsigned char* out) {
  size_t k = 0;
  k += pb_varint(((unsigned long long)field << 3) | (packed ? 2 : 1), out ? out + k : nullptr);
  if (packed) k += pb_varint((unsigned long long)n * 8, out ? out + k : nullptr);
  if (out) memcpy(out + k, v, (size_t)n * 8);  // hosts of this engine are little-endian
  return k + (size_t)n * 8;
}
bool pb_read_varint(const unsigned char* buf, int len, int& pos, unsigned long long& v) {
  v = 0;
  for (int shift = 0; pos < len && shift < 64; shift += 7) {
    const unsigned char c = buf[pos++];
    v |= (unsigned long long)(c & 0x7f) << shift;
    if (!(c & 0x80)) return true;
  }
  return false;
}
}  // namespace

int hb_state_to_proto(hb_batch* b, int env, unsigned char* buf, int cap) {
  if (!b || env < 0 || env >= b->n_env || cap < 0) return HB_EINVAL;
  const Model& m = b->model->m;
  const int ns = b->D.dm.nstate;
  std::vector<float> rec(ns);
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  HB_HIP(hipMemcpy(rec.data(), b->d_state + (size_t)env * ns, (size_t)ns * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<double> d(rec.begin(), rec.end());
  const size_t need = pb_doubles(1, &d[0], 1, false, nullptr) + pb_doubles(2, &d[1], m.nq, true, nullptr) + pb_doubles(3, &d[1 + m.nq], m.nv, true, nullptr);
  if (buf && (size_t)cap >= need) {
    size_t k = pb_doubles(1, &d[0], 1, false, buf);
    k += pb_doubles(2, &d[1], m.nq, true, buf + k);
    k += pb_doubles(3, &d[1 + m.nq], m.nv, true, buf + k);
  }
  return (int)need;
}

int hb_state_from_proto(hb_batch* b, int env, const unsigned char* buf, int len) {
  if (!b || env < 0 || env >= b->n_env || !buf || len < 0) return HB_EINVAL;
  const Model& m = b->model->m;
  const int ns = b->D.dm.nstate;
  std::vector<float> rec(ns);
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  HB_HIP(hipMemcpy(rec.data(), b->d_state + (size_t)env * ns, (size_t)ns * sizeof(float), hipMemcpyDeviceToHost));
  int pos = 0, nqpos = 0, nqvel = 0;  // repeated doubles may arrive packed or one by one; both are appended in order
  bool touched = false;
  while (pos < len) {
    unsigned long long key, l;
    if (!pb_read_varint(buf, len, pos, key)) return HB_EINVAL;
    const int field = (int)(key >> 3), wt = (int)(key & 7);
    if (wt == 1) {  // one double
      if (pos + 8 > len) return HB_EINVAL;
      double v; memcpy(&v, buf + pos, 8); pos += 8;
      if (field == 1) rec[0] = (float)v;
      else if (field == 2) { if (nqpos >= m.nq) return HB_EINVAL; rec[1 + nqpos++] = (float)v; }
      else if (field == 3) { if (nqvel >= m.nv) return HB_EINVAL; rec[1 + m.nq + nqvel++] = (float)v; }
      else if (field >= 4 && field <= 7) return HB_EUNSUPPORTED;
      touched = true;
    } else if (wt == 2) {  // packed doubles (or an unknown length-delimited field)
      if (!pb_read_varint(buf, len, pos, l) || l > (unsigned long long)(len - pos)) return HB_EINVAL;
      if (field >= 4 && field <= 7) { if (l) return HB_EUNSUPPORTED; }
      else if (field == 2 || field == 3) {
        if (l % 8) return HB_EINVAL;
        for (unsigned long long k = 0; k < l / 8; k++) {
          double v; memcpy(&v, buf + pos + 8 * k, 8);
          if (field == 2) { if (nqpos >= m.nq) return HB_EINVAL; rec[1 + nqpos++] = (float)v; }
          else { if (nqvel >= m.nv) return HB_EINVAL; rec[1 + m.nq + nqvel++] = (float)v; }
        }
        touched = true;
      }
      pos += (int)l;
    } else if (wt == 0) { if (!pb_read_varint(buf, len, pos, l)) return HB_EINVAL; }
    else if (wt == 5) { if (pos + 4 > len) return HB_EINVAL; pos += 4; }
    else return HB_EINVAL;
  }
  if ((nqpos && nqpos != m.nq) || (nqvel && nqvel != m.nv)) return HB_EINVAL;  // a partial vector is an error, an absent one is not
  if (touched) for (int i = 0; i < m.nv; i++) rec[1 + m.nq + m.nv + i] = 0.f;
  HB_HIP(hipMemcpy(b->d_state + (size_t)env * ns, rec.data(), (size_t)ns * sizeof(float), hipMemcpyHostToDevice));
  return HB_OK;
}

// the row of a spec (with tail parts: of a model with these sizes)
static SensorRow spec_row(const hb_sensor_spec& s, int tail = 0, int nq = 0, int nv = 0, int nu = 0) {
  return sensor_row(s.n_framepos, s.subtree_body >= 0, s.n_frameaxis, s.n_framelinvel, s.n_subtreelinvel, s.n_touch, s.n_contactforce, s.n_imu, s.n_frameacc, tail, nq, nv, nu);
}
int hb_sensor_size(const hb_sensor_spec* spec) {
  if (!spec || spec->n_framepos < 0 || spec->n_framepos > HB_MAX_FRAMEPOS) return HB_EINVAL;
  if (spec->n_frameaxis < 0 || spec->n_frameaxis > 8 || spec->n_framelinvel < 0 || spec->n_framelinvel > 8 || spec->n_subtreelinvel < 0 || spec->n_subtreelinvel > 4) return HB_EINVAL;
  if (spec->n_touch < 0 || spec->n_touch > 8 || spec->n_contactforce < 0 || spec->n_contactforce > 4) return HB_EINVAL;
  if (spec->n_imu < 0 || spec->n_imu > 4 || spec->n_frameacc < 0 || spec->n_frameacc > 4) return HB_EINVAL;
  return spec_row(*spec).width;
}
int hb_sensor_row(const hb_sensor_spec* spec, struct hb_sensor_row* out) {
  static_assert(sizeof(struct hb_sensor_row) == offsetof(SensorRow, width) + sizeof(int), "hb_sensor_row is SensorRow up to its width");
  if (!out || hb_sensor_size(spec) <= 0) return HB_EINVAL;
  const SensorRow row = spec_row(*spec);
  memcpy(out, &row, sizeof *out);
  return HB_OK;
}

extern "C++" {
namespace hb {
// The sensor read-out of `spec` on this model with the tail parts `tail` (kSensor*): the spec checked, the row laid out and every part's
// table filled (S.out stays null).  Needs no batch: tools/hb_sensor_check.cpp runs it on the host.
int sensor_args(const Model& m, const DevModel& dm, const hb_sensor_spec* spec, int tail, SensorArgs& S) {
  memset(&S, 0, sizeof S);  // (BatchPtrs is compared byte for byte)
  if (hb_sensor_size(spec) <= 0) return HB_EINVAL;
  if (spec->n_imu + spec->n_frameacc > 0 && (dm.nfric || dm.neq_rows)) return HB_EUNSUPPORTED;  // (friction loss, equality rows: no kernel with the body-acceleration read-out)
  S.row = spec_row(*spec, tail, dm.nq, dm.nv, dm.nu);
  const SensorRow& R = S.row;
  // a part's bodies, each in [first, nbody)
  auto bodies = [&](const int* body, int n, int first, auto&& put) {
    for (int k = 0; k < n; k++) { if (body[k] < first || body[k] >= m.nbody) return false; put(k, body[k]); }
    return true;
  };
  const auto into = [](int* t) { return [t](int k, int id) { t[k] = id; }; };
  const auto packed = [](auto& t) { return [&t](int k, int id) { t.set(k, id); }; };
  if (!bodies(spec->framepos_body, R.n_framepos, 0, into(S.body)) || !bodies(spec->frameaxis_body, R.n_axis, 0, into(S.axis_body)) ||
      !bodies(spec->framelinvel_body, R.n_linvel, 1, into(S.linvel_body)) || !bodies(spec->touch_body, R.n_touch, 0, packed(S.touch_body)) ||
      !bodies(spec->contactforce_body, R.n_cfrc, 0, packed(S.cfrc_body)) || !bodies(spec->imu_body, R.n_imu, 0, packed(S.imu_body)) ||
      !bodies(spec->frameacc_body, R.n_facc, 0, packed(S.facc_body)))
    return HB_EINVAL;
  for (int k = 0; k < R.n_framepos; k++) for (int i = 0; i < 3; i++) S.off[k][i] = spec->framepos_offset[k][i];
  for (int k = 0; k < R.n_imu; k++) for (int i = 0; i < 3; i++) S.imu_off[k][i] = spec->imu_offset[k][i];
  if (R.n_subtree) {
    if (spec->subtree_body < 1 || spec->subtree_body >= m.nbody || m.body_parentid[spec->subtree_body] != 0) return HB_EINVAL;  // a tree root
    for (int bd = 1; bd < spec->subtree_body; bd++) if (m.body_parentid[bd] == 0) S.tree++;
  }
  for (int k = 0; k < R.n_axis; k++) {
    if (spec->frameaxis_which[k] != 0 && spec->frameaxis_which[k] != 2) return HB_EINVAL;
    S.axis_which |= (unsigned)spec->frameaxis_which[k] << (2 * k);
  }
  for (int k = 0; k < R.n_sub; k++) {
    const int root = spec->subtreelinvel_body[k];
    if (root < 1 || root >= m.nbody) return HB_EINVAL;
    double mass = 0;
    for (int bd = 1; bd < m.nbody; bd++)
      for (int a = bd; a > 0; a = m.body_parentid[a])
        if (a == root) { S.submask[k] |= 1ull << bd; mass += m.body_mass[bd]; break; }
    S.subinv[k] = mass > 1e-15 ? (float)(1.0 / mass) : 0.f;
  }
  return HB_OK;
}
}  // namespace hb
}  // extern "C++"

// the sensor read-out of `spec` with the tail parts `tail` in P, the device buffer sized for T rows per env, and the read-outs the
// contact and acceleration parts are written by
static int sensor_setup(hb_batch* b, const hb_sensor_spec* spec, int tail, int T, BatchPtrs& P) {
  int rc = sensor_args(b->model->m, b->D.dm, spec, tail, P.sensor);
  if (rc != HB_OK) return rc;
  const SensorRow& R = P.sensor.row;
  if ((rc = b->d_sensor_out.reserve((size_t)T * b->n_env * R.stride)) != HB_OK) return rc;
  P.sensor.out = b->d_sensor_out;
  if (R.n_touch + R.n_cfrc > 0) {  // written by the step kernel's contact-force epilogue, so the launch carries the read-out buffers
    if (alloc_contact_readout(b) != HB_OK) return HB_ENOMEM;
    P.contact_force = b->d_contact_force; P.body_contact = b->d_body_contact;
  }
  if (R.n_imu + R.n_facc > 0) {  // written by the body-acceleration epilogue, likewise
    if (alloc_body_acc_readout(b) != HB_OK) return HB_ENOMEM;
    P.body_acc = b->d_body_acc; P.body_acc_park = b->d_body_acc_park;
  }
  return HB_OK;
}

int hb_rollout_sensors(hb_batch* b, const float* ctrl, int T, const hb_sensor_spec* spec, float* sensor_out, float* qpos_out) {
  if (!b || T < 1 || !spec || !sensor_out || (!ctrl && b->D.dm.nu > 0)) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  int rc = rollout_open(b, ctrl, T, qpos_out != nullptr);
  if (rc != HB_OK) return rc;
  const size_t nq_out = (size_t)T * b->n_env * b->D.dm.nq;
  BatchPtrs P = make_ptrs(b);
  P.ctrl = b->d_ctrl; P.ctrl_mode = 1; P.qpos_out = qpos_out ? b->d_qpos_out.get() : nullptr;
  rc = sensor_setup(b, spec, 0, T, P);
  if (rc != HB_OK) return rc;
  rc = launch_steps(b, P, T);
  if (rc != HB_OK) return rc;
  HB_HIP(hipMemcpyAsync(sensor_out, b->d_sensor_out, (size_t)T * b->n_env * P.sensor.row.stride * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  if (qpos_out) HB_HIP(hipMemcpyAsync(qpos_out, b->d_qpos_out, nq_out * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

// Trajectory::Rollout's data flow for a task cost on the device: `horizon - 1` steps from the current state with the
// read-out row of every step (sensors of `spec`, then the state / control parts in `tail`), then one mj_forward with the
// last action repeated (zero when horizon = 1) for the terminal row.  Leaves `horizon` rows laid out as `*row` in
// b->d_sensor_out and room for horizon + 1 floats per env in b->d_task_out; the status words are cleared first.
static int rollout_rows(hb_batch* b, const float* ctrl, int H, const hb_sensor_spec* spec, int tail, SensorRow* row) {
  const DevModel& dm = b->D.dm;
  const int N = b->n_env, nu = dm.nu;
  const size_t n = (size_t)(H - 1) * N * nu;
  int rc = HB_OK;
  if (ctrl == HB_CTRL_TAPE) {
    if (H < 2 || b->tape_steps < H - 1) return HB_EINVAL;  // the tape hb_ctrl_tape_splines left is shorter than this rollout
  } else {
    rc = ensure_ctrl(b, std::max<size_t>(std::max<size_t>(n, (size_t)N * nu), 1));
    if (rc != HB_OK) return rc;
    b->tape_steps = 0;
    if (n) HB_HIP(hipMemcpyAsync(ctrl_for_write(b), ctrl, n * sizeof(float), hipMemcpyHostToDevice, main_stream(b)));
    else if (nu) HB_HIP(hipMemsetAsync(ctrl_for_write(b), 0, (size_t)N * nu * sizeof(float), main_stream(b)));
  }
  // failure is a property of THIS rollout (CheckWarnings looks at the warnings of the rollout's own mjData)
  HB_HIP(hipMemsetAsync(b->d_status, 0, (size_t)N * sizeof(int), main_stream(b)));
  BatchPtrs P = make_ptrs(b);
  rc = sensor_setup(b, spec, tail, H, P);
  if (rc != HB_OK) return rc;
  *row = P.sensor.row;
  if ((rc = b->d_task_out.reserve((size_t)(H + 1) * N)) != HB_OK) return rc;
  if (H > 1) {
    P.ctrl = b->d_ctrl; P.ctrl_mode = 1;
    rc = launch_steps(b, P, H - 1);
    if (rc != HB_OK) return rc;
  }
  // final mj_forward with the last action repeated (trajectory.cc:188-202)
  BatchPtrs F = P;
  F.ctrl = b->d_ctrl + (H > 1 ? (size_t)(H - 2) * N * nu : 0); F.ctrl_mode = 0; F.integrate = 0;
  F.sensor.out = b->d_sensor_out + (size_t)(H - 1) * N * row->stride;
  F.blk0 = 0; F.nblk = N;
  HB_HIP(launch_batch_step(b, F, 1, main_stream(b)));
  return HB_OK;
}

static int task_results(hb_batch* b, int H, float* total_return, float* costs) {
  const int N = b->n_env;
  HB_HIP(hipMemcpyAsync(total_return, b->d_task_out, (size_t)N * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  if (costs) HB_HIP(hipMemcpyAsync(costs, b->d_task_out + N, (size_t)H * N * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

int hb_task_walk_default(const hb_model* h, hb_task_walk* t) {
  if (!h || !t) return HB_EINVAL;
  memset(t, 0, sizeof *t);
  const char* names[5] = {"torso", "pelvis", "foot_right", "foot_left", "waist_lower"};
  int id[5];
  for (int k = 0; k < 5; k++) if ((id[k] = hb_model_name2id(h, "body", names[k])) < 0) return HB_EINVAL;
  t->torso_body = id[0]; t->pelvis_body = id[1]; t->foot_right_body = id[2]; t->foot_left_body = id[3]; t->waist_lower_body = id[4];
  t->height_goal = 1.35f; t->speed_goal = 0.5f;
  hb_sizes sz;
  hb_model_sizes(h, &sz);
  // user sensors of tasks/humanoid/walk/task.xml:28-35: name, dim, "norm weight lo hi [p [q]]"
  const int dim[8] = {1, 1, 2, 8, sz.nq - 7, 2, 1, sz.nu}, norm[8] = {7, 8, 1, 2, 0, 7, 7, 3};
  const float w[8] = {5.f, 1.f, 5.f, 5.f, 0.025f, 0.625f, 1.f, 0.1f};
  const float p[8] = {0.1f, 0.05f, 0.02f, 0.01f, 0.f, 0.2f, 0.5f, 0.3f}, q[8] = {4.f, 0.f, 4.f, 0.f, 0.f, 4.f, 3.f, 0.f};
  t->n_term = 8;
  for (int k = 0; k < 8; k++) { t->dim[k] = dim[k]; t->norm[k] = norm[k]; t->weight[k] = w[k]; t->norm_p[k][0] = p[k]; t->norm_p[k][1] = q[k]; }
  return HB_OK;
}

int hb_rollout_task_walk(hb_batch* b, const float* ctrl, int H, const hb_task_walk* task, float* total_return, float* costs) {
  if (!b || !task || !total_return || H < 1 || (H > 1 && !ctrl && b->D.dm.nu > 0)) return HB_EINVAL;
  const Model& m = b->model->m;
  const DevModel& dm = b->D.dm;
  const int bodies[5] = {task->torso_body, task->pelvis_body, task->foot_right_body, task->foot_left_body, task->waist_lower_body};
  for (int bd : bodies) if (bd < 1 || bd >= m.nbody) return HB_EINVAL;
  if (dm.nq < 7 || task->n_term < 1 || task->n_term > 8) return HB_EINVAL;
  const int nres = 1 + 1 + 2 + 8 + (dm.nq - 7) + 1 + 2 + dm.nu;
  int total_dim = 0;
  for (int k = 0; k < task->n_term; k++) {
    if (task->dim[k] < 1 || task->norm[k] < -1 || task->norm[k] > 8 || task->norm[k] == 4) return HB_EINVAL;
    total_dim += task->dim[k];
  }
  if (total_dim != nres || nres > 96) return HB_EINVAL;  // "mismatch between total user-sensor dimension and actual length of residual" (walk.cc:150-162)
  HB_HIP(hipSetDevice(b->device));
  // read-out rows: framepos (objtype body: inertial frames) torso, foot_right, foot_left, pelvis | subtreecom, subtreelinvel (torso's tree)
  // | up axes x4, forward axes x4 | framelinvel torso, foot_right, foot_left | subtreelinvel waist_lower | qpos | ctrl
  hb_sensor_spec spec;
  memset(&spec, 0, sizeof spec);
  const int fp[4] = {task->torso_body, task->foot_right_body, task->foot_left_body, task->pelvis_body};
  spec.n_framepos = 4;
  for (int k = 0; k < 4; k++) {
    spec.framepos_body[k] = fp[k];
    for (int i = 0; i < 3; i++) spec.framepos_offset[k][i] = (float)m.body_ipos[3 * fp[k] + i];
  }
  int root = task->torso_body;
  while (m.body_parentid[root] != 0) root = m.body_parentid[root];
  if (root != task->torso_body) return HB_EINVAL;  // torso_subcom / torso_subcomvel are read as a whole tree
  spec.subtree_body = root;
  const int axb[4] = {task->torso_body, task->pelvis_body, task->foot_right_body, task->foot_left_body};
  spec.n_frameaxis = 8;
  for (int k = 0; k < 4; k++) { spec.frameaxis_body[k] = axb[k]; spec.frameaxis_which[k] = 2; spec.frameaxis_body[4 + k] = axb[k]; spec.frameaxis_which[4 + k] = 0; }
  spec.n_framelinvel = 3;
  spec.framelinvel_body[0] = task->torso_body; spec.framelinvel_body[1] = task->foot_right_body; spec.framelinvel_body[2] = task->foot_left_body;
  spec.n_subtreelinvel = 1;
  spec.subtreelinvel_body[0] = task->waist_lower_body;
  SensorRow R;
  int rc = rollout_rows(b, ctrl, H, &spec, kSensorQpos | kSensorCtrl, &R);
  if (rc != HB_OK) return rc;
  WalkTask K;
  memset(&K, 0, sizeof K);
  K.o_torso = R.framepos; K.o_foot_r = R.framepos + 3; K.o_foot_l = R.framepos + 6; K.o_pelvis = R.framepos + 9; K.o_com = R.subtree; K.o_vel = R.subtree + 3;
  K.o_axes = R.axis; K.o_linvel = R.linvel; K.o_sub = R.sub; K.o_qpos = R.qpos; K.o_ctrl = R.ctrl; K.nq = dm.nq; K.nu = dm.nu; K.stride = R.stride;
  K.height_goal = task->height_goal; K.speed_goal = task->speed_goal; K.risk = task->risk; K.nterm = task->n_term;
  for (int k = 0; k < task->n_term; k++) { K.dim[k] = task->dim[k]; K.norm[k] = task->norm[k]; K.weight[k] = task->weight[k]; K.p[k] = task->norm_p[k][0]; K.q[k] = task->norm_p[k][1]; }
  HB_HIP(launch_walk_cost(b->d_sensor_out, H, b->n_env, K, b->d_status, b->d_task_out, costs ? b->d_task_out + b->n_env : nullptr, main_stream(b)));
  return task_results(b, H, total_return, costs);
}

int hb_task_stand_default(const hb_model* h, hb_task_stand* t) {
  if (!h || !t) return HB_EINVAL;
  memset(t, 0, sizeof *t);
  const int head = hb_model_name2id(h, "body", "head"), fl = hb_model_name2id(h, "body", "foot_left"), fr = hb_model_name2id(h, "body", "foot_right"),
            torso = hb_model_name2id(h, "body", "torso");
  if (head < 0 || fl < 0 || fr < 0 || torso < 0) return HB_EINVAL;
  t->head_body = head; t->subtree_body = torso; t->n_feet = 4;
  const int fb[4] = {fl, fl, fr, fr};
  const float fx[4] = {-0.07f, 0.14f, -0.07f, 0.14f};
  for (int k = 0; k < 4; k++) { t->foot_body[k] = fb[k]; t->foot_offset[k][0] = fx[k]; }
  t->height_goal = 1.4f;
  const int norm[5] = {6, 6, 0, 0, 3};
  const float w[5] = {100.f, 50.f, 10.f, 0.01f, 0.025f}, p[5] = {0.1f, 0.1f, 0.f, 0.f, 0.3f};
  for (int k = 0; k < 5; k++) { t->norm[k] = norm[k]; t->weight[k] = w[k]; t->norm_p[k][0] = p[k]; }
  return HB_OK;
}

int hb_rollout_task_stand(hb_batch* b, const float* ctrl, int H, const hb_task_stand* task, float* total_return, float* costs) {
  if (!b || !task || !total_return || H < 1 || (H > 1 && !ctrl && b->D.dm.nu > 0)) return HB_EINVAL;
  const Model& m = b->model->m;
  const DevModel& dm = b->D.dm;
  if (task->n_feet < 1 || task->n_feet > 4 || task->head_body < 0 || task->head_body >= m.nbody || dm.nv < 6) return HB_EINVAL;
  for (int k = 0; k < task->n_feet; k++) if (task->foot_body[k] < 0 || task->foot_body[k] >= m.nbody) return HB_EINVAL;
  for (int k = 0; k < 5; k++) if (task->norm[k] < -1 || task->norm[k] > 8 || task->norm[k] == 4) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  // read-out rows: [head | feet | subtreecom | subtreelinvel | qvel | ctrl]
  hb_sensor_spec spec;
  memset(&spec, 0, sizeof spec);
  spec.n_framepos = 1 + task->n_feet;
  spec.framepos_body[0] = task->head_body;
  // "head_position" is a framepos with objtype="body": MuJoCo's body objtype is the INERTIAL frame (xipos = xpos + R ipos)
  for (int i = 0; i < 3; i++) spec.framepos_offset[0][i] = (float)m.body_ipos[3 * task->head_body + i];
  for (int k = 0; k < task->n_feet; k++) {
    spec.framepos_body[1 + k] = task->foot_body[k];
    for (int i = 0; i < 3; i++) spec.framepos_offset[1 + k][i] = task->foot_offset[k][i];
  }
  spec.subtree_body = task->subtree_body;
  if (spec.subtree_body < 0) return HB_EINVAL;
  SensorRow R;
  int rc = rollout_rows(b, ctrl, H, &spec, kSensorQvel | kSensorCtrl, &R);
  if (rc != HB_OK) return rc;
  StandTask K;
  memset(&K, 0, sizeof K);
  K.n_feet = task->n_feet; K.o_head = R.framepos; K.o_feet = R.framepos + 3; K.o_com = R.subtree; K.o_vel = R.subtree + 3; K.o_qvel = R.qvel; K.o_ctrl = R.ctrl;
  K.nv = dm.nv; K.nu = dm.nu; K.stride = R.stride;
  K.height_goal = task->height_goal; K.risk = task->risk;
  for (int k = 0; k < 5; k++) { K.norm[k] = task->norm[k]; K.weight[k] = task->weight[k]; K.p[k] = task->norm_p[k][0]; K.q[k] = task->norm_p[k][1]; }
  HB_HIP(launch_stand_cost(b->d_sensor_out, H, b->n_env, K, b->d_status, b->d_task_out, costs ? b->d_task_out + b->n_env : nullptr, main_stream(b)));
  return task_results(b, H, total_return, costs);
}

int hb_sensors(hb_batch* b, const float* ctrl, const hb_sensor_spec* spec, float* sensor_out) {
  if (!b || !spec || !sensor_out) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  const size_t n = (size_t)b->n_env * b->D.dm.nu;
  if (ctrl && n) HB_HIP(hipMemcpyAsync(ctrl_for_write(b), ctrl, n * sizeof(float), hipMemcpyHostToDevice, main_stream(b)));
  else if (n) HB_HIP(hipMemsetAsync(ctrl_for_write(b), 0, n * sizeof(float), main_stream(b)));
  BatchPtrs P = make_ptrs(b);
  P.ctrl = b->d_ctrl; P.ctrl_mode = 0; P.integrate = 0;
  int rc = sensor_setup(b, spec, 0, 1, P);
  if (rc != HB_OK) return rc;
  HB_HIP(launch_batch_step(b, P, 1, main_stream(b)));
  HB_HIP(hipMemcpyAsync(sensor_out, b->d_sensor_out, (size_t)b->n_env * P.sensor.row.stride * sizeof(float), hipMemcpyDeviceToHost, main_stream(b)));
  HB_HIP(hipStreamSynchronize(main_stream(b)));
  return HB_OK;
}

int hb_rollout_halton(hb_batch* b, int T, int t0, int env_offset, float* qpos_out_dev) {
  if (!b || T < 1) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  BatchPtrs P = make_ptrs(b);
  P.ctrl = nullptr; P.ctrl_mode = 2; P.t0 = t0; P.env_offset = env_offset; P.qpos_out = qpos_out_dev;
  return launch_steps(b, P, T);
}

int hb_halton_ctrl_dev(hb_batch* b, int T, int t0, int env_offset, float* out_dev) {
  if (!b || T < 1 || !out_dev) return HB_EINVAL;
  HB_HIP(hipSetDevice(b->device));
  HB_HIP(launch_halton_ctrl(out_dev, T, b->n_env, b->D.dm.nu, t0, env_offset, main_stream(b)));
  return HB_OK;
}

}  // extern "C"
