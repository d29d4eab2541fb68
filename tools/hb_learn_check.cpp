// hb_learn_check - the learners' host arithmetic (humanoid_mujoco_amd/csrc/hb_learn_host.hpp) and the refresh of the packed operands
// (hb_device.hpp: learn_refresh) run on the host over heap buffers of exactly the size the device ones have (no GPU, nothing of HIP
// linked).  Meant to be built with -fsanitize=address,undefined as well: make build/hb_learn_check_san.
// For the PPO networks [48,20,33,21] with [48,20,33,1] and [48,42] with [48,1], and the SAC networks [48,20,33,42] with [69,20,33,1]
// and [48,42] with [69,1], it checks that
//   - the layout equals the one the learners computed before they shared it (the two loops below);
//   - the segments of every Adam and Polyak launch tile their stretch of the record without gap or overlap;
//   - every packed index learn_refresh forms is inside its operand, every entry of W reaches its place in both, and with k0 = nobs
//     the rows below k0 reach no place in the transpose;
//   - the reversed networks name the transposes top down; the scratch carve hands out aligned pieces inside what it counted.
// Prints "ok <case>" per case; exit 0, or 1 at the first failure.
#include "../humanoid_mujoco_amd/csrc/hb_learn_host.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
using namespace hb;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s fails (%s)\n", __FILE__, __LINE__, #c, what); exit(1); } } while (0)
static const char* what = "";

struct Net { std::vector<int> sizes; int k0; };

// ---- the layouts as hb_api_ppo.cpp and hb_api_sac.cpp computed them
static int ref_layout_ppo(const std::vector<int> sz[2], int nu, int off_w[2][4], int off_b[2][4], int& off_log_std) {
  int o = 0;
  for (int k = 0; k < 2; k++) {
    const int layers = (int)sz[k].size() - 1;
    for (int l = 0; l < layers; l++) {
      off_w[k][l] = o; o += sz[k][l] * sz[k][l + 1];
      off_b[k][l] = o; o += sz[k][l + 1];
    }
    if (k == 0) { off_log_std = o; o += nu; }
  }
  return o;
}
static int ref_layout_sac(const std::vector<int> sz[3], int off_w[3][4], int off_b[3][4], int& off_q, int& PT) {
  int o = 0;
  for (int k = 0; k < 3; k++) {
    if (k == 1) off_q = o;
    const int layers = (int)sz[k].size() - 1;
    for (int l = 0; l < layers; l++) {
      off_w[k][l] = o; o += sz[k][l] * sz[k][l + 1];
      off_b[k][l] = o; o += sz[k][l + 1];
    }
  }
  PT = o - off_q;
  return o + 1;
}

static size_t packed_size(int K, int N) { return (size_t)((N + 15) / 16) * ((K + 3) / 4) * 64; }

// a network's view over heap operands of the device's sizes, filled with NaN
struct HostNet {
  LearnNet v;
  std::unique_ptr<float[]> w[4], b[4], wt[4];
  HostNet(const Net& n, bool with_t) {
    memset(&v, 0, sizeof v);
    v.layers = (int)n.sizes.size() - 1; v.k0 = n.k0;
    int widest = 1;
    for (int l = 0; l <= v.layers; l++) { v.sizes[l] = n.sizes[l]; widest = std::max(widest, n.sizes[l]); }
    v.ldx = widest + 4;
    for (int l = 0; l < v.layers; l++) {
      const int K = v.sizes[l], N = v.sizes[l + 1];
      auto fill = [](std::unique_ptr<float[]>& p, size_t n) { p.reset(new float[n]); for (size_t i = 0; i < n; i++) p[i] = NAN; return p.get(); };
      v.w[l] = fill(w[l], packed_size(K, N));
      v.b[l] = fill(b[l], N);
      v.wt[l] = with_t && v.has_t(l) ? fill(wt[l], packed_size(N, K - v.t0(l))) : nullptr;
    }
  }
};

static float value_of(int i) { return (float)(i + 1); }

// the segments tile [lo, hi); every entry refreshed; every tensor's entries stand where the kernels read them
static void check_segments(const ParamSeg* seg, int nseg, int lo, int hi) {
  CHECK(nseg >= 1 && nseg <= kLearnMaxSeg && seg[0].start == lo);
  for (int s = 0; s < nseg; s++) {
    const int len = seg[s].K ? seg[s].K * seg[s].N : seg[s].N;
    CHECK(len > 0 && seg[s].start + len == (s + 1 < nseg ? seg[s + 1].start : hi));
  }
  for (int i = lo; i < hi; i++) {
    // (the indices learn_refresh is about to form)
    int sgi = 0;
    while (sgi + 1 < nseg && i >= seg[sgi + 1].start) sgi++;
    const ParamSeg& sg = seg[sgi];
    if (sg.K) {
      const int j = i - sg.start, k = j / sg.N, n = j - k * sg.N;
      CHECK(packed_b_index(k, n, sg.K) < packed_size(sg.K, sg.N));
      if (sg.dst_t && k >= sg.k0) CHECK(packed_b_index(n, k - sg.k0, sg.N) < packed_size(sg.N, sg.K - sg.k0));
    }
    learn_refresh(seg, nseg, i, value_of(i));
  }
  for (int s = 0; s < nseg; s++) {
    const ParamSeg& sg = seg[s];
    if (!sg.K) {
      if (sg.dst) for (int n = 0; n < sg.N; n++) CHECK(sg.dst[n] == value_of(sg.start + n));
      continue;
    }
    CHECK(sg.dst);
    size_t written = 0, written_t = 0;
    for (size_t x = 0; x < packed_size(sg.K, sg.N); x++) written += !std::isnan(sg.dst[x]);
    CHECK(written == (size_t)sg.K * sg.N);
    for (int k = 0; k < sg.K; k++)
      for (int n = 0; n < sg.N; n++) {
        CHECK(sg.dst[packed_b_index(k, n, sg.K)] == value_of(sg.start + k * sg.N + n));
        if (sg.dst_t && k >= sg.k0) CHECK(sg.dst_t[packed_b_index(n, k - sg.k0, sg.N)] == value_of(sg.start + k * sg.N + n));
      }
    if (sg.dst_t) {
      for (size_t x = 0; x < packed_size(sg.N, sg.K - sg.k0); x++) written_t += !std::isnan(sg.dst_t[x]);
      CHECK(written_t == (size_t)(sg.K - sg.k0) * sg.N);  // (the rows below k0 went nowhere)
    }
  }
}

static void check_reversed(const LearnNet& v, int n_in) {
  static const float zero[1] = {0.f};
  const PolicyDesc r = learn_reversed(v, n_in, zero);
  CHECK(r.nl == (n_in > 0 ? v.layers : v.layers - 1) && r.ldx == v.ldx && r.act == 0);
  for (int j = 0; j <= v.layers - 1; j++) CHECK(r.sizes[j] == v.sizes[v.layers - j]);
  if (n_in > 0) CHECK(r.sizes[v.layers] == n_in && v.sizes[0] - v.k0 == n_in);
  for (int j = 0; j < 4; j++) {
    if (j < r.nl) CHECK(r.w[j] && r.w[j] == v.wt[v.layers - 1 - j] && r.b[j] == zero);
    else CHECK(!r.w[j] && !r.b[j]);
  }
}

// pieces of odd lengths, as a minibatch of mb rows takes them
static void check_carve(size_t mb, const std::vector<int>& widths) {
  auto carve = [&](ScratchCarve c, std::vector<float*>* out) {
    for (int w : widths) { float* p = c.take(mb * w); if (out) out->push_back(p); }
    return c.used;
  };
  const size_t need = carve(ScratchCarve{}, nullptr);
  std::unique_ptr<float[]> buf(new float[need]);
  std::vector<float*> piece;
  CHECK(carve(ScratchCarve{buf.get(), 0}, &piece) == need);
  for (size_t i = 0; i < piece.size(); i++) {
    const size_t len = mb * widths[i];
    CHECK(piece[i] && (piece[i] - buf.get()) % 4 == 0);
    CHECK(piece[i] + len <= (i + 1 < piece.size() ? piece[i + 1] : buf.get() + need));
    piece[i][0] = 1.f; piece[i][len - 1] = 1.f;
  }
}

static void check_ppo(const char* name, const std::vector<int>& actor, const std::vector<int>& critic) {
  what = name;
  const int nu = actor.back();
  const std::vector<int> sz[2] = {actor, critic};
  int ref_w[2][4] = {}, ref_b[2][4] = {}, ref_ls = 0;
  const int ref_P = ref_layout_ppo(sz, nu, ref_w, ref_b, ref_ls);
  HostNet net[2] = {HostNet(Net{actor, -1}, true), HostNet(Net{critic, -1}, true)};
  const int off_log_std = learn_layout(net[0].v.layers, net[0].v.sizes, 0, net[0].v.off_w, net[0].v.off_b);
  const int P = learn_layout(net[1].v.layers, net[1].v.sizes, off_log_std + nu, net[1].v.off_w, net[1].v.off_b);
  CHECK(P == ref_P && off_log_std == ref_ls);
  for (int k = 0; k < 2; k++)
    for (int l = 0; l < net[k].v.layers; l++) CHECK(net[k].v.off_w[l] == ref_w[k][l] && net[k].v.off_b[l] == ref_b[k][l]);
  // hb_ppo_adam_dev
  ParamSeg seg[kLearnMaxSeg];
  int nseg = learn_segments(net[0].v, 0, seg);
  seg[nseg++] = ParamSeg{off_log_std, 0, nu, 0, nullptr, nullptr};
  nseg += learn_segments(net[1].v, 0, seg + nseg);
  check_segments(seg, nseg, 0, P);
  for (int k = 0; k < 2; k++) {
    CHECK(!net[k].v.wt[0]);  // (layer 0 has no transpose)
    check_reversed(net[k].v, 0);
  }
  std::vector<int> widths = {actor[0]};
  for (int k = 0; k < 2; k++) {
    for (size_t l = 1; l + 1 < sz[k].size(); l++) widths.push_back(sz[k][l]);
    for (size_t l = 1; l < sz[k].size(); l++) widths.push_back(sz[k][l]);
    widths.push_back(sz[k].back());
  }
  widths.push_back(nu); widths.push_back(5);
  check_carve(100, widths);
  check_carve(4112, widths);
  printf("ok %s: P %d\n", name, P);
}

static void check_sac(const char* name, const std::vector<int>& actor, const std::vector<int>& q) {
  what = name;
  const int nobs = actor[0], nu = q[0] - nobs;
  const std::vector<int> sz[3] = {actor, q, q};
  int ref_w[3][4] = {}, ref_b[3][4] = {}, ref_q = 0, ref_PT = 0;
  const int ref_P = ref_layout_sac(sz, ref_w, ref_b, ref_q, ref_PT);
  HostNet net[3] = {HostNet(Net{actor, -1}, true), HostNet(Net{q, nobs}, true), HostNet(Net{q, nobs}, true)};
  const int off_q = learn_layout(net[0].v.layers, net[0].v.sizes, 0, net[0].v.off_w, net[0].v.off_b);
  int end = learn_layout(net[1].v.layers, net[1].v.sizes, off_q, net[1].v.off_w, net[1].v.off_b);
  end = learn_layout(net[2].v.layers, net[2].v.sizes, end, net[2].v.off_w, net[2].v.off_b);
  const int PT = end - off_q, P = end + 1;
  CHECK(P == ref_P && PT == ref_PT && off_q == ref_q);
  for (int k = 0; k < 3; k++)
    for (int l = 0; l < net[k].v.layers; l++) CHECK(net[k].v.off_w[l] == ref_w[k][l] && net[k].v.off_b[l] == ref_b[k][l]);
  // hb_sac_step_dev: Adam over Q1, Q2 and log_ent_coef; Adam over the actor; the Polyak step over the targets
  ParamSeg seg[kLearnMaxSeg];
  int nseg = learn_segments(net[1].v, 0, seg);
  nseg += learn_segments(net[2].v, 0, seg + nseg);
  seg[nseg++] = ParamSeg{P - 1, 0, 1, 0, nullptr, nullptr};
  check_segments(seg, nseg, off_q, P);
  nseg = learn_segments(net[0].v, 0, seg);
  check_segments(seg, nseg, 0, off_q);
  HostNet tq[2] = {HostNet(Net{q, nobs}, false), HostNet(Net{q, nobs}, false)};
  for (int k = 0; k < 2; k++)
    for (int l = 0; l < tq[k].v.layers; l++) { tq[k].v.off_w[l] = net[k + 1].v.off_w[l]; tq[k].v.off_b[l] = net[k + 1].v.off_b[l]; }
  nseg = learn_segments(tq[0].v, off_q, seg);
  nseg += learn_segments(tq[1].v, off_q, seg + nseg);
  for (int s = 0; s < nseg; s++) CHECK(!seg[s].dst_t);
  check_segments(seg, nseg, 0, PT);
  CHECK(!net[0].v.wt[0] && net[1].v.wt[0] && net[2].v.wt[0]);
  check_reversed(net[0].v, 0);
  for (int k = 1; k < 3; k++) { check_reversed(net[k].v, 0); check_reversed(net[k].v, nu); }
  std::vector<int> widths = {nobs};
  for (size_t l = 1; l + 1 < actor.size(); l++) widths.push_back(actor[l]);
  for (size_t l = 1; l < actor.size(); l++) widths.push_back(actor[l]);
  for (int w : {2 * nu, 2 * nu, nu, nu, nu, 1, 1, nobs + nu}) widths.push_back(w);
  for (int k = 0; k < 2; k++) {
    for (size_t l = 1; l + 1 < q.size(); l++) widths.push_back(q[l]);
    for (size_t l = 1; l < q.size(); l++) widths.push_back(q[l]);
    for (int w : {1, 1, 1, nu}) widths.push_back(w);
  }
  widths.push_back(kSacSrow);
  check_carve(100, widths);
  check_carve(4112, widths);
  printf("ok %s: P %d, targets %d\n", name, P, PT);
}

int main() {
  check_ppo("ppo [48,20,33,21] [48,20,33,1]", {48, 20, 33, 21}, {48, 20, 33, 1});
  check_ppo("ppo [48,42] [48,1]", {48, 42}, {48, 1});
  check_sac("sac [48,20,33,42] [69,20,33,1]", {48, 20, 33, 42}, {69, 20, 33, 1});
  check_sac("sac [48,42] [69,1]", {48, 42}, {69, 1});
  return 0;
}
