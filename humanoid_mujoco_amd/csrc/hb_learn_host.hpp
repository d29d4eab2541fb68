// hb_learn_host.hpp - the host arithmetic both learners share (hb_api_ppo.cpp, hb_api_sac.cpp through LearnerCore, hb_batch.hpp): where
// a network's tensors stand in the flat record, the record's tensors as Adam / Polyak segments, the reversed network of the backward
// pass, and the carve of the minibatch scratch.  Plain C++ over plain data, no HIP runtime call: tools/hb_learn_check.cpp runs all of
// it, and learn_refresh (hb_device.hpp) over its segments, on the host.
#pragma once
#include "hb_device.hpp"
#include <cstring>

namespace hb {

// One network of a learner's flat record: its widths, where its tensors stand in the record, the device operands that follow them,
// and the rule of its packed transposes - every layer l > 0 has the transpose of all its rows (dA = dZ W^T); layer 0 that of its rows
// k0 .. (a Q network's action rows, for dQ / da), or none (k0 < 0).
struct LearnNet {
  int layers, ldx, k0;   // ldx: DevMlp::desc()'s
  int sizes[5];
  int off_w[4], off_b[4];
  float *w[4], *b[4];    // the packed B operand of W and the bias the forward pass reads
  float* wt[4];          // the packed transposes (null: none, or not this view's to refresh)
  bool has_t(int l) const { return l > 0 || k0 >= 0; }
  int t0(int l) const { return l == 0 && k0 > 0 ? k0 : 0; }  // the first row of layer l that its transpose holds
};

// the layers W | b of a network from entry o of the record on; returns the entry behind them
inline int learn_layout(int layers, const int* sizes, int o, int* off_w, int* off_b) {
  for (int l = 0; l < layers; l++) {
    off_w[l] = o; o += sizes[l] * sizes[l + 1];
    off_b[l] = o; o += sizes[l + 1];
  }
  return o;
}

// the tensors of a network as segments (2 per layer), starts relative to `base`; returns their number
inline int learn_segments(const LearnNet& n, int base, ParamSeg* seg) {
  int ns = 0;
  for (int l = 0; l < n.layers; l++) {
    seg[ns++] = ParamSeg{n.off_w[l] - base, n.sizes[l], n.sizes[l + 1], n.t0(l), n.w[l], n.wt[l]};
    seg[ns++] = ParamSeg{n.off_b[l] - base, 0, n.sizes[l + 1], 0, n.b[l], nullptr};
  }
  return ns;
}

// the reversed network: the widths from the top down, w[j] = the packed transpose of layer L - 1 - j, b = zeros; L - 1 steps down to
// dZ_0, or with n_in > 0 all L, into the last n_in inputs of layer 0
inline PolicyDesc learn_reversed(const LearnNet& n, int n_in, const float* zero) {
  const int nl = n.layers;
  PolicyDesc r;
  memset(&r, 0, sizeof r);
  r.nl = n_in > 0 ? nl : nl - 1;
  r.ldx = n.ldx;
  for (int j = 0; j <= nl - 1; j++) r.sizes[j] = n.sizes[nl - j];
  if (n_in > 0) r.sizes[nl] = n_in;
  for (int j = 0; j < r.nl; j++) { r.w[j] = n.wt[nl - 1 - j]; r.b[j] = zero; }
  return r;
}

// The carve of the minibatch scratch into 16-byte-aligned pieces.  A call takes its pieces twice, in the same order: over no buffer,
// which counts (`used` is the need), then over the buffer reserved for that need.
struct ScratchCarve {
  float* base = nullptr;
  size_t used = 0;
  float* take(size_t n) {
    float* q = base ? base + used : nullptr;
    used += (n + 3) & ~(size_t)3;
    return q;
  }
};

}  // namespace hb
