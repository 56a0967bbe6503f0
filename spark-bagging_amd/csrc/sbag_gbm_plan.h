// sbag_gbm_plan.h — what the host and k_gbm_step (sbag_host.cpp, sbag_gbm.hip) must agree on:
// the row tile, the staged node, the LDS layout, the switch to the general path, and the loss
// arithmetic itself (host + device, so tests/c/gbm_plan_check.cpp runs the same lines on the host
// against the plain formulas).  No HIP in it beyond the host / device marker.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "sbag_div.h"

namespace sbag {

// sbag_gbm_state_create's loss and mode (= SBAG_GBM_* of sbag.h)
constexpr int kGbmSquared = 0, kGbmAbsolute = 1, kGbmHuber = 2, kGbmQuantile = 3;
constexpr int kGbmResidual = 0, kGbmLoss = 1;

// ---- work split: a workgroup of 256 lanes owns kGbmTileRows contiguous rows; lane t owns rows
// t, t + 256, ... of the tile (kGbmLaneRows rows: so many code gathers of a lane are in flight)
constexpr int kGbmBlock = 256;
constexpr int kGbmWaves = kGbmBlock / 64;
constexpr int kGbmLaneRows = 4;
constexpr int kGbmTileRows = kGbmBlock * kGbmLaneRows;

// ---- the staged node, 16 bytes (one ds_read_b128).  internal: left >= 0, go left iff the row's
// code of dataset column `col` is < `cut` (cut = 1 + the largest code whose value <= threshold:
// TreePoint's `value <= threshold` in the dataset's code space).  leaf: left = -1 and (col, cut)
// are the low and high words of the leaf value.
struct alignas(16) GbmNode {
  int32_t left, right;
  uint32_t col, cut;
};
inline GbmNode gbm_leaf(double value) {
  uint64_t b;
  std::memcpy(&b, &value, 8);
  return GbmNode{-1, -1, (uint32_t)b, (uint32_t)(b >> 32)};
}
// the cut of `threshold` on a feature's sorted distinct values (upper_bound)
inline uint32_t gbm_code_cut(const double* dict, size_t n, double threshold) {
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (dict[mid] <= threshold) lo = mid + 1; else hi = mid;
  }
  return (uint32_t)lo;
}

// ---- LDS: the block reduction's words, then the tree.  A tree of more than kGbmLdsNodes nodes
// (a full tree of depth 11 and deeper) is read from global memory instead: the general path.
// 32 KB of nodes keeps four workgroups and more on a CU; the walk is a chain of dependent
// gathers, and resident waves are what hides them.
constexpr int kGbmLdsNodes = 2048;
constexpr size_t kGbmRedBytes = (size_t)kGbmWaves * 4 * 8;  // per wave: smax, kmin, kmax, amax
SBAG_HD inline bool gbm_tree_in_lds(int num_nodes) { return num_nodes <= kGbmLdsNodes; }
SBAG_HD inline size_t gbm_lds_bytes(int num_nodes) {
  return kGbmRedBytes + (gbm_tree_in_lds(num_nodes) ? (size_t)num_nodes * sizeof(GbmNode) : 0);
}
SBAG_HD inline int64_t gbm_blocks(int64_t N) { return (N + kGbmTileRows - 1) / kGbmTileRows; }

// ---- arithmetic: GBMRegressorParams.lossFunction / gradFunction (GBMRegressor.scala:93-118),
// one rounded fp64 operation per line of the formula, never contracted (-ffp-contract=off).

// sqrt, correctly rounded for 0 < x < inf: the device's sqrt is a refined estimate, so its
// result s is held to Tuckerman's test, pred(s) * s < x <= s * succ(s), each product's
// comparison made exact by one fma, and moved one ulp where the test says so.
SBAG_HD inline double gbm_sqrt(double x) {
  double s = std::sqrt(x);
  if (x > 0.0 && x < INFINITY) {
    int64_t b;
    std::memcpy(&b, &s, 8);
    const int64_t bm = b - 1, bp = b + 1;
    double sm, sp;
    std::memcpy(&sm, &bm, 8);
    std::memcpy(&sp, &bp, 8);
    if (std::fma(s, sm, -x) >= 0.0)
      s = sm;
    else if (std::fma(s, sp, -x) < 0.0)
      s = sp;
  }
  return s;
}

// -grad(y, p): the pseudo-residual.  The reference negates the gradient's own leading minus;
// two negations cancel bit for bit (NaN included), so neither is made.
SBAG_HD inline double gbm_residual(int loss, double alpha, double y, double p) {
  const double d = y - p;
  if (loss == kGbmSquared) return d;
  if (loss == kGbmAbsolute) return d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : d;  // Math.signum: +-0.0, NaN themselves
  if (loss == kGbmHuber) {
    const double t = div_rn(d, alpha);
    const double q = gbm_sqrt(1.0 + t * t);
    return -div_rn(-d, q);
  }
  return p > y ? alpha - 1.0 : alpha;  // quantile: -(-(alpha - 1)), -(-alpha)
}

// lossf(y, p)
SBAG_HD inline double gbm_loss(int loss, double alpha, double y, double p) {
  const double d = y - p;
  if (loss == kGbmSquared) return (d * d) * 0.5;  // = / 2.0 bit for bit, subnormal quotients too
  if (loss == kGbmAbsolute) return std::fabs(d);
  if (loss == kGbmHuber) {
    const double t = div_rn(d, alpha);
    return (alpha * alpha) * (gbm_sqrt(1.0 + t * t) - 1.0);
  }
  return p > y ? (alpha - 1.0) * d : alpha * d;
}

}  // namespace sbag
