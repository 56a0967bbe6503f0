// sbag_contrib_plan.h — the packed path table of the feature-contribution pass (sbag_host.cpp,
// sbag_contrib.hip) and the LDS arithmetic of k_contrib_tiled.  Plain host / device structs and
// host code with no HIP in it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace sbag {

constexpr int kContribThreads = 256;   // k_contrib_tiled: 16 groups of 16 lanes, or 32 of 8
constexpr int kContribTiledM = 15;     // distinct features of a path on the tiled pass (lane 0: pw[0])
constexpr int kContribNarrowM = 7;     // the forest's largest m up to which groups are 8 lanes
constexpr int kContribMaxM = 64;       // distinct features of a path at all (k_contrib_walk's pw[65])
constexpr size_t kContribLdsCap = 160 * 1024 - 512;  // = plan_tiled's bound
constexpr size_t kContribTableCap = (size_t)2 << 30;  // bytes of a packed path table

// One root-to-leaf path, leaves in forest order and pre-order within a tree.
struct ContribLeaf {
  int32_t first;  // its first element in the element table
  int32_t m;      // distinct features the path tests (0: a single-leaf tree)
  double vw;      // the leaf value, times weights[t] when there are weights
  double b;       // vw * z_1 * ... * z_m: the path's share of the bias
};
// One distinct feature of a path, in code space (k_contrib_tiled): o = 1 iff lo <= code <= hi,
// the intersection of the path's tests on the feature with PNode's cuts (left iff code < tc + 1).
// An interval that holds no code is lo = 1, hi = 0.
struct ContribElem {
  int32_t feat;  // global feature
  uint16_t lo, hi;
  double z, rz;  // the cover fraction of the path's tests on the feature, and 1.0 / z
};
// The same in value space (k_contrib_walk): o = 1 iff !(v <= lo) && v <= hi over the largest
// threshold of the path's right turns and the smallest of its left turns.  An end without a test
// holds -inf / +inf and is open, not compared: a NaN goes right at every test, as
// Split.shouldGoLeft sends it, and passes an element with right turns only; -inf goes left at
// every test and passes one with left turns only.
struct ContribElemF {
  int32_t feat, pad;
  double lo, hi, z, rz;
};
static_assert(sizeof(ContribLeaf) == 24 && sizeof(ContribElem) == 24 && sizeof(ContribElemF) == 40,
              "packed path table layout");

// Q(a, b) = (double)a / (double)b for 0 <= a <= M + 1, 1 <= b <= M + 1, at q[b * (M + 2) + a]
inline size_t contrib_q_count(int M) { return (size_t)(M + 2) * (M + 2); }

// lanes of a group of k_contrib_tiled for a forest whose largest m is M
inline int contrib_lanes(int M) { return M <= kContribNarrowM ? 8 : 16; }
// LDS of k_contrib_tiled: the staged code rows at `pitch` bytes (rounded to 16), the
// accumulators fp64 [rows][F + 1], the Q table, and a slot of `lanes` doubles (a row's pw) for
// every row a group works on at once: [groups][rows a group][lanes], at least one row a group
inline size_t contrib_lds(int rows, int pitch, int F, int M) {
  const size_t slots = (size_t)std::max(rows * contrib_lanes(M), kContribThreads);
  return (((size_t)rows * pitch + 15) & ~(size_t)15) + (size_t)rows * (F + 1) * 8 + contrib_q_count(M) * 8 +
         slots * 8;
}
// rows of a tile: 64, 32 or 16, whichever fits; 0: not even 16 rows fit (the general path)
inline int contrib_tile_rows(int pitch, int F, int M) {
  for (int rows = 64; rows >= 16; rows >>= 1)
    if (contrib_lds(rows, pitch, F, M) <= kContribLdsCap) return rows;
  return 0;
}

}  // namespace sbag
