// sbag_pd_plan.h — host arithmetic of the partial dependence pass (sbag_host.cpp, sbag_pd.hip):
// the LDS budget of k_pd_count, its tree groups and row slices, and the stack a tree's range
// walk needs.  Plain host code with no HIP in it.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <tuple>
#include <vector>

namespace sbag {

constexpr int kPdMaxGrid = 256;      // grid points: lo and hi of a range take 9 bits each
constexpr int kPdTileRows = 512;     // rows staged at a time
constexpr int kPdThreads = 1024;     // k_pd_count: a row per thread, two trees side by side
constexpr int kPdStack = 8;          // pending right branches a thread of k_pd_count holds
constexpr int kPdMaxTreeNodes = 1 << 14;            // a stack word: node 14 bits, lo 9, hi 9
constexpr size_t kPdLdsCap = 160 * 1024 - 512;      // = plan_tiled's bound

// the staged row tile, rows at `pitch` bytes, rounded to 16
inline size_t pd_tile_lds(int pitch) { return ((size_t)kPdTileRows * pitch + 15) & ~(size_t)15; }
// one tree in the LDS: its packed nodes and its leaves' difference counters, int32 [G + 1] each
inline size_t pd_tree_lds(int64_t nodes, int64_t leaves, int G) {
  return (size_t)nodes * 8 + (size_t)leaves * (G + 1) * 4;
}

// Tree groups: consecutive trees, as many as the LDS holds beside the row tile (at most
// max_trees): every tree of a group walks a staged tile, so the rows are read from global memory
// once a group.  ends[k] = one past the last tree of group k.  false: a tree does not fit.
inline bool pd_plan_groups(const std::vector<int64_t>& nodes, const std::vector<int64_t>& leaves, int G,
                           size_t tile_bytes, int max_trees, std::vector<int>& ends) {
  ends.clear();
  if (tile_bytes >= kPdLdsCap) return false;
  const size_t budget = kPdLdsCap - tile_bytes;
  size_t used = 0;
  int held = 0;
  for (size_t t = 0; t < nodes.size(); t++) {
    const size_t b = pd_tree_lds(nodes[t], leaves[t], G);
    if (b > budget) return false;
    if (held > 0 && (used + b > budget || held >= max_trees)) {
      ends.push_back((int)t);
      used = 0;
      held = 0;
    }
    used += b;
    held++;
  }
  if (held > 0) ends.push_back((int)nodes.size());
  return true;
}

// Tiles of a row slice.  A workgroup of k_pd_count fills a compute unit's LDS, so one is
// resident a unit; with about `cus` workgroups in all, every group's workgroup of a slice runs
// at the same time as the others and walks the slice at their pace: a tile that one of them
// fetched is in the L2 / MALL for the rest.  More slices would only add flushes.
inline int64_t pd_slice_tiles(int64_t ntiles, int ngroups, int cus) {
  const int64_t slices = std::max<int64_t>(1, std::min<int64_t>(ntiles, cus / std::max(ngroups, 1)));
  return (ntiles + slices - 1) / slices;
}

// The pending right branches a range walk of one tree can hold at once.  s[i] >= 0: node i
// tests the feature, its left range [lo, min(hi, s)) and its right [max(lo, s), hi); -1: any
// other node (either child, the range unchanged).  A node pushes its right child when both
// ranges are non-empty, and the push is pending while the left subtree is walked.  The ranges
// do not depend on the row, so this is exact.  INT_MAX: gave up (node arrays that share
// subtrees can take very many visits).
inline int pd_stack_need(const int32_t* left, const int32_t* right, const int32_t* s, int64_t n, int G) {
  int need = 0;
  int64_t visits = 0;
  std::vector<std::tuple<int32_t, int, int, int>> todo{{0, 0, G, 0}};
  while (!todo.empty()) {
    auto [i, lo, hi, pend] = todo.back();
    todo.pop_back();
    if (++visits > 64 * n + 64) return INT_MAX;
    need = std::max(need, pend);
    if (left[i] < 0) continue;
    if (s[i] < 0) {
      todo.push_back({left[i], lo, hi, pend});
      todo.push_back({right[i], lo, hi, pend});
      continue;
    }
    const int lh = std::min(hi, (int)s[i]), rl = std::max(lo, (int)s[i]);
    const bool l = lo < lh, r = rl < hi;
    if (l) todo.push_back({left[i], lo, lh, pend + (r ? 1 : 0)});
    if (r) todo.push_back({right[i], rl, hi, pend});
  }
  return need;
}

}  // namespace sbag
