// sbag_spread_plan.h — host arithmetic of the per-row quantiles (sbag_host.cpp,
// sbag_spread.hip): the forest-wide dictionary of leaf values, a leaf's rank in it, the sort
// width of a row's keys and the row tile of k_quant_tiled.  Plain host code with no HIP in it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sbag {

constexpr int kSpreadMaxTrees = 1024;  // keys of one wave sort: 16 a lane
constexpr int kSpreadMaxProbs = 64;    // one lane of a wave per probability
constexpr int kSpreadTileRows = 512;   // the row tile predict_tiled_lds sizes
constexpr size_t kSpreadLdsCap = 160 * 1024 - 512;  // = plan_tiled's bound
constexpr size_t kSpreadMinChunk = 4096;            // = plan_tiled's smallest chunk

inline double spread_canon(double v) { return v == 0.0 ? 0.0 : v; }  // -0.0 -> 0.0

// the sorted distinct canonical leaf values of a forest; false: a leaf predicts NaN
inline bool spread_dictionary(const std::vector<double>& leaves, std::vector<double>& dict) {
  dict.clear();
  dict.reserve(leaves.size());
  for (double p : leaves) {
    if (p != p) return false;
    dict.push_back(spread_canon(p));
  }
  std::sort(dict.begin(), dict.end());
  dict.erase(std::unique(dict.begin(), dict.end()), dict.end());
  return true;
}

inline uint32_t spread_rank(const std::vector<double>& dict, double v) {
  return (uint32_t)(std::lower_bound(dict.begin(), dict.end(), spread_canon(v)) - dict.begin());
}

// keys of a row's sort: the power of two >= max(L, 64)
inline int spread_lpad(int L) {
  int p = 64;
  while (p < L) p <<= 1;
  return p;
}

// the u16 rank matrix [L][R + 2] of a tile: trees major, two keys of padding a tree so that a
// wave reading one row's column (key p from lane p % 64) steps one LDS bank per key
inline size_t spread_matrix_lds(int L, int R) { return ((size_t)L * (R + 2) * 2 + 15) & ~(size_t)15; }

// the row tile of k_quant_tiled: the largest of 512, 256, 128, 64 whose rows (at `pitch`
// bytes), rank matrix and a chunk of at least 4 KB fit the LDS; 0: none does
inline int spread_tile_rows(int pitch, int L) {
  for (int R = kSpreadTileRows; R >= 64; R >>= 1)
    if ((size_t)R * pitch + spread_matrix_lds(L, R) + kSpreadMinChunk <= kSpreadLdsCap) return R;
  return 0;
}

}  // namespace sbag
