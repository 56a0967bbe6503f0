// sbag_stack_plan.h — host arithmetic of stacking (sbag_host.cpp): a base tree's leaf values as
// ranks, a stack node's threshold as a rank cut, and a level-1 feature's dictionary from its
// tree's reached leaves.  Plain host code with no HIP in it, so tests/c/stack_plan_check.cpp
// sweeps it on its own (also under ASan + UBSan).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace sbag {

inline double stack_canon(double v) { return v == 0.0 ? 0.0 : v; }  // -0.0 -> 0.0

// the sorted distinct values of a tree's leaf predictions (-0.0 == 0.0; a NaN prediction, which
// compares false with every threshold, is left out and ranks past every value)
inline std::vector<double> stack_sorted_values(const std::vector<double>& leaves) {
  std::vector<double> v;
  for (double p : leaves)
    if (p == p) v.push_back(stack_canon(p));
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}

// rank of a leaf value among its tree's values `vals` (stack_sorted_values)
inline uint32_t stack_rank_of(const std::vector<double>& vals, double v) {
  if (v != v) return (uint32_t)vals.size();
  return (uint32_t)(std::lower_bound(vals.begin(), vals.end(), stack_canon(v)) - vals.begin());
}

// a stack node's cut: prediction <= threshold <=> rank < cut (cut - 1 = the largest rank whose
// value is <= threshold); nothing is <= NaN
inline uint32_t stack_rank_cut(const std::vector<double>& vals, double thr) {
  if (thr != thr) return 0;
  return (uint32_t)(std::upper_bound(vals.begin(), vals.end(), thr) - vals.begin());
}

// One level-1 feature's dictionary from its tree's leaf values lv[0, nl) and reached flags: the
// sorted distinct values of the reached leaves, code[i] = leaf i's code (0 for a leaf no row
// reaches: never read).  false: a reached leaf predicts NaN.
inline bool stack_leaf_dict(const double* lv, const uint32_t* present, int nl, std::vector<double>& dict,
                            uint16_t* code) {
  dict.clear();
  for (int i = 0; i < nl; i++)
    if (present[i]) {
      if (lv[i] != lv[i]) return false;
      dict.push_back(stack_canon(lv[i]));
    }
  std::sort(dict.begin(), dict.end());
  dict.erase(std::unique(dict.begin(), dict.end()), dict.end());
  for (int i = 0; i < nl; i++)
    code[i] = present[i] ? (uint16_t)(std::lower_bound(dict.begin(), dict.end(), stack_canon(lv[i])) - dict.begin())
                         : (uint16_t)0;
  return true;
}

}  // namespace sbag
