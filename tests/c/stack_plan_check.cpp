// stack_plan_check.cpp — stand-alone sweep of sbag_stack_plan.h (no HIP, no device): a base
// tree's leaf values as ranks and a stack node's threshold as a rank cut must reproduce the fp64
// compare the reference makes (prediction <= threshold), and a level-1 feature's dictionary must
// be what a sort + unique over the reached values gives.  Leaf values and thresholds are drawn
// from a pool with the awkward ones in it: -0.0 and 0.0, equal values, infinities, NaN,
// denormals, neighbours one ulp apart.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <set>
#include <vector>

#include "sbag_stack_plan.h"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> pool = {0.0, -0.0, 1.0, -1.0, 1.5, std::nextafter(1.5, 2.0), std::nextafter(1.5, 1.0),
                              inf, -inf, nan, 4.9e-324, -4.9e-324, 1e300, -1e300, 7.0, 7.0, 10.0, 2.5, -1.5};
  for (int i = 0; i < 24; i++) pool.push_back((double)((int64_t)(rnd() % 41) - 20) / 4.0);
  long cases = 0, compares = 0, failures = 0;
  for (int trial = 0; trial < 4000; trial++) {
    const int nl = 1 + (int)(rnd() % 40);
    std::vector<double> lv(nl);
    std::vector<uint32_t> present(nl);
    bool nan_reached = false;
    for (int i = 0; i < nl; i++) {
      lv[i] = pool[rnd() % pool.size()];
      present[i] = (rnd() % 4) != 0;
      if (trial % 3 == 0 && lv[i] != lv[i]) lv[i] = 3.0;  // a third of the trees without NaN leaves
      nan_reached = nan_reached || (present[i] && lv[i] != lv[i]);
    }
    // ranks and cuts: rank(v) < cut(t)  <=>  v <= t, for every leaf and every threshold of the pool
    const std::vector<double> vals = sbag::stack_sorted_values(lv);
    for (size_t k = 0; k < vals.size(); k++)
      if (vals[k] != vals[k] || (vals[k] == 0.0 && std::signbit(vals[k])) || (k && !(vals[k - 1] < vals[k]))) failures++;
    for (int i = 0; i < nl; i++) {
      const uint32_t r = sbag::stack_rank_of(vals, lv[i]);
      if (lv[i] == lv[i]) {
        if (r >= vals.size() || !(vals[r] == lv[i])) failures++;
      } else if (r != vals.size()) {
        failures++;
      }
      for (double t : pool) {
        compares++;
        if ((r < sbag::stack_rank_cut(vals, t)) != (lv[i] <= t)) {
          failures++;
          std::printf("rank/cut: leaf %a threshold %a\n", lv[i], t);
        }
      }
    }
    // the dictionary of the reached leaves
    std::vector<double> dict;
    std::vector<uint16_t> code(nl, 0xffff);
    const bool ok = sbag::stack_leaf_dict(lv.data(), present.data(), nl, dict, code.data());
    cases++;
    if (ok == nan_reached) {
      failures++;
      continue;
    }
    if (!ok) continue;
    std::set<double> want;  // (-0.0 and 0.0 compare equal: one element)
    for (int i = 0; i < nl; i++)
      if (present[i]) want.insert(lv[i] == 0.0 ? 0.0 : lv[i]);
    if (dict.size() != want.size()) failures++;
    size_t k = 0;
    for (double w : want) {
      if (k < dict.size() && !same_bits(dict[k], w)) failures++;
      k++;
    }
    for (int i = 0; i < nl; i++) {
      if (!present[i]) {
        if (code[i] != 0) failures++;
      } else if (code[i] >= dict.size() || !(dict[code[i]] == lv[i])) {
        failures++;
      }
    }
  }
  std::printf("stack_plan_check: %ld cases, %ld compares, %ld failures\n", cases, compares, failures);
  return failures ? 1 : 0;
}
