// gbm_plan_check.cpp — stand-alone sweep of sbag_gbm_plan.h (no HIP, no device): k_gbm_step's
// loss arithmetic against the formulas written plainly (GBMRegressor.scala:93-118) with the
// host's own division and sqrt, bit for bit; code cuts against `value <= threshold`; the sizes.
// Operands: +-0.0, denormals, neighbours one ulp apart, huge values, infinities, NaN, random bits.
#include <cstdio>
#include <limits>
#include <vector>

#include "sbag_gbm_plan.h"

using namespace sbag;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static bool same(double a, double b) { return (a != a && b != b) || std::memcmp(&a, &b, 8) == 0; }

static double plain_residual(int loss, double alpha, double y, double p) {
  const double d = y - p;
  if (loss == kGbmSquared) return -(-d);
  if (loss == kGbmAbsolute) return -(-(d > 0 ? 1.0 : d < 0 ? -1.0 : d));
  if (loss == kGbmHuber) return -(-d / std::sqrt(1.0 + (d / alpha) * (d / alpha)));
  return -(p > y ? -(alpha - 1.0) : -alpha);
}
static double plain_loss(int loss, double alpha, double y, double p) {
  const double d = y - p;
  if (loss == kGbmSquared) return d * d / 2.0;
  if (loss == kGbmAbsolute) return std::fabs(d);
  if (loss == kGbmHuber) return (alpha * alpha) * (std::sqrt(1.0 + (d / alpha) * (d / alpha)) - 1.0);
  return p > y ? (alpha - 1.0) * d : alpha * d;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> pool = {0.0, -0.0, 1.0, -1.0, 1e-310, -3e-310, 4.9e-324, 2.5e-308, 1e-160, 0.3, -0.7,
                              1.0 / 3.0, std::nextafter(1.0, 2.0), 1e154, -1e200, 1e308, inf, -inf, nan, 8388608.0};
  for (int i = 0; i < 200; i++) {
    uint64_t b = rnd();
    if (i % 4 == 0) b &= 0x800FFFFFFFFFFFFFull;  // a denormal
    double v;
    std::memcpy(&v, &b, 8);
    pool.push_back(v == v ? v : 1.5);
  }
  long cases = 0, failures = 0;
  for (double alpha : {0.9, 1.0 / 3.0, 0.5, 1e-3})
    for (int loss = kGbmSquared; loss <= kGbmQuantile; loss++)
      for (double y : pool)
        for (double p : pool) {
          cases += 2;
          if (!same(gbm_residual(loss, alpha, y, p), plain_residual(loss, alpha, y, p)) ||
              !same(gbm_loss(loss, alpha, y, p), plain_loss(loss, alpha, y, p))) {
            failures++;
            std::printf("loss %d alpha %a y %a p %a\n", loss, alpha, y, p);
          }
        }
  for (int i = 0; i < 2000000; i++) {  // gbm_sqrt on [1, inf): where huber takes it
    uint64_t b = (rnd() & 0x7FFFFFFFFFFFFFFFull) % 0x4010000000000000ull + 0x3FF0000000000000ull;
    double x;
    std::memcpy(&x, &b, 8);
    cases++;
    if (!same(gbm_sqrt(x), std::sqrt(x))) failures++;
  }
  // cuts: code < cut  <=>  dict[code] <= threshold
  std::vector<double> dict = {-inf, -2.5, -1e-310, 0.0, 4.9e-324, 1.0, std::nextafter(1.0, 2.0), 7.0, inf};
  for (double t : pool)
    for (size_t n = 0; n <= dict.size(); n++) {
      const uint32_t cut = gbm_code_cut(dict.data(), n, t);
      for (size_t c = 0; c < n; c++, cases++)
        if ((c < cut) != (dict[c] <= t)) failures++;
    }
  // the plan: a tile is whole lanes, a staged tree fits the LDS the launch asks for
  if (kGbmTileRows != kGbmBlock * kGbmLaneRows || sizeof(GbmNode) != 16 || kGbmRedBytes % 16) failures++;
  if (!gbm_tree_in_lds(kGbmLdsNodes) || gbm_tree_in_lds(kGbmLdsNodes + 1)) failures++;
  if (gbm_lds_bytes(kGbmLdsNodes) > 64 * 1024 || gbm_lds_bytes(kGbmLdsNodes + 1) != kGbmRedBytes) failures++;
  if (gbm_blocks(1) != 1 || gbm_blocks(kGbmTileRows) != 1 || gbm_blocks(kGbmTileRows + 1) != 2) failures++;
  std::printf("gbm_plan_check: %ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
