// Sweep of hist_word_budget (spark-bagging_amd/csrc/sbag_budget.h) at the edges of the packed
// LDS word's bit budget; every property is checked in unsigned __int128, no doubles.
// Built and run by tests/test_hist_budget_host.py (plain and under ASan/UBSan).
// Exit status 0 and a last line "budget_check: N cases (...), 0 failures" when every case holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sbag_budget.h"

typedef unsigned __int128 u128;

static u128 pow2(int b) { return (u128)1 << b; }

// can one workgroup hold f entries of one node between two flushes?
static bool feasible(u128 f, u128 cmax, u128 kspan, u128 kabs, bool gini, bool f64) {
  const u128 w = f * cmax;
  if (gini) return w < pow2(32);
  if (!f64 && w * kabs * kabs >= pow2(64)) return false;
  for (int c = 1; c <= 63; c++)
    if (w * (kspan - 1) < pow2(c) && w < pow2(64 - c)) return true;
  return false;
}

static long long failures = 0;

static void fail(const char* what, int64_t kmin, int64_t kmax, unsigned cmax, int64_t N, int mode,
                 int64_t fs, const HistWordBudget& b) {
  if (failures++ < 25)
    fprintf(stderr, "FAIL %s: k [%lld, %lld] cmax %u N %lld %s flush_start %lld -> flush %lld cshift %d "
            "int_range %d\n", what, (long long)kmin, (long long)kmax, cmax, (long long)N,
            mode == 0 ? "gini" : mode == 1 ? "variance" : "fp64", (long long)fs, (long long)b.flush_limit,
            b.cshift, (int)b.int_range);
}

int main() {
  std::vector<int64_t> ks{0, 1, -1};
  const int ps[] = {7, 8, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23};
  for (int p : ps)
    for (int64_t d = -1; d <= 1; d++) {
      const int64_t k = ((int64_t)1 << p) + d;
      if (k < ((int64_t)1 << 23)) {  // |k| < 2^23: the labels' fixed-point image
        ks.push_back(k);
        ks.push_back(-k);
      }
    }
  const unsigned cmaxs[] = {1, 2, 9, 127, 128, 255};
  const int64_t Ns[] = {1, (int64_t)1 << 10, (int64_t)1 << 20, (int64_t)1 << 30, ((int64_t)1 << 32) - 1};
  const int64_t starts[] = {(int64_t)1 << 22, (int64_t)1 << 16, 256};
  long long cases = 0, ranged = 0, raised = 0;
  for (int64_t kmin : ks)
    for (int64_t kmax : ks) {
      if (kmin > kmax) continue;  // (one-sided ranges and [-2^22, 2^22] are among the pairs)
      const u128 kspan = (u128)(kmax - kmin + 1);
      const int64_t ka = -kmin > kmax ? -kmin : kmax, kb = kmin > -kmax ? kmin : -kmax;
      const u128 kabs = (u128)(ka > kb ? ka : kb);
      for (unsigned cmax : cmaxs)
        for (int64_t N : Ns)
          for (int64_t fs : starts)
            for (int mode = 0; mode < 3; mode++) {
              const bool gini = mode == 0, f64 = mode == 2, integer = mode == 1;
              const HistWordBudget b = hist_word_budget(kmin, kmax, cmax, N, gini, f64, fs);
              cases++;
              const bool over53 = (u128)N * cmax * kabs * kabs >= pow2(53);
              if (integer && b.int_range != over53) fail("int_range != (N cmax kabs^2 >= 2^53)", kmin, kmax, cmax, N, mode, fs, b);
              if (!integer && b.int_range) fail("int_range off the integer engine", kmin, kmax, cmax, N, mode, fs, b);
              if (b.int_range) {
                ranged++;
                continue;
              }
              if (b.flush_limit == 0) {  // refused: nothing may fit
                if (feasible(256, cmax, kspan, kabs, gini, f64)) fail("refused though 256 entries fit", kmin, kmax, cmax, N, mode, fs, b);
                continue;
              }
              const u128 f = (u128)b.flush_limit, w = f * cmax;
              if (b.flush_limit < 256 || b.flush_limit > fs || (b.flush_limit & (b.flush_limit - 1)))
                fail("flush_limit not a power of two in [256, flush_start]", kmin, kmax, cmax, N, mode, fs, b);
              if (gini) {
                if (!(w < pow2(32))) fail("gini count wraps 32 bits", kmin, kmax, cmax, N, mode, fs, b);
              } else {
                if (b.cshift < 1 || b.cshift > 63) {
                  fail("cshift outside [1, 63]", kmin, kmax, cmax, N, mode, fs, b);
                  continue;
                }
                if (!(w * (kspan - 1) < pow2(b.cshift))) fail("low field carries into the count", kmin, kmax, cmax, N, mode, fs, b);
                if (!(w < pow2(64 - b.cshift))) fail("count field wraps", kmin, kmax, cmax, N, mode, fs, b);
                if (integer && !(w * kabs * kabs < pow2(64))) fail("sum of squares wraps 64 bits", kmin, kmax, cmax, N, mode, fs, b);
                // rl_words: __umul24(c, k + K0) and its 32-bit low half
                if (!(kspan - 1 < pow2(24))) fail("k + K0 past 24 bits", kmin, kmax, cmax, N, mode, fs, b);
                if (!((u128)cmax * (kspan - 1) < pow2(32))) fail("c (k + K0) past 32 bits", kmin, kmax, cmax, N, mode, fs, b);
                if (b.cshift == 32) raised++;
              }
              // the largest power of two: twice as many entries must not fit
              if (2 * b.flush_limit <= fs && feasible(2 * f, cmax, kspan, kabs, gini, f64))
                fail("flush_limit gives away range", kmin, kmax, cmax, N, mode, fs, b);
            }
    }
  printf("budget_check: %lld cases (%lld handed to fp64, %lld at cshift 32), %lld failures\n", cases, ranged,
         raised, failures);
  return failures ? 1 : 0;
}
