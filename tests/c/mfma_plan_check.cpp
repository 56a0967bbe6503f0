// Sweep of mfma_digit_plan / mfma_label_digits (spark-bagging_amd/csrc/sbag_mfma_plan.h): the MFMA
// root's label digit planes at the edges of every plane count, for every image range with
// |k| < 2^23 and each forced encoding; every bound is checked in __int128.
// Built and run by tests/test_mfma_plan_host.py (plain and under ASan/UBSan).
// Exit status 0 and a last line "mfma_plan_check: N ranges, M labels, max planes auto A / 7-bit
// U / balanced B, 0 failures" when every case holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sbag_mfma_plan.h"

typedef __int128 i128;

static const int64_t kLim = ((int64_t)1 << 23) - 1;  // |k| <= kLim: the labels' fixed-point image
static const int64_t kSlice = 65536;                 // rows of one workgroup (kMfSlice)
static const int64_t kCount = 127;                   // the largest count the gate lets through
static const int64_t kRows = (int64_t)1 << 30;       // N <= 2^30

static long long failures = 0, ranges = 0, labels = 0;
static int max_nd[3] = {0, 0, 0};

static void fail(const char* what, int64_t kmin, int64_t kmax, int force, const MfmaDigitPlan& p, int64_t k) {
  if (failures++ < 25)
    fprintf(stderr, "FAIL %s: k [%lld, %lld] force %d -> nd1 %d balanced %d dbits %d dK0 %lld (k %lld)\n", what,
            (long long)kmin, (long long)kmax, force, p.nd1, (int)p.balanced, p.dbits, (long long)p.dK0,
            (long long)k);
}

// m = (256^n - 1) / 255: n balanced digits cover [-128 m, 127 m]
static int64_t bal_m(int n) { return (((int64_t)1 << (8 * n)) - 1) / 255; }

static void check_label(int64_t kmin, int64_t kmax, int force, const MfmaDigitPlan& p, int64_t k) {
  if (k < kmin || k > kmax) return;
  labels++;
  uint8_t d[16];
  for (int j = 0; j < 16; j++) d[j] = 0xAA;
  const int64_t v = k + p.dK0;
  mfma_label_digits(v, p.nd1, p.balanced, d, 1);
  i128 sum = 0;
  for (int j = 0; j < p.nd1; j++) {
    const int64_t dj = p.balanced ? (int64_t)(int8_t)d[j] : (int64_t)d[j];
    if (!p.balanced && dj > 127) fail("unsigned digit past 127", kmin, kmax, force, p, k);
    // (a balanced digit is an int8 by construction: [-128, 127]); the int32 accumulator of a slice
    const i128 acc = (i128)kCount * (dj < 0 ? -dj : dj) * kSlice;
    if (!(acc < ((i128)1 << 31))) fail("127 |d| 65536 >= 2^31", kmin, kmax, force, p, k);
    sum += (i128)dj * ((i128)1 << (p.dbits * j));
  }
  if (sum != (i128)v) fail("digits do not sum to k + dK0", kmin, kmax, force, p, k);
  if (d[p.nd1] != 0xAA) fail("wrote past plane nd1 - 1", kmin, kmax, force, p, k);
}

static void check_range(int64_t kmin, int64_t kmax) {
  if (kmin > kmax || kmin < -kLim || kmax > kLim) return;
  ranges++;
  MfmaDigitPlan pl[3];
  const int forces[3] = {0, 7, 8};
  for (int fi = 0; fi < 3; fi++) {
    const int force = forces[fi];
    const MfmaDigitPlan p = pl[fi] = mfma_digit_plan(kmin, kmax, force);
    if (p.nd1 > max_nd[fi]) max_nd[fi] = p.nd1;
    if (force == 7 && p.balanced) fail("forced 7 took balanced digits", kmin, kmax, force, p, 0);
    if (force == 8 && !p.balanced) fail("forced 8 took unsigned digits", kmin, kmax, force, p, 0);
    if (p.dbits != (p.balanced ? 8 : 7)) fail("dbits", kmin, kmax, force, p, 0);
    if (p.dK0 != (int64_t)(int32_t)p.dK0) fail("dK0 does not fit int32", kmin, kmax, force, p, 0);
    if (p.nd1 < 1 || p.nd1 > 4) {
      fail("plane count outside [1, 4]", kmin, kmax, force, p, 0);
      continue;
    }
    const int64_t lo = kmin + p.dK0, hi = kmax + p.dK0;  // the range of k + dK0
    if (p.balanced) {
      // nd1 digits hold the range, nd1 - 1 do not
      if (lo < -128 * bal_m(p.nd1) || hi > 127 * bal_m(p.nd1)) fail("balanced range past nd1 digits", kmin, kmax, force, p, 0);
      if (p.nd1 > 1 && lo >= -128 * bal_m(p.nd1 - 1) && hi <= 127 * bal_m(p.nd1 - 1))
        fail("balanced plane count not minimal", kmin, kmax, force, p, 0);
      // the offset is the midpoint: the two sides differ by at most one
      if (hi + lo < 0 || hi + lo > 1) fail("dK0 is not the midpoint", kmin, kmax, force, p, 0);
    } else {
      if (lo != 0) fail("unsigned digits not of k - kmin", kmin, kmax, force, p, 0);
      if (((uint64_t)hi >> (7 * p.nd1)) != 0) fail("unsigned range past nd1 digits", kmin, kmax, force, p, 0);
      if (p.nd1 > 1 && ((uint64_t)hi >> (7 * (p.nd1 - 1))) == 0)
        fail("unsigned plane count not minimal", kmin, kmax, force, p, 0);
    }
    // k_hist_mfma's recombination of one slice, sk = Σ v_j 2^(dbits j) - K0 cnt in int64, and the
    // histogram word Σ c k over N <= 2^30 rows
    const i128 dmax = p.balanced ? 128 : 127;
    i128 sk = 0;
    for (int j = 0; j < p.nd1; j++) sk += (kCount * dmax * kSlice) << (p.dbits * j);
    const i128 a0 = p.dK0 < 0 ? -(i128)p.dK0 : (i128)p.dK0;
    sk += a0 * kCount * kSlice;
    if (!(sk < ((i128)1 << 63))) fail("slice recombination past int64", kmin, kmax, force, p, 0);
    const i128 vmax = (-lo > hi ? -lo : hi), kabs = (-kmin > kmax ? -kmin : kmax);
    if (!((i128)kRows * kCount * (vmax + a0 + kabs) < ((i128)1 << 63)))
      fail("histogram word past int64", kmin, kmax, force, p, 0);
    // labels: both ends, around the midpoint, and every carry point of either encoding
    const int64_t mid = kmin + (kmax - kmin) / 2;
    for (int64_t e = -2; e <= 2; e++) {
      check_label(kmin, kmax, force, p, kmin + e);
      check_label(kmin, kmax, force, p, kmax + e);
      check_label(kmin, kmax, force, p, mid + e);
    }
    static const int64_t mult[] = {1, 63, 64, 127, 128, 129, 255, 256, 257, 32639, 32640, 32767, 32768, 32896, 32897};
    for (int sh = 0; sh <= 21; sh++)
      if (sh % 7 == 0 || sh % 8 == 0)  // (digit j of either base)
        for (int64_t mu : mult)
          for (int sg = -1; sg <= 1; sg += 2)
            for (int64_t e = -1; e <= 1; e++) check_label(kmin, kmax, force, p, sg * (mu * ((int64_t)1 << sh)) + e - p.dK0);
  }
  // auto takes the smaller plane count (unsigned on a tie)
  const int want = pl[2].nd1 < pl[1].nd1 ? pl[2].nd1 : pl[1].nd1;
  if (pl[0].nd1 != want || pl[0].balanced != (pl[2].nd1 < pl[1].nd1)) fail("auto is not the smaller plane count", kmin, kmax, 0, pl[0], 0);
}

int main() {
  // spans kmax - kmin at the edges of every plane count of either encoding
  std::vector<int64_t> spans{0, 1, 2, 3};
  for (int n = 1; n <= 4; n++)
    for (int64_t e = -2; e <= 2; e++) {
      spans.push_back(((int64_t)1 << (7 * n)) + e);                                  // unsigned: 2^(7n) - 1 | 2^(7n)
      if (n <= 3) {
        spans.push_back(254 * bal_m(n) + e);  // balanced about the midpoint: 254 m | 254 m + 1
        spans.push_back(255 * bal_m(n) + e);  // (the digits' own span)
      }
    }
  spans.push_back(2 * kLim);
  spans.push_back(2 * kLim - 1);
  for (int64_t span : spans) {
    if (span < 0 || span > 2 * kLim) continue;
    // where the range sits: both limits, about zero (even and odd midpoints), one-sided
    const int64_t los[] = {-kLim, kLim - span, -(span / 2), -(span / 2) - 1, -(span / 2) + 1, 0, 1, -span, -span - 1,
                           12345 - span / 2, -54321 - span / 2};
    for (int64_t lo : los) check_range(lo, lo + span);
  }
  // and every small span, where the two encodings trade places
  for (int64_t span = 0; span <= 70000; span++) {
    check_range(-(span / 3), -(span / 3) + span);
    check_range(kLim - span, kLim);
  }
  printf("mfma_plan_check: %lld ranges, %lld labels, max planes auto %d / 7-bit %d / balanced %d, %lld failures\n",
         ranges, labels, max_nd[0], max_nd[1], max_nd[2], failures);
  return failures ? 1 : 0;
}
