// Bit budget of the packed LDS histogram word (fit_range_impl's "LDS packing"): pure host
// arithmetic, no HIP, so that tests/c/budget_check.cpp can sweep it in a program of its own.
//
// A variance word is (c << cshift) + c * (k + K0) with K0 = -kmin: between two flushes the
// low field holds sum c (k - kmin) <= flush_limit * cmax * (kspan - 1) and the count field
// sum c <= flush_limit * cmax.  The exact fallback's sum-of-squares plane holds sum c k^2 in
// an unsigned 64-bit word of its own.  A gini word is a 32-bit count.
#pragma once
#include <cmath>
#include <cstdint>

struct HistWordBudget {
  int64_t flush_limit;  // entries of one node between two flushes (a power of two); 0: none fits
  int cshift;           // bit of the count field (variance words)
  bool int_range;       // the integer engine cannot hold the sums: refit on the fp64 engine
};

// kmin..kmax: the labels' fixed-point range (|k| < 2^23); cmax: the largest draw count (<= 255);
// N: rows; f64: the fp64 engine's image (no squares plane, no 2^53 bound); flush_start: where
// the search for flush_limit starts (a power of two, 2^22 unless SBAG_HIST_FLUSH_LIMIT lowers it)
inline HistWordBudget hist_word_budget(int64_t kmin, int64_t kmax, unsigned int cmax, int64_t N,
                                       bool gini, bool f64, int64_t flush_start) {
  typedef unsigned __int128 u128;
  const u128 kspan = (u128)(kmax - kmin + 1);
  const int64_t amin = kmin < 0 ? -kmin : kmin, amax = kmax < 0 ? -kmax : kmax;
  const u128 kabs = (u128)(amin > amax ? amin : amax);
  int64_t flush_limit = flush_start;
  int cshift = 40;
  for (;; flush_limit /= 2) {
    if (flush_limit < 256) return HistWordBudget{0, cshift, !gini && !f64};
    const u128 wmax = (u128)flush_limit * cmax;
    if (gini) {
      if (wmax < ((u128)1 << 32)) break;
      continue;
    }
    // the smallest count bit the low field stays under: wmax (kspan - 1) < 2^cshift.
    // (ceil(log2(wmax * kspan + 1.0)) until tests/c/budget_check.cpp: one bit too many when
    // wmax * kspan is a power of two, and then half the flush_limit the word has room for)
    const u128 low = wmax * (kspan - 1);
    for (cshift = 1; cshift < 64 && (low >> cshift) != 0; cshift++) {
    }
    // (the sum-of-squares plane of the exact fallback needs wmax k^2 in 64 bits; the fp64
    // path never builds it)
    if (cshift <= 63 && wmax < ((u128)1 << (64 - cshift)) && (f64 || wmax * kabs * kabs < ((u128)1 << 64))) break;
  }
  // the row-lane histogram builds the word as (c << cshift) + c*(k + K0) with a 32-bit
  // low half: raise cshift to 32 when the count field keeps room for flush_limit * cmax
  if (!gini && cshift < 32 && (double)flush_limit * cmax < 4294967296.0) cshift = 32;
  if (!gini && !f64 && (double)N * cmax * (double)kabs * (double)kabs >= std::ldexp(1.0, 53))
    return HistWordBudget{flush_limit, cshift, true};
  return HistWordBudget{flush_limit, cshift, false};
}
