// The MFMA root's label digit planes (k_hist_mfma, sbag_mfma.hip): which encoding the host
// picks for a label image range, and the digits of one label.  Pure integer arithmetic, no
// HIP, so that tests/c/mfma_plan_check.cpp can sweep it in a program of its own.
//
// The planes hold the digits of k + dK0, either
//   unsigned 7-bit: dK0 = -kmin, k + dK0 >= 0, plane j = ((k + dK0) >> 7j) & 127, or
//   balanced base 256: dK0 = -(the range's midpoint), int8 digits d_j in [-128, 127] with
//     k + dK0 = Σ d_j 256^j (each digit the low byte read as signed, the rest carried up); n
//     of them cover [-128 m, 127 m], m = (256^n - 1) / 255,
// whichever needs fewer planes.  |count x digit| <= 127 x 128 keeps a 65536-row int32 sum exact.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBAG_PLAN_HD __host__ __device__
#else
#define SBAG_PLAN_HD
#endif

struct MfmaDigitPlan {
  int nd1;          // planes of k + dK0
  bool balanced;    // balanced base-256 digits (else unsigned 7-bit)
  int dbits;        // the digit base's bits: 8 balanced, 7 unsigned
  int64_t dK0;      // the digits are of k + dK0
};

// kmin..kmax: the labels' fixed-point range (|k| < 2^23); force: 7 / 8 takes that encoding
// (SBAG_MFMA_DIGITS, tests), anything else the one with fewer planes (unsigned on a tie)
inline MfmaDigitPlan mfma_digit_plan(int64_t kmin, int64_t kmax, int force) {
  int nd1 = 1;
  while (nd1 < 10 && ((uint64_t)(kmax - kmin) >> (7 * nd1)) != 0) nd1++;
  const int64_t kmid = kmin + (kmax - kmin) / 2;
  int nds = 1;
  for (; nds < 8; nds++) {
    const int64_t m = (((int64_t)1 << (8 * nds)) - 1) / 255;
    if (kmin - kmid >= -128 * m && kmax - kmid <= 127 * m) break;
  }
  const bool balanced = force == 8 || (force != 7 && nds < nd1);
  return MfmaDigitPlan{balanced ? nds : nd1, balanced, balanced ? 8 : 7, balanced ? -kmid : -kmin};
}

// the nd1 digits of v = k + dK0 to out[j * stride], j < nd1 (unsigned: v >= 0)
SBAG_PLAN_HD inline void mfma_label_digits(int64_t v, int nd1, bool balanced, uint8_t* out, int64_t stride) {
  if (balanced) {
    for (int j = 0; j < nd1; j++) {
      const int64_t d = (int64_t)(int8_t)(uint8_t)(v & 0xFF);
      out[(int64_t)j * stride] = (uint8_t)d;
      v = (v - d) / 256;  // (exact)
    }
  } else {
    const uint64_t kp = (uint64_t)v;
    for (int j = 0; j < nd1; j++) out[(int64_t)j * stride] = (uint8_t)((kp >> (7 * j)) & 127u);
  }
}
