// sbag_div.h — fp64 division rounded as IEEE 754 (the JVM, the host) rounds it when the
// quotient is subnormal.
//
// The GPU's fp64 division is a sequence (v_div_scale, v_rcp, Newton steps, v_div_fmas,
// v_div_fixup) whose last step rounds q + r * rcp once -- an approximation of the quotient
// good to about 2^-100, not the quotient.  For a normal quotient that is enough: a / b is
// never a midpoint of two doubles.  A subnormal quotient can be one (Spark's impurity of a
// node whose labels are near 1e-160: (7.5 ulp) rounds to even, 8), and there the sequence
// goes either way (measured: tests/test_gpu_f64_label_range.py, cpusmall y pi 2^-537 and
// 2^-525, a gain one ulp off).  div_rn takes the sequence's quotient unless it is below
// 2^-1021, and then rounds by hand: the operands scaled into [1, 2) (exact), their quotient
// qn (normal: correctly rounded), the sign of the exact remainder an - qn bn (one fma), and
// qn shifted onto the subnormal grid with round-to-nearest-even, the remainder breaking the
// tie when qn itself sits on a midpoint.  (If qn is not on a midpoint, the quotient lies on
// qn's side of every midpoint: midpoints of the subnormal grid are doubles, and rounding to
// 53 bits is monotonic.)
//
// Plain host + device code (tests/c/div_check.cpp sweeps div_rn_small on the host against
// the host's own division).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define SBAG_HD __host__ __device__
#else
#define SBAG_HD
#endif

namespace sbag {

// |v| = m 2^(e - 52), m in [2^52, 2^53), for finite v != 0 (subnormals too)
SBAG_HD inline void div_split(double v, uint64_t* m, int* e) {
  int adj = 0;
  v = std::fabs(v);
  if (v < 0x1p-1000) {  // out of the subnormal range first: exact
    v *= 0x1p200;
    adj = -200;
  }
  uint64_t bits;
  std::memcpy(&bits, &v, 8);
  *m = (bits & ((1ull << 52) - 1)) | (1ull << 52);
  *e = (int)((bits >> 52) & 0x7FF) - 1023 + adj;
}

// a / b for finite a != 0, b != 0 with |a / b| < 2^-1021, by hand
SBAG_HD inline double div_rn_small(double a, double b) {
  uint64_t ma, mb;
  int ea, eb;
  div_split(a, &ma, &ea);
  div_split(b, &mb, &eb);
  const double an = (double)ma * 0x1p-52, bn = (double)mb * 0x1p-52;  // in [1, 2), exact
  const double qn = an / bn;                                          // in (1/2, 2)
  const double r = std::fma(-qn, bn, an);                             // exact
  uint64_t mq;
  int eq;
  div_split(qn, &mq, &eq);
  // |a / b| ~ mq 2^(eq - 52 + ea - eb) = mq 2^-sh units of 2^-1074
  const int sh = -(eq - 52 + ea - eb + 1074);
  uint64_t n;
  if (sh <= 0) {
    n = mq << (sh < -10 ? 10 : -sh);  // (only just below 2^-1021: sh is 0 or -1)
  } else if (sh >= 64) {
    n = 0;
  } else {
    const uint64_t fl = mq >> sh, rem = mq & ((1ull << sh) - 1), half = 1ull << (sh - 1);
    const bool up = rem > half || (rem == half && (r > 0.0 || (r == 0.0 && (fl & 1))));
    n = fl + (up ? 1 : 0);
  }
  const double q = (double)n * 0x1p-537 * 0x1p-537;  // n 2^-1074: n < 2^55 even past 2^53, exact
  return ((a < 0.0) != (b < 0.0)) ? -q : q;
}

SBAG_HD inline double div_rn(double a, double b) {
  const double q = a / b;
  if (!(std::fabs(q) < 0x1p-1021) || a == 0.0 || std::isinf(b)) return q;  // (NaN: returned)
  return div_rn_small(a, b);
}

}  // namespace sbag
