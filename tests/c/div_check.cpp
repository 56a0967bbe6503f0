// div_check — div_rn_small (spark-bagging_amd/csrc/sbag_div.h: the by-hand rounding of a
// subnormal quotient the kernels use where the GPU's division sequence is not exact) against
// the host's IEEE division, bit for bit: small multiples of the smallest subnormal over small
// counts (exact ties: k + 1/2 ulps), random operands of every magnitude whose quotient is
// below 2^-1021, subnormal divisors, both signs, quotients that round to 0 and to 2^-1022.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "sbag_div.h"

static uint64_t bits_of(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static long long cases = 0, ties = 0, failures = 0;

static void check(double a, double b) {
  const double want = a / b;
  if (!(std::fabs(want) < 0x1p-1021) || a == 0.0) return;
  if (std::isinf(b)) {  // div_rn keeps the sequence's +-0; div_rn_small is for finite operands
    if (bits_of(sbag::div_rn(a, b)) != bits_of(want)) failures++;
    return;
  }
  cases++;
  const double got = sbag::div_rn_small(a, b);
  if (bits_of(got) != bits_of(want)) {
    if (failures++ < 20) std::printf("FAIL %a / %a: %a, want %a\n", a, b, got, want);
  }
  if (bits_of(sbag::div_rn(a, b)) != bits_of(want)) failures++;
  // an exact tie: twice the quotient in ulps is an odd integer
  const double twice = std::ldexp(a, 1075) / b;
  if (std::fabs(twice) < 0x1p53 && twice == std::floor(twice) && std::fmod(std::fabs(twice), 2.0) == 1.0 &&
      std::fma(-twice, b, std::ldexp(a, 1075)) == 0.0)
    ties++;
}

int main() {
  const double ulp = 0x1p-1074;
  // k ulps over a count: every remainder, ties at k = c (n + 1/2) for even c
  for (int k = 0; k <= 4000; k++)
    for (int c = 1; c <= 300; c++) {
      check(k * ulp, (double)c);
      check(-(k * ulp), (double)c);
    }
  // the same a few binades up, where the quotient keeps more bits
  for (int s = 1; s <= 52; s += 3)
    for (int k = 1; k <= 300; k++)
      for (int c = 1; c <= 64; c++) check(std::ldexp((double)(2 * k + 1), s - 1074), (double)(2 * c));
  // random operands of every magnitude, the quotient steered below 2^-1021
  for (int i = 0; i < 4000000; i++) {
    const uint64_t ra = next_u64(), rb = next_u64(), rc = next_u64();
    const double ma = 1.0 + (double)(ra >> 12) * 0x1p-52, mb = 1.0 + (double)(rb >> 12) * 0x1p-52;
    const int eq = -1021 - (int)(rc % 60);              // the quotient's binade, down past 2^-1074
    const int eb = (int)((rc >> 8) % 2040) - 1070;      // the divisor's, subnormal ones too
    int ea = eq + eb;
    if (ea > 1023 || ea < -1074) continue;
    double a = std::ldexp(ma, ea), b = std::ldexp(mb, eb);
    if (rc & (1ull << 40)) a = -a;
    if (rc & (1ull << 41)) b = -b;
    if (b == 0.0 || !std::isfinite(a)) continue;
    check(a, b);
    // and a divisor with few bits, so that ties happen
    check(a, std::ldexp((double)(1 + (rb % 255)), eb));
    check(std::ldexp((double)(1 + (ra % 4095)), ea), std::ldexp((double)(1 + (rb % 255)), eb));
  }
  // the edges: quotients rounding to 0, to one ulp, to 2^-1022 and just below 2^-1021
  const double edge[] = {0x1p-1074, 0x1.8p-1074, 0x1p-1073, 0x1.fffffffffffffp-1023, 0x1p-1022,
                         0x1.0000000000001p-1022, 0x1.fffffffffffffp-1022};
  for (double e : edge)
    for (double d : {1.0, 2.0, 3.0, 4.0, 0x1.fffffffffffffp0, 0x1.0000000000001p0, 0x1p1000}) {
      check(e, d);
      check(e * d, d * d);
    }
  std::printf("div_check: %lld cases (%lld exact ties), %lld failures\n", cases, ties, failures);
  return failures ? 1 : 0;
}
