// sbag_boostbag.hip — the boosted bag of BoostingParams.extractBoostedBag
// (ml/boosting/BoostingParams.scala:127-148): row j of partition i with prob != 0.0 gets a
// PoissonDistribution(prob) of its own, reseeded with seed + i + j, and one sample().
//
// Every row therefore pays a whole Well19937c seeding (AbstractWell.setSeed(long): 622 steps
// of v[i] = 1812433253 * (v[i-2] ^ v[i-2] >> 30) + i, two independent chains on the even and
// the odd indices) for a draw that reads a handful of state words.  Generator step t works at
// ring index (624 - t) % 624: it reads v[idx] (step 0: v[0]; later the z4 the step before
// wrote), v[idx + 70], v[idx + 179], v[idx + 449], the top bit of v[idx - 1] and the low bits
// of v[idx - 2], and for t < 70 all of those but v[idx] still hold the seeding's values.
//
//  * k_boost_fast, one lane per row: the two chains run in registers, and the words the
//    first kBbSteps steps read (four windows of the initial state ending at indices 70, 179,
//    449 and 623, and word 0) are kept as they go by, at compile-time indices (the
//    iterations that cover a window are unrolled, the stretches between them are plain
//    loops).  No state is stored.  The lane then replays PoissonDistribution.nextPoisson
//    (mean < 40) for up to kBbSteps / 2 doubles; a row that is still open after them is
//    appended to a list.  kBbSteps = 32 is measured: 16 leaves 3.4 % of a
//    concentrated bag's rows to the second pass, 48 and 64 cost registers (2 and 1 waves
//    per SIMD).
//  * k_boost_ring, one lane per listed row: the whole 624-word state in LDS, word-major
//    (word w of lane l at w * 64 + l: every access of a wave is conflict-free and a lane
//    touches its own column only, so the kernel has no barrier), seeded again and stepped as
//    AbstractWell does, for as many doubles as the row takes.  64 rows fill a CU's LDS.
//
// Both paths evaluate p = FastMath.exp(-mean) per row from the tables of sbag_fastmath.h
// (uploaded by the host), every product and sum rounded separately (-ffp-contract=off), and
// compare with the arithmetic of oracle/sbag_oracle.c well_next / well_next_double /
// poisson_sample, including the loop bound n < 1000 * mean.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sbag_internal.h"
#include "sbag_well.h"

namespace sbag {

namespace {

#ifndef SBAG_BB_STEPS
#define SBAG_BB_STEPS 32
#endif
constexpr int kBbSteps = SBAG_BB_STEPS;  // generator steps of the register path (2 per double)
static_assert(kBbSteps % 2 == 0 && kBbSteps >= 2 && kBbSteps <= 64,
              "from step 70 on the +70 read lands on a rewritten word");
constexpr int kBbRingRows = 64;  // rows of a k_boost_ring block: 64 x 624 words = 156 KB

// FastMath.exp(x), -41 < x <= 0: sbag_fm_exp_neg (sbag_fastmath.h) on the device, the four
// tables concatenated (int_a[42], int_b[42], frac_a[1025], frac_b[1025])
__device__ __forceinline__ double bb_exp_neg(const double* __restrict__ tab, double x) {
  int int_val = (int)x;
  int_val -= 1;
  const double ipa = tab[-int_val], ipb = tab[42 - int_val];
  const int int_frac = (int)((x - int_val) * 1024.0);
  const double fpa = tab[84 + int_frac], fpb = tab[84 + 1025 + int_frac];
  const double epsilon = x - (int_val + int_frac / 1024.0);
  double z = 0.04168701738764507;
  z = z * epsilon + 0.1666666505023083;
  z = z * epsilon + 0.5000000000042687;
  z = z * epsilon + 1.0;
  z = z * epsilon + -3.940510424527919E-20;
  const double temp_a = ipa * fpa;
  const double temp_b = ipa * fpb + ipb * fpa + ipb * fpb;
  const double temp_c = temp_b + temp_a;
  return temp_c * z + temp_b + temp_a;
}

// partition of row r: the last i with part_off[i] <= r (empty partitions share an offset
// with their successor and are skipped by it)
__device__ __forceinline__ int bb_partition(const int64_t* __restrict__ part_off, int P, int64_t r) {
  int lo = 0, hi = P;  // part_off[lo] <= r < part_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (part_off[mid] <= r)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// setSeed((long)(seed + i + j)): 64-bit wrapping addition
__device__ __forceinline__ uint64_t bb_row_seed(int64_t seed, int i, int64_t j) {
  return (uint64_t)seed + (uint64_t)(int64_t)i + (uint64_t)j;
}

__device__ __forceinline__ uint32_t bb_seed_step(uint32_t x, int i) {
  return 1812433253u * (x ^ (uint32_t)((int32_t)x >> 30)) + (uint32_t)i;
}

// The seeding moves both chains one word each per iteration (words i and i + 1, i even).
// A window of N words ending at word HI is kept by the unrolled iterations [I0, I1) that
// cover it; the stretches between the windows run as plain loops and keep nothing.
template <int HI, int N>
struct BbWin {
  static constexpr int LO = HI - N + 1;
  static constexpr int I0 = LO & ~1, I1 = (HI | 1) + 1;
};
template <int FROM, int TO>
__device__ __forceinline__ void bb_seed_skip(uint32_t& xe, uint32_t& xo) {
  static_assert(FROM % 2 == 0 && TO % 2 == 0 && FROM <= TO, "whole pairs");
#pragma unroll 4
  for (int i = FROM; i < TO; i += 2) {
    xe = bb_seed_step(xe, i);
    xo = bb_seed_step(xo, i + 1);
  }
}
template <int HI, int N>  // w[k] = v[HI - k]
__device__ __forceinline__ void bb_seed_keep(uint32_t& xe, uint32_t& xo, uint32_t (&w)[N]) {
  using W = BbWin<HI, N>;
#pragma unroll
  for (int i = W::I0; i < W::I1; i += 2) {
    xe = bb_seed_step(xe, i);
    xo = bb_seed_step(xo, i + 1);
    if (i >= W::LO && i <= HI) w[HI - i] = xe;
    if (i + 1 >= W::LO && i + 1 <= HI) w[HI - (i + 1)] = xo;
  }
}

// one Well19937c step from its six input words: z3 (the new v[idx]) and z4 (the new
// v[idx - 1], the next step's v0, and the output before tempering)
__device__ __forceinline__ void bb_well_step(uint32_t v0, uint32_t vM1, uint32_t vM2, uint32_t vM3,
                                             uint32_t hb, uint32_t lo, uint32_t& z3, uint32_t& z4) {
  const uint32_t z0 = (0x80000000u & hb) ^ (0x7FFFFFFFu & lo);
  const uint32_t z1 = (v0 ^ (v0 << 25)) ^ (vM1 ^ (vM1 >> 27));
  const uint32_t z2 = (vM2 >> 9) ^ (vM3 ^ (vM3 >> 1));
  z3 = z1 ^ z2;
  z4 = z0 ^ (z1 ^ (z1 << 9)) ^ (z2 ^ (z2 << 21)) ^ (z3 ^ (z3 >> 21));
}

// BitsStreamGenerator.nextDouble from the two next(26)
__device__ __forceinline__ double bb_double(uint32_t hi26, uint32_t lo26) {
  return (double)(int64_t)(((uint64_t)hi26 << 26) | (uint64_t)lo26) * 0x1.0p-52;
}

// error bits of both kernels
constexpr int kBbErrInvalid = 1, kBbErrLarge = 2, kBbErrCap = 4;

// flags: [0] error bits, [1] length of the list, [2] rows with mean 0
__global__ __launch_bounds__(256) void k_boost_fast(const double* __restrict__ mean, int64_t N,
                                                    const int64_t* __restrict__ part_off, int P,
                                                    int64_t seed, const double* __restrict__ tab,
                                                    uint8_t* __restrict__ counts,
                                                    uint32_t* __restrict__ list,
                                                    unsigned int* __restrict__ flags) {
  constexpr int T = kBbSteps;
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= N) return;
  const double m = mean[r];
  if (!(m >= 0.0) || !(m <= 1.7976931348623157e308)) {  // negative, NaN or infinite
    atomicOr(&flags[0], (unsigned int)kBbErrInvalid);
    return;
  }
  if (m >= 40.0) {
    atomicOr(&flags[0], (unsigned int)kBbErrLarge);
    return;
  }
  if (m == 0.0) {  // prob == 0.0: no distribution, no draw
    counts[r] = 0;
    atomicAdd(&flags[2], 1u);
    return;
  }
  const int part = bb_partition(part_off, P, r);
  const uint64_t s64 = bb_row_seed(seed, part, r - part_off[part]);
  // the seeding in registers; wa[k] = v[70 - k], wb[k] = v[179 - k], wc[k] = v[449 - k],
  // wh[k] = v[623 - k] as the chains pass them
  uint32_t wa[T], wb[T], wc[T], wh[T + 1];
  uint32_t xe = (uint32_t)(s64 >> 32), xo = (uint32_t)s64;
  const uint32_t v0 = xe;
  bb_seed_skip<2, BbWin<70, T>::I0>(xe, xo);
  bb_seed_keep<70, T>(xe, xo, wa);
  bb_seed_skip<BbWin<70, T>::I1, BbWin<179, T>::I0>(xe, xo);
  bb_seed_keep<179, T>(xe, xo, wb);
  bb_seed_skip<BbWin<179, T>::I1, BbWin<449, T>::I0>(xe, xo);
  bb_seed_keep<449, T>(xe, xo, wc);
  bb_seed_skip<BbWin<449, T>::I1, BbWin<623, T + 1>::I0>(xe, xo);
  bb_seed_keep<623, T + 1>(xe, xo, wh);
  static_assert(BbWin<623, T + 1>::I1 == 624, "the last window ends the state");
  const double p = bb_exp_neg(tab, -m);
  const double bound = 1000.0 * m;
  // PoissonDistribution.nextPoisson: while (n < 1000 * mean) { r *= nextDouble();
  // if (r >= p) n++; else return n; } return n;
  int n = 0;
  double prod = 1.0;
  bool open = (double)n < bound;
  uint32_t z4 = v0;
#pragma unroll
  for (int t = 0; t < T; t += 2) {
    if (!open) break;
    uint32_t z3, o[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint32_t v0t = z4;
      bb_well_step(v0t, wa[t + h], wb[t + h], wc[t + h], wh[t + h], wh[t + h + 1], z3, z4);
      o[h] = well_temper26(z4);
    }
    prod *= bb_double(o[0], o[1]);
    if (prod >= p) {
      n++;
      open = (double)n < bound;
    } else {
      open = false;
    }
  }
  if (!open) {
    counts[r] = (uint8_t)n;  // n <= T / 2
  } else {
    list[atomicAdd(&flags[1], 1u)] = (uint32_t)r;
  }
}

__global__ __launch_bounds__(kBbRingRows) void k_boost_ring(
    const double* __restrict__ mean, const int64_t* __restrict__ part_off, int P, int64_t seed,
    const double* __restrict__ tab, uint8_t* __restrict__ counts, const uint32_t* __restrict__ list,
    unsigned int nlist, unsigned int* __restrict__ flags) {
  __shared__ uint32_t ring[624 * kBbRingRows];
  const unsigned int k = blockIdx.x * kBbRingRows + threadIdx.x;
  if (k >= nlist) return;
  uint32_t* v = ring + threadIdx.x;  // v[w * kBbRingRows]: the lane's own column
  const int64_t r = (int64_t)list[k];
  const double m = mean[r];
  const int part = bb_partition(part_off, P, r);
  const uint64_t s64 = bb_row_seed(seed, part, r - part_off[part]);
  {
    uint32_t xe = (uint32_t)(s64 >> 32), xo = (uint32_t)s64;
    v[0] = xe;
    v[kBbRingRows] = xo;
    for (int i = 2; i < 624; i += 2) {
      xe = bb_seed_step(xe, i);
      xo = bb_seed_step(xo, i + 1);
      v[i * kBbRingRows] = xe;
      v[(i + 1) * kBbRingRows] = xo;
    }
  }
  const double p = bb_exp_neg(tab, -m);
  const double bound = 1000.0 * m;
  int n = 0, idx = 0;
  double prod = 1.0;
  auto next26 = [&]() {
    const int iRm1 = wrap624(idx - 1), iRm2 = wrap624(idx - 2);
    const uint32_t hb = v[iRm1 * kBbRingRows], lo = v[iRm2 * kBbRingRows];
    uint32_t z3, z4;
    bb_well_step(v[idx * kBbRingRows], v[wrap624(idx + 70) * kBbRingRows],
                 v[wrap624(idx + 179) * kBbRingRows], v[wrap624(idx + 449) * kBbRingRows], hb, lo,
                 z3, z4);
    v[idx * kBbRingRows] = z3;
    v[iRm1 * kBbRingRows] = z4;
    v[iRm2 * kBbRingRows] = lo & 0x80000000u;
    idx = iRm1;
    return well_temper26(z4);
  };
  while ((double)n < bound) {
    const uint32_t hi = next26();
    const uint32_t lo = next26();
    prod *= bb_double(hi, lo);
    if (!(prod >= p)) break;
    n++;
    if (n > 255) break;  // the bag column is u8: reported, nothing is returned
  }
  if (n > 255) {
    atomicOr(&flags[0], (unsigned int)kBbErrCap);
    return;
  }
  counts[r] = (uint8_t)n;
}

}  // namespace

int boost_fast_doubles() { return kBbSteps / 2; }

void launch_boost_fast(hipStream_t st, const double* d_mean, int64_t N, const int64_t* d_part_off,
                       int P, int64_t seed, const double* d_tab, uint8_t* d_counts, uint32_t* d_list,
                       unsigned int* d_flags) {
  const int64_t blocks = (N + 255) / 256;
  hipLaunchKernelGGL(k_boost_fast, dim3((unsigned int)blocks), dim3(256), 0, st, d_mean, N, d_part_off,
                     P, seed, d_tab, d_counts, d_list, d_flags);
}

void launch_boost_ring(hipStream_t st, const double* d_mean, const int64_t* d_part_off, int P,
                       int64_t seed, const double* d_tab, uint8_t* d_counts, const uint32_t* d_list,
                       unsigned int nlist, unsigned int* d_flags) {
  const unsigned int blocks = (nlist + kBbRingRows - 1) / kBbRingRows;
  hipLaunchKernelGGL(k_boost_ring, dim3(blocks), dim3(kBbRingRows), 0, st, d_mean, d_part_off, P, seed,
                     d_tab, d_counts, d_list, nlist, d_flags);
}

}  // namespace sbag
