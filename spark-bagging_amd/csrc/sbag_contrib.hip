// sbag_contrib.hip — per-row feature contributions (path-dependent TreeSHAP) of a forest for
// gfx950 (MI355X, CDNA4), over the packed path table of sbag_contrib_plan.h.  The rule, every
// operation of it and their order, is sbag.h's (sbag_predict_contributions); __dmul_rn /
// __dadd_rn / __ddiv_rn are never contracted and the file is built with -ffp-contract=off.
//
//   k_contrib_tiled  u8 / u16 codes, paths of at most 15 distinct features.  A workgroup of 256
//                    threads stages a tile of 64 / 32 / 16 code rows (k_wpred_tiled's pitch and
//                    16-byte pieces) beside the tile's accumulators fp64 [rows][F + 1] and the
//                    Q table in LDS.  It is 16 groups of 16 lanes (32 of 8 when no path of the
//                    forest has more than 7 features); group g owns rows g, g + groups, ... of
//                    the tile and their accumulator rows, RPG of them, and every group goes over
//                    every path of the forest in order.  Lane k (1 <= k <= m) of a group holds
//                    element k of the path, read once per path and used for all of the group's
//                    rows; lane j holds pw[j] of each of these rows.  An extension step takes
//                    old[j - 1] by a DPP row_shr:1 of the two halves of the double, z_u by
//                    ds_bpermute from lane u, o_u from a ballot, Q(., u + 1) from LDS.  In the
//                    unwound sum lane k runs element k; pw[i] comes from a W-double LDS slot
//                    per (group, row) that the lanes fill once per path (measured 5.6 % faster
//                    than a ds_bpermute per step).  Lane k then adds its term to acc[row][e_k]: the e_k of a path are
//                    distinct, a row's accumulators belong to one group, a group is within one
//                    wave and a wave's LDS operations keep their order, so a row's additions
//                    happen in path order with no atomics.  After a barrier the tile's
//                    rows x (F + 1) doubles leave as one contiguous block, divided by the tree
//                    count for the mean, the bias column taken from the host.
//   k_contrib_walk   the general path: one thread per row, pw[65] in private memory, the row of
//                    out as accumulators, the elements as fp64 intervals over X or over codes
//                    and dictionaries.  The same operations in the same order: the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

#include "sbag_internal.h"

namespace sbag {

namespace {

// (as sbag_kernels.hip's: the dynamic-LDS cap of a kernel, once per (kernel, device))
void contrib_set_max_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> g(mu);
  if (done.count({fn, dev})) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess)
    done.insert({fn, dev});
}

// the double of the lane below within the 16-lane DPP row, 0.0 at the row's first lane
__device__ __forceinline__ double row_shr1(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x111 /* row_shr:1 */, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x111, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

}  // namespace

// W lanes a group, RPG rows a group: A.rows == RPG * (256 / W), or 16 rows over 32 groups of
// which the upper 16 own nothing.  A row past the tile's rows computes on row 0's codes and adds
// nothing.
template <typename CT, int W, int RPG>
__global__ __launch_bounds__(kContribThreads) void k_contrib_tiled(ContribArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int NG = kContribThreads / W;
  const int tid = threadIdx.x, lane = tid & (W - 1), grp = tid / W;
  const int F1 = A.F + 1, Q2 = A.M + 2, R = A.rows;
  const int rb = A.S * (int)sizeof(CT);  // bytes of one row (S is a multiple of 16)
  const int pitch = rb + 4, vpr = rb >> 4;
  unsigned char* rows = smem;
  double* acc = (double*)(smem + (((size_t)R * pitch + 15) & ~(size_t)15));  // [R][F1]
  double* qt = acc + (size_t)R * F1;                                         // [Q2][Q2]
  double* slot = qt + Q2 * Q2;  // [groups][RPG][W]: a row's pw, written and read by its own group
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int tile_rows = (int)(A.N - row0 < R ? A.N - row0 : R);
  for (int q = tid; q < R * vpr; q += kContribThreads) {
    const int r = q / vpr, w = q - r * vpr;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (r < tile_rows) v = *(const uint4*)((const unsigned char*)A.codes + (row0 + r) * rb + w * 16);
    uint32_t* d = (uint32_t*)(rows + r * pitch + w * 16);
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
    d[3] = v.w;
  }
  for (int i = tid; i < R * F1; i += kContribThreads) acc[i] = 0.0;
  for (int i = tid; i < Q2 * Q2; i += kContribThreads) qt[i] = A.q[i];
  block_sync();

  const CT* rp[RPG];
  double* ap[RPG];
  bool valid[RPG];
#pragma unroll
  for (int r = 0; r < RPG; r++) {
    const int row = grp + r * NG;
    valid[r] = row < tile_rows;
    rp[r] = (const CT*)(rows + (valid[r] ? row : 0) * pitch);
    ap[r] = acc + (size_t)(valid[r] ? row : 0) * F1;
  }
  const int gbase = (tid & 63) & ~(W - 1);  // the group's first lane within its wave
  const ContribElem* elems = (const ContribElem*)A.elems;
  for (int64_t l = 0; l < A.nleaves; l++) {
    const ContribLeaf lf = A.leaves[l];
    const int m = lf.m;
    if (m == 0) continue;
    const bool mine = lane >= 1 && lane <= m;
    ContribElem e;
    e.feat = 0;
    e.lo = 1;
    e.hi = 0;
    e.z = 1.0;
    e.rz = 1.0;
    if (mine) e = elems[(int64_t)lf.first + lane - 1];
    bool o[RPG];
    uint32_t om[RPG];  // bit u: o_u of the row
    double pw[RPG];
#pragma unroll
    for (int r = 0; r < RPG; r++) {
      const uint32_t code = rp[r][e.feat];
      o[r] = code >= e.lo && code <= e.hi;
      om[r] = (uint32_t)(__ballot(o[r]) >> gbase);
      pw[r] = lane == 0 ? 1.0 : 0.0;
    }
    // pw over the path's m elements: lane j holds pw[j]
    for (int u = 1; u <= m; u++) {
      const double zu = __shfl(e.z, u, W);
      const bool act = lane <= u;
      const double* qr = qt + (u + 1) * Q2;
      const double q1 = qr[act ? u - lane : 0], q2 = qr[act ? lane : 0];
#pragma unroll
      for (int r = 0; r < RPG; r++) {
        const double prev = row_shr1(pw[r]);
        double v = __dmul_rn(__dmul_rn(zu, pw[r]), q1);
        if (((om[r] >> u) & 1u) && lane > 0) v = __dadd_rn(v, __dmul_rn(prev, q2));
        if (act) pw[r] = v;
      }
    }
    // the unwound sum of element `lane`
    double next[RPG], tot[RPG];
#pragma unroll
    for (int r = 0; r < RPG; r++) {
      slot[(grp * RPG + r) * W + lane] = pw[r];
      tot[r] = 0.0;
    }
#pragma unroll
    for (int r = 0; r < RPG; r++) next[r] = slot[(grp * RPG + r) * W + m];
    for (int i = m - 1; i >= 0; i--) {
      const double qa = qt[(i + 1) * Q2 + m + 1], qb = qt[(m + 1) * Q2 + m - i], qc = qt[(m - i) * Q2 + m + 1];
#pragma unroll
      for (int r = 0; r < RPG; r++) {
        const double p = slot[(grp * RPG + r) * W + i];  // pw[i] of the row: one address a group
        if (o[r]) {
          const double tmp = __dmul_rn(next[r], qa);
          tot[r] = __dadd_rn(tot[r], tmp);
          next[r] = __dsub_rn(p, __dmul_rn(__dmul_rn(tmp, e.z), qb));
        } else {
          tot[r] = __dadd_rn(tot[r], __dmul_rn(__dmul_rn(p, e.rz), qc));
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RPG; r++)
      if (mine && valid[r]) {
        const double d = o[r] ? __dsub_rn(1.0, e.z) : -e.z;
        double* a = ap[r] + e.feat;
        *a = __dadd_rn(*a, __dmul_rn(__dmul_rn(tot[r], d), lf.vw));
      }
  }
  block_sync();  // every accumulator row is final before other threads read it
  double* gtile = A.out + row0 * F1;
  const double div = (double)A.trees;
  for (int j = tid; j < tile_rows * F1; j += kContribThreads) {
    const int c = j % F1;
    const double v = acc[j];
    gtile[j] = c == A.F ? A.bias : A.trees ? __ddiv_rn(v, div) : v;
  }
}

void launch_contrib_tiled(hipStream_t st, const ContribArgs& a) {
  const int pitch = a.S * a.code_bytes + 4;
  const size_t lds = contrib_lds(a.rows, pitch, a.F, a.M);
  const dim3 grid((unsigned)((a.N + a.rows - 1) / a.rows));
#define SBAG_CONTRIB_LAUNCH(CT, W, RPG)                                                         \
  do {                                                                                          \
    contrib_set_max_lds((const void*)k_contrib_tiled<CT, W, RPG>, 160 * 1024);                  \
    hipLaunchKernelGGL((k_contrib_tiled<CT, W, RPG>), grid, dim3(kContribThreads), lds, st, a); \
  } while (0)
#define SBAG_CONTRIB_SHAPE(CT)                                  \
  do {                                                          \
    if (a.lanes == 8) {                                         \
      if (a.rows == 64)                                         \
        SBAG_CONTRIB_LAUNCH(CT, 8, 2);                          \
      else                                                      \
        SBAG_CONTRIB_LAUNCH(CT, 8, 1);                          \
    } else if (a.rows == 64) {                                  \
      SBAG_CONTRIB_LAUNCH(CT, 16, 4);                           \
    } else if (a.rows == 32) {                                  \
      SBAG_CONTRIB_LAUNCH(CT, 16, 2);                           \
    } else {                                                    \
      SBAG_CONTRIB_LAUNCH(CT, 16, 1);                           \
    }                                                           \
  } while (0)
  if (a.code_bytes == 1)
    SBAG_CONTRIB_SHAPE(uint8_t);
  else
    SBAG_CONTRIB_SHAPE(uint16_t);
#undef SBAG_CONTRIB_SHAPE
#undef SBAG_CONTRIB_LAUNCH
}

// One thread per row; the row's F + 1 doubles of out are the thread's accumulators.
__global__ __launch_bounds__(256) void k_contrib_walk(const double* __restrict__ X,
                                                      const void* __restrict__ codes, int code_bytes,
                                                      const double* __restrict__ dict,
                                                      const int64_t* __restrict__ dict_off, int32_t S,
                                                      ContribArgs A) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= A.N) return;
  const int F = A.F, Q2 = A.M + 2;
  double* out = A.out + row * (F + 1);
  for (int g = 0; g <= F; g++) out[g] = 0.0;
  const ContribElemF* elems = (const ContribElemF*)A.elems;
  double pw[kContribMaxM + 1];
  for (int64_t l = 0; l < A.nleaves; l++) {
    const ContribLeaf lf = A.leaves[l];
    const int m = lf.m;
    if (m == 0) continue;
    const ContribElemF* el = elems + lf.first;  // el[k - 1]: element k, 1 <= k <= m
    uint64_t om = 0;                                // bit k - 1: o_k
    for (int k = 1; k <= m; k++) {
      const int g = el[k - 1].feat;
      double v;
      if (X) {
        v = X[row * F + g];
      } else {
        const int64_t c = code_bytes == 1   ? (int64_t)((const uint8_t*)codes)[row * S + g]
                          : code_bytes == 2 ? (int64_t)((const uint16_t*)codes)[row * S + g]
                                            : (int64_t)((const uint32_t*)codes)[row * S + g];
        v = dict[dict_off[g] + c];
      }
      // an infinite end is open: a NaN goes right at every test and -inf left, as in the walk
      const double lo = el[k - 1].lo, hi = el[k - 1].hi;
      if ((lo == -INFINITY || !(v <= lo)) && (hi == INFINITY || v <= hi)) om |= 1ull << (k - 1);
    }
    pw[0] = 1.0;
    for (int j = 1; j <= m; j++) pw[j] = 0.0;
    for (int u = 1; u <= m; u++) {
      const double zu = el[u - 1].z;
      const bool ou = (om >> (u - 1)) & 1ull;
      const double* qr = A.q + (u + 1) * Q2;
      for (int j = u; j >= 0; j--) {  // downwards: pw[j - 1] is still the old one
        double v = __dmul_rn(__dmul_rn(zu, pw[j]), qr[u - j]);
        if (ou && j > 0) v = __dadd_rn(v, __dmul_rn(pw[j - 1], qr[j]));
        pw[j] = v;
      }
    }
    for (int k = 1; k <= m; k++) {
      const double z = el[k - 1].z, rz = el[k - 1].rz;
      const bool ok = (om >> (k - 1)) & 1ull;
      double tot = 0.0;
      if (ok) {
        double next = pw[m];
        for (int i = m - 1; i >= 0; i--) {
          const double tmp = __dmul_rn(next, A.q[(i + 1) * Q2 + m + 1]);
          tot = __dadd_rn(tot, tmp);
          next = __dsub_rn(pw[i], __dmul_rn(__dmul_rn(tmp, z), A.q[(m + 1) * Q2 + m - i]));
        }
      } else {
        for (int i = m - 1; i >= 0; i--)
          tot = __dadd_rn(tot, __dmul_rn(__dmul_rn(pw[i], rz), A.q[(m - i) * Q2 + m + 1]));
      }
      const double d = ok ? __dsub_rn(1.0, z) : -z;
      double* a = out + el[k - 1].feat;
      *a = __dadd_rn(*a, __dmul_rn(__dmul_rn(tot, d), lf.vw));
    }
  }
  const double div = (double)A.trees;
  if (A.trees)
    for (int g = 0; g < F; g++) out[g] = __ddiv_rn(out[g], div);
  out[F] = A.bias;
}

void launch_contrib_walk(hipStream_t st, const double* X, const void* codes, int code_bytes,
                         const double* dict, const int64_t* dict_off, int32_t S, const ContribArgs& a) {
  hipLaunchKernelGGL(k_contrib_walk, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, st, X, codes,
                     code_bytes, dict, dict_off, S, a);
}

}  // namespace sbag
