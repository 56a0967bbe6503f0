// sbag_gbm.hip — one boosting step of GBMRegressor over a resident dataset for gfx950 (MI355X,
// CDNA4): the state of the boosting loop (the current model S and the pseudo-residuals, or the
// per-row validation losses) stays on the device between boosters.
//
//   k_gbm_step   per row: p = the new tree's leaf value, S = S + (p * weight) with the product
//                rounded first (BLAS.dot), then
//                  kGbmResidual  val = -grad(y, S + konst), and the label analysis of val
//                                (k_label_stats' six words) reduced in the same pass;
//                  kGbmLoss      val = lossf(y, S + konst).
//                `init`: S = +0.0 and no tree (the state's first residuals / losses).
//
// Work split (sbag_gbm_plan.h): a workgroup owns kGbmTileRows contiguous rows, lane t rows
// t + 256 k of the tile, so every load and store of y, S and val is a contiguous 2 KB per wave.
// The tree (16-byte GbmNodes, thresholds already cuts in the dataset's code space) is staged once
// per workgroup into LDS; LDS = false reads the same nodes from global memory (a tree past
// kGbmLdsNodes): same instructions after the node fetch, so the same bytes.
//
// Row data: the codes a walk needs are gathered straight from the resident code matrix
// [N][S].  A walk of depth d reads d codes of one row; those lie in the row's own S * code_bytes
// bytes, so from HBM the gather moves at most what staging the tile's rows into LDS would
// (the whole row), and less for a row wider than d memory lines, and it has no LDS round trip
// and no barrier per tile.  The lane's kGbmLaneRows walks advance level by level
// together: their node reads, then their code gathers, are issued back to back, so a lane has
// that many gathers in flight.
//
// Arithmetic: fp64, one rounded operation per operation of the formula (gbm_residual /
// gbm_loss of sbag_gbm_plan.h; the file is built with -ffp-contract=off as the library is).
//
// Label analysis: per lane over its rows, then across the wave in registers (DPP within the
// rows of 16 lanes, readlane across them), across the workgroup's waves through LDS, and one set
// of atomics per workgroup.  or / min / max only: the result does not depend on the order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sbag_internal.h"
#include "sbag_gbm_plan.h"

namespace sbag {

namespace {

template <int CTRL>
__device__ __forceinline__ uint64_t gbm_dpp64(uint64_t v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ uint64_t gbm_readlane64(uint64_t v, int lane) {
  const int lo = __builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const int hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
// the largest v of the wave's 64 lanes (all active), in every lane: lane ^ 1, lane ^ 2, the
// other quad of the half row, the other half of the row, then the four rows
__device__ __forceinline__ uint64_t gbm_wave_max(uint64_t v) {
  v = max(v, gbm_dpp64<0xB1>(v));   // quad_perm [1,0,3,2]
  v = max(v, gbm_dpp64<0x4E>(v));   // quad_perm [2,3,0,1]
  v = max(v, gbm_dpp64<0x141>(v));  // row_half_mirror
  v = max(v, gbm_dpp64<0x140>(v));  // row_mirror
  return max(max(gbm_readlane64(v, 0), gbm_readlane64(v, 16)), max(gbm_readlane64(v, 32), gbm_readlane64(v, 48)));
}

__device__ __forceinline__ uint64_t gbm_dkey(double v) {  // order-preserving key (k_label_stats')
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ uint32_t gbm_code(const void* __restrict__ codes, int code_bytes, int64_t at) {
  return code_bytes == 1   ? (uint32_t)((const uint8_t*)codes)[at]
         : code_bytes == 2 ? (uint32_t)((const uint16_t*)codes)[at]
                           : ((const uint32_t*)codes)[at];
}

__device__ __forceinline__ GbmNode gbm_node(const GbmNode* nodes, int id) {
  const uint4 w = *(const uint4*)(nodes + id);
  return GbmNode{(int32_t)w.x, (int32_t)w.y, w.z, w.w};
}

}  // namespace

template <int MODE, bool LDS>
__global__ __launch_bounds__(kGbmBlock) void k_gbm_step(GbmArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint64_t* red = (uint64_t*)smem;  // [kGbmWaves][4]
  const int tid = threadIdx.x;
  const GbmNode* nodes = LDS ? (const GbmNode*)(smem + kGbmRedBytes) : A.nodes;
  if (LDS) {
    uint4* ln = (uint4*)(smem + kGbmRedBytes);
    for (int i = tid; i < A.num_nodes; i += kGbmBlock) ln[i] = ((const uint4*)A.nodes)[i];
    block_sync();
  }
  const int64_t row0 = (int64_t)blockIdx.x * kGbmTileRows + tid;
  int64_t row[kGbmLaneRows];
  bool live[kGbmLaneRows];
  double y[kGbmLaneRows], s[kGbmLaneRows], p[kGbmLaneRows];
#pragma unroll
  for (int k = 0; k < kGbmLaneRows; k++) {
    row[k] = row0 + (int64_t)k * kGbmBlock;
    live[k] = row[k] < A.N;
    if (!live[k]) row[k] = A.N - 1;  // a row past the end walks the last row; nothing of it is kept
    y[k] = A.y[row[k]];
    s[k] = A.init ? 0.0 : A.Sx[row[k]];
    p[k] = 0.0;
  }
  if (!A.init) {
    int id[kGbmLaneRows];
#pragma unroll
    for (int k = 0; k < kGbmLaneRows; k++) id[k] = 0;
    for (;;) {
      GbmNode n[kGbmLaneRows];
      bool any = false;
#pragma unroll
      for (int k = 0; k < kGbmLaneRows; k++) {
        n[k] = gbm_node(nodes, id[k]);
        any = any || n[k].left >= 0;
      }
      if (!any) {
#pragma unroll
        for (int k = 0; k < kGbmLaneRows; k++) p[k] = __hiloint2double((int)n[k].cut, (int)n[k].col);
        break;
      }
      uint32_t code[kGbmLaneRows];
#pragma unroll
      for (int k = 0; k < kGbmLaneRows; k++)  // (a walk already at its leaf reads column 0: in bounds, unused)
        code[k] = gbm_code(A.codes, A.code_bytes, row[k] * A.S + (n[k].left >= 0 ? n[k].col : 0u));
#pragma unroll
      for (int k = 0; k < kGbmLaneRows; k++)
        if (n[k].left >= 0) id[k] = code[k] < n[k].cut ? n[k].left : n[k].right;
    }
  }
  uint32_t nf = 0, ni = 0;
  uint64_t smax = 0, kmin = ~0ull, kmax = 0, amax = 0;
#pragma unroll
  for (int k = 0; k < kGbmLaneRows; k++) {
    if (!live[k]) continue;
    const double sn = A.init ? 0.0 : __dadd_rn(s[k], __dmul_rn(p[k], A.weight));
    A.Sx[row[k]] = sn;
    const double pred = __dadd_rn(sn, A.konst);
    if (MODE == kGbmLoss) {
      A.val[row[k]] = gbm_loss(A.loss, A.alpha, y[k], pred);
      continue;
    }
    const double v = gbm_residual(A.loss, A.alpha, y[k], pred);
    A.val[row[k]] = v;
    // k_label_stats, per value
    const uint64_t bits = (uint64_t)__double_as_longlong(v);
    const int E = (int)((bits >> 52) & 0x7FF);
    if (E == 0x7FF) {  // NaN / inf
      nf = 1;
      ni = 1;
      continue;
    }
    int si = 0;
    if (v != 0.0) {
      const uint64_t M = bits & ((1ull << 52) - 1);
      const uint64_t sig = E ? (M | (1ull << 52)) : M;
      const int low = (E ? E - 1075 : -1074) + (int)__builtin_ctzll(sig);  // v = odd 2^low
      si = low < 0 ? -low : 0;
    }
    smax = max(smax, (uint64_t)si);
    if (!(v >= 0 && si == 0 && v < 8388608.0)) ni = 1;
    const uint64_t key = gbm_dkey(v);
    kmin = min(kmin, key);
    kmax = max(kmax, key);
    amax = max(amax, bits & 0x7FFFFFFFFFFFFFFFull);  // |v|: its bits order as the value
  }
  if (MODE != kGbmResidual) return;
  // (every lane of the workgroup is here: rows past the end hold the neutral values)
  const bool wnf = __ballot(nf != 0) != 0, wni = __ballot(ni != 0) != 0;
  smax = gbm_wave_max(smax);
  kmin = ~gbm_wave_max(~kmin);
  kmax = gbm_wave_max(kmax);
  amax = gbm_wave_max(amax);
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
    red[wave * 4 + 0] = smax | (wnf ? 1ull << 32 : 0) | (wni ? 1ull << 33 : 0);
    red[wave * 4 + 1] = kmin;
    red[wave * 4 + 2] = kmax;
    red[wave * 4 + 3] = amax;
  }
  block_sync();
  if (tid == 0) {
    uint64_t flags = 0;
    smax = 0, kmin = ~0ull, kmax = 0, amax = 0;
    for (int w = 0; w < kGbmWaves; w++) {
      flags |= red[w * 4 + 0] >> 32;
      smax = max(smax, red[w * 4 + 0] & 0xFFFFFFFFull);
      kmin = min(kmin, red[w * 4 + 1]);
      kmax = max(kmax, red[w * 4 + 2]);
      amax = max(amax, red[w * 4 + 3]);
    }
    if (flags & 1) atomicOr((unsigned long long*)&A.acc[0], 1ull);
    if (flags & 2) atomicOr((unsigned long long*)&A.acc[1], 1ull);
    atomicMax((unsigned long long*)&A.acc[2], (unsigned long long)smax);
    atomicMin((unsigned long long*)&A.acc[3], (unsigned long long)kmin);
    atomicMax((unsigned long long*)&A.acc[4], (unsigned long long)kmax);
    atomicMax((unsigned long long*)&A.acc[5], (unsigned long long)amax);
  }
}

void launch_gbm_step(hipStream_t st, const GbmArgs& a) {
  if (a.N <= 0) return;
  const bool lds = gbm_tree_in_lds(a.num_nodes);
  const size_t sh = gbm_lds_bytes(a.num_nodes);
  const dim3 grid((unsigned)gbm_blocks(a.N)), block(kGbmBlock);
  if (a.mode == kGbmResidual) {
    if (lds)
      hipLaunchKernelGGL((k_gbm_step<kGbmResidual, true>), grid, block, sh, st, a);
    else
      hipLaunchKernelGGL((k_gbm_step<kGbmResidual, false>), grid, block, sh, st, a);
  } else {
    if (lds)
      hipLaunchKernelGGL((k_gbm_step<kGbmLoss, true>), grid, block, sh, st, a);
    else
      hipLaunchKernelGGL((k_gbm_step<kGbmLoss, false>), grid, block, sh, st, a);
  }
}

}  // namespace sbag
