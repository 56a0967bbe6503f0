// sbag_spread.hip — per-row quantiles across a forest's trees for gfx950 (MI355X, CDNA4).
//
// For row r the predictions of the trees concerned (all of them, or with `counts` those whose
// bag left the row out), -0.0 read as +0.0, sorted ascending: v[0, n).  For probability p:
//   h = (double)(n - 1) * p; lo = floor(h); g = h - lo
//   out = v[lo] when g == 0, else v[lo] + g * (v[lo + 1] - v[lo]); NaN when n == 0
// with the product, the subtraction and the sum each rounded on their own (__dmul_rn /
// __dsub_rn / __dadd_rn; the file is built with -ffp-contract=off as the rest of the library).
//
// A row's values travel as ranks in the forest-wide dictionary of sorted distinct leaf values
// (sbag_spread_plan.h): order statistics of ranks are order statistics of values, and only the
// two ranks a probability lands between are turned back into doubles.  The all-ones key is
// "in bag / padding" and sorts last, so n is the number of keys below it.
//
//   k_quant_tiled   walk, then select, in one launch.  Walk: k_wpred_tiled's geometry (rows
//                   staged in 16-byte pieces at pitch S * code_bytes + 4, forest chunks in LDS,
//                   thresholds in code space) with the row tile R one of 512, 256, 128, 64 and a
//                   leaf node carrying its rank: no leaf values in the chunk.  The 512 walk
//                   slots of a step (two a thread) cover 512 / R trees side by side; slot
//                   (tree t, row r) stores its rank at ranks[t][r], u16 [L][R + 2] in LDS, a
//                   wave's stores contiguous.  Nothing is accumulated, so no slot depends on
//                   another.  Select: after one barrier each wave takes the tile's rows in turn
//                   (sort_select below).
//   k_quant_walk    the general path's walk: one thread per row over DevNodes in global
//                   memory, u32 ranks to a workspace [L][rows of the batch].
//   k_quant_select  the general path's select: a wave per row, the same sort on u32 keys.
//
// sort_select<KT, K>: the wave's 64 lanes hold the row's Lpad = 64 K keys, K a lane.  Key p is
// loaded by lane p % 64 (one LDS bank per lane at the matrix's pitch); a bitonic network sorts
// by position lane * K + k: the strides below K are compare-exchanges inside the lane, those
// from K up exchange whole registers with lane ^ (stride / K) (ds_swizzle below 32 lanes,
// a shuffle at 32).  u16 keys with K >= 2 sit two to a register and go through the packed u16
// min / max: one exchange and one min / max pair serve both keys, and the stride-1 step is
// a min / max against the register's own halves swapped.  The sorted keys go back to LDS, and
// lanes 0 .. Q - 1 each take one probability: lo and g from n, two keys, two dictionary values
// (global memory, L2-resident), the interpolation, and the row's Q doubles leave as one
// contiguous store of the wave.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

#include "sbag_internal.h"

namespace sbag {

namespace {

constexpr int kQtThreads = 256;
constexpr int kQtSlots = 512;  // walk slots of a step: two a thread

// (as sbag_kernels.hip's: the dynamic-LDS cap of a kernel, once per (kernel, device))
void quant_set_max_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> g(mu);
  if (done.count({fn, dev})) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess)
    done.insert({fn, dev});
}

__device__ __forceinline__ double quant_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

template <bool PK>
__device__ __forceinline__ uint32_t key_min(uint32_t a, uint32_t b) {
  if constexpr (PK)
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a),
                                                                  __builtin_bit_cast(u16x2, b)));
  else
    return a < b ? a : b;
}
template <bool PK>
__device__ __forceinline__ uint32_t key_max(uint32_t a, uint32_t b) {
  if constexpr (PK)
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a),
                                                                  __builtin_bit_cast(u16x2, b)));
  else
    return a > b ? a : b;
}

// the register of lane ^ LS
template <int LS>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v) {
  if constexpr (LS < 32)  // bit mode within 32 lanes: and 0x1f, or 0, xor LS
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (LS << 10) | 0x1f);
  else
    return (uint32_t)__shfl_xor((int)v, LS, 64);
}

template <typename KT, int K>
struct SortShape {
  static constexpr bool PK = sizeof(KT) == 2 && K >= 2;  // two u16 keys a register
  static constexpr int NR = PK ? K / 2 : K;              // registers a lane
};

// The bitonic network over positions lane * K + k, ascending, from the step (SIZE, STRIDE) on.
// A pair (p, p ^ STRIDE) is ordered ascending where p & SIZE == 0.
template <typename KT, int K, int SIZE, int STRIDE>
__device__ __forceinline__ void bitonic_from(uint32_t* x, int lane) {
  constexpr bool PK = SortShape<KT, K>::PK;
  constexpr int NR = SortShape<KT, K>::NR;
  if constexpr (STRIDE >= K) {  // whole registers against lane ^ LS: SIZE >= 2 K, the
    constexpr int LS = STRIDE / K;  // direction is the lane's alone
    const bool keep_min = ((lane & LS) == 0) == ((lane & (SIZE / K)) == 0);
#pragma unroll
    for (int j = 0; j < NR; j++) {
      const uint32_t o = lane_xor<LS>(x[j]);
      const uint32_t mn = key_min<PK>(x[j], o), mx = key_max<PK>(x[j], o);
      x[j] = keep_min ? mn : mx;
    }
  } else if constexpr (PK && STRIDE == 1) {  // the two halves of a register
#pragma unroll
    for (int j = 0; j < NR; j++) {
      const bool asc = ((lane * K + 2 * j) & SIZE) == 0;
      const uint32_t sw = (x[j] >> 16) | (x[j] << 16);
      const uint32_t mn = key_min<true>(x[j], sw), mx = key_max<true>(x[j], sw);
      x[j] = asc ? (mn & 0xffffu) | (mx & 0xffff0000u) : (mx & 0xffffu) | (mn & 0xffff0000u);
    }
  } else {  // registers RS apart (packed: both halves share the direction, SIZE >= 4)
    constexpr int RS = PK ? STRIDE / 2 : STRIDE, PER = PK ? 2 : 1;
#pragma unroll
    for (int j = 0; j < NR; j++)
      if ((j & RS) == 0) {
        const bool asc = ((lane * K + j * PER) & SIZE) == 0;
        const uint32_t mn = key_min<PK>(x[j], x[j + RS]), mx = key_max<PK>(x[j], x[j + RS]);
        x[j] = asc ? mn : mx;
        x[j + RS] = asc ? mx : mn;
      }
  }
  if constexpr (STRIDE > 1)
    bitonic_from<KT, K, SIZE, STRIDE / 2>(x, lane);
  else if constexpr (SIZE < 64 * K)
    bitonic_from<KT, K, SIZE * 2, SIZE>(x, lane);
}

// One row by one wave.  load(p): key p of the row, p < L.  sorted: where the sorted keys go,
// key q at sorted[q * sstride] for q < L (may be the place load reads).  Lane q < nq writes
// orow[q] for its probability p; lane 0 writes *n_out (null: not wanted).
template <typename KT, int K, typename LD>
__device__ __forceinline__ void sort_select(LD load, KT* sorted, int sstride, int L, int lane, int nq,
                                            double p, const double* __restrict__ dict, double* orow,
                                            int32_t* n_out) {
  constexpr bool PK = SortShape<KT, K>::PK;
  constexpr int NR = SortShape<KT, K>::NR;
  constexpr uint32_t kLast = (uint32_t)(KT) ~(KT)0;
  uint32_t x[NR];
  int n = 0;
#pragma unroll
  for (int j = 0; j < NR; j++) x[j] = 0;
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int pos = k * 64 + lane;
    const uint32_t v = pos < L ? (uint32_t)load(pos) : kLast;
    n += v != kLast ? 1 : 0;
    if constexpr (PK)
      x[k >> 1] |= v << (16 * (k & 1));
    else
      x[k] = v;
  }
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) n += __shfl_xor(n, h, 64);
  bitonic_from<KT, K, 2, 1>(x, lane);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // every lane's loads are done
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int q = lane * K + k;
    const uint32_t v = PK ? (x[k >> 1] >> (16 * (k & 1))) & 0xffffu : x[k];
    if (q < L) sorted[(size_t)q * sstride] = (KT)v;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // the wave's keys are in LDS, in order
  if (lane < nq) {
    double o = quant_nan();
    if (n > 0) {
      const double h = __dmul_rn((double)(n - 1), p);
      const double fl = floor(h);
      const int lo = (int)fl;
      const double g = __dsub_rn(h, fl);
      o = dict[sorted[(size_t)lo * sstride]];
      if (g != 0.0) {  // h is no integer: lo + 1 <= n - 1
        const double v1 = dict[sorted[(size_t)(lo + 1) * sstride]];
        o = __dadd_rn(o, __dmul_rn(g, __dsub_rn(v1, o)));
      }
    }
    orow[lane] = o;
  }
  if (n_out && lane == 0) *n_out = n;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the keys are read before `sorted` is reused
}

// sort_select at the K of L trees (64 K the power of two >= max(L, 64))
template <typename KT, typename LD>
__device__ __forceinline__ void sort_select_any(LD load, KT* sorted, int sstride, int L, int lane, int nq,
                                                double p, const double* __restrict__ dict, double* orow,
                                                int32_t* n_out) {
  if (L <= 64)
    sort_select<KT, 1>(load, sorted, sstride, L, lane, nq, p, dict, orow, n_out);
  else if (L <= 128)
    sort_select<KT, 2>(load, sorted, sstride, L, lane, nq, p, dict, orow, n_out);
  else if (L <= 256)
    sort_select<KT, 4>(load, sorted, sstride, L, lane, nq, p, dict, orow, n_out);
  else if (L <= 512)
    sort_select<KT, 8>(load, sorted, sstride, L, lane, nq, p, dict, orow, n_out);
  else
    sort_select<KT, 16>(load, sorted, sstride, L, lane, nq, p, dict, orow, n_out);
}

}  // namespace

// LDS: [R rows x (S code bytes + 4)] [chunk_bytes: packed nodes] [ranks u16 [L][R + 2]].
// Walk slot s = tid, tid + 256: row s % R of the tile, tree lane s / R of the 512 / R trees of
// a step.  Slot (t, r) alone writes ranks[t][r]; after the barrier wave w sorts the columns of
// rows w, w + 4, ... in place.  A row past N, and with OOB a row the tree's bag holds, walks
// nothing and stores the last key.
template <typename CT, bool OOB>
__global__ __launch_bounds__(kQtThreads) void k_quant_tiled(PredictArgs A, QuantArgs Q) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int R = Q.R, Rp = R + 2;
  const int pitch = A.S * (int)sizeof(CT) + 4;
  unsigned char* rows = smem;
  unsigned char* chunk = smem + (size_t)R * pitch;
  uint16_t* ranks = (uint16_t*)(chunk + A.chunk_bytes);  // [L][Rp]
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int rb = A.S * (int)sizeof(CT);  // bytes of one row (S is a multiple of 16)
  const int vpr = rb >> 4;               // 16-byte pieces of one row
  for (int q = tid; q < R * vpr; q += kQtThreads) {
    const int r = q / vpr, w = q - r * vpr;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row0 + r < A.N) v = *(const uint4*)((const unsigned char*)A.codes + (row0 + r) * rb + w * 16);
    uint32_t* d = (uint32_t*)(rows + r * pitch + w * 16);
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
    d[3] = v.w;
  }
  const int G = kQtSlots / R;  // trees of a step
  const int r0 = tid & (R - 1), g0 = tid / R;
  const int r1 = (tid + kQtThreads) & (R - 1), g1 = (tid + kQtThreads) / R;
  const bool in0 = row0 + r0 < A.N, in1 = row0 + r1 < A.N;
  const unsigned char* r0p = rows + r0 * pitch;
  const unsigned char* r1p = rows + r1 * pitch;
  const uint8_t* c0p = OOB ? Q.counts + row0 + r0 : nullptr;
  const uint8_t* c1p = OOB ? Q.counts + row0 + r1 : nullptr;
  for (int c = 0; c < A.nchunks; c++) {
    const PredictChunk ch = A.chunks[c];
    // the bag multiplicities of a slot's next tree, loaded a step ahead (lanes coalesced over
    // rows); the chunk's first ones while the chunk is copied
    uint32_t k0n = 0, k1n = 0;
    if (OOB) {
      if (in0 && ch.t0 + g0 < ch.t1) k0n = c0p[(int64_t)(ch.t0 + g0) * A.N];
      if (in1 && ch.t0 + g1 < ch.t1) k1n = c1p[(int64_t)(ch.t0 + g1) * A.N];
    }
    block_sync();  // the row tile is written; the previous chunk is done
    for (int i = tid; i < (int)(ch.n1 - ch.n0); i += kQtThreads) ((PNode*)chunk)[i] = A.nodes[ch.n0 + i];
    block_sync();
    for (int tb = ch.t0; tb < ch.t1; tb += G) {
      const int t0 = tb + g0, t1 = tb + g1;
      const bool have0 = t0 < ch.t1, have1 = t1 < ch.t1;
      const bool walk0 = have0 && in0 && k0n == 0, walk1 = have1 && in1 && k1n == 0;
      if (OOB) {
        if (in0 && t0 + G < ch.t1) k0n = c0p[(int64_t)(t0 + G) * A.N];
        if (in1 && t1 + G < ch.t1) k1n = c1p[(int64_t)(t1 + G) * A.N];
      }
      const PNode* tn0 = (const PNode*)chunk + (A.tree_node[have0 ? t0 : ch.t0] - ch.n0);
      const PNode* tn1 = (const PNode*)chunk + (A.tree_node[have1 ? t1 : ch.t0] - ch.n0);
      PNode a0 = tn0[0], a1 = tn1[0];
      if (!walk0) a0.a = 0x8000ffffu;  // already at a leaf, its rank the last key
      if (!walk1) a1.a = 0x8000ffffu;
      while (!((a0.a & a1.a) & 0x80000000u)) {  // until both walks reach a leaf
        if (!(a0.a & 0x80000000u)) {
          const uint32_t code = ((const CT*)r0p)[a0.b >> 17];
          a0 = tn0[a0.a + (code < (a0.b & 0x1ffffu) ? 0u : 1u)];
        }
        if (!(a1.a & 0x80000000u)) {
          const uint32_t code = ((const CT*)r1p)[a1.b >> 17];
          a1 = tn1[a1.a + (code < (a1.b & 0x1ffffu) ? 0u : 1u)];
        }
      }
      if (have0) ranks[t0 * Rp + r0] = (uint16_t)a0.a;
      if (have1) ranks[t1 * Rp + r1] = (uint16_t)a1.a;
    }
  }
  block_sync();  // every rank of the tile is stored
  const int wave = tid >> 6, lane = tid & 63;
  const int tile_rows = (int)(A.N - row0 < R ? A.N - row0 : R);
  const double p = lane < Q.Q ? Q.probs[lane] : 0.0;
  for (int r = wave; r < tile_rows; r += kQtThreads / 64) {
    uint16_t* col = ranks + r;
    sort_select_any<uint16_t>([&](int pos) { return col[pos * Rp]; }, col, Rp, A.L, lane, Q.Q, p, Q.dict,
                              Q.out + (row0 + r) * Q.Q, OOB && Q.n_oob ? Q.n_oob + row0 + r : nullptr);
  }
}

void launch_quant_tiled(hipStream_t st, const PredictArgs& a, const QuantArgs& q) {
  const size_t pitch = (size_t)a.S * a.code_bytes + 4;
  const size_t lds = (size_t)q.R * pitch + (size_t)a.chunk_bytes + (((size_t)a.L * (q.R + 2) * 2 + 15) & ~(size_t)15);
  const dim3 grid((unsigned)((a.N + q.R - 1) / q.R));
#define SBAG_QUANT_LAUNCH(CT, OOB)                                                           \
  do {                                                                                       \
    quant_set_max_lds((const void*)k_quant_tiled<CT, OOB>, 160 * 1024);                      \
    hipLaunchKernelGGL((k_quant_tiled<CT, OOB>), grid, dim3(kQtThreads), lds, st, a, q);     \
  } while (0)
  if (a.code_bytes == 1) {
    if (q.counts)
      SBAG_QUANT_LAUNCH(uint8_t, true);
    else
      SBAG_QUANT_LAUNCH(uint8_t, false);
  } else {
    if (q.counts)
      SBAG_QUANT_LAUNCH(uint16_t, true);
    else
      SBAG_QUANT_LAUNCH(uint16_t, false);
  }
#undef SBAG_QUANT_LAUNCH
}

// One thread per row of the batch; keys[l][row] = the rank of the leaf tree l sends the row to,
// or the last key where the tree's bag holds the row (counts at row stride `cstride`).
__global__ __launch_bounds__(256) void k_quant_walk(const double* __restrict__ X,
                                                    const void* __restrict__ codes, int code_bytes,
                                                    const double* __restrict__ dict,
                                                    const int64_t* __restrict__ dict_off, int64_t n,
                                                    int32_t F, int32_t S,
                                                    const DevNode* __restrict__ nodes,
                                                    const int64_t* __restrict__ tree_off,
                                                    const uint32_t* __restrict__ leaf_rank,
                                                    const int64_t* __restrict__ leaf_off, int L,
                                                    const uint8_t* __restrict__ counts, int64_t cstride,
                                                    uint32_t* __restrict__ keys) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  for (int l = 0; l < L; l++) {
    if (counts && counts[(int64_t)l * cstride + row] != 0) {
      keys[(int64_t)l * n + row] = 0xffffffffu;
      continue;
    }
    const DevNode* t = nodes + tree_off[l];
    int id = 0;
    while (t[id].left >= 0) {
      const int g = t[id].gfeat;
      double v;
      if (X) {
        v = X[row * F + g];
      } else {
        const int64_t c = code_bytes == 1   ? (int64_t)((const uint8_t*)codes)[row * S + g]
                          : code_bytes == 2 ? (int64_t)((const uint16_t*)codes)[row * S + g]
                                            : (int64_t)((const uint32_t*)codes)[row * S + g];
        v = dict[dict_off[g] + c];
      }
      id = (v <= t[id].value) ? t[id].left : t[id].right;
    }
    keys[(int64_t)l * n + row] = leaf_rank[leaf_off[l] + t[id].pad];
  }
}

void launch_quant_walk(hipStream_t st, const double* X, const void* codes, int code_bytes,
                       const double* dict, const int64_t* dict_off, int64_t n, int32_t F, int32_t S,
                       const DevNode* nodes, const int64_t* tree_off, const uint32_t* leaf_rank,
                       const int64_t* leaf_off, int L, const uint8_t* counts, int64_t cstride,
                       uint32_t* keys) {
  hipLaunchKernelGGL(k_quant_walk, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, X, codes,
                     code_bytes, dict, dict_off, n, F, S, nodes, tree_off, leaf_rank, leaf_off, L, counts,
                     cstride, keys);
}

// A wave per row of the batch: keys [L][n] from k_quant_walk, sorted through the wave's own
// 1024 words of LDS (L <= 1024).  Q.out / Q.n_oob are the batch's first row's.
__global__ __launch_bounds__(256) void k_quant_select(const uint32_t* __restrict__ keys, int64_t n, int L,
                                                      QuantArgs Q) {
  __shared__ uint32_t sorted[4][1024];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= n) return;  // (no barrier below)
  const double p = lane < Q.Q ? Q.probs[lane] : 0.0;
  const uint32_t* col = keys + row;
  sort_select_any<uint32_t>([&](int pos) { return col[(int64_t)pos * n]; }, sorted[wave], 1, L, lane, Q.Q, p,
                            Q.dict, Q.out + row * Q.Q, Q.n_oob ? Q.n_oob + row : nullptr);
}

void launch_quant_select(hipStream_t st, const uint32_t* keys, int64_t n, int L, const QuantArgs& q) {
  hipLaunchKernelGGL(k_quant_select, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, keys, n, L, q);
}

}  // namespace sbag
