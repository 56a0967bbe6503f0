// sbag_proba.hip — per-class raw predictions of a gini forest for gfx950 (MI355X, CDNA4).
//
// raw[row][c] over the trees that count for the row (every tree, or for the out-of-bag
// form the learners i with counts[i][row] == 0), in learner order:
//   kRawVotes  hard voting: the number of those trees whose prediction is class c
//   kRawLeaf   soft voting (RandomForestClassificationModel.predictRaw): s[c] = 0.0, then
//              for every tree s[c] = s[c] + st[c] / total, st the class counts of the leaf
//              the row reaches and total their left-to-right sum; nothing when total == 0
// The division is made once per leaf when the forest is packed (one IEEE division either
// way); a leaf whose total is 0, and the classes past a tree's own count, hold +0.0 there:
// s + 0.0 == s bit for bit for every s this sum can reach (s is never -0.0).
//
//   k_proba_tiled  the fused pass in k_predict_oob's geometry: 512 staged rows per
//                  workgroup at pitch S * code_bytes + 4, two walks per thread, forest
//                  chunks (packed nodes + per-leaf payload) in LDS, thresholds in code space,
//                  an in-bag row treated as already at a leaf.  Accumulators [C][512] in
//                  LDS (u16 counters, or fp64 sums for kRawLeaf), column `row` owned by the
//                  thread that walks the row: no atomics, additions in tree order (up to 8
//                  classes the soft sums live in the thread's registers in between).  The
//                  tile's rows x Cout doubles leave (and, between learner batches, enter)
//                  through LDS as one contiguous block of global memory.
//   k_proba_walk   the general path: one thread per row over DevNodes and fractions in
//                  global memory, accumulating in the thread's own output row (u32 codes,
//                  trees or class counts the LDS does not hold).  Same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

#include "sbag_internal.h"

namespace sbag {

namespace {

constexpr int kPrRows = 512;  // = k_predict_tiled's tile (predict_tiled_lds sizes the LDS)
constexpr int kPrThreads = 256;

// (as sbag_kernels.hip's: the dynamic-LDS cap of a kernel, once per (kernel, device))
void proba_set_max_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> g(mu);
  if (done.count({fn, dev})) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess)
    done.insert({fn, dev});
}

template <int KIND>
struct AccOf {
  typedef uint16_t type;
};
template <>
struct AccOf<kRawLeaf> {
  typedef double type;
};

}  // namespace

size_t proba_acc_lds(int kind, int C) {
  return (size_t)C * kPrRows * (kind == kRawLeaf ? 8 : 2);
}

// LDS: [512 rows x (S code bytes + 4)] [chunk_bytes: packed nodes + leaf payload]
// [accumulators [C][512]].  Thread tid owns rows row0 + tid and row0 + tid + 256 and their
// accumulator columns; consecutive lanes touch consecutive words of a class plane (no bank
// conflict on the hot path).  Other threads touch a column only in the prologue (carried
// state in) and the epilogue (result out), each fenced by a barrier.
// CW > 0 (kRawLeaf with C == CW, 2..8 classes): the thread keeps its two columns' sums in
// registers between those two points, so a (tree, row) costs CW LDS reads of fractions and
// no LDS read-modify-write; the additions and their order are the same.
template <typename CT, int KIND, int CW>
__global__ __launch_bounds__(kPrThreads) void k_proba_tiled(PredictArgs A, ProbaArgs Q) {
  typedef typename AccOf<KIND>::type AT;
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int pitch = A.S * (int)sizeof(CT) + 4;
  unsigned char* rows = smem;
  unsigned char* chunk = smem + (size_t)kPrRows * pitch;
  AT* acc = (AT*)(chunk + A.chunk_bytes);  // [C][kPrRows]
  const int64_t row0 = (int64_t)blockIdx.x * kPrRows;
  const int rb = A.S * (int)sizeof(CT);  // bytes of one row
  for (int q = tid; q < kPrRows * (rb >> 2); q += kPrThreads) {
    const int r = q / (rb >> 2), w = q - r * (rb >> 2);
    uint32_t v = 0;
    if (row0 + r < A.N) v = *(const uint32_t*)((const unsigned char*)A.codes + (row0 + r) * rb + w * 4);
    *(uint32_t*)(rows + r * pitch + w * 4) = v;
  }
  const int C = Q.C, Cout = Q.Cout;
  const int tile_rows = (int)(A.N - row0 < kPrRows ? A.N - row0 : kPrRows);
  const int tile_vals = tile_rows * Cout;  // the tile's block of raw: [tile_rows][Cout]
  double* gtile = Q.raw + row0 * Cout;
  for (int i = tid; i < C * kPrRows; i += kPrThreads) acc[i] = (AT)0;
  if (!Q.first) {
    block_sync();  // the zeros before the carried values
    for (int j = tid; j < tile_vals; j += kPrThreads) {
      const int r = j / Cout, c = j - r * Cout;
      if (c < C) acc[c * kPrRows + r] = (AT)gtile[j];
    }
  }
  const int64_t ra = row0 + tid, rbw = ra + kPrThreads;
  const bool in0 = ra < A.N, in1 = rbw < A.N;
  int n0 = 0, n1 = 0;
  if (!Q.first && Q.n_oob) {
    if (in0) n0 = Q.n_oob[ra];
    if (in1) n1 = Q.n_oob[rbw];
  }
  const unsigned char* r0p = rows + tid * pitch;
  const unsigned char* r1p = rows + (tid + kPrThreads) * pitch;
  // the bag multiplicities of the next tree, loaded a tree ahead (lanes coalesced over
  // rows); rows past N count as in bag: no walk, nothing accumulated
  const uint8_t* cp = Q.counts;
  uint32_t k0n = in0 ? 0 : 1, k1n = in1 ? 0 : 1;
  if (cp && Q.t0 < Q.t1) {
    if (in0) k0n = cp[ra];
    if (in1) k1n = cp[rbw];
  }
  block_sync();  // the row tile and the accumulators are written
  double r0[CW > 0 ? CW : 1], r1[CW > 0 ? CW : 1];
  if (CW > 0) {
#pragma unroll
    for (int k = 0; k < CW; k++) {
      r0[k] = (double)acc[k * kPrRows + tid];
      r1[k] = (double)acc[k * kPrRows + tid + kPrThreads];
    }
  }
  for (int c = 0; c < A.nchunks; c++) {
    const PredictChunk ch = A.chunks[c];
    const int ta = ch.t0 > Q.t0 ? ch.t0 : Q.t0, tb = ch.t1 < Q.t1 ? ch.t1 : Q.t1;
    if (ta >= tb) continue;  // (uniform: no tree of this batch in the chunk)
    block_sync();            // previous chunk done
    const int nb = (int)(ch.n1 - ch.n0) * 8, lb = (int)(ch.l1 - ch.l0) * 8;
    for (int i = tid; i < (nb >> 3); i += kPrThreads) ((PNode*)chunk)[i] = A.nodes[ch.n0 + i];
    for (int i = tid; i < (lb >> 3); i += kPrThreads)
      ((double*)(chunk + nb))[i] = A.leaves[ch.l0 + i];
    block_sync();
    for (int t = ta; t < tb; t++) {
      const PNode* tn = (const PNode*)chunk + (A.tree_node[t] - ch.n0);
      const double* tl = (const double*)(chunk + nb) + (A.tree_leaf[t] - ch.l0);
      const bool oob0 = k0n == 0, oob1 = k1n == 0;
      if (cp && t + 1 < Q.t1) {
        cp += A.N;
        if (in0) k0n = cp[ra];
        if (in1) k1n = cp[rbw];
      }
      PNode a0 = tn[0], a1 = a0;
      if (!oob0) a0.a = 0x80000000u;  // in bag (or past N): already at a leaf
      if (!oob1) a1.a = 0x80000000u;
      while (!((a0.a & a1.a) & 0x80000000u)) {  // until both walks reach a leaf
        if (!(a0.a & 0x80000000u)) {
          const uint32_t code = ((const CT*)r0p)[a0.b >> 17];
          a0 = tn[a0.a + (code < (a0.b & 0x1ffffu) ? 0u : 1u)];
        }
        if (!(a1.a & 0x80000000u)) {
          const uint32_t code = ((const CT*)r1p)[a1.b >> 17];
          a1 = tn[a1.a + (code < (a1.b & 0x1ffffu) ? 0u : 1u)];
        }
      }
      n0 += oob0 ? 1 : 0;
      n1 += oob1 ? 1 : 0;
      if (KIND == kRawLeaf) {
        // Both rows, four classes at a time: the loads of a group are issued before its
        // stores (the fractions and the sums share the LDS, so a store would otherwise
        // order every later load behind it).  A row that does not count adds +0.0, which
        // leaves every bit of its sums (never -0.0) as it is; its leaf index is 0.
        const double* f0 = tl + (size_t)(a0.a & 0x7fffffffu) * C;
        const double* f1 = tl + (size_t)(a1.a & 0x7fffffffu) * C;
        AT* s0 = acc + tid;
        AT* s1 = acc + tid + kPrThreads;
        if (CW > 0) {
#pragma unroll
          for (int k = 0; k < CW; k++) {
            r0[k] += oob0 ? f0[k] : 0.0;
            r1[k] += oob1 ? f1[k] : 0.0;
          }
        }
        for (int k0 = 0; CW == 0 && k0 < C; k0 += 4) {
          double x0[4], x1[4], y0[4], y1[4];
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (k0 + j < C) {
              x0[j] = f0[k0 + j];
              x1[j] = f1[k0 + j];
              y0[j] = (double)s0[(k0 + j) * kPrRows];
              y1[j] = (double)s1[(k0 + j) * kPrRows];
            }
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (k0 + j < C) {
              s0[(k0 + j) * kPrRows] = (AT)(y0[j] + (oob0 ? x0[j] : 0.0));
              s1[(k0 + j) * kPrRows] = (AT)(y1[j] + (oob1 ? x1[j] : 0.0));
            }
        }
      } else {
        if (oob0) acc[(int)tl[a0.a & 0x7fffffffu] * kPrRows + tid] += (AT)1;
        if (oob1) acc[(int)tl[a1.a & 0x7fffffffu] * kPrRows + tid + kPrThreads] += (AT)1;
      }
    }
  }
  if (Q.n_oob) {
    if (in0) Q.n_oob[ra] = n0;
    if (in1) Q.n_oob[rbw] = n1;
  }
  if (CW > 0) {
#pragma unroll
    for (int k = 0; k < CW; k++) {
      acc[k * kPrRows + tid] = (AT)r0[k];
      acc[k * kPrRows + tid + kPrThreads] = (AT)r1[k];
    }
  }
  block_sync();  // every column is final before other threads read it
  for (int j = tid; j < tile_vals; j += kPrThreads) {
    const int r = j / Cout, c = j - r * Cout;
    gtile[j] = c < C ? (double)acc[c * kPrRows + r] : 0.0;
  }
}

void launch_proba_tiled(hipStream_t st, const PredictArgs& a, const ProbaArgs& q) {
  PredictArgs b = a;
  b.agg = kAggMean;  // predict_tiled_lds: the row tile and the chunk only
  const size_t lds = predict_tiled_lds(b) + proba_acc_lds(q.kind, q.C);
  const dim3 grid((unsigned)((a.N + kPrRows - 1) / kPrRows));
#define SBAG_PROBA_LAUNCH(CT, KIND, CW)                                                      \
  do {                                                                                       \
    proba_set_max_lds((const void*)k_proba_tiled<CT, KIND, CW>, 160 * 1024);                 \
    hipLaunchKernelGGL((k_proba_tiled<CT, KIND, CW>), grid, dim3(kPrThreads), lds, st, b, q); \
  } while (0)
#define SBAG_PROBA_LEAF(CT)                               \
  switch (q.C) {                                          \
    case 2: SBAG_PROBA_LAUNCH(CT, kRawLeaf, 2); break;    \
    case 3: SBAG_PROBA_LAUNCH(CT, kRawLeaf, 3); break;    \
    case 4: SBAG_PROBA_LAUNCH(CT, kRawLeaf, 4); break;    \
    case 5: SBAG_PROBA_LAUNCH(CT, kRawLeaf, 5); break;    \
    case 6: SBAG_PROBA_LAUNCH(CT, kRawLeaf, 6); break;    \
    case 7: SBAG_PROBA_LAUNCH(CT, kRawLeaf, 7); break;    \
    case 8: SBAG_PROBA_LAUNCH(CT, kRawLeaf, 8); break;    \
    default: SBAG_PROBA_LAUNCH(CT, kRawLeaf, 0); break;   \
  }
  if (a.code_bytes == 1) {
    if (q.kind == kRawLeaf)
      SBAG_PROBA_LEAF(uint8_t)
    else
      SBAG_PROBA_LAUNCH(uint8_t, kRawVotes, 0);
  } else {
    if (q.kind == kRawLeaf)
      SBAG_PROBA_LEAF(uint16_t)
    else
      SBAG_PROBA_LAUNCH(uint16_t, kRawVotes, 0);
  }
#undef SBAG_PROBA_LEAF
#undef SBAG_PROBA_LAUNCH
}

// One thread per row; the row's Cout doubles of raw are the thread's accumulators (zeroed
// here when `first`), so learner batches need no other state than raw and n_oob.
__global__ __launch_bounds__(256) void k_proba_walk(const double* __restrict__ X,
                                                    const void* __restrict__ codes, int code_bytes,
                                                    const double* __restrict__ dict,
                                                    const int64_t* __restrict__ dict_off, int64_t N,
                                                    int32_t F, int32_t S,
                                                    const DevNode* __restrict__ nodes,
                                                    const int64_t* __restrict__ tree_off,
                                                    const double* __restrict__ frac,
                                                    const int64_t* __restrict__ leaf_off, ProbaArgs Q) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= N) return;
  double* o = Q.raw + row * Q.Cout;
  int n = 0;
  if (Q.first) {
    for (int c = 0; c < Q.Cout; c++) o[c] = 0.0;
  } else if (Q.n_oob) {
    n = Q.n_oob[row];
  }
  for (int l = Q.t0; l < Q.t1; l++) {
    if (Q.counts && Q.counts[(int64_t)(l - Q.t0) * N + row] != 0) continue;
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
    n++;
    if (Q.kind == kRawLeaf) {
      const double* fr = frac + (leaf_off[l] + t[id].pad) * Q.C;
      for (int c = 0; c < Q.C; c++) o[c] += fr[c];
    } else {
      o[(int)t[id].value] += 1.0;
    }
  }
  if (Q.n_oob) Q.n_oob[row] = n;
}

void launch_proba_walk(hipStream_t st, const double* X, const void* codes, int code_bytes,
                       const double* dict, const int64_t* dict_off, int64_t N, int32_t F, int32_t S,
                       const DevNode* nodes, const int64_t* tree_off, const double* frac,
                       const int64_t* leaf_off, const ProbaArgs& q) {
  hipLaunchKernelGGL(k_proba_walk, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, X, codes,
                     code_bytes, dict, dict_off, N, F, S, nodes, tree_off, frac, leaf_off, q);
}

}  // namespace sbag
