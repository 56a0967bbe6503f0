// sbag_wpred.hip — weighted sums over a forest's trees for gfx950 (MI355X, CDNA4): the
// transforms of the boosted model families in one pass.
//
// out[row][c] starts at +0.0; then, for every tree t in forest order,
//   kWDot    out[row][t % C] = out[row][t % C] + (tree_t(row) * weights[t])
//            (GBMRegressionModel / BoostingRegressionModel.predict's BLAS.dot at C = 1, the
//            res of GBMClassificationModel.predictRaw at C = numClasses, trees iteration-major)
//   kWClass  out[row][cls] = out[row][cls] + weights[t], cls the class tree_t(row) predicts
//            (BoostingClassificationModel.predictRaw)
// The product is rounded to fp64 before the addition: __dmul_rn / __dadd_rn are never
// contracted, and the file is built with -ffp-contract=off as the rest of the library.
//
//   k_wpred_tiled  the fused pass in k_proba_tiled's geometry: 512 staged rows per workgroup
//                  at pitch S * code_bytes + 4 (copied in 16-byte pieces), two walks per thread,
//                  forest chunks (packed
//                  nodes + one fp64 per leaf) in LDS, thresholds in code space.  kWDot: the
//                  leaf value is the product prediction * weights[t], rounded once when the
//                  plan is packed (one IEEE multiplication either way); kWClass: the class id,
//                  weights[t] read per tree.  Accumulators [C][512] fp64 in LDS, column `row`
//                  owned by the thread that walks the row: no atomics, additions in tree
//                  order.  REG (kWDot, C == 1): the thread's two sums live in registers from
//                  the first tree to the last.  The tile's rows x C doubles leave through LDS
//                  as one contiguous block of global memory.
//   k_wpred_walk   the general path: one thread per row over DevNodes in global memory,
//                  accumulating in the thread's own output row (u32 codes, trees or column
//                  counts the LDS does not hold).  Same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

#include "sbag_internal.h"

namespace sbag {

namespace {

constexpr int kWpRows = 512;  // = k_predict_tiled's tile (predict_tiled_lds sizes the LDS)
constexpr int kWpThreads = 256;

// (as sbag_kernels.hip's: the dynamic-LDS cap of a kernel, once per (kernel, device))
void wpred_set_max_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> g(mu);
  if (done.count({fn, dev})) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess)
    done.insert({fn, dev});
}

}  // namespace

size_t wpred_acc_lds(int C) { return (size_t)C * kWpRows * 8; }

// LDS: [512 rows x (S code bytes + 4)] [chunk_bytes: packed nodes + leaf values]
// [accumulators [C][512] fp64].  Thread tid owns rows row0 + tid and row0 + tid + 256 and
// their accumulator columns; consecutive lanes touch consecutive doubles of a column plane.
// Other threads touch a column only when it is zeroed and in the epilogue, each fenced by a
// barrier.  A row past N walks nothing and adds nothing.
template <typename CT, int KIND, bool REG>
__global__ __launch_bounds__(kWpThreads) void k_wpred_tiled(PredictArgs A, WpredArgs Q) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int pitch = A.S * (int)sizeof(CT) + 4;
  unsigned char* rows = smem;
  unsigned char* chunk = smem + (size_t)kWpRows * pitch;
  double* acc = (double*)(chunk + A.chunk_bytes);  // [C][kWpRows]
  const int64_t row0 = (int64_t)blockIdx.x * kWpRows;
  const int rb = A.S * (int)sizeof(CT);  // bytes of one row (S is a multiple of 16)
  const int vpr = rb >> 4;               // 16-byte pieces of one row (as sbag_stack.hip's stage_rows)
  for (int q = tid; q < kWpRows * vpr; q += kWpThreads) {
    const int r = q / vpr, w = q - r * vpr;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row0 + r < A.N) v = *(const uint4*)((const unsigned char*)A.codes + (row0 + r) * rb + w * 16);
    uint32_t* d = (uint32_t*)(rows + r * pitch + w * 16);
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
    d[3] = v.w;
  }
  const int C = Q.C;
  const int tile_rows = (int)(A.N - row0 < kWpRows ? A.N - row0 : kWpRows);
  const int tile_vals = tile_rows * C;  // the tile's block of out: [tile_rows][C]
  double* gtile = Q.out + row0 * C;
  for (int i = tid; i < C * kWpRows; i += kWpThreads) acc[i] = 0.0;
  const bool in0 = row0 + tid < A.N, in1 = row0 + tid + kWpThreads < A.N;
  const unsigned char* r0p = rows + tid * pitch;
  const unsigned char* r1p = rows + (tid + kWpThreads) * pitch;
  double s0 = 0.0, s1 = 0.0;  // REG: the two rows' sums
  int col = 0;                // kWDot: t % C of the next tree (uniform)
  for (int c = 0; c < A.nchunks; c++) {
    const PredictChunk ch = A.chunks[c];
    block_sync();  // the row tile and the zeros are written; the previous chunk is done
    const int nb = (int)(ch.n1 - ch.n0) * 8, lb = (int)(ch.l1 - ch.l0) * 8;
    for (int i = tid; i < (nb >> 3); i += kWpThreads) ((PNode*)chunk)[i] = A.nodes[ch.n0 + i];
    for (int i = tid; i < (lb >> 3); i += kWpThreads)
      ((double*)(chunk + nb))[i] = A.leaves[ch.l0 + i];
    block_sync();
    for (int t = ch.t0; t < ch.t1; t++) {
      const PNode* tn = (const PNode*)chunk + (A.tree_node[t] - ch.n0);
      const double* tl = (const double*)(chunk + nb) + (A.tree_leaf[t] - ch.l0);
      PNode a0 = tn[0], a1 = a0;
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
      const double v0 = tl[a0.a & 0x7fffffffu], v1 = tl[a1.a & 0x7fffffffu];
      if (KIND == kWDot) {
        if (REG) {
          s0 = __dadd_rn(s0, v0);
          s1 = __dadd_rn(s1, v1);
        } else {
          double* p0 = acc + col * kWpRows + tid;
          const double y0 = p0[0], y1 = p0[kWpThreads];
          if (in0) p0[0] = __dadd_rn(y0, v0);
          if (in1) p0[kWpThreads] = __dadd_rn(y1, v1);
          col = col + 1 == C ? 0 : col + 1;
        }
      } else {
        const double w = Q.weights[t];
        if (in0) {
          double* p = acc + (int)v0 * kWpRows + tid;
          *p = __dadd_rn(*p, w);
        }
        if (in1) {
          double* p = acc + (int)v1 * kWpRows + tid + kWpThreads;
          *p = __dadd_rn(*p, w);
        }
      }
    }
  }
  if (REG) {
    acc[tid] = s0;
    acc[tid + kWpThreads] = s1;
  }
  block_sync();  // every column is final before other threads read it
  for (int j = tid; j < tile_vals; j += kWpThreads) {
    const int r = j / C, c = j - r * C;
    gtile[j] = acc[c * kWpRows + r];
  }
}

void launch_wpred_tiled(hipStream_t st, const PredictArgs& a, const WpredArgs& q) {
  PredictArgs b = a;
  b.agg = kAggMean;  // predict_tiled_lds: the row tile and the chunk only
  const size_t lds = predict_tiled_lds(b) + wpred_acc_lds(q.C);
  const dim3 grid((unsigned)((a.N + kWpRows - 1) / kWpRows));
#define SBAG_WPRED_LAUNCH(CT, KIND, REG)                                                      \
  do {                                                                                        \
    wpred_set_max_lds((const void*)k_wpred_tiled<CT, KIND, REG>, 160 * 1024);                 \
    hipLaunchKernelGGL((k_wpred_tiled<CT, KIND, REG>), grid, dim3(kWpThreads), lds, st, b, q); \
  } while (0)
#define SBAG_WPRED_KIND(CT)                            \
  do {                                                 \
    if (q.kind == kWClass)                             \
      SBAG_WPRED_LAUNCH(CT, kWClass, false);           \
    else if (q.C == 1)                                 \
      SBAG_WPRED_LAUNCH(CT, kWDot, true);              \
    else                                               \
      SBAG_WPRED_LAUNCH(CT, kWDot, false);             \
  } while (0)
  if (a.code_bytes == 1)
    SBAG_WPRED_KIND(uint8_t);
  else
    SBAG_WPRED_KIND(uint16_t);
#undef SBAG_WPRED_KIND
#undef SBAG_WPRED_LAUNCH
}

// One thread per row; the row's C doubles of out are the thread's accumulators.
__global__ __launch_bounds__(256) void k_wpred_walk(const double* __restrict__ X,
                                                    const void* __restrict__ codes, int code_bytes,
                                                    const double* __restrict__ dict,
                                                    const int64_t* __restrict__ dict_off, int64_t N,
                                                    int32_t F, int32_t S,
                                                    const DevNode* __restrict__ nodes,
                                                    const int64_t* __restrict__ tree_off, int L,
                                                    WpredArgs Q) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= N) return;
  double* o = Q.out + row * Q.C;
  for (int c = 0; c < Q.C; c++) o[c] = 0.0;
  int col = 0;
  for (int l = 0; l < L; l++) {
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
    const double w = Q.weights[l];
    if (Q.kind == kWDot) {
      o[col] = __dadd_rn(o[col], __dmul_rn(t[id].value, w));
      col = col + 1 == Q.C ? 0 : col + 1;
    } else {
      const int k = (int)t[id].value;
      o[k] = __dadd_rn(o[k], w);
    }
  }
}

void launch_wpred_walk(hipStream_t st, const double* X, const void* codes, int code_bytes,
                       const double* dict, const int64_t* dict_off, int64_t N, int32_t F, int32_t S,
                       const DevNode* nodes, const int64_t* tree_off, int L, const WpredArgs& q) {
  hipLaunchKernelGGL(k_wpred_walk, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, X, codes,
                     code_bytes, dict, dict_off, N, F, S, nodes, tree_off, L, q);
}

}  // namespace sbag
