// sbag_stack.hip — stacking for gfx950 (MI355X, CDNA4): the level-1 dataset of a forest of base
// learners, and the two-level transform of a stacking model, both in code space.
//
// The level-1 feature k of a row is base tree k's prediction, so it takes at most as many
// distinct values as the tree has leaves: its dictionary is the sorted distinct values of the
// leaves some row reaches, and a row's code is known when its walk reaches a leaf.
//
//   k_stack_walk       k_predict_tiled's geometry (512 staged rows per workgroup, two walks per
//                      thread, forest chunks of packed nodes in LDS, thresholds in code space):
//                      idx[t][row] = the index the reached leaf carries in tree t.  With
//                      `present` the chunk's leaves have a flag word each in LDS (where
//                      k_predict_tiled keeps the leaf values); after the chunk's trees a set
//                      flag goes to global memory with one atomic, and only when the global
//                      flag is not set yet.
//   k_stack_codes      idx -> final codes through the per-tree map the host compacts from the
//                      flags; 64 rows x up to 128 columns per workgroup, transposed through
//                      LDS so that both the reads of idx and the writes of the rows coalesce;
//                      writes the padding columns.
//   k_predict_stacked  the fused transform: base trees, stack tree, its fp64 leaf values and
//                      the row tile in LDS.  A row walks the stack tree and evaluates base tree
//                      k only when a stack node tests feature k (a repeated test walks the
//                      base tree again: no per-row cache); every compare is an integer compare
//                      on codes or ranks.  Two rows per thread, one step of each in turn.
//   k_stack_top        the general path: the stack tree over level-1 ranks [K][N] in global
//                      memory (written by k_stack_walk chunk by chunk, or by k_stack_rank_walk)
//   k_stack_rank_walk  ranks by a node walk from global memory (u32 codes, trees past the LDS
//                      chunk): one thread per row.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

#include "sbag_internal.h"

namespace sbag {

namespace {

constexpr int kStRows = 512;  // = k_predict_tiled's tile (predict_tiled_lds sizes the LDS)
constexpr int kStThreads = 256;

// (as sbag_kernels.hip's: the dynamic-LDS cap of a kernel, once per (kernel, device))
void stack_set_max_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> g(mu);
  if (done.count({fn, dev})) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess)
    done.insert({fn, dev});
}

// the row tile of a workgroup: kStRows rows of codes at `pitch` bytes, zeros past N.  A row is a
// multiple of 16 bytes and the tile's rows are contiguous in global memory, so consecutive
// lanes load consecutive 16-byte pieces; the pitch (row + 4 bytes: rows on distinct banks)
// is not, so a piece goes to LDS as four words.
template <typename CT>
__device__ __forceinline__ void stage_rows(unsigned char* rows, const void* codes, int S, int64_t N,
                                           int64_t row0, int tid) {
  const int pitch = S * (int)sizeof(CT) + 4;
  const int rb = S * (int)sizeof(CT);  // bytes of one row (a multiple of 16)
  const int vpr = rb >> 4;             // 16-byte pieces of one row
  for (int q = tid; q < kStRows * vpr; q += kStThreads) {
    const int r = q / vpr, w = q - r * vpr;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row0 + r < N) v = *(const uint4*)((const unsigned char*)codes + (row0 + r) * rb + w * 16);
    uint32_t* d = (uint32_t*)(rows + r * pitch + w * 16);
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
    d[3] = v.w;
  }
}

}  // namespace

// LDS: [512 rows x (S code bytes + 4)] [chunk_bytes: packed nodes, then one u32 flag per leaf
// of the chunk (a chunk holds 8 bytes per leaf, the flags use 4)].
template <typename CT>
__global__ __launch_bounds__(kStThreads) void k_stack_walk(PredictArgs A, uint16_t* __restrict__ idx,
                                                           uint32_t* __restrict__ present) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int pitch = A.S * (int)sizeof(CT) + 4;
  unsigned char* rows = smem;
  unsigned char* chunk = smem + (size_t)kStRows * pitch;
  const int64_t row0 = (int64_t)blockIdx.x * kStRows;
  stage_rows<CT>(rows, A.codes, A.S, A.N, row0, tid);
  const unsigned char* r0p = rows + tid * pitch;
  const unsigned char* r1p = rows + (tid + kStThreads) * pitch;
  const bool in0 = row0 + tid < A.N, in1 = row0 + tid + kStThreads < A.N;
  for (int c = 0; c < A.nchunks; c++) {
    const PredictChunk ch = A.chunks[c];
    block_sync();  // previous chunk done (and the row tile written)
    const int nn = (int)(ch.n1 - ch.n0), nl = (int)(ch.l1 - ch.l0);
    uint32_t* flags = (uint32_t*)(chunk + nn * 8);
    for (int i = tid; i < nn; i += kStThreads) ((PNode*)chunk)[i] = A.nodes[ch.n0 + i];
    if (present)
      for (int i = tid; i < nl; i += kStThreads) flags[i] = 0;
    block_sync();
    for (int t = ch.t0; t < ch.t1; t++) {
      const PNode* tn = (const PNode*)chunk + (A.tree_node[t] - ch.n0);
      PNode a0 = tn[0], a1 = tn[0];
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
      const uint32_t k0 = a0.a & 0x7fffffffu, k1 = a1.a & 0x7fffffffu;
      const int64_t o = (int64_t)t * A.N + row0 + tid;
      if (in0) idx[o] = (uint16_t)k0;
      if (in1) idx[o + kStThreads] = (uint16_t)k1;
      if (present) {  // (every writer stores the same word)
        const int lb = (int)(A.tree_leaf[t] - ch.l0);
        if (in0) flags[lb + (int)k0] = 1u;
        if (in1) flags[lb + (int)k1] = 1u;
      }
    }
    if (present) {
      block_sync();  // every walk of the chunk has set its flags
      for (int i = tid; i < nl; i += kStThreads)
        if (flags[i] && present[ch.l0 + i] == 0u) atomicOr(&present[ch.l0 + i], 1u);
    }
  }
}

void launch_stack_walk(hipStream_t st, const PredictArgs& a, uint16_t* idx, uint32_t* present) {
  PredictArgs b = a;
  b.agg = kAggMean;  // predict_tiled_lds: the row tile and the chunk only
  const size_t lds = predict_tiled_lds(b);
  const dim3 grid((unsigned)((a.N + kStRows - 1) / kStRows));
  stack_set_max_lds((const void*)k_stack_walk<uint8_t>, 160 * 1024);
  stack_set_max_lds((const void*)k_stack_walk<uint16_t>, 160 * 1024);
  if (a.code_bytes == 1)
    hipLaunchKernelGGL(k_stack_walk<uint8_t>, grid, dim3(kStThreads), lds, st, b, idx, present);
  else
    hipLaunchKernelGGL(k_stack_walk<uint16_t>, grid, dim3(kStThreads), lds, st, b, idx, present);
}

// One workgroup: rows [64 blockIdx.x, +64) x columns [128 blockIdx.y, +CW), CW = min(S, 128)
// (S <= 64, or a multiple of 128).  Lanes run over rows when idx is read (64 consecutive u16
// of one tree) and over the words of a row when the tile is written.
constexpr int kScRows = 64, kScCols = 128;
template <typename OT>
__global__ __launch_bounds__(256) void k_stack_codes(const uint16_t* __restrict__ idx, int64_t N, int32_t K,
                                                     int32_t S, const uint16_t* __restrict__ map,
                                                     const int32_t* __restrict__ map_off,
                                                     OT* __restrict__ out) {
  __shared__ __align__(16) uint32_t tile_w[kScRows * (kScCols * sizeof(OT) / 4 + 1)];
  const int tid = threadIdx.x;
  const int CW = S < kScCols ? S : kScCols;
  const int pw = CW * (int)sizeof(OT) / 4 + 1;  // tile pitch in words (odd: rows on distinct banks)
  const int64_t row0 = (int64_t)blockIdx.x * kScRows;
  const int c0 = blockIdx.y * kScCols;
  for (int q = tid; q < CW * kScRows; q += 256) {
    const int cc = q / kScRows, r = q - cc * kScRows;
    const int k = c0 + cc;
    uint32_t v = 0;
    if (k < K && row0 + r < N) v = map[map_off[k] + idx[(int64_t)k * N + row0 + r]];
    ((OT*)(tile_w + r * pw))[cc] = (OT)v;
  }
  block_sync();
  const int ww = CW * (int)sizeof(OT) / 4;  // words of a tile row
  for (int q = tid; q < kScRows * ww; q += 256) {
    const int r = q / ww, w = q - r * ww;
    if (row0 + r < N)
      *(uint32_t*)((unsigned char*)out + ((row0 + r) * S + c0) * (int64_t)sizeof(OT) + w * 4) = tile_w[r * pw + w];
  }
}

void launch_stack_codes(hipStream_t st, const uint16_t* idx, int64_t N, int32_t K, int32_t S,
                        const uint16_t* map, const int32_t* map_off, void* out, int code_bytes) {
  const dim3 grid((unsigned)((N + kScRows - 1) / kScRows), (unsigned)((S + kScCols - 1) / kScCols));
  if (code_bytes == 1)
    hipLaunchKernelGGL(k_stack_codes<uint8_t>, grid, dim3(256), 0, st, idx, N, K, S, map, map_off,
                       (uint8_t*)out);
  else
    hipLaunchKernelGGL(k_stack_codes<uint16_t>, grid, dim3(256), 0, st, idx, N, K, S, map, map_off,
                       (uint16_t*)out);
}

// ---- the fused two-level transform
size_t predict_stacked_lds(const StackArgs& a) {
  const size_t pitch = (size_t)a.S * a.code_bytes + 4;
  const size_t b = (size_t)kStRows * pitch + (size_t)a.nnodes * 8 + (size_t)a.nleaves * 8 + (size_t)a.nroot * 4;
  return (b + 15) & ~(size_t)15;
}

namespace {
// One walk: `cur` is the node the row stands on, in the stack tree or (inb) in the base tree
// that the stack node (left child sa, cut scut) tests.
struct StWalk {
  PNode cur;
  uint32_t sa, scut;
  bool inb;
  __device__ __forceinline__ bool done() const { return !inb && (cur.a & 0x80000000u); }
};
template <typename CT>
__device__ __forceinline__ void st_step(StWalk& w, const PNode* nd, const int32_t* root,
                                        const unsigned char* rp) {
  if (w.inb) {
    if (w.cur.a & 0x80000000u) {  // the base prediction's rank decides the stack node
      const uint32_t rank = w.cur.a & 0x7fffffffu;
      w.cur = nd[w.sa + (rank < w.scut ? 0u : 1u)];
      w.inb = false;
    } else {
      const uint32_t code = ((const CT*)rp)[w.cur.b >> 17];
      w.cur = nd[w.cur.a + (code < (w.cur.b & 0x1ffffu) ? 0u : 1u)];
    }
  } else {  // a stack node that tests a base tree: walk that tree first
    w.sa = w.cur.a;
    w.scut = w.cur.b & 0x1ffffu;
    w.cur = nd[root[w.cur.b >> 17]];
    w.inb = true;
  }
}
}  // namespace

// LDS: [512 rows x (S code bytes + 4)] [nodes] [stack leaf values fp64] [roots]
template <typename CT>
__global__ __launch_bounds__(kStThreads) void k_predict_stacked(StackArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int pitch = A.S * (int)sizeof(CT) + 4;
  unsigned char* rows = smem;
  PNode* nd = (PNode*)(smem + (size_t)kStRows * pitch);
  double* lv = (double*)(nd + A.nnodes);
  int32_t* root = (int32_t*)(lv + A.nleaves);
  const int64_t row0 = (int64_t)blockIdx.x * kStRows;
  stage_rows<CT>(rows, A.codes, A.S, A.N, row0, tid);
  for (int i = tid; i < A.nnodes; i += kStThreads) nd[i] = A.nodes[i];
  for (int i = tid; i < A.nleaves; i += kStThreads) lv[i] = A.leaves[i];
  for (int i = tid; i < A.nroot; i += kStThreads) root[i] = A.root[i];
  block_sync();  // the row tile and the trees are written
  const unsigned char* r0p = rows + tid * pitch;
  const unsigned char* r1p = rows + (tid + kStThreads) * pitch;
  StWalk w0, w1;
  w0.cur = nd[A.sroot];
  w0.sa = w0.scut = 0;
  w0.inb = false;
  w1 = w0;
  while (!(w0.done() && w1.done())) {
    if (!w0.done()) st_step<CT>(w0, nd, root, r0p);
    if (!w1.done()) st_step<CT>(w1, nd, root, r1p);
  }
  if (row0 + tid < A.N) A.out[row0 + tid] = lv[w0.cur.a & 0x7fffffffu];
  if (row0 + tid + kStThreads < A.N) A.out[row0 + tid + kStThreads] = lv[w1.cur.a & 0x7fffffffu];
}

void launch_predict_stacked(hipStream_t st, const StackArgs& a) {
  const size_t lds = predict_stacked_lds(a);
  const dim3 grid((unsigned)((a.N + kStRows - 1) / kStRows));
  stack_set_max_lds((const void*)k_predict_stacked<uint8_t>, 160 * 1024);
  stack_set_max_lds((const void*)k_predict_stacked<uint16_t>, 160 * 1024);
  if (a.code_bytes == 1)
    hipLaunchKernelGGL(k_predict_stacked<uint8_t>, grid, dim3(kStThreads), lds, st, a);
  else
    hipLaunchKernelGGL(k_predict_stacked<uint16_t>, grid, dim3(kStThreads), lds, st, a);
}

// ---- the general path
template <typename RT>
__global__ __launch_bounds__(256) void k_stack_top(const StackTopNode* __restrict__ nodes,
                                                   const double* __restrict__ leaves,
                                                   const RT* __restrict__ ranks, int64_t N,
                                                   double* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= N) return;
  StackTopNode n = nodes[0];
  while (!(n.a & 0x80000000u)) {
    const uint32_t rank = ranks[(int64_t)n.k * N + row];
    n = nodes[n.a + (rank < n.cut ? 0u : 1u)];
  }
  out[row] = leaves[n.a & 0x7fffffffu];
}

void launch_stack_top(hipStream_t st, const StackTopNode* nodes, const double* leaves, const void* ranks,
                      int rank_bytes, int64_t N, double* out) {
  const dim3 grid((unsigned)((N + 255) / 256));
  if (rank_bytes == 2)
    hipLaunchKernelGGL(k_stack_top<uint16_t>, grid, dim3(256), 0, st, nodes, leaves, (const uint16_t*)ranks,
                       N, out);
  else
    hipLaunchKernelGGL(k_stack_top<uint32_t>, grid, dim3(256), 0, st, nodes, leaves, (const uint32_t*)ranks,
                       N, out);
}

__global__ __launch_bounds__(256) void k_stack_rank_walk(const double* __restrict__ X,
                                                         const void* __restrict__ codes, int code_bytes,
                                                         const double* __restrict__ dict,
                                                         const int64_t* __restrict__ dict_off, int64_t N,
                                                         int32_t F, int32_t S,
                                                         const DevNode* __restrict__ nodes,
                                                         const int64_t* __restrict__ tree_off, int K,
                                                         const uint32_t* __restrict__ rank_tab,
                                                         const int64_t* __restrict__ leaf_off,
                                                         uint32_t* __restrict__ ranks) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= N) return;
  for (int l = 0; l < K; l++) {
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
    ranks[(int64_t)l * N + row] = rank_tab[leaf_off[l] + t[id].pad];
  }
}

void launch_stack_rank_walk(hipStream_t st, const double* X, const void* codes, int code_bytes,
                            const double* dict, const int64_t* dict_off, int64_t N, int32_t F, int32_t S,
                            const DevNode* nodes, const int64_t* tree_off, int K, const uint32_t* rank_tab,
                            const int64_t* leaf_off, uint32_t* ranks) {
  hipLaunchKernelGGL(k_stack_rank_walk, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, X, codes,
                     code_bytes, dict, dict_off, N, F, S, nodes, tree_off, K, rank_tab, leaf_off, ranks);
}

}  // namespace sbag
