// sbag_prox.hip — forest proximities for gfx950 (MI355X, CDNA4): in how many trees two rows
// reach the same leaf (include/sbag.h states the rule).
//
// Stage A turns a row into its signature: the leaf code of every tree (the number of leaves
// before the reached one in the tree's node array), u8 when no tree has more than 256 leaves,
// else u16, the trees' codes contiguous and zero padded to a multiple of 16 bytes.
//   k_leaf_tiled   k_quant_tiled's walk (rows staged in 16-byte pieces at pitch S * code_bytes
//                  + 4, forest chunks in LDS, thresholds in code space, two walk slots a thread)
//                  over a plan whose leaf nodes hold 0x80000000 | leaf code.  Slot (tree t, row
//                  r) stores its code into the tile's signatures in LDS ([R][tpad + 4] bytes,
//                  zeroed first, so the padding is zero); after the last chunk the tile leaves
//                  as one contiguous run of 16-byte stores.
//   k_leaf_walk    the general path: one thread per row over DevNodes in global memory, the same
//                  signatures (a leaf's DevNode.pad is its code).
//   k_leaf_ids     sbag_predict_leaves: code -> node id through the forest's table.
//   k_sig_gather   the moments' reference rows in group order.
//
// Stage B counts, for every (query, reference) pair, the codes that differ: a GEMM-shaped
// kernel whose inner product is a packed compare.
//   k_prox_tiled<ST, MOMENTS>
//     A block owns kProxBM x kProxBN pairs, its 256 threads as 16 x 16 (ty, tx), thread
//     (ty, tx) the 8 x 8 pairs of rows ty + 16 a and columns tx + 16 b.  Both signature tiles
//     are staged through LDS in K chunks of 128 bytes a row (a whole 128-tree u8 signature) at a
//     pitch of 144 bytes, read back with ds_read_b128: a wave's 64 lanes are 4 ty x 16 tx, so a
//     query read has 4 addresses (broadcast over tx) and a reference read 16 consecutive rows,
//     which at 36 dwords a row fall into 16 different groups of four banks.
//     Per 16 bytes of K a thread loads its 8 query quads, then for each of its 8 columns one
//     reference quad, and for each of the 64 pairs and 4 dwords: x = q ^ r, the non-zero codes
//     of x marked in their top bits by m = (((x & LO) + LO) | x) & HI (LO = 0x7f7f7f7f or
//     0x7fff7fff: the add cannot carry out of a code), diff += popcount(m).
//     Counts mode (one column block a block): cnt = trees - diff as u16 through LDS
//     ([kProxBM][kProxBN + 2], in the tiles' place) so that a wave stores 64 consecutive u16 of a
//     row.
//     Moments mode: the block walks a run of column blocks (the reference rows ordered by group,
//     no block spanning two groups; a block's tail masked by its column count).  A lane folds
//     cnt (u32) and cnt^2 (u64) over its 8 columns, the 16 tx lanes of a row fold by xor
//     shuffles, lane tx == 0 adds into the row's u64 pair in LDS, and at every change of group
//     the block adds the 128 pairs into out[row][group][2] with u64 atomics: integer sums, so
//     the order is irrelevant.  With one K chunk (tpad <= 128) the query tile is staged once.
//   k_prox_topk<ST>, k_topk_merge
//     Top-k mode: the same tile and compare; the k best reference rows of every query row are
//     kept in LDS over a run of column blocks and the runs' lists merged a wave a row (below).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

#include "sbag_internal.h"
#include "sbag_prox_plan.h"

namespace sbag {

namespace {

constexpr int kLtThreads = 256;
constexpr int kLtSlots = 512;  // walk slots of a step: two a thread

// (as sbag_spread.hip's: the dynamic-LDS cap of a kernel, once per (kernel, device))
void leaf_set_max_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> g(mu);
  if (done.count({fn, dev})) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess)
    done.insert({fn, dev});
}

// the non-zero codes of x, added to acc
template <typename ST>
__device__ __forceinline__ uint32_t add_nonzero_codes(uint32_t x, uint32_t acc) {
  constexpr uint32_t LO = sizeof(ST) == 1 ? 0x7f7f7f7fu : 0x7fff7fffu;
  const uint32_t m = (((x & LO) + LO) | x) & ~LO;
  return (uint32_t)__popc(m) + acc;
}

}  // namespace

// LDS: [R rows x (S code bytes + 4)] [chunk_bytes: packed nodes] [signatures [R][tpad + 4]].
// Walk slot s = tid, tid + 256: row s % R of the tile, tree lane s / R of the 512 / R trees of
// a step.  Slot (t, r) alone writes code t of row r.  A row past N walks nothing and is not
// written out.
template <typename CT, typename ST>
__global__ __launch_bounds__(kLtThreads) void k_leaf_tiled(PredictArgs A, LeafArgs Q) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int R = Q.R;
  const int pitch = A.S * (int)sizeof(CT) + 4;
  const int spitch = Q.tpad + 4;
  unsigned char* rows = smem;
  unsigned char* chunk = smem + (size_t)R * pitch;
  unsigned char* sig = chunk + A.chunk_bytes;
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int rb = A.S * (int)sizeof(CT);  // bytes of one row (S is a multiple of 16)
  const int vpr = rb >> 4;               // 16-byte pieces of one row
  for (int q = tid; q < R * vpr; q += kLtThreads) {
    const int r = q / vpr, w = q - r * vpr;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row0 + r < A.N) v = *(const uint4*)((const unsigned char*)A.codes + (row0 + r) * rb + w * 16);
    uint32_t* d = (uint32_t*)(rows + r * pitch + w * 16);
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
    d[3] = v.w;
  }
  for (int q = tid; q < R * (spitch >> 2); q += kLtThreads) ((uint32_t*)sig)[q] = 0u;
  const int G = kLtSlots / R;  // trees of a step
  const int r0 = tid & (R - 1), g0 = tid / R;
  const int r1 = (tid + kLtThreads) & (R - 1), g1 = (tid + kLtThreads) / R;
  const bool in0 = row0 + r0 < A.N, in1 = row0 + r1 < A.N;
  const unsigned char* r0p = rows + r0 * pitch;
  const unsigned char* r1p = rows + r1 * pitch;
  ST* s0p = (ST*)(sig + r0 * spitch);
  ST* s1p = (ST*)(sig + r1 * spitch);
  for (int c = 0; c < A.nchunks; c++) {
    const PredictChunk ch = A.chunks[c];
    block_sync();  // the tiles are written; the previous chunk is done
    for (int i = tid; i < (int)(ch.n1 - ch.n0); i += kLtThreads) ((PNode*)chunk)[i] = A.nodes[ch.n0 + i];
    block_sync();
    for (int tb = ch.t0; tb < ch.t1; tb += G) {
      const int t0 = tb + g0, t1 = tb + g1;
      const bool have0 = t0 < ch.t1, have1 = t1 < ch.t1;
      const PNode* tn0 = (const PNode*)chunk + (A.tree_node[have0 ? t0 : ch.t0] - ch.n0);
      const PNode* tn1 = (const PNode*)chunk + (A.tree_node[have1 ? t1 : ch.t0] - ch.n0);
      PNode a0 = tn0[0], a1 = tn1[0];
      if (!(have0 && in0)) a0.a = 0x80000000u;  // already at a leaf
      if (!(have1 && in1)) a1.a = 0x80000000u;
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
      if (have0) s0p[t0] = (ST)a0.a;
      if (have1) s1p[t1] = (ST)a1.a;
    }
  }
  block_sync();  // every code of the tile is stored
  const int tile_rows = (int)(A.N - row0 < R ? A.N - row0 : R);
  const int pieces = Q.tpad >> 4;
  for (int q = tid; q < tile_rows * pieces; q += kLtThreads) {
    const int r = q / pieces, w = q - r * pieces;
    const uint32_t* s = (const uint32_t*)(sig + r * spitch + w * 16);
    *(uint4*)(Q.sig + (row0 + r) * Q.tpad + w * 16) = make_uint4(s[0], s[1], s[2], s[3]);
  }
}

void launch_leaf_tiled(hipStream_t st, const PredictArgs& a, const LeafArgs& q) {
  const size_t pitch = (size_t)a.S * a.code_bytes + 4;
  const size_t lds = (size_t)q.R * pitch + (size_t)a.chunk_bytes + prox_sig_lds(q.tpad, q.R);
  const dim3 grid((unsigned)((a.N + q.R - 1) / q.R));
#define SBAG_LEAF_LAUNCH(CT, ST)                                                        \
  do {                                                                                  \
    leaf_set_max_lds((const void*)k_leaf_tiled<CT, ST>, 160 * 1024);                    \
    hipLaunchKernelGGL((k_leaf_tiled<CT, ST>), grid, dim3(kLtThreads), lds, st, a, q);  \
  } while (0)
  if (a.code_bytes == 1) {
    if (q.code_bytes == 1)
      SBAG_LEAF_LAUNCH(uint8_t, uint8_t);
    else
      SBAG_LEAF_LAUNCH(uint8_t, uint16_t);
  } else {
    if (q.code_bytes == 1)
      SBAG_LEAF_LAUNCH(uint16_t, uint8_t);
    else
      SBAG_LEAF_LAUNCH(uint16_t, uint16_t);
  }
#undef SBAG_LEAF_LAUNCH
}

// One thread per row of the batch: the row's whole signature, padding included.
template <typename ST>
__global__ __launch_bounds__(256) void k_leaf_walk(const double* __restrict__ X, const void* __restrict__ codes,
                                                   int code_bytes, const double* __restrict__ dict,
                                                   const int64_t* __restrict__ dict_off, int64_t n, int32_t F,
                                                   int32_t S, const DevNode* __restrict__ nodes,
                                                   const int64_t* __restrict__ tree_off, int L, LeafArgs Q) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  ST* out = (ST*)(Q.sig + row * Q.tpad);
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
    out[l] = (ST)t[id].pad;
  }
  for (int l = L; l < Q.tpad / (int)sizeof(ST); l++) out[l] = (ST)0;
}

void launch_leaf_walk(hipStream_t st, const double* X, const void* codes, int code_bytes, const double* dict,
                      const int64_t* dict_off, int64_t n, int32_t F, int32_t S, const DevNode* nodes,
                      const int64_t* tree_off, int L, const LeafArgs& q) {
  const dim3 grid((unsigned)((n + 255) / 256));
  if (q.code_bytes == 1)
    hipLaunchKernelGGL(k_leaf_walk<uint8_t>, grid, dim3(256), 0, st, X, codes, code_bytes, dict, dict_off, n, F,
                       S, nodes, tree_off, L, q);
  else
    hipLaunchKernelGGL(k_leaf_walk<uint16_t>, grid, dim3(256), 0, st, X, codes, code_bytes, dict, dict_off, n, F,
                       S, nodes, tree_off, L, q);
}

// out[row][t] = node_of[leaf_off[t] + code t of the row], one thread per (row, tree)
__global__ __launch_bounds__(256) void k_leaf_ids(LeafArgs Q, int64_t n, int L, const int32_t* __restrict__ node_of,
                                                  const int64_t* __restrict__ leaf_off, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * L) return;
  const int64_t row = i / L;
  const int t = (int)(i - row * L);
  const unsigned char* s = Q.sig + row * Q.tpad;
  const uint32_t code = Q.code_bytes == 1 ? (uint32_t)s[t] : (uint32_t)((const uint16_t*)s)[t];
  out[i] = node_of[leaf_off[t] + code];
}

void launch_leaf_ids(hipStream_t st, const LeafArgs& q, int64_t n, int L, const int32_t* node_of,
                     const int64_t* leaf_off, int32_t* out) {
  hipLaunchKernelGGL(k_leaf_ids, dim3((unsigned)((n * L + 255) / 256)), dim3(256), 0, st, q, n, L, node_of,
                     leaf_off, out);
}

// dst row p = src row perm[p], in 16-byte pieces
__global__ __launch_bounds__(256) void k_sig_gather(const unsigned char* __restrict__ src,
                                                    const int64_t* __restrict__ perm, int64_t n, int tpad,
                                                    unsigned char* __restrict__ dst) {
  const int pieces = tpad >> 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * pieces) return;
  const int64_t p = i / pieces;
  const int w = (int)(i - p * pieces);
  *(uint4*)(dst + p * tpad + w * 16) = *(const uint4*)(src + perm[p] * tpad + w * 16);
}

void launch_sig_gather(hipStream_t st, const unsigned char* src, const int64_t* perm, int64_t n, int tpad,
                       unsigned char* dst) {
  hipLaunchKernelGGL(k_sig_gather, dim3((unsigned)((n * (tpad >> 4) + 255) / 256)), dim3(256), 0, st, src, perm,
                     n, tpad, dst);
}

// rows [r0, r0 + nrows) of a signature matrix, K bytes [k0, k0 + 16 pieces): into a tile at
// kProxPitch; rows past `nrows` are zero
__device__ __forceinline__ void prox_stage(unsigned char* tile, const unsigned char* __restrict__ sig, int tpad,
                                           int64_t r0, int64_t nrows, int k0, int pieces, int tile_rows, int tid) {
  for (int q = tid; q < tile_rows * pieces; q += kProxThreads) {
    const int r = q / pieces, w = q - r * pieces;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (r < nrows) v = *(const uint4*)(sig + (r0 + r) * tpad + k0 + w * 16);
    *(uint4*)(tile + r * kProxPitch + w * 16) = v;
  }
}

// grid.x: counts: the column blocks; moments: the runs of column blocks.  grid.y: the row blocks.
template <typename ST, bool MOMENTS>
__global__ __launch_bounds__(kProxThreads) void k_prox_tiled(ProxArgs P) {
  __shared__ __align__(16) unsigned char lds[kProxTileLds];
  __shared__ unsigned long long sums[MOMENTS ? kProxBM * 2 : 2];
  unsigned char* qt = lds;
  unsigned char* rt = lds + kProxBM * kProxPitch;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t row0 = (int64_t)blockIdx.y * kProxBM;
  const int64_t qrows = P.nq - row0 < kProxBM ? P.nq - row0 : kProxBM;
  const int nk = (P.tpad + kProxKC - 1) / kProxKC;
  int cb0 = (int)blockIdx.x, cb1 = cb0 + 1;
  if (MOMENTS) {
    cb0 = (int)blockIdx.x * P.run;
    cb1 = cb0 + P.run < P.nblocks ? cb0 + P.run : P.nblocks;
    for (int i = tid; i < kProxBM * 2; i += kProxThreads) sums[i] = 0ull;
  }
  int group = -1;
  for (int cb = cb0; cb < cb1; cb++) {
    int64_t col0 = (int64_t)cb * kProxBN;
    int ncols = (int)(P.nr - col0 < kProxBN ? P.nr - col0 : kProxBN);
    if (MOMENTS) {
      const ProxColBlock b = P.blocks[cb];
      col0 = b.col0;
      ncols = b.ncols;
      if (b.group != group && group >= 0) {  // the finished group's sums leave the block
        block_sync();
        for (int i = tid; i < (int)qrows * 2; i += kProxThreads) {
          atomicAdd(P.moments + ((row0 + (i >> 1)) * P.G + group) * 2 + (i & 1), sums[i]);
          sums[i] = 0ull;
        }
      }
      group = b.group;
    }
    uint32_t diff[kProxTM][kProxTN];
#pragma unroll
    for (int a = 0; a < kProxTM; a++)
#pragma unroll
      for (int b = 0; b < kProxTN; b++) diff[a][b] = 0u;
    for (int kc = 0; kc < nk; kc++) {
      const int k0 = kc * kProxKC;
      const int pieces = (P.tpad - k0 < kProxKC ? P.tpad - k0 : kProxKC) >> 4;
      block_sync();  // the previous chunk's reads (and the sums' updates) are done
      if (nk > 1 || cb == cb0) prox_stage(qt, P.sigq, P.tpad, row0, qrows, k0, pieces, kProxBM, tid);
      prox_stage(rt, P.sigr, P.tpad, col0, ncols, k0, pieces, kProxBN, tid);
      block_sync();
      for (int w = 0; w < pieces; w++) {
        uint4 qv[kProxTM];
#pragma unroll
        for (int a = 0; a < kProxTM; a++) qv[a] = *(const uint4*)(qt + (ty + 16 * a) * kProxPitch + w * 16);
#pragma unroll
        for (int b = 0; b < kProxTN; b++) {
          const uint4 rv = *(const uint4*)(rt + (tx + 16 * b) * kProxPitch + w * 16);
#pragma unroll
          for (int a = 0; a < kProxTM; a++) {
            uint32_t d = diff[a][b];
            d = add_nonzero_codes<ST>(qv[a].x ^ rv.x, d);
            d = add_nonzero_codes<ST>(qv[a].y ^ rv.y, d);
            d = add_nonzero_codes<ST>(qv[a].z ^ rv.z, d);
            d = add_nonzero_codes<ST>(qv[a].w ^ rv.w, d);
            diff[a][b] = d;
          }
        }
      }
    }
    if (MOMENTS) {
#pragma unroll
      for (int a = 0; a < kProxTM; a++) {
        uint32_t s1 = 0u;
        unsigned long long s2 = 0ull;
#pragma unroll
        for (int b = 0; b < kProxTN; b++) {
          const uint32_t cnt = tx + 16 * b < ncols ? (uint32_t)P.L - diff[a][b] : 0u;
          s1 += cnt;
          s2 += (unsigned long long)cnt * cnt;
        }
#pragma unroll
        for (int h = 8; h >= 1; h >>= 1) {  // the 16 tx lanes of the row are 16 consecutive lanes
          s1 += __shfl_xor(s1, h, 64);
          s2 += __shfl_xor(s2, h, 64);
        }
        if (tx == 0) {  // row ty + 16 a belongs to this lane alone
          sums[(ty + 16 * a) * 2] += s1;
          sums[(ty + 16 * a) * 2 + 1] += s2;
        }
      }
    } else {
      uint16_t* ct = (uint16_t*)lds;  // [kProxBM][kProxBN + 2]
      block_sync();                   // the tiles have been read
#pragma unroll
      for (int a = 0; a < kProxTM; a++)
#pragma unroll
        for (int b = 0; b < kProxTN; b++)
          ct[(ty + 16 * a) * (kProxBN + 2) + tx + 16 * b] = (uint16_t)((uint32_t)P.L - diff[a][b]);
      block_sync();
      for (int i = tid; i < kProxBM * kProxBN; i += kProxThreads) {
        const int r = i / kProxBN, cidx = i - r * kProxBN;
        if (r < qrows && cidx < ncols) P.counts[(row0 + r) * P.nr + col0 + cidx] = ct[r * (kProxBN + 2) + cidx];
      }
    }
  }
  if (MOMENTS && group >= 0) {
    block_sync();
    for (int i = tid; i < (int)qrows * 2; i += kProxThreads)
      atomicAdd(P.moments + ((row0 + (i >> 1)) * P.G + group) * 2 + (i & 1), sums[i]);
  }
}

void launch_prox_tiled(hipStream_t st, const ProxArgs& p) {
  const bool moments = p.moments != nullptr;
  const unsigned nx = moments ? (unsigned)((p.nblocks + p.run - 1) / p.run)
                              : (unsigned)((p.nr + kProxBN - 1) / kProxBN);
  const dim3 grid(nx, (unsigned)((p.nq + kProxBM - 1) / kProxBM));
  if (p.code_bytes == 1) {
    if (moments)
      hipLaunchKernelGGL((k_prox_tiled<uint8_t, true>), grid, dim3(kProxThreads), 0, st, p);
    else
      hipLaunchKernelGGL((k_prox_tiled<uint8_t, false>), grid, dim3(kProxThreads), 0, st, p);
  } else {
    if (moments)
      hipLaunchKernelGGL((k_prox_tiled<uint16_t, true>), grid, dim3(kProxThreads), 0, st, p);
    else
      hipLaunchKernelGGL((k_prox_tiled<uint16_t, false>), grid, dim3(kProxThreads), 0, st, p);
  }
}

// ---- top-k mode: the k best reference rows of every query row, selected while the block sweeps
// its run of column blocks.  Row ty + 16 a of a tile is held by the 16 lanes of one ty, which lie
// in one wave (ty >> 2): a row's list, staging area, fill count and bound are touched by that
// wave alone, so the selection needs no barrier of the block, only the order in which one wave
// issues its LDS operations.
//   bound    dthr[row]: a pair passes iff diff < dthr.  L + 1 while the list has an empty place,
//            then L - (the smallest count of the list): a pair that ties the list's last count
//            comes from a later column, so it loses (sbag_prox_plan.h: the key).  0 for a row
//            past the queries.  The bound only rises between merges, so a stale one lets too
//            many through, never too few.
//   filter   a lane takes the minimum of its 8 differences of a row (v_min3) and compares it
//            with the bound: 8 broadcast LDS reads and fewer than 100 VALU operations a tile
//            beside the 11 264 of the compare loop.  Only when some lane of the wave passes does the wave
//            enter topk_collect.
//   collect  every passing pair that is a real column (not the tail of the last block, not the
//            row's own column) takes a place of the row's staging area through an LDS atomic on
//            its fill count.  A pair that finds the area full stays pending; the wave merges its
//            full rows, which raises their bounds, and the pending pairs try again: nothing is
//            dropped, and every round places at least one key of every row that still has any.
//   merge    by rank, no network: the list is sorted, the keys are distinct, so a key's place in
//            the union is its own index plus the number of larger keys on the other side
//            (counted with broadcast reads over the staging area, by bisection over the list).
//            Every lane holds one list entry and one staged key, and the k largest go back
//            sorted.  A row merges when its area is full and at the end of the run, not after
//            every tile: the bound is then a little stale, and a row merges once per 16
//            survivors instead of once per tile.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A: k keys, descending, the empty places (0) last.  B: nb <= 64 keys in any order, 0 = none.
// Both in LDS and the calling wave's own.  The k largest of their union go into A, descending.
__device__ __forceinline__ void topk_rank_merge(unsigned long long* A, int k, const unsigned long long* B, int nb,
                                                int lane) {
  const bool ina = lane < k, inb = lane < nb;
  const unsigned long long a = ina ? A[lane] : 0ull, b = inb ? B[lane] : 0ull;
  int ra = lane, rb = 0;  // an empty place of A goes behind every key of B and stays behind its own
  for (int x = 0; x < nb; x++) {
    const unsigned long long v = B[x];
    ra += v > a ? 1 : 0;
    rb += v > b ? 1 : 0;
  }
  int lo = 0, hi = inb && b != 0ull ? k : 0;  // the entries of A above b
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (A[mid] > b)
      lo = mid + 1;
    else
      hi = mid;
  }
  rb += lo;
  wave_lds_order();  // every lane has read A and B
  if (ina && ra < k) A[ra] = a;
  if (inb && b != 0ull && rb < k) A[rb] = b;
  wave_lds_order();
}

struct TopkLds {
  unsigned long long* list;   // [kProxBM][k]
  unsigned long long* stage;  // [kProxBM][kTopkStage]
  uint32_t* nstage;           // [kProxBM] keys asked for a place since the row's last merge
  uint32_t* dthr;             // [kProxBM]
};

// the staged keys of one row into its list; the whole wave
__device__ __forceinline__ void topk_flush(const TopkLds& S, int row, int k, uint32_t L, int lane) {
  const uint32_t asked = S.nstage[row];
  const int nb = asked < (uint32_t)kTopkStage ? (int)asked : kTopkStage;
  topk_rank_merge(S.list + row * k, k, S.stage + row * kTopkStage, nb, lane);
  if (lane == 0) {
    const unsigned long long last = S.list[row * k + k - 1];
    S.nstage[row] = 0u;
    S.dthr[row] = last ? L - (uint32_t)(last >> 32) : L + 1u;
  }
  wave_lds_order();
}

// the rows of wave w: ty = 4 w + (lr & 3), a = lr >> 2
__device__ __forceinline__ int topk_wave_row(int w, int lr) { return 4 * w + (lr & 3) + 16 * (lr >> 2); }

// the wave's rows whose staging area holds at least `least` keys go into their lists
__device__ __forceinline__ void topk_flush_rows(const TopkLds& S, int w, uint32_t least, int k, uint32_t L, int lane) {
  unsigned long long due = __ballot(lane < 32 && S.nstage[topk_wave_row(w, lane & 31)] >= least);
  while (due) {
    const int lr = __ffsll((long long)due) - 1;
    due &= due - 1;
    topk_flush(S, topk_wave_row(w, lr), k, L, lane);
  }
}

// the passing pairs of one tile into the staging areas of the wave's rows; the whole wave
__device__ __forceinline__ void topk_collect(const TopkLds& S, const uint32_t (&diff)[kProxTM][kProxTN], int tx, int ty,
                                             int64_t col0, int ncols, int64_t self0, int k, uint32_t L, int lane) {
  unsigned long long pend = 0ull;  // bit 8 a + b: pair (a, b) still wants a place
#pragma unroll
  for (int a = 0; a < kProxTM; a++)
#pragma unroll
    for (int b = 0; b < kProxTN; b++) {
      const int row = ty + 16 * a, col = tx + 16 * b;
      if (diff[a][b] < S.dthr[row] && col < ncols && col0 + col != self0 + row) pend |= 1ull << (8 * a + b);
    }
  while (__any(pend != 0ull)) {
#pragma unroll
    for (int a = 0; a < kProxTM; a++)
#pragma unroll
      for (int b = 0; b < kProxTN; b++) {
        const unsigned long long bit = 1ull << (8 * a + b);
        if (pend & bit) {
          const int row = ty + 16 * a;
          if (diff[a][b] >= S.dthr[row]) {  // a merge has raised the bound since
            pend &= ~bit;
          } else {
            const uint32_t slot = atomicAdd(&S.nstage[row], 1u);
            if (slot < (uint32_t)kTopkStage) {
              const uint32_t j = (uint32_t)(col0 + tx + 16 * b);
              S.stage[row * kTopkStage + slot] = ((unsigned long long)(L - diff[a][b]) << 32) | (uint32_t)~j;
              pend &= ~bit;
            }
          }
        }
      }
    wave_lds_order();
    topk_flush_rows(S, ty >> 2, (uint32_t)kTopkStage, k, L, lane);
  }
}

// grid.x: the runs of column blocks; grid.y: the row blocks.  Dynamic LDS: prox_topk_lds(k).
// The LDS admits two blocks a CU at most (sbag_prox_plan.h), two waves a SIMD, so the kernel
// may take 256 registers a lane and is asked not to take more.
template <typename ST>
__global__ __launch_bounds__(kProxThreads, 2) void k_prox_topk(ProxArgs P, TopkArgs T) {
  __shared__ __align__(16) unsigned char lds[kProxTileLds];
  extern __shared__ __align__(16) unsigned char topk_lds[];
  unsigned char* qt = lds;
  unsigned char* rt = lds + kProxBM * kProxPitch;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, w = tid >> 6;
  const int k = T.k;
  const uint32_t L = (uint32_t)P.L;
  TopkLds S;
  S.list = (unsigned long long*)topk_lds;
  S.stage = S.list + kProxBM * k;
  S.nstage = (uint32_t*)(S.stage + kProxBM * kTopkStage);
  S.dthr = S.nstage + kProxBM;
  const int64_t row0 = (int64_t)blockIdx.y * kProxBM;
  const int64_t qrows = P.nq - row0 < kProxBM ? P.nq - row0 : kProxBM;
  const int nk = (P.tpad + kProxKC - 1) / kProxKC;
  const int cb0 = (int)blockIdx.x * P.run;
  const int cb1 = cb0 + P.run < P.nblocks ? cb0 + P.run : P.nblocks;
  for (int i = lane; i < 32 * k; i += 64) {  // the wave's own 32 rows
    const int lr = i / k;
    S.list[topk_wave_row(w, lr) * k + (i - lr * k)] = 0ull;
  }
  if (lane < 32) {
    const int row = topk_wave_row(w, lane);
    S.nstage[row] = 0u;
    S.dthr[row] = row < qrows ? L + 1u : 0u;
  }
  wave_lds_order();
  for (int cb = cb0; cb < cb1; cb++) {
    const int64_t col0 = (int64_t)cb * kProxBN;
    const int ncols = (int)(P.nr - col0 < kProxBN ? P.nr - col0 : kProxBN);
    uint32_t diff[kProxTM][kProxTN];
#pragma unroll
    for (int a = 0; a < kProxTM; a++)
#pragma unroll
      for (int b = 0; b < kProxTN; b++) diff[a][b] = 0u;
    for (int kc = 0; kc < nk; kc++) {
      const int k0 = kc * kProxKC;
      const int pieces = (P.tpad - k0 < kProxKC ? P.tpad - k0 : kProxKC) >> 4;
      block_sync();  // the previous chunk's reads are done
      if (nk > 1 || cb == cb0) prox_stage(qt, P.sigq, P.tpad, row0, qrows, k0, pieces, kProxBM, tid);
      prox_stage(rt, P.sigr, P.tpad, col0, ncols, k0, pieces, kProxBN, tid);
      block_sync();
      for (int p = 0; p < pieces; p++) {
        uint4 qv[kProxTM];
#pragma unroll
        for (int a = 0; a < kProxTM; a++) qv[a] = *(const uint4*)(qt + (ty + 16 * a) * kProxPitch + p * 16);
#pragma unroll
        for (int b = 0; b < kProxTN; b++) {
          const uint4 rv = *(const uint4*)(rt + (tx + 16 * b) * kProxPitch + p * 16);
#pragma unroll
          for (int a = 0; a < kProxTM; a++) {
            uint32_t d = diff[a][b];
            d = add_nonzero_codes<ST>(qv[a].x ^ rv.x, d);
            d = add_nonzero_codes<ST>(qv[a].y ^ rv.y, d);
            d = add_nonzero_codes<ST>(qv[a].z ^ rv.z, d);
            d = add_nonzero_codes<ST>(qv[a].w ^ rv.w, d);
            diff[a][b] = d;
          }
        }
      }
    }
    bool pass = false;
#pragma unroll
    for (int a = 0; a < kProxTM; a++) {
      uint32_t m = diff[a][0];
#pragma unroll
      for (int b = 1; b < kProxTN; b++) m = m < diff[a][b] ? m : diff[a][b];
      pass |= m < S.dthr[ty + 16 * a];
    }
    if (__any(pass)) topk_collect(S, diff, tx, ty, col0, ncols, T.self_base + row0, k, L, lane);
  }
  topk_flush_rows(S, w, 1u, k, L, lane);
  unsigned long long* out = T.part + (row0 * T.nruns + blockIdx.x) * k;
  for (int i = lane; i < 32 * k; i += 64) {
    const int lr = i / k, e = i - lr * k, row = topk_wave_row(w, lr);
    if (row < qrows) out[(int64_t)row * T.nruns * k + e] = S.list[row * k + e];
  }
}

// a wave a row: the row's nruns lists (each descending) into one, and keys into (index, count)
__global__ __launch_bounds__(256) void k_topk_merge(TopkArgs T, int64_t nq) {
  __shared__ unsigned long long buf[4][2][kTopkMaxK];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + w;
  if (row >= nq) return;  // the whole wave
  const int k = T.k;
  unsigned long long* A = buf[w][0];
  unsigned long long* B = buf[w][1];
  const unsigned long long* p = T.part + row * T.nruns * k;
  if (lane < k) A[lane] = p[lane];
  for (int r = 1; r < T.nruns; r++) {
    if (lane < k) B[lane] = p[(int64_t)r * k + lane];
    wave_lds_order();
    topk_rank_merge(A, k, B, k, lane);
  }
  wave_lds_order();
  if (lane < k) {
    const unsigned long long key = A[lane];
    T.idx[row * k + lane] = key ? (int32_t)~(uint32_t)key : -1;
    T.cnt[row * k + lane] = (uint16_t)(key >> 32);
  }
}

void launch_prox_topk(hipStream_t st, const ProxArgs& p, const TopkArgs& t) {
  const dim3 grid((unsigned)t.nruns, (unsigned)((p.nq + kProxBM - 1) / kProxBM));
  const size_t lds = prox_topk_lds(t.k);
  if (p.code_bytes == 1) {
    leaf_set_max_lds((const void*)k_prox_topk<uint8_t>, (int)prox_topk_lds(kTopkMaxK));
    hipLaunchKernelGGL((k_prox_topk<uint8_t>), grid, dim3(kProxThreads), lds, st, p, t);
  } else {
    leaf_set_max_lds((const void*)k_prox_topk<uint16_t>, (int)prox_topk_lds(kTopkMaxK));
    hipLaunchKernelGGL((k_prox_topk<uint16_t>), grid, dim3(kProxThreads), lds, st, p, t);
  }
  hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)((p.nq + 3) / 4)), dim3(256), 0, st, t, p.nq);
}

}  // namespace sbag
