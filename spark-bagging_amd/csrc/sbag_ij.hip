// sbag_ij.hip — the infinitesimal-jackknife variance of a bagged prediction for gfx950 (MI355X,
// CDNA4): Efron (2014), Wager, Hastie & Efron (2014).
//
// With c[b][i] the bag count of training row i in learner b, t_b(x) tree b's prediction,
// m their mean, d_b = t_b - m and T trees,
//
//   V_IJ(x) = (1 / T^2) sum_i ( sum_b c[b][i] d_b )^2 = (1 / T^2) d' G d,   G = C C'
//
// (sum_b d_b = 0, so centring the counts changes nothing).  G is T x T exact integers and does
// not depend on x: it is contracted once per model, and every row then costs T^2 / 2 fp64
// multiply-adds in the pass that walks its trees (sbag.h states the order of every operation).
//
//   k_gram_mfma  G by v_mfma_i32_32x32x32_i8.  A workgroup (8 waves) takes a slice of at most
//                65 536 rows (127 * 127 * 65 536 < 2^31: int32 accumulators are exact) and the
//                32 x 32 learner-tile pairs of one unit of sbag_ij_plan.h, at most 5 a wave.  The
//                slice's counts go through LDS a 256-row chunk at a time (pitch 272 bytes, the next
//                chunk prefetched into registers during the MFMAs); both operands of a pair are
//                read from that one tile, tile x by row for A and tile y by row for B (B is C'),
//                so the fragment addressing is the same and only the tile differs.  Rows of any
//                alignment: a 16-byte piece is five aligned words funnel-shifted, its bytes past
//                the slice masked.  The exact partials are added to the int64 T x T buffer with
//                vector atomics, lower triangle only.  A byte >= 128 (not an int8) raises a flag
//                with a plain vector store and the host runs k_gram_dot instead.
//   k_gram_dot   the same staging, slices of 32 768 rows (255 * 255 * 32 768 < 2^31), a lane 16
//                entries of a pair by unsigned packed-byte dot products: any byte.
//   k_ij_tiled   k_quant_tiled's geometry (rows staged at pitch S * code_bytes + 4, forest chunks
//                in LDS, two walk slots a thread) at R = 256, 128, 64 or 32 rows.  The walk stores
//                t_b at M[b][r], fp64 [T][R] in LDS, a wave's lanes on consecutive rows.  Then
//                thread r owns row r: the mean, d_b in place, and the chain c.  The chains s_a
//                are independent: a unit is (64 rows, 4 consecutive a), a lane a row, its four
//                sums in registers so one LDS read of d_b feeds four multiply-adds, G[a][b] read
//                through wave-uniform loads from the fp64 copy of G in global memory.  Units go
//                in passes of one a wave, a descending, so that d_a * u_a can overwrite M[a][r]
//                after the pass's barrier (no later unit reads that slot), and thread r runs the
//                q chain in order.  Every chain keeps its own order: the split changes no bit.
//   k_ij_form    the general path: one thread per row over per-tree predictions [T][n] in global
//                memory (the per-tree predict path wrote them), the same rule, the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

#include "sbag_ij_plan.h"
#include "sbag_internal.h"

namespace sbag {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

typedef __attribute__((address_space(4))) double ConstF64;

constexpr int kIjThreads = 256;
constexpr int kIjSlots = 512;  // walk slots of a step: two a thread

// (as sbag_spread.hip's: the dynamic-LDS cap of a kernel, once per (kernel, device))
void ij_set_max_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> g(mu);
  if (done.count({fn, dev})) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess)
    done.insert({fn, dev});
}

// bytes [off, off + 16) of `base` (4-byte aligned, readable 20 bytes past off), the bytes from
// `valid` on zeroed
__device__ __forceinline__ uint4 gram_load16(const uint8_t* __restrict__ base, int64_t off, int valid) {
  const uint32_t* p = (const uint32_t*)(base + (off & ~(int64_t)3));
  const uint32_t sh = (uint32_t)(off & 3);
  const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3], w4 = p[4];
  uint32_t v[4];
  v[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
  v[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
  v[2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
  v[3] = __builtin_amdgcn_alignbyte(w4, w3, sh);
  if (valid < 16) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int nb = valid - 4 * j;
      v[j] = nb >= 4 ? v[j] : nb <= 0 ? 0u : v[j] & ((1u << (8 * nb)) - 1u);
    }
  }
  return make_uint4(v[0], v[1], v[2], v[3]);
}

// The workgroup of both Gram kernels.  LDS: two buffers of [256 learner rows][kGramPitch].
// Piece group i of a chunk is LDS tile i: thread tid loads the 16 bytes of learner row
// 32 i + (tid >> 4), rows 16 (tid & 15) of the chunk; learners past T and rows past the slice are 0.
template <bool DOT>
__device__ __forceinline__ void gram_body(const uint8_t* __restrict__ counts, int T, int64_t N,
                                          unsigned long long* __restrict__ gram, int* __restrict__ flag) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int64_t kSlice = DOT ? kGramSliceDot : kGramSliceMfma;
  constexpr int kBuf = kGramLdsRows * kGramPitch;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nunits = gram_units(T);
  const int unit = (int)(blockIdx.x % (unsigned)nunits);
  const int64_t slice = blockIdx.x / (unsigned)nunits;
  int I, J;
  gram_unit(unit, I, J);
  const int ntl = I == J ? gram_block_tiles(T, I) : 8;  // LDS tiles staged
  const int npairs = gram_unit_pairs(T, I, J);
  const int64_t n0 = slice * kSlice;
  const int64_t n1 = n0 + kSlice < N ? n0 + kSlice : N;
  int px[kGramPairs], py[kGramPairs];
#pragma unroll
  for (int p = 0; p < kGramPairs; p++) {
    const int k = wave + kGramWaves * p;
    px[p] = py[p] = 0;
    if (k < npairs) gram_pair(I, J, k, px[p], py[p]);
  }
  const int b = lane & 31, h = lane >> 5;
  uint4 ra[8];
  uint32_t bad = 0;
  auto prefetch = [&](int64_t c0) {
    const int64_t row = c0 + 16 * (tid & 15);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      ra[i] = make_uint4(0u, 0u, 0u, 0u);
      if (i < ntl) {
        const int learner = gram_tile_learner(T, I, J, i) + (tid >> 4);
        if (learner < T && row < n1) {
          const int64_t left = n1 - row;
          ra[i] = gram_load16(counts, (int64_t)learner * N + row, left < 16 ? (int)left : 16);
          bad |= (ra[i].x | ra[i].y | ra[i].z | ra[i].w) & 0x80808080u;
        }
      }
    }
  };
  auto commit = [&](int buf) {
    unsigned char* d = smem + buf * kBuf;
#pragma unroll
    for (int i = 0; i < 8; i++)
      if (i < ntl) *(uint4*)(d + (32 * i + (tid >> 4)) * kGramPitch + 16 * (tid & 15)) = ra[i];
  };
  v16i acc[kGramPairs];
#pragma unroll
  for (int p = 0; p < kGramPairs; p++) acc[p] = v16i{};
  int buf = 0;
  prefetch(n0);
  commit(0);
  block_sync();
  for (int64_t c0 = n0; c0 < n1; c0 += kGramChunk) {
    const bool more = c0 + kGramChunk < n1;
    if (more) prefetch(c0 + kGramChunk);
    const unsigned char* cA = smem + buf * kBuf;
    if constexpr (!DOT) {
      // A: row b of tile x, B: column b of C' = row b of tile y; 16 rows of the chunk a lane half
#pragma unroll 2
      for (int ks = 0; ks < kGramChunk; ks += 32) {
#pragma unroll
        for (int p = 0; p < kGramPairs; p++)
          if (wave + kGramWaves * p < npairs) {
            const uint4 a4 = *(const uint4*)(cA + (px[p] * 32 + b) * kGramPitch + ks + 16 * h);
            const uint4 b4 = *(const uint4*)(cA + (py[p] * 32 + b) * kGramPitch + ks + 16 * h);
            acc[p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4i{(int)a4.x, (int)a4.y, (int)a4.z, (int)a4.w},
                                                           v4i{(int)b4.x, (int)b4.y, (int)b4.z, (int)b4.w},
                                                           acc[p], 0, 0, 0);
          }
      }
    } else {
      // lane (b, h): learner b of tile y against learners 16 h .. 16 h + 15 of tile x
      for (int ks = 0; ks < kGramChunk; ks += 16) {
#pragma unroll
        for (int p = 0; p < kGramPairs; p++)
          if (wave + kGramWaves * p < npairs) {
            const uint4 y4 = *(const uint4*)(cA + (py[p] * 32 + b) * kGramPitch + ks);
#pragma unroll
            for (int i = 0; i < 16; i++) {
              const uint4 x4 = *(const uint4*)(cA + (px[p] * 32 + 16 * h + i) * kGramPitch + ks);
              uint32_t s = (uint32_t)acc[p][i];
              s = __builtin_amdgcn_udot4(x4.x, y4.x, s, false);
              s = __builtin_amdgcn_udot4(x4.y, y4.y, s, false);
              s = __builtin_amdgcn_udot4(x4.z, y4.z, s, false);
              s = __builtin_amdgcn_udot4(x4.w, y4.w, s, false);
              acc[p][i] = (int)s;
            }
          }
      }
    }
    if (more) commit(buf ^ 1);
    block_sync();  // the next chunk is in LDS; this one may be overwritten
    buf ^= 1;
  }
  if (!DOT && bad) *flag = 1;  // (a vector store: the lanes that saw such a byte)
  // MFMA D: column = lane & 31 (tile y), row = (reg & 3) + 8 (reg >> 2) + 4 h (tile x)
#pragma unroll
  for (int p = 0; p < kGramPairs; p++) {
    if (wave + kGramWaves * p >= npairs) continue;
    const int la0 = gram_tile_learner(T, I, J, px[p]), lb = gram_tile_learner(T, I, J, py[p]) + b;
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int la = la0 + (DOT ? 16 * h + reg : (reg & 3) + 8 * (reg >> 2) + 4 * h);
      const int64_t v = DOT ? (int64_t)(uint32_t)acc[p][reg] : (int64_t)acc[p][reg];
      if (la < T && lb <= la && v != 0) atomicAdd(&gram[(int64_t)la * T + lb], (unsigned long long)v);
    }
  }
}

}  // namespace

__global__ __launch_bounds__(kGramWaves * 64, 1) void k_gram_mfma(const uint8_t* __restrict__ counts, int T,
                                                                  int64_t N, unsigned long long* __restrict__ gram,
                                                                  int* __restrict__ flag) {
  gram_body<false>(counts, T, N, gram, flag);
}

__global__ __launch_bounds__(kGramWaves * 64, 1) void k_gram_dot(const uint8_t* __restrict__ counts, int T,
                                                                 int64_t N, unsigned long long* __restrict__ gram,
                                                                 int* __restrict__ flag) {
  gram_body<true>(counts, T, N, gram, flag);
}

// gram [T][T] (zeroed by the caller) += the lower triangle of counts counts'; `dot`: k_gram_dot.
// counts is readable 32 bytes past its end.
void launch_gram(hipStream_t st, const uint8_t* counts, int T, int64_t N, unsigned long long* gram, int* flag,
                 bool dot) {
  if (N <= 0 || T <= 0) return;
  const int64_t slice = dot ? kGramSliceDot : kGramSliceMfma;
  const dim3 grid((unsigned)((N + slice - 1) / slice * gram_units(T)));
  const size_t lds = (size_t)2 * kGramLdsRows * kGramPitch;
  if (dot) {
    ij_set_max_lds((const void*)k_gram_dot, 160 * 1024);
    hipLaunchKernelGGL(k_gram_dot, grid, dim3(kGramWaves * 64), lds, st, counts, T, N, gram, flag);
  } else {
    ij_set_max_lds((const void*)k_gram_mfma, 160 * 1024);
    hipLaunchKernelGGL(k_gram_mfma, grid, dim3(kGramWaves * 64), lds, st, counts, T, N, gram, flag);
  }
}

// sbag.h's rule from the mean on, for one row whose d_b the caller reads through d(b):
// every operation rounded on its own
namespace {
__device__ __forceinline__ void ij_finish(double q, double c, double m, const IjArgs& Q, double* o) {
  const double v = q / Q.tt;
  o[0] = m;
  o[1] = v;
  o[2] = __dsub_rn(v, __dmul_rn(Q.w, c) / Q.tt);
}
}  // namespace

// LDS: [R rows x (S code bytes + 4)] [chunk_bytes: packed nodes, leaf values] [M fp64 [T][R]].
// Walk slot s = tid, tid + 256: row s % R of the tile, tree lane s / R of the 512 / R trees of a
// step; slot (t, r) alone writes M[t][r] (0.0 for a row past N).
template <typename CT>
__global__ __launch_bounds__(kIjThreads) void k_ij_tiled(PredictArgs A, IjArgs Q) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int R = Q.R, T = A.L;
  const int pitch = A.S * (int)sizeof(CT) + 4;
  unsigned char* rows = smem;
  unsigned char* chunk = smem + (size_t)R * pitch;
  double* M = (double*)(chunk + A.chunk_bytes);  // [T][R]
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int rb = A.S * (int)sizeof(CT);  // bytes of one row (S is a multiple of 16)
  const int vpr = rb >> 4;
  for (int q = tid; q < R * vpr; q += kIjThreads) {
    const int r = q / vpr, w = q - r * vpr;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row0 + r < A.N) v = *(const uint4*)((const unsigned char*)A.codes + (row0 + r) * rb + w * 16);
    uint32_t* d = (uint32_t*)(rows + r * pitch + w * 16);
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
    d[3] = v.w;
  }
  const int G = kIjSlots / R;  // trees of a step (2 .. 16)
  const int r0 = tid & (R - 1), g0 = tid / R;
  const int r1 = (tid + kIjThreads) & (R - 1), g1 = (tid + kIjThreads) / R;
  const bool in0 = row0 + r0 < A.N, in1 = row0 + r1 < A.N;
  const unsigned char* r0p = rows + r0 * pitch;
  const unsigned char* r1p = rows + r1 * pitch;
  for (int c = 0; c < A.nchunks; c++) {
    const PredictChunk ch = A.chunks[c];
    block_sync();  // the row tile is written; the previous chunk is done
    const int nn = (int)(ch.n1 - ch.n0), nl = (int)(ch.l1 - ch.l0);
    for (int i = tid; i < nn; i += kIjThreads) ((PNode*)chunk)[i] = A.nodes[ch.n0 + i];
    for (int i = tid; i < nl; i += kIjThreads) ((double*)chunk)[nn + i] = A.leaves[ch.l0 + i];
    block_sync();
    for (int tb = ch.t0; tb < ch.t1; tb += G) {
      const int t0 = tb + g0, t1 = tb + g1;
      const bool have0 = t0 < ch.t1, have1 = t1 < ch.t1;
      const bool walk0 = have0 && in0, walk1 = have1 && in1;
      const int u0 = have0 ? t0 : ch.t0, u1 = have1 ? t1 : ch.t0;
      const PNode* tn0 = (const PNode*)chunk + (A.tree_node[u0] - ch.n0);
      const PNode* tn1 = (const PNode*)chunk + (A.tree_node[u1] - ch.n0);
      const double* tl0 = (const double*)chunk + nn + (A.tree_leaf[u0] - ch.l0);
      const double* tl1 = (const double*)chunk + nn + (A.tree_leaf[u1] - ch.l0);
      PNode a0 = tn0[0], a1 = tn1[0];
      if (!walk0) a0.a = 0x80000000u;  // already at a leaf
      if (!walk1) a1.a = 0x80000000u;
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
      if (have0) M[t0 * R + r0] = walk0 ? tl0[a0.a & 0x7fffffffu] : 0.0;
      if (have1) M[t1 * R + r1] = walk1 ? tl1[a1.a & 0x7fffffffu] : 0.0;
    }
  }
  block_sync();  // every t_b of the tile is stored
  // thread r owns row r: the mean, d_b in place, c
  double m = 0.0, cc = 0.0;
  if (tid < R) {
    double s = 0.0;
    for (int b = 0; b < T; b++) s = __dadd_rn(s, M[b * R + tid]);
    m = s / (double)T;
    for (int b = 0; b < T; b++) {
      const double d = __dsub_rn(M[b * R + tid], m);
      M[b * R + tid] = d;
      cc = __dadd_rn(cc, __dmul_rn(d, d));
    }
  }
  block_sync();
  // The chains.  Unit u = (group g of 4 consecutive a, block of 64 rows), groups descending,
  // pass p gives unit 4 p + wave to each wave.  A unit reads d_b for b up to its own a, so a
  // pass's products d_a * u_a (written to M[a][r] after the pass's barrier, when every wave has
  // finished the pass's reads) land only on slots no later unit reads: later units have lower
  // groups, or the same group on other rows (the row blocks of a group share a pass: 1, 2 or 4
  // blocks over 4 waves).
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int nrb = (R + 63) >> 6, ng = (T + kIjGroup - 1) / kIjGroup;
  const int nunits = ng * nrb;
  // (the constant address space: a wave-uniform address then loads through the scalar cache)
  const ConstF64* Gd = (const ConstF64*)Q.G;
  for (int p0 = 0; p0 < nunits; p0 += kIjThreads / 64) {
    const int u = p0 + wave;
    const bool active = u < nunits;
    const int g = active ? ng - 1 - u / nrb : 0;
    const int a0 = g * kIjGroup;
    const int rr = (active ? u % nrb : 0) * 64 + lane;
    const bool lane_ok = active && rr < R;
    const int r = rr < R ? rr : R - 1;
    double pk[kIjGroup] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
      const ConstF64* gk[kIjGroup];
#pragma unroll
      for (int k = 0; k < kIjGroup; k++) gk[k] = Gd + (size_t)(a0 + k < T ? a0 + k : T - 1) * T;
      double s[kIjGroup] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
      for (int b = 0; b < a0; b++) {
        const double db = M[b * R + r];
#pragma unroll
        for (int k = 0; k < kIjGroup; k++) s[k] = __dadd_rn(s[k], __dmul_rn(gk[k][b], db));
      }
      double da[kIjGroup];
#pragma unroll
      for (int k = 0; k < kIjGroup; k++) da[k] = a0 + k < T ? M[(a0 + k) * R + r] : 0.0;
#pragma unroll
      for (int j = 0; j < kIjGroup - 1; j++)  // b = a0 + j feeds the chains a > b of the group
#pragma unroll
        for (int k = j + 1; k < kIjGroup; k++)
          if (a0 + k < T) s[k] = __dadd_rn(s[k], __dmul_rn(gk[k][a0 + j], da[j]));
#pragma unroll
      for (int k = 0; k < kIjGroup; k++) {
        const int a = a0 + k < T ? a0 + k : T - 1;
        const double uu = __dadd_rn(__dadd_rn(s[k], s[k]), __dmul_rn(gk[k][a], da[k]));
        pk[k] = __dmul_rn(da[k], uu);
      }
    }
    block_sync();  // the pass's reads of d are done
    if (lane_ok) {
#pragma unroll
      for (int k = 0; k < kIjGroup; k++)
        if (a0 + k < T) M[(a0 + k) * R + r] = pk[k];
    }
  }
  block_sync();
  if (tid < R && row0 + tid < A.N) {
    double q = 0.0;
    for (int a = 0; a < T; a++) q = __dadd_rn(q, M[a * R + tid]);
    ij_finish(q, cc, m, Q, Q.out + (row0 + tid) * 3);
  }
}

void launch_ij_tiled(hipStream_t st, const PredictArgs& a, const IjArgs& q) {
  const size_t pitch = (size_t)a.S * a.code_bytes + 4;
  const size_t lds = (size_t)q.R * pitch + (size_t)a.chunk_bytes + ij_matrix_lds(a.L, q.R);
  const dim3 grid((unsigned)((a.N + q.R - 1) / q.R));
  if (a.code_bytes == 1) {
    ij_set_max_lds((const void*)k_ij_tiled<uint8_t>, 160 * 1024);
    hipLaunchKernelGGL((k_ij_tiled<uint8_t>), grid, dim3(kIjThreads), lds, st, a, q);
  } else {
    ij_set_max_lds((const void*)k_ij_tiled<uint16_t>, 160 * 1024);
    hipLaunchKernelGGL((k_ij_tiled<uint16_t>), grid, dim3(kIjThreads), lds, st, a, q);
  }
}

// One thread per row of a batch of n: tp [T][n] holds the trees' predictions of the rows (and d
// afterwards); Q.out is the batch's first row's.
__global__ __launch_bounds__(256) void k_ij_form(double* __restrict__ tp, int64_t n, int T, IjArgs Q) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  double* col = tp + row;
  double s = 0.0;
  for (int b = 0; b < T; b++) s = __dadd_rn(s, col[(int64_t)b * n]);
  const double m = s / (double)T;
  for (int b = 0; b < T; b++) col[(int64_t)b * n] = __dsub_rn(col[(int64_t)b * n], m);
  double q = 0.0, c = 0.0;
  for (int a = 0; a < T; a++) {
    const double* ga = Q.G + (size_t)a * T;
    s = 0.0;
    for (int b = 0; b < a; b++) s = __dadd_rn(s, __dmul_rn(ga[b], col[(int64_t)b * n]));
    const double da = col[(int64_t)a * n];
    const double u = __dadd_rn(__dadd_rn(s, s), __dmul_rn(ga[a], da));
    q = __dadd_rn(q, __dmul_rn(da, u));
    c = __dadd_rn(c, __dmul_rn(da, da));
  }
  ij_finish(q, c, m, Q, Q.out + row * 3);
}

void launch_ij_form(hipStream_t st, double* tp, int64_t n, int T, const IjArgs& q) {
  hipLaunchKernelGGL(k_ij_form, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tp, n, T, q);
}

}  // namespace sbag
