// sbag_staged.hip — staged evaluation of a bagged ensemble for gfx950 (MI355X, CDNA4): the
// score of the forest's first l + 1 trees for every l, in one pass over the rows.
//
// Stage l is the ensemble of trees [0, l].  A row's stage prediction is sbag_predict_oob's
// aggregation (sbag_oob.hip) over the learners i <= l whose bag left the row out (every
// learner when there is no mask): the running sum over the running count, or the running
// first-to-max mode; the row is covered at stage l when that count is >= 1.  Per stage:
//   covered  the covered rows
//   correct  mode: the covered rows whose stage prediction equals the label
//   sum_se   mean: sum over the covered rows of e * e, e = pred - y
//   sum_ae   mean: sum over the covered rows of |e|
// The two fp64 sums have a fixed order (sbag.h): a row's term is rounded on its own (a row
// that is not covered or lies past N contributes +0.0); the 512 terms of a tile are summed
// by halving, v[i] = v[i] + v[i + h] for h = 256, 128, ..., 1; the tile sums are added left
// to right from 0.0.  __dadd_rn / __dmul_rn / __dsub_rn are never contracted.
//
//   k_eval_staged  the fused pass: k_predict_oob's geometry (512 staged rows per workgroup,
//                  256 threads, thread tid owns rows tid and tid + 256, forest chunks in LDS,
//                  thresholds in code space, bag counts loaded a tree ahead) and its carried
//                  state for learner batches (OobArgs).  After each tree a thread holds its
//                  two rows' terms; their sum is the h = 256 step.  The per-thread partials
//                  of G consecutive stages are parked in LDS ([G][256] fp64 per sum) and
//                  reduced together: wave w takes every fourth (stage, sum) pair, lane i
//                  adds (v[i] + v[i + 128]) + (v[i + 64] + v[i + 192]) (h = 128, 64) and the
//                  wave finishes with __shfl_down (h = 32 ... 1).  Two barriers per G trees.
//                  covered / correct: ballot popcounts per wave, parked beside the partials.
//   k_staged_agg   the general path: the same running aggregation, park and reduction over a
//                  learner batch's per-tree predictions votes [K][N] and bag counts [K][N]
//                  (u32 codes, trees past the LDS chunk, more classes than the LDS counters
//                  hold), mode counters in global memory as k_aggregate_oob keeps them.
//   k_stage_fold   one lane per (stage, quantity) adds the tile partials [tiles][trees] in
//                  tile order and writes the stage's field.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

#include "sbag_internal.h"

namespace sbag {

namespace {

constexpr int kSgRows = 512;  // = k_predict_oob's tile (predict_tiled_lds sizes the LDS)
constexpr int kSgThreads = 256;

// (as sbag_kernels.hip's: the dynamic-LDS cap of a kernel, once per (kernel, device))
void staged_set_max_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> g(mu);
  if (done.count({fn, dev})) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess)
    done.insert({fn, dev});
}

// A row's state after a tree -> its terms.  n == 0 (not covered, or past N): +0.0 / false.
__device__ __forceinline__ void stage_terms(bool mode_agg, double acc, int n, double y, double& se,
                                            double& ae, bool& cor) {
  se = 0.0;
  ae = 0.0;
  cor = false;
  if (n == 0) return;
  if (mode_agg) {
    cor = acc == y;
  } else {
    const double e = __dsub_rn(acc / (double)n, y);
    se = __dmul_rn(e, e);
    ae = fabs(e);
  }
}

// A thread's two rows of one stage into slot g of the park: the h = 256 step of the two
// sums, and the wave's covered / correct counts (lane 0).  pd: [2][G][256] fp64 (mean
// only), pi: [G][4 waves][2].
__device__ __forceinline__ void stage_park(bool mode_agg, int tid, int g, int G, double* pd, int* pi,
                                           double se0, double se1, double ae0, double ae1, bool cov0,
                                           bool cov1, bool cor0, bool cor1) {
  if (!mode_agg) {
    pd[g * kSgThreads + tid] = __dadd_rn(se0, se1);
    pd[(G + g) * kSgThreads + tid] = __dadd_rn(ae0, ae1);
  }
  const int ncov = __popcll(__ballot(cov0)) + __popcll(__ballot(cov1));
  const int ncor = __popcll(__ballot(cor0)) + __popcll(__ballot(cor1));
  if ((tid & 63) == 0) {
    pi[(g * 4 + (tid >> 6)) * 2] = ncov;
    pi[(g * 4 + (tid >> 6)) * 2 + 1] = ncor;
  }
}

// The parked stages [stage0, stage0 + ng) of tile `tile` reduced into the tile partials.
// Every thread of the block calls it (two barriers).
__device__ __forceinline__ void stage_flush(bool mode_agg, int tid, int ng, int G, const double* pd,
                                            const int* pi, const StagedArgs& S, int64_t tile, int stage0) {
  block_sync();  // the park is written
  const int w = tid >> 6, lane = tid & 63;
  if (!mode_agg) {
    for (int p = w; p < 2 * ng; p += 4) {  // (uniform per wave)
      const int g = p >> 1, q = p & 1;
      const double* v = pd + (q * G + g) * kSgThreads;
      // h = 128 then h = 64: v[i] = (v[i] + v[i + 128]) + (v[i + 64] + v[i + 192]), i < 64
      double x = __dadd_rn(__dadd_rn(v[lane], v[lane + 128]), __dadd_rn(v[lane + 64], v[lane + 192]));
      for (int h = 32; h >= 1; h >>= 1) x = __dadd_rn(x, __shfl_down(x, h, 64));
      if (lane == 0) (q ? S.t_ae : S.t_se)[tile * S.trees + stage0 + g] = x;
    }
  }
  if (tid < 2 * ng) {
    const int g = tid >> 1, q = tid & 1;
    const int* v = pi + g * 8 + q;
    (q ? S.t_cor : S.t_cov)[tile * S.trees + stage0 + g] = v[0] + v[2] + v[4] + v[6];
  }
  block_sync();  // the park is read: the next group may overwrite it
}

}  // namespace

size_t staged_park_lds(int agg, int G) {
  return (agg == kAggMode ? 0 : (size_t)2 * G * kSgThreads * 8) + (size_t)G * 8 * 4;
}

// LDS: [512 rows x (S code bytes + 4)] [chunk_bytes: packed nodes + leaf values]
// [mode: u16 counters [nclasses][512]] (= predict_tiled_lds) [park: staged_park_lds].
// Thread tid owns rows row0 + tid and row0 + tid + 256 and their counter columns.
template <typename CT>
__global__ __launch_bounds__(kSgThreads) void k_eval_staged(PredictArgs A, OobArgs O, StagedArgs S) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int pitch = A.S * (int)sizeof(CT) + 4;
  const bool mode_agg = A.agg == kAggMode;
  const int G = S.G;
  unsigned char* rows = smem;
  unsigned char* chunk = smem + (size_t)kSgRows * pitch;
  uint16_t* cnt = (uint16_t*)(chunk + A.chunk_bytes);  // [nclasses][kSgRows]
  size_t base = (size_t)kSgRows * pitch + (size_t)A.chunk_bytes;
  if (mode_agg) base += (size_t)A.nclasses * kSgRows * 2;
  base = (base + 15) & ~(size_t)15;  // = predict_tiled_lds(A)
  double* pd = (double*)(smem + base);
  int* pi = (int*)(smem + base + (mode_agg ? 0 : (size_t)2 * G * kSgThreads * 8));
  const int64_t row0 = (int64_t)blockIdx.x * kSgRows;
  const int rb = A.S * (int)sizeof(CT);  // bytes of one row
  for (int q = tid; q < kSgRows * (rb >> 2); q += kSgThreads) {
    const int r = q / (rb >> 2), w = q - r * (rb >> 2);
    uint32_t v = 0;
    if (row0 + r < A.N) v = *(const uint32_t*)((const unsigned char*)A.codes + (row0 + r) * rb + w * 4);
    *(uint32_t*)(rows + r * pitch + w * 4) = v;
  }
  const int64_t ra = row0 + tid, rbw = ra + kSgThreads;
  const bool in0 = ra < A.N, in1 = rbw < A.N;
  double acc0 = 0.0, acc1 = 0.0;  // running sum (mean) or running mode
  int n0 = 0, n1 = 0, max0 = 0, max1 = 0;
  const double y0 = in0 ? S.y[ra] : 0.0, y1 = in1 ? S.y[rbw] : 0.0;
  if (!O.first) {
    if (in0) {
      acc0 = A.out[ra];
      n0 = O.n_oob[ra];
    }
    if (in1) {
      acc1 = A.out[rbw];
      n1 = O.n_oob[rbw];
    }
    if (mode_agg) {
      if (in0) max0 = O.gmax[ra];
      if (in1) max1 = O.gmax[rbw];
    }
  }
  if (mode_agg) {
    for (int c = 0; c < A.nclasses; c++) {
      uint16_t c0 = 0, c1 = 0;
      if (!O.first) {
        if (in0) c0 = O.gcnt[(int64_t)c * A.N + ra];
        if (in1) c1 = O.gcnt[(int64_t)c * A.N + rbw];
      }
      cnt[c * kSgRows + tid] = c0;
      cnt[c * kSgRows + tid + kSgThreads] = c1;
    }
  }
  // the rows' terms: they change only when a tree counts for the row
  double se0, se1, ae0, ae1;
  bool cor0, cor1;
  stage_terms(mode_agg, acc0, n0, y0, se0, ae0, cor0);
  stage_terms(mode_agg, acc1, n1, y1, se1, ae1, cor1);
  const unsigned char* r0p = rows + tid * pitch;
  const unsigned char* r1p = rows + (tid + kSgThreads) * pitch;
  // the bag multiplicities of the next tree, loaded a tree ahead (lanes coalesced over
  // rows); rows past N count as in bag: no walk, nothing accumulated.  No mask (counts
  // null): every tree counts for every row of the dataset.
  const uint8_t* cp = O.counts;
  uint32_t k0n = in0 ? 0 : 1, k1n = in1 ? 0 : 1;
  if (cp && O.t0 < O.t1) {
    if (in0) k0n = cp[ra];
    if (in1) k1n = cp[rbw];
  }
  int gi = 0;  // stages parked since the last flush (uniform)
  for (int c = 0; c < A.nchunks; c++) {
    const PredictChunk ch = A.chunks[c];
    const int ta = ch.t0 > O.t0 ? ch.t0 : O.t0, tb = ch.t1 < O.t1 ? ch.t1 : O.t1;
    if (ta >= tb) continue;  // (uniform: no tree of this batch in the chunk)
    block_sync();            // previous chunk done (and the row tile written)
    const int nb = (int)(ch.n1 - ch.n0) * 8, lb = (int)(ch.l1 - ch.l0) * 8;
    for (int i = tid; i < (nb >> 3); i += kSgThreads) ((PNode*)chunk)[i] = A.nodes[ch.n0 + i];
    for (int i = tid; i < (lb >> 3); i += kSgThreads)
      ((double*)(chunk + nb))[i] = A.leaves[ch.l0 + i];
    block_sync();
    for (int t = ta; t < tb; t++) {
      const PNode* tn = (const PNode*)chunk + (A.tree_node[t] - ch.n0);
      const double* tl = (const double*)(chunk + nb) + (A.tree_leaf[t] - ch.l0);
      const bool oob0 = k0n == 0, oob1 = k1n == 0;
      if (cp && t + 1 < O.t1) {
        cp += A.N;
        if (in0) k0n = cp[ra];
        if (in1) k1n = cp[rbw];
      }
      PNode a0 = tn[0], a1 = a0;
      if (!oob0) a0.a = 0x80000000u;  // in bag: already at a leaf
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
      if (oob0) {
        const double p0 = tl[a0.a & 0x7fffffffu];
        n0++;
        if (mode_agg) {
          const int k = ++cnt[(int)p0 * kSgRows + tid];
          if (k > max0) {
            max0 = k;
            acc0 = p0;
          }
        } else {
          acc0 = __dadd_rn(acc0, p0);
        }
        stage_terms(mode_agg, acc0, n0, y0, se0, ae0, cor0);
      }
      if (oob1) {
        const double p1 = tl[a1.a & 0x7fffffffu];
        n1++;
        if (mode_agg) {
          const int k = ++cnt[(int)p1 * kSgRows + tid + kSgThreads];
          if (k > max1) {
            max1 = k;
            acc1 = p1;
          }
        } else {
          acc1 = __dadd_rn(acc1, p1);
        }
        stage_terms(mode_agg, acc1, n1, y1, se1, ae1, cor1);
      }
      stage_park(mode_agg, tid, gi, G, pd, pi, se0, se1, ae0, ae1, n0 > 0, n1 > 0, cor0, cor1);
      if (++gi == G || t + 1 == O.t1) {
        stage_flush(mode_agg, tid, gi, G, pd, pi, S, (int64_t)blockIdx.x, t + 1 - gi);
        gi = 0;
      }
    }
  }
  if (O.last) return;  // nothing reads a row's state after the last stage
  if (in0) {
    A.out[ra] = acc0;
    O.n_oob[ra] = n0;
  }
  if (in1) {
    A.out[rbw] = acc1;
    O.n_oob[rbw] = n1;
  }
  if (mode_agg) {
    if (in0) O.gmax[ra] = max0;
    if (in1) O.gmax[rbw] = max1;
    for (int c = 0; c < A.nclasses; c++) {
      if (in0) O.gcnt[(int64_t)c * A.N + ra] = cnt[c * kSgRows + tid];
      if (in1) O.gcnt[(int64_t)c * A.N + rbw] = cnt[c * kSgRows + tid + kSgThreads];
    }
  }
}

void launch_eval_staged(hipStream_t st, const PredictArgs& a, const OobArgs& o, const StagedArgs& s) {
  const size_t lds = predict_tiled_lds(a) + staged_park_lds(a.agg, s.G);
  staged_set_max_lds((const void*)k_eval_staged<uint8_t>, 160 * 1024);
  staged_set_max_lds((const void*)k_eval_staged<uint16_t>, 160 * 1024);
  const dim3 grid((unsigned)((a.N + kSgRows - 1) / kSgRows));
  if (a.code_bytes == 1)
    hipLaunchKernelGGL(k_eval_staged<uint8_t>, grid, dim3(kSgThreads), lds, st, a, o, s);
  else
    hipLaunchKernelGGL(k_eval_staged<uint16_t>, grid, dim3(kSgThreads), lds, st, a, o, s);
}

// One workgroup per 512-row tile of [row_begin, row_end) (row_begin a multiple of 512) over
// a learner batch's per-tree predictions votes [K][N] and bag counts [K][N] (null: no
// mask); the batch's stages are [t0, t0 + K).  Mode counters are u16 [nclasses][row_end -
// row_begin] in global memory (zeroed by the launcher before the first batch); the rest of
// a row's state goes through out / n_oob / gmax between batches.
__global__ __launch_bounds__(kSgThreads) void k_staged_agg(const double* __restrict__ votes,
                                                          const uint8_t* __restrict__ counts, int K,
                                                          int64_t N, int agg, double* __restrict__ out,
                                                          int32_t* __restrict__ n_oob,
                                                          int32_t* __restrict__ gmax,
                                                          uint16_t* __restrict__ gcnt, int first, int last,
                                                          int64_t row_begin, int64_t row_end, int t0,
                                                          StagedArgs S) {
  __shared__ double pd[2 * kStagedMaxGroup * kSgThreads];
  __shared__ int pi[kStagedMaxGroup * 8];
  const int tid = threadIdx.x;
  const bool mode_agg = agg == kAggMode;
  const int G = S.G;
  const int64_t tile = row_begin / kSgRows + blockIdx.x;
  const int64_t ra = tile * kSgRows + tid, rbw = ra + kSgThreads;
  const bool in0 = ra < row_end, in1 = rbw < row_end;
  const int64_t cstride = row_end - row_begin;
  uint16_t* cnt0 = gcnt + (ra - row_begin);
  uint16_t* cnt1 = gcnt + (rbw - row_begin);
  double acc0 = 0.0, acc1 = 0.0;
  int n0 = 0, n1 = 0, max0 = 0, max1 = 0;
  const double y0 = in0 ? S.y[ra] : 0.0, y1 = in1 ? S.y[rbw] : 0.0;
  if (!first) {
    if (in0) {
      acc0 = out[ra];
      n0 = n_oob[ra];
      if (mode_agg) max0 = gmax[ra];
    }
    if (in1) {
      acc1 = out[rbw];
      n1 = n_oob[rbw];
      if (mode_agg) max1 = gmax[rbw];
    }
  }
  double se0, se1, ae0, ae1;
  bool cor0, cor1;
  stage_terms(mode_agg, acc0, n0, y0, se0, ae0, cor0);
  stage_terms(mode_agg, acc1, n1, y1, se1, ae1, cor1);
  int gi = 0;
  for (int l = 0; l < K; l++) {
    if (in0 && (!counts || counts[(int64_t)l * N + ra] == 0)) {
      const double v = votes[(int64_t)l * N + ra];
      n0++;
      if (mode_agg) {
        const int k = ++cnt0[(int64_t)(int)v * cstride];
        if (k > max0) {
          max0 = k;
          acc0 = v;
        }
      } else {
        acc0 = __dadd_rn(acc0, v);
      }
      stage_terms(mode_agg, acc0, n0, y0, se0, ae0, cor0);
    }
    if (in1 && (!counts || counts[(int64_t)l * N + rbw] == 0)) {
      const double v = votes[(int64_t)l * N + rbw];
      n1++;
      if (mode_agg) {
        const int k = ++cnt1[(int64_t)(int)v * cstride];
        if (k > max1) {
          max1 = k;
          acc1 = v;
        }
      } else {
        acc1 = __dadd_rn(acc1, v);
      }
      stage_terms(mode_agg, acc1, n1, y1, se1, ae1, cor1);
    }
    stage_park(mode_agg, tid, gi, G, pd, pi, se0, se1, ae0, ae1, n0 > 0, n1 > 0, cor0, cor1);
    if (++gi == G || l + 1 == K) {
      stage_flush(mode_agg, tid, gi, G, pd, pi, S, tile, t0 + l + 1 - gi);
      gi = 0;
    }
  }
  if (last) return;
  if (in0) {
    out[ra] = acc0;
    n_oob[ra] = n0;
    if (mode_agg) gmax[ra] = max0;
  }
  if (in1) {
    out[rbw] = acc1;
    n_oob[rbw] = n1;
    if (mode_agg) gmax[rbw] = max1;
  }
}

void launch_staged_agg(hipStream_t st, const double* votes, const uint8_t* counts, int K, int64_t N,
                       int agg, int nclasses, double* out, int32_t* n_oob, int32_t* gmax, uint16_t* gcnt,
                       int64_t gcnt_rows, bool first, bool last, int t0, const StagedArgs& s) {
  const bool mode_agg = agg == kAggMode;
  // (row ranges of whole tiles: gcnt_rows is a multiple of 512 or >= N)
  const int64_t step = mode_agg ? std::max<int64_t>(gcnt_rows, kSgRows) : std::max<int64_t>(N, 1);
  for (int64_t r0 = 0; r0 < N; r0 += step) {
    const int64_t r1 = std::min(N, r0 + step);
    if (mode_agg && first) (void)hipMemsetAsync(gcnt, 0, (size_t)nclasses * (size_t)(r1 - r0) * 2, st);
    hipLaunchKernelGGL(k_staged_agg, dim3((unsigned)((r1 - r0 + kSgRows - 1) / kSgRows)), dim3(kSgThreads), 0,
                       st, votes, counts, K, N, agg, out, n_oob, gmax, gcnt, first ? 1 : 0, last ? 1 : 0, r0,
                       r1, t0, s);
  }
}

// Thread (q, stage): quantity q of the stage, its tile partials added in tile order from
// zero.  q = 0 sum_se, 1 sum_ae, 2 covered, 3 correct; the quantities the aggregation does
// not define are written as zero without a read.
__global__ __launch_bounds__(256) void k_stage_fold(StagedArgs S, int64_t tiles, int agg,
                                                    StageStats* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 4 * S.trees) return;
  const int q = idx / S.trees, stage = idx - q * S.trees;
  const bool mode_agg = agg == kAggMode;
  if (q < 2) {
    double s = 0.0;
    if (!mode_agg) {
      const double* p = (q ? S.t_ae : S.t_se) + stage;
      int64_t k = 0;
      for (; k + 8 <= tiles; k += 8) {  // eight loads in flight, the additions still in tile order
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = p[(k + j) * S.trees];
#pragma unroll
        for (int j = 0; j < 8; j++) s = __dadd_rn(s, v[j]);
      }
      for (; k < tiles; k++) s = __dadd_rn(s, p[k * S.trees]);
    }
    if (q)
      out[stage].sum_ae = s;
    else
      out[stage].sum_se = s;
  } else {
    int64_t s = 0;
    if (q == 2 || mode_agg) {
      const int32_t* p = (q == 3 ? S.t_cor : S.t_cov) + stage;
      int64_t k = 0;
      for (; k + 8 <= tiles; k += 8) {
        int32_t v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = p[(k + j) * S.trees];
#pragma unroll
        for (int j = 0; j < 8; j++) s += v[j];
      }
      for (; k < tiles; k++) s += p[k * S.trees];
    }
    if (q == 3)
      out[stage].correct = s;
    else
      out[stage].covered = s;
  }
}

void launch_stage_fold(hipStream_t st, const StagedArgs& s, int64_t tiles, int agg, StageStats* out) {
  hipLaunchKernelGGL(k_stage_fold, dim3((unsigned)((4 * s.trees + 255) / 256)), dim3(256), 0, st, s, tiles,
                     agg, out);
}

}  // namespace sbag
