// sbag_oobperm.hip — out-of-bag predictions under permuted features for gfx950 (MI355X,
// CDNA4): the device side of Breiman's permutation importance.
//
// Slot k of a feature batch asks for the out-of-bag prediction of every row r with one
// change: the value of feature feat[k] is row src[k][r]'s (in the dataset's code space:
// both rows share the feature's dictionary, so the substitution is exact).  Bags, trees,
// learner order and aggregation are sbag_predict_oob's (sbag_oob.hip).
//
//   k_predict_oob_perm  k_predict_oob's geometry (512 staged rows per workgroup, two rows
//                       per thread, forest chunks in LDS, thresholds in code space, the
//                       next tree's counts loaded a tree ahead) serving up to 64 slots per
//                       launch.  A row walks a tree once on its own codes and ORs, per node
//                       on the path, the set of slots that permute the node's feature.  A
//                       walk tests at most depth features, so for a slot outside that set
//                       the permuted walk is the same walk and its vote the same bits: the
//                       slot takes the baseline vote.  Only the slots in the set walk again,
//                       reading that one feature from the staged permuted code.  Every slot
//                       takes one vote per (out-of-bag learner, row), in learner order, so
//                       the fp64 sum and the running mode are those of the definition.  A
//                       slot all of whose votes for a row were the baseline's bits so far
//                       has the baseline's state and keeps none of its own; it forks (a
//                       copy of the baseline's state) at the first vote that differs.
//   k_permute_column    the fallback's substitution in a copy of the code matrix (u32
//                       codes, trees past the LDS chunk, more classes than the LDS counts):
//                       one column from the source rows, and back.
// Learner batches carry every slot's state in global memory, as OobArgs does for one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

#include "sbag_internal.h"

namespace sbag {

namespace {

constexpr int kRows = 512;  // = k_predict_oob's tile
constexpr int kThreads = 256;

void perm_set_max_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> g(mu);
  if (done.count({fn, dev})) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess)
    done.insert({fn, dev});
}

__device__ __forceinline__ double perm_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// the slots' accumulators of one workgroup (LDS); column = row of the tile, so consecutive
// lanes hit consecutive addresses
struct SlotAcc {
  double* sum;     // mean: [kb][kRows] running sums
  uint16_t* cnt;   // mode: [kb][nclasses][kRows] class counters
  uint16_t* best;  // mode: [kb][kRows] running maximum count
  uint16_t* cls;   // mode: [kb][kRows] running mode
  int nclasses;
  bool mode;
};

// one vote of slot k for the row in column col
__device__ __forceinline__ void slot_vote(const SlotAcc& s, int k, int col, double v) {
  if (s.mode) {
    const int c = (int)v;
    const uint16_t n = ++s.cnt[(k * s.nclasses + c) * kRows + col];
    if (n > s.best[k * kRows + col]) {
      s.best[k * kRows + col] = n;
      s.cls[k * kRows + col] = (uint16_t)c;
    }
  } else {
    s.sum[k * kRows + col] = s.sum[k * kRows + col] + v;
  }
}

// slot k of the row in column col leaves the baseline: its state becomes a copy of the
// baseline's (running sum / running mode acc, running maximum best, the row's counter
// column cnt)
__device__ __forceinline__ void slot_fork(const SlotAcc& s, int k, int col, double acc, int best,
                                          const uint16_t* cnt) {
  if (s.mode) {
    for (int c = 0; c < s.nclasses; c++) s.cnt[(k * s.nclasses + c) * kRows + col] = cnt[c * kRows];
    s.best[k * kRows + col] = (uint16_t)best;
    s.cls[k * kRows + col] = (uint16_t)(int)acc;
  } else {
    s.sum[k * kRows + col] = acc;
  }
}

}  // namespace

size_t oobperm_lds_fixed(int F) { return (size_t)F * 8 + kOobPermSlots * 4; }
size_t oobperm_lds_slot(int code_bytes, int agg, int nclasses) {
  return (size_t)kRows * ((size_t)code_bytes + (agg == kAggMode ? 2 * (size_t)nclasses + 4 : 8));
}

// LDS: k_predict_oob's [row tile][chunk][mode: baseline counters], then
// [fmask u64 [F]: the slots permuting each feature] [sfeat i32 [64]: each slot's feature]
// [the slots' accumulators (SlotAcc)] [pc CT [kb][512]: the permuted codes].
// Thread tid owns rows row0 + tid and row0 + tid + 256 and their columns everywhere.
template <typename CT>
__global__ __launch_bounds__(kThreads) void k_predict_oob_perm(PredictArgs A, OobArgs O, OobPermArgs Q) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int KB = Q.kb;
  const int pitch = A.S * (int)sizeof(CT) + 4;
  const bool mode_agg = A.agg == kAggMode;
  unsigned char* rows = smem;
  unsigned char* chunk = smem + (size_t)kRows * pitch;
  uint16_t* cnt = (uint16_t*)(chunk + A.chunk_bytes);  // baseline [nclasses][kRows]
  size_t base = (size_t)kRows * pitch + (size_t)A.chunk_bytes;
  if (mode_agg) base += (size_t)A.nclasses * kRows * 2;
  base = (base + 15) & ~(size_t)15;  // = predict_tiled_lds(A)
  unsigned long long* fmask = (unsigned long long*)(smem + base);
  int* sfeat = (int*)(fmask + Q.F);
  unsigned char* accp = (unsigned char*)(sfeat + kOobPermSlots);
  SlotAcc sa;
  sa.mode = mode_agg;
  sa.nclasses = A.nclasses;
  sa.sum = (double*)accp;
  sa.cnt = (uint16_t*)accp;
  sa.best = sa.cnt + (size_t)KB * A.nclasses * kRows;
  sa.cls = sa.best + (size_t)KB * kRows;
  CT* pc = (CT*)(accp + (size_t)KB * kRows * (mode_agg ? 2 * (size_t)A.nclasses + 4 : 8));

  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int rb = A.S * (int)sizeof(CT);  // bytes of one row
  for (int q = tid; q < kRows * (rb >> 2); q += kThreads) {
    const int r = q / (rb >> 2), w = q - r * (rb >> 2);
    uint32_t v = 0;
    if (row0 + r < A.N) v = *(const uint32_t*)((const unsigned char*)A.codes + (row0 + r) * rb + w * 4);
    *(uint32_t*)(rows + r * pitch + w * 4) = v;
  }
  for (int g = tid; g < Q.F; g += kThreads) fmask[g] = 0ull;
  if (tid < kOobPermSlots) sfeat[tid] = tid < KB ? Q.feat[tid] : -1;
  block_sync();
  if (tid == 0)  // (serial: a feature may sit in several slots)
    for (int k = 0; k < KB; k++) fmask[sfeat[k]] |= 1ull << k;
  // the permuted codes of the tile: codes[src[k][row]][feat[k]], once for all trees
  for (int q = tid; q < KB * kRows; q += kThreads) {
    const int k = q / kRows, r = q - k * kRows;
    CT v = 0;
    if (row0 + r < A.N) {
      const int64_t s = Q.src[(int64_t)k * A.N + row0 + r];
      v = ((const CT*)A.codes)[s * A.S + sfeat[k]];
    }
    pc[q] = v;
  }

  const int64_t ra = row0 + tid, rbw = ra + kThreads;
  const bool in0 = ra < A.N, in1 = rbw < A.N;
  double acc0 = 0.0, acc1 = 0.0;  // baseline: running sum (mean) or running mode
  int n0 = 0, n1 = 0, max0 = 0, max1 = 0;
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
      cnt[c * kRows + tid] = c0;
      cnt[c * kRows + tid + kThreads] = c1;
    }
  }
  // (first: no slot has a state of its own yet, nothing to load)
  for (int k = 0; k < KB && !O.first; k++) {
    if (mode_agg) {
      uint16_t b0 = 0, b1 = 0, m0 = 0, m1 = 0;
      if (in0) {
        b0 = (uint16_t)Q.pmax[(int64_t)k * A.N + ra];
        m0 = (uint16_t)(int)Q.pout[(int64_t)k * A.N + ra];
      }
      if (in1) {
        b1 = (uint16_t)Q.pmax[(int64_t)k * A.N + rbw];
        m1 = (uint16_t)(int)Q.pout[(int64_t)k * A.N + rbw];
      }
      sa.best[k * kRows + tid] = b0;
      sa.best[k * kRows + tid + kThreads] = b1;
      sa.cls[k * kRows + tid] = m0;
      sa.cls[k * kRows + tid + kThreads] = m1;
      for (int c = 0; c < A.nclasses; c++) {
        const int64_t o = ((int64_t)k * A.nclasses + c) * A.N;
        uint16_t c0 = 0, c1 = 0;
        if (in0) c0 = Q.pcnt[o + ra];
        if (in1) c1 = Q.pcnt[o + rbw];
        sa.cnt[(k * A.nclasses + c) * kRows + tid] = c0;
        sa.cnt[(k * A.nclasses + c) * kRows + tid + kThreads] = c1;
      }
    } else {
      double s0 = 0.0, s1 = 0.0;
      if (in0) s0 = Q.pout[(int64_t)k * A.N + ra];
      if (in1) s1 = Q.pout[(int64_t)k * A.N + rbw];
      sa.sum[k * kRows + tid] = s0;
      sa.sum[k * kRows + tid + kThreads] = s1;
    }
  }
  // d0 / d1: the slots whose state has left the baseline's.  A slot all of whose votes so
  // far were the baseline's bits has the baseline's state, bit for bit, and keeps none of
  // its own: it costs nothing until a re-walk first ends in another value (slot_fork).
  // State carried in from an earlier learner batch is every slot's own.
  const unsigned long long all_slots = KB >= 64 ? ~0ull : (1ull << KB) - 1ull;
  unsigned long long d0 = O.first ? 0ull : all_slots, d1 = d0;
  const unsigned char* r0p = rows + tid * pitch;
  const unsigned char* r1p = rows + (tid + kThreads) * pitch;
  const uint8_t* cp = O.counts;
  uint32_t k0n = 1, k1n = 1;  // rows past N count as in bag
  if (O.t0 < O.t1) {
    if (in0) k0n = cp[ra];
    if (in1) k1n = cp[rbw];
  }
  for (int c = 0; c < A.nchunks; c++) {
    const PredictChunk ch = A.chunks[c];
    const int ta = ch.t0 > O.t0 ? ch.t0 : O.t0, tb = ch.t1 < O.t1 ? ch.t1 : O.t1;
    if (ta >= tb) continue;  // (uniform: no tree of this batch in the chunk)
    block_sync();            // previous chunk done (and the tile, fmask and pc written)
    const int nb = (int)(ch.n1 - ch.n0) * 8, lb = (int)(ch.l1 - ch.l0) * 8;
    for (int i = tid; i < (nb >> 3); i += kThreads) ((PNode*)chunk)[i] = A.nodes[ch.n0 + i];
    for (int i = tid; i < (lb >> 3); i += kThreads)
      ((double*)(chunk + nb))[i] = A.leaves[ch.l0 + i];
    block_sync();
    for (int t = ta; t < tb; t++) {
      const PNode* tn = (const PNode*)chunk + (A.tree_node[t] - ch.n0);
      const double* tl = (const double*)(chunk + nb) + (A.tree_leaf[t] - ch.l0);
      const bool oob0 = k0n == 0, oob1 = k1n == 0;
      if (t + 1 < O.t1) {
        cp += A.N;
        if (in0) k0n = cp[ra];
        if (in1) k1n = cp[rbw];
      }
      // the baseline walk; w0 / w1: the slots whose feature the path tested
      PNode a0 = tn[0], a1 = a0;
      if (!oob0) a0.a = 0x80000000u;  // in bag: already at a leaf
      if (!oob1) a1.a = 0x80000000u;
      unsigned long long w0 = 0ull, w1 = 0ull;
      while (!((a0.a & a1.a) & 0x80000000u)) {  // until both walks reach a leaf
        if (!(a0.a & 0x80000000u)) {
          const uint32_t g = a0.b >> 17;
          const uint32_t code = ((const CT*)r0p)[g];
          w0 |= fmask[g];
          a0 = tn[a0.a + (code < (a0.b & 0x1ffffu) ? 0u : 1u)];
        }
        if (!(a1.a & 0x80000000u)) {
          const uint32_t g = a1.b >> 17;
          const uint32_t code = ((const CT*)r1p)[g];
          w1 |= fmask[g];
          a1 = tn[a1.a + (code < (a1.b & 0x1ffffu) ? 0u : 1u)];
        }
      }
      double p0 = 0.0, p1 = 0.0;  // the baseline votes
      if (oob0) p0 = tl[a0.a & 0x7fffffffu];
      if (oob1) p1 = tl[a1.a & 0x7fffffffu];
      // the slots in the path's set walk again, each lane through its own set, lowest slot
      // first, with the slot's feature read from the permuted code; until every lane's sets
      // are empty.  (Before the baseline takes its vote: a slot that forks here copies the
      // baseline's state of the trees so far.)
      const unsigned long long t0m = w0, t1m = w1;
      while (w0 | w1) {
        int s0 = -1, s1 = -1;
        uint32_t g0 = 0xffffffffu, g1 = 0xffffffffu, c0 = 0, c1 = 0;
        PNode b0, b1;
        b0.a = b1.a = 0x80000000u;
        b0.b = b1.b = 0;
        if (w0) {
          s0 = __ffsll((long long)w0) - 1;
          w0 &= w0 - 1;
          g0 = (uint32_t)sfeat[s0];
          c0 = pc[s0 * kRows + tid];
          b0 = tn[0];
        }
        if (w1) {
          s1 = __ffsll((long long)w1) - 1;
          w1 &= w1 - 1;
          g1 = (uint32_t)sfeat[s1];
          c1 = pc[s1 * kRows + tid + kThreads];
          b1 = tn[0];
        }
        while (!((b0.a & b1.a) & 0x80000000u)) {
          if (!(b0.a & 0x80000000u)) {
            const uint32_t g = b0.b >> 17;
            const uint32_t own = ((const CT*)r0p)[g];
            const uint32_t code = g == g0 ? c0 : own;
            b0 = tn[b0.a + (code < (b0.b & 0x1ffffu) ? 0u : 1u)];
          }
          if (!(b1.a & 0x80000000u)) {
            const uint32_t g = b1.b >> 17;
            const uint32_t own = ((const CT*)r1p)[g];
            const uint32_t code = g == g1 ? c1 : own;
            b1 = tn[b1.a + (code < (b1.b & 0x1ffffu) ? 0u : 1u)];
          }
        }
        if (s0 >= 0) {
          const double q = tl[b0.a & 0x7fffffffu];
          if ((d0 >> s0) & 1ull) {
            slot_vote(sa, s0, tid, q);
          } else if (__double_as_longlong(q) != __double_as_longlong(p0)) {
            slot_fork(sa, s0, tid, acc0, max0, cnt + tid);
            slot_vote(sa, s0, tid, q);
            d0 |= 1ull << s0;
          }
        }
        if (s1 >= 0) {
          const double q = tl[b1.a & 0x7fffffffu];
          if ((d1 >> s1) & 1ull) {
            slot_vote(sa, s1, tid + kThreads, q);
          } else if (__double_as_longlong(q) != __double_as_longlong(p1)) {
            slot_fork(sa, s1, tid + kThreads, acc1, max1, cnt + tid + kThreads);
            slot_vote(sa, s1, tid + kThreads, q);
            d1 |= 1ull << s1;
          }
        }
      }
      if (oob0) {
        n0++;
        if (mode_agg) {
          const int k = ++cnt[(int)p0 * kRows + tid];
          if (k > max0) {
            max0 = k;
            acc0 = p0;
          }
        } else {
          acc0 += p0;
        }
      }
      if (oob1) {
        n1++;
        if (mode_agg) {
          const int k = ++cnt[(int)p1 * kRows + tid + kThreads];
          if (k > max1) {
            max1 = k;
            acc1 = p1;
          }
        } else {
          acc1 += p1;
        }
      }
      // the slots with a state of their own that did not walk again vote as the baseline does
      const unsigned long long v0 = oob0 ? d0 & ~t0m : 0ull, v1 = oob1 ? d1 & ~t1m : 0ull;
      for (int k = 0; k < KB; k++) {
        if ((v0 >> k) & 1ull) slot_vote(sa, k, tid, p0);
        if ((v1 >> k) & 1ull) slot_vote(sa, k, tid + kThreads, p1);
      }
    }
  }
  if (O.last) {
    if (in0) {
      A.out[ra] = n0 == 0 ? perm_nan() : mode_agg ? acc0 : acc0 / (double)n0;
      O.n_oob[ra] = n0;
    }
    if (in1) {
      A.out[rbw] = n1 == 0 ? perm_nan() : mode_agg ? acc1 : acc1 / (double)n1;
      O.n_oob[rbw] = n1;
    }
    for (int k = 0; k < KB; k++) {  // (a slot without a state of its own ends as the baseline)
      if (in0) {
        double v = acc0;
        if ((d0 >> k) & 1ull) v = mode_agg ? (double)sa.cls[k * kRows + tid] : sa.sum[k * kRows + tid];
        Q.pout[(int64_t)k * A.N + ra] = n0 == 0 ? perm_nan() : mode_agg ? v : v / (double)n0;
      }
      if (in1) {
        double v = acc1;
        if ((d1 >> k) & 1ull)
          v = mode_agg ? (double)sa.cls[k * kRows + tid + kThreads] : sa.sum[k * kRows + tid + kThreads];
        Q.pout[(int64_t)k * A.N + rbw] = n1 == 0 ? perm_nan() : mode_agg ? v : v / (double)n1;
      }
    }
    return;
  }
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
      if (in0) O.gcnt[(int64_t)c * A.N + ra] = cnt[c * kRows + tid];
      if (in1) O.gcnt[(int64_t)c * A.N + rbw] = cnt[c * kRows + tid + kThreads];
    }
  }
  // every slot goes out with a state of its own: the baseline's where it never left it
  for (int k = 0; k < KB; k++) {
    const bool own0 = (d0 >> k) & 1ull, own1 = (d1 >> k) & 1ull;
    if (mode_agg) {
      if (in0) {
        Q.pout[(int64_t)k * A.N + ra] = own0 ? (double)sa.cls[k * kRows + tid] : acc0;
        Q.pmax[(int64_t)k * A.N + ra] = own0 ? (int32_t)sa.best[k * kRows + tid] : max0;
      }
      if (in1) {
        Q.pout[(int64_t)k * A.N + rbw] = own1 ? (double)sa.cls[k * kRows + tid + kThreads] : acc1;
        Q.pmax[(int64_t)k * A.N + rbw] = own1 ? (int32_t)sa.best[k * kRows + tid + kThreads] : max1;
      }
      for (int c = 0; c < A.nclasses; c++) {
        const int64_t o = ((int64_t)k * A.nclasses + c) * A.N;
        if (in0) Q.pcnt[o + ra] = own0 ? sa.cnt[(k * A.nclasses + c) * kRows + tid] : cnt[c * kRows + tid];
        if (in1)
          Q.pcnt[o + rbw] =
              own1 ? sa.cnt[(k * A.nclasses + c) * kRows + tid + kThreads] : cnt[c * kRows + tid + kThreads];
      }
    } else {
      if (in0) Q.pout[(int64_t)k * A.N + ra] = own0 ? sa.sum[k * kRows + tid] : acc0;
      if (in1) Q.pout[(int64_t)k * A.N + rbw] = own1 ? sa.sum[k * kRows + tid + kThreads] : acc1;
    }
  }
}

void launch_predict_oob_perm(hipStream_t st, const PredictArgs& a, const OobArgs& o, const OobPermArgs& q) {
  const size_t lds = (predict_tiled_lds(a) + oobperm_lds_fixed(q.F) +
                      (size_t)q.kb * oobperm_lds_slot(a.code_bytes, a.agg, a.nclasses) + 15) & ~(size_t)15;
  perm_set_max_lds((const void*)k_predict_oob_perm<uint8_t>, 160 * 1024);
  perm_set_max_lds((const void*)k_predict_oob_perm<uint16_t>, 160 * 1024);
  const dim3 grid((unsigned)((a.N + kRows - 1) / kRows));
  if (a.code_bytes == 1)
    hipLaunchKernelGGL(k_predict_oob_perm<uint8_t>, grid, dim3(kThreads), lds, st, a, o, q);
  else
    hipLaunchKernelGGL(k_predict_oob_perm<uint16_t>, grid, dim3(kThreads), lds, st, a, o, q);
}

// dst[r][g] = orig[src[r]][g] (src == nullptr: orig[r][g], the column restored)
template <typename CT>
__global__ __launch_bounds__(256) void k_permute_column(CT* __restrict__ dst, const CT* __restrict__ orig,
                                                        const int32_t* __restrict__ src, int64_t N,
                                                        int32_t S, int32_t g) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  const int64_t s = src ? (int64_t)src[r] : r;
  dst[r * S + g] = orig[s * S + g];
}

void launch_permute_column(hipStream_t st, void* dst, const void* orig, int code_bytes, int64_t N,
                           int32_t S, int32_t g, const int32_t* src) {
  const dim3 grid((unsigned)((N + 255) / 256));
  if (code_bytes == 1)
    hipLaunchKernelGGL(k_permute_column<uint8_t>, grid, dim3(256), 0, st, (uint8_t*)dst,
                       (const uint8_t*)orig, src, N, S, g);
  else if (code_bytes == 2)
    hipLaunchKernelGGL(k_permute_column<uint16_t>, grid, dim3(256), 0, st, (uint16_t*)dst,
                       (const uint16_t*)orig, src, N, S, g);
  else
    hipLaunchKernelGGL(k_permute_column<uint32_t>, grid, dim3(256), 0, st, (uint32_t*)dst,
                       (const uint32_t*)orig, src, N, S, g);
}

}  // namespace sbag
