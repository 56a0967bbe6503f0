// sbag_pd.hip — partial dependence of a forest on one feature for gfx950 (MI355X, CDNA4).
//
// A tree's response to the feature is piecewise constant: with a sorted grid, a node that tests
// the feature sends the grid points below s = #{g : grid[g] <= threshold} left and the rest
// right, whatever the row holds.  So a row's walk through a tree with "the feature = every grid
// point at once" is a depth-first walk over grid ranges: a range [lo, hi) that reaches such a
// node continues left as [lo, min(hi, s)) and right as [max(lo, s), hi), an empty side is not
// walked, and every other node sends the whole range the way the row's own value points.  The
// ranges that arrive at the leaves partition [0, G), and the result of the whole call is
// cnt[leaf][g], the number of rows whose range at `leaf` holds g: integers, exact in any order.
//
//   k_pd_count  the hot path (u8 / u16 codes).  A workgroup owns a tree group and a row slice
//               and stays resident over the slice's 512-row tiles.  LDS: the staged tile (rows
//               in 16-byte pieces at pitch S * code_bytes + 4, as k_predict_tiled), the group's
//               packed nodes, and int32 difference counters [leaves of the group][G + 1].
//               1024 threads: thread (h, r) walks row r of the tile through the group's trees
//               t0 + h, t0 + h + 2, ...  The pending right branches are a stack of kPdStack
//               packed words (node, lo, hi) kept in registers as a shift register, so no index
//               is dynamic and nothing goes to scratch; the host sends a forest whose walk could
//               hold more to k_pd_walk.  At a leaf: ds_add +1 at diff[leaf][lo], -1 at
//               diff[leaf][hi] when hi < G.  The counters wrap mod 2^32, harmlessly: every
//               prefix sum is a number of rows of the slice.  After the last tile each thread
//               prefix-sums leaf rows of the table and adds the non-zero counts to the global
//               u64 table: one flush a workgroup.
//   k_pd_walk   the general path: a thread per row over DevNodes in global memory, the stack in
//               scratch (at most G - 1 ranges are ever pending: they are disjoint and non-empty),
//               +1 / -1 with 64-bit global atomics into the same table, which k_pd_prefix then
//               sums along g in place.
//   k_pd_fold   cnt -> tree_pd / votes -> pd, in the order sbag.h fixes: a tree's leaves in
//               pre-order, then the trees in order, every product and sum rounded on its own.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

#include "sbag_internal.h"
#include "sbag_pd_plan.h"

namespace sbag {

namespace {

// (as sbag_kernels.hip's: the dynamic-LDS cap of a kernel, once per (kernel, device))
void pd_set_max_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> g(mu);
  if (done.count({fn, dev})) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess)
    done.insert({fn, dev});
}

__device__ __forceinline__ uint32_t pd_word(uint32_t node, uint32_t lo, uint32_t hi) {
  return node | (lo << 14) | (hi << 23);
}

}  // namespace

template <typename CT>
__global__ __launch_bounds__(kPdThreads) void k_pd_count(PdCountArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const PdGroup g = A.groups[blockIdx.y];
  const int G = A.G, Gp = G + 1;
  const int pitch = A.S * (int)sizeof(CT) + 4;
  unsigned char* rows = smem;
  PNode* nodes = (PNode*)(smem + A.tile_bytes);
  int32_t* diff = (int32_t*)(nodes + g.nn);  // [g.nl][Gp]
  for (int i = tid; i < g.nn; i += kPdThreads) nodes[i] = A.nodes[g.n0 + i];
  for (int i = tid; i < g.nl * Gp; i += kPdThreads) diff[i] = 0;
  const int64_t ntiles = (A.N + kPdTileRows - 1) / kPdTileRows;
  const int64_t tile0 = (int64_t)blockIdx.x * A.slice_tiles;
  const int64_t tile1 = tile0 + A.slice_tiles < ntiles ? tile0 + A.slice_tiles : ntiles;
  const int rb = A.S * (int)sizeof(CT);  // bytes of one row (S is a multiple of 16)
  const int vpr = rb >> 4;               // 16-byte pieces of one row
  const int r = tid & (kPdTileRows - 1), h = tid >> 9;
  const CT* rp = (const CT*)(rows + r * pitch);
  for (int64_t tile = tile0; tile < tile1; tile++) {
    const int64_t row0 = tile * kPdTileRows;
    block_sync();  // the nodes and the zeroed table are written; the previous tile is walked
    for (int q = tid; q < kPdTileRows * vpr; q += kPdThreads) {
      const int rr = q / vpr, w = q - rr * vpr;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (row0 + rr < A.N) v = *(const uint4*)((const unsigned char*)A.codes + (row0 + rr) * rb + w * 16);
      uint32_t* d = (uint32_t*)(rows + rr * pitch + w * 16);
      d[0] = v.x;
      d[1] = v.y;
      d[2] = v.z;
      d[3] = v.w;
    }
    block_sync();
    if (row0 + r >= A.N) continue;  // (the barriers above are reached by every thread)
    for (int t = g.t0 + h; t < g.t1; t += kPdThreads / kPdTileRows) {
      const PNode* tn = nodes + (A.tree_node[t] - g.n0);
      uint32_t st[kPdStack];  // st[0] the top; only ever indexed by constants
#pragma unroll
      for (int k = 0; k < kPdStack; k++) st[k] = 0;
      int sp = 0;
      uint32_t node = 0, lo = 0, hi = (uint32_t)G;
      for (;;) {
        const PNode n = tn[node];
        if (n.a & 0x80000000u) {
          int32_t* d = diff + (n.a & 0x3fffffffu) * Gp;
          __hip_atomic_fetch_add(d + lo, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (hi < (uint32_t)G) __hip_atomic_fetch_add(d + hi, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (sp == 0) break;
          const uint32_t top = st[0];
#pragma unroll
          for (int k = 0; k + 1 < kPdStack; k++) st[k] = st[k + 1];
          sp--;
          node = top & 0x3fffu;
          lo = (top >> 14) & 0x1ffu;
          hi = top >> 23;
        } else if (n.a & kPdTestsFeature) {
          const uint32_t s = n.b & 0x1ffffu, c = n.a & 0x3fffu;
          const uint32_t lh = hi < s ? hi : s, rl = lo > s ? lo : s;
          const bool left = lo < lh, right = rl < hi;
          if (left && right) {  // (the host made sure that sp < kPdStack here)
#pragma unroll
            for (int k = kPdStack - 1; k > 0; k--) st[k] = st[k - 1];
            st[0] = pd_word(c + 1, rl, hi);
            sp++;
            node = c;
            hi = lh;
          } else {
            node = left ? c : c + 1;
          }
        } else {
          const uint32_t code = rp[n.b >> 17];
          node = n.a + (code < (n.b & 0x1ffffu) ? 0u : 1u);
        }
      }
    }
  }
  block_sync();  // every walk of the slice has counted
  for (int i = tid; i < g.nl; i += kPdThreads) {
    const int32_t* d = diff + i * Gp;
    unsigned long long* o = A.cnt + (g.l0 + i) * G;
    int32_t run = 0;
    for (int k = 0; k < G; k++) {
      run += d[k];
      if (run != 0)
        __hip_atomic_fetch_add(o + k, (unsigned long long)(uint32_t)run, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

void launch_pd_count(hipStream_t st, const PdCountArgs& a) {
  const int64_t ntiles = (a.N + kPdTileRows - 1) / kPdTileRows;
  const dim3 grid((unsigned)((ntiles + a.slice_tiles - 1) / a.slice_tiles), (unsigned)a.ngroups);
  const size_t lds = (size_t)a.tile_bytes + (size_t)a.group_bytes;
  if (a.code_bytes == 1) {
    pd_set_max_lds((const void*)k_pd_count<uint8_t>, 160 * 1024);
    hipLaunchKernelGGL((k_pd_count<uint8_t>), grid, dim3(kPdThreads), lds, st, a);
  } else {
    pd_set_max_lds((const void*)k_pd_count<uint16_t>, 160 * 1024);
    hipLaunchKernelGGL((k_pd_count<uint16_t>), grid, dim3(kPdThreads), lds, st, a);
  }
}

__global__ __launch_bounds__(256) void k_pd_walk(const double* __restrict__ X, const void* __restrict__ codes,
                                                 int code_bytes, const double* __restrict__ dict,
                                                 const int64_t* __restrict__ dict_off, int64_t n, int32_t F,
                                                 int32_t S, const DevNode* __restrict__ nodes,
                                                 const int64_t* __restrict__ tree_off,
                                                 const int32_t* __restrict__ jcut,
                                                 const int64_t* __restrict__ leaf_off, int L, int G,
                                                 unsigned long long* __restrict__ cnt) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  int32_t st_node[kPdMaxGrid];  // pending ranges are disjoint and non-empty: at most G - 1
  uint32_t st_rng[kPdMaxGrid];
  for (int l = 0; l < L; l++) {
    const DevNode* t = nodes + tree_off[l];
    const int32_t* jc = jcut + tree_off[l];
    int sp = 0, id = 0;
    int lo = 0, hi = G;
    for (;;) {
      if (t[id].left < 0) {
        unsigned long long* o = cnt + (leaf_off[l] + t[id].pad) * G;
        __hip_atomic_fetch_add(o + lo, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (hi < G) __hip_atomic_fetch_add(o + hi, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (sp == 0) break;
        sp--;
        id = st_node[sp];
        lo = (int)(st_rng[sp] & 0xffffu);
        hi = (int)(st_rng[sp] >> 16);
        continue;
      }
      const int s = jc[id];
      if (s >= 0) {
        const int lh = hi < s ? hi : s, rl = lo > s ? lo : s;
        const bool left = lo < lh, right = rl < hi;
        if (left && right) {
          st_node[sp] = t[id].right;
          st_rng[sp] = (uint32_t)rl | ((uint32_t)hi << 16);
          sp++;
          id = t[id].left;
          hi = lh;
        } else {
          id = left ? t[id].left : t[id].right;
        }
        continue;
      }
      const int gf = t[id].gfeat;
      double v;
      if (X) {
        v = X[row * F + gf];
      } else {
        const int64_t c = code_bytes == 1   ? (int64_t)((const uint8_t*)codes)[row * S + gf]
                          : code_bytes == 2 ? (int64_t)((const uint16_t*)codes)[row * S + gf]
                                            : (int64_t)((const uint32_t*)codes)[row * S + gf];
        v = dict[dict_off[gf] + c];
      }
      id = (v <= t[id].value) ? t[id].left : t[id].right;
    }
  }
}

void launch_pd_walk(hipStream_t st, const double* X, const void* codes, int code_bytes, const double* dict,
                    const int64_t* dict_off, int64_t n, int32_t F, int32_t S, const DevNode* nodes,
                    const int64_t* tree_off, const int32_t* jcut, const int64_t* leaf_off, int L, int G,
                    unsigned long long* cnt) {
  hipLaunchKernelGGL(k_pd_walk, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, X, codes, code_bytes,
                     dict, dict_off, n, F, S, nodes, tree_off, jcut, leaf_off, L, G, cnt);
}

// differences -> counts, a thread per leaf
__global__ __launch_bounds__(256) void k_pd_prefix(unsigned long long* __restrict__ cnt, int64_t leaves, int G) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= leaves) return;
  unsigned long long run = 0;
  for (int k = 0; k < G; k++) {
    run += cnt[i * G + k];
    cnt[i * G + k] = run;
  }
}

void launch_pd_prefix(hipStream_t st, unsigned long long* cnt, int64_t leaves, int G) {
  hipLaunchKernelGGL(k_pd_prefix, dim3((unsigned)((leaves + 255) / 256)), dim3(256), 0, st, cnt, leaves, G);
}

__global__ __launch_bounds__(256) void k_pd_zero(unsigned long long* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0;
}

void launch_pd_zero(hipStream_t st, unsigned long long* p, int64_t n) {
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_pd_zero, dim3((unsigned)(blocks < 4096 ? (blocks > 0 ? blocks : 1) : 4096)), dim3(256), 0,
                     st, p, n);
}

// A workgroup folds 32 grid points: thread (tl, gl) takes grid point 32 blockIdx.x + gl and the
// trees tl, tl + 32, ... (a wave's loads of cnt run along g), then lane tl == 0 of a grid point
// sums the trees in order.  A value another thread of the workgroup wrote is read with an
// atomic load, past the vector cache.
__global__ __launch_bounds__(1024) void k_pd_fold(PdFoldArgs A) {
  const int tid = threadIdx.x;
  const int gl = tid & 31, tl = tid >> 5;
  const int g = blockIdx.x * 32 + gl;
  const int G = A.G;
  if (!A.votes_kind) {
    if (g < G)
      for (int t = tl; t < A.L; t += 32) {
        double s = 0.0;
        for (int64_t l = A.leaf_off[t]; l < A.leaf_off[t + 1]; l++)
          s = __dadd_rn(s, __dmul_rn((double)A.cnt[l * G + g], A.leaf_val[l]));
        A.tree_pd[(int64_t)t * G + g] = __ddiv_rn(s, (double)A.N);
      }
    block_sync_mem();
    if (tl == 0 && g < G) {
      double s = 0.0;
      for (int t = 0; t < A.L; t++) {
        const double v = __longlong_as_double((long long)__hip_atomic_load(
            (const unsigned long long*)A.tree_pd + (int64_t)t * G + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        s = __dadd_rn(s, A.weights ? __dmul_rn(v, A.weights[t]) : v);
      }
      A.out[g] = A.weights ? s : __ddiv_rn(s, (double)A.L);
    }
  } else {
    const int C = A.C;
    if (g < G)
      for (int t = tl; t < A.L; t += 32)
        for (int64_t l = A.leaf_off[t]; l < A.leaf_off[t + 1]; l++) {
          const unsigned long long c = A.cnt[l * G + g];
          if (c)
            __hip_atomic_fetch_add(A.votes + (int64_t)g * C + (int)A.leaf_val[l], c, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    block_sync_mem();
    const double den = __dmul_rn((double)A.N, (double)A.L);
    for (int64_t i = tid; i < (int64_t)32 * C; i += 1024) {
      const int64_t gg = (int64_t)blockIdx.x * 32 + i / C;
      if (gg >= G) break;
      const int64_t at = gg * C + i % C;
      A.out[at] = __ddiv_rn(
          (double)__hip_atomic_load(A.votes + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), den);
    }
  }
}

void launch_pd_fold(hipStream_t st, const PdFoldArgs& a) {
  hipLaunchKernelGGL(k_pd_fold, dim3((unsigned)((a.G + 31) / 32)), dim3(1024), 0, st, a);
}

}  // namespace sbag
