// sbag_ingest.hip — the ingest on the device for gfx950 (MI355X, CDNA4): per-feature
// dictionaries of the distinct values and the [N][S] value codes, from raw feature values that
// went up as they are (sbag_ingest_plan.h holds the keys, the set geometry and the tiles).
//
//   k_ingest_distinct  discovery.  A value becomes its order-preserving u64 key and is put into
//                      its feature's open-addressed set in HBM (2^17 slots, 64-bit atomicCAS on
//                      an empty slot only; an occupied slot is read, not written).  A workgroup
//                      (4 waves) walks row tiles of 64 rows for one group of at most 64 features.
//                      Dense rows are loaded row-major, 16 bytes a lane where the row length
//                      allows, and transposed through LDS at pitch 65, so that a wave holds one
//                      feature across the 64 rows; columns are read as they lie.  In front of the
//                      set an LDS filter of 64 keys a feature remembers keys known to be in the
//                      set: with real data nearly every value is a repeat and takes no global
//                      access at all.  Feature j of the group belongs to wave j % 4 for the life
//                      of the workgroup, so no two waves share a filter row.  A NaN raises a flag
//                      by ballot; a feature whose counter passes 65 536 raises the wide flag and
//                      takes no more inserts.  The set of keys does not depend on the schedule.
//   k_ingest_compact   the occupied slots of each set to a dense list: ballot prefix, one atomic
//                      a wave.  The host sorts these (at most 65 536 a feature).
//   k_ingest_rank      sorted entry i of a feature with more than 256 values is found or put in
//                      the feature's (emptied) set and i is written to the u16 table beside it.
//   k_ingest_encode    codes.  A workgroup assembles a tile of R rows in LDS at pitch
//                      S * code_bytes + 4 (padding columns stay zero) and writes the rows whole,
//                      16 bytes a lane.  Dictionaries of at most 256 values are searched in LDS
//                      (padded to a power of two: a branch-free lower bound of at most 8 steps);
//                      larger ones by the read-only probe of the set, whose slot names the rank.
//                      Dense rows: a wave's lanes on consecutive features of a row (coalesced,
//                      no staging); columns: lanes on consecutive rows.
//
// Plain vector loads, stores and atomics only; every barrier is block_sync.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

#include "sbag_ingest_plan.h"
#include "sbag_internal.h"

namespace sbag {

namespace {

// (as sbag_spread.hip's: the dynamic-LDS cap of a kernel, once per (kernel, device))
void ingest_set_max_lds(const void* fn) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> g(mu);
  if (done.count({fn, dev})) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess)
    done.insert({fn, dev});
}

// KIND 0: dense fp64 [n][F]; 1 / 2 / 3: columns [F][n] of fp64 / fp32 / u8.  The fp64 bits.
template <int KIND>
__device__ __forceinline__ uint64_t ingest_bits(const void* __restrict__ raw, int64_t n, int F, int64_t row,
                                                int f) {
  if constexpr (KIND == 0) return ((const uint64_t*)raw)[row * F + f];
  if constexpr (KIND == 1) return ((const uint64_t*)raw)[(int64_t)f * n + row];
  if constexpr (KIND == 2) return (uint64_t)__double_as_longlong((double)((const float*)raw)[(int64_t)f * n + row]);
  return (uint64_t)__double_as_longlong((double)((const uint8_t*)raw)[(int64_t)f * n + row]);
}

// key into set [kIngestSlots]; true: the key is in the set afterwards.  At most kIngestSlots
// probes, so a set that filled up (only a wide feature's can) ends the search.
__device__ __forceinline__ bool ingest_insert(uint64_t* __restrict__ set, uint32_t* __restrict__ count,
                                              int32_t* __restrict__ flags, uint64_t key) {
  uint32_t s = ingest_slot(key);
  for (uint32_t p = 0; p < kIngestSlots; p++, s = (s + 1) & (kIngestSlots - 1)) {
    uint64_t cur = __hip_atomic_load(&set[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == key) return true;
    if (cur != kIngestEmpty) continue;
    if (__hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > kIngestMaxValues) break;
    cur = atomicCAS((unsigned long long*)&set[s], (unsigned long long)kIngestEmpty, (unsigned long long)key);
    if (cur == kIngestEmpty) {
      if (atomicAdd(count, 1u) + 1u > kIngestMaxValues) flags[1] = 1;
      return true;
    }
    if (cur == key) return true;
  }
  flags[1] = 1;
  return false;
}

}  // namespace

// grid (row chunks, feature groups of the set group).  LDS: filter [64 features][64] u64, then
// (dense) the tile [64 rows][pitch 65] u64.
template <int KIND, bool VEC>
__global__ __launch_bounds__(kIngestThreads) void k_ingest_distinct(IngestArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint64_t* filter = (uint64_t*)smem;
  uint64_t* tile = filter + kIngestFeat * kIngestFilter;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fg0 = A.f0 + (int)blockIdx.y * kIngestFeat;
  const int nf = A.f1 - fg0 < kIngestFeat ? A.f1 - fg0 : kIngestFeat;
  for (int i = tid; i < kIngestFeat * kIngestFilter; i += kIngestThreads) filter[i] = kIngestEmpty;
  block_sync();
  const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_wg;
  for (int64_t t = t0; t < t0 + A.tiles_per_wg; t++) {
    const int64_t row0 = t * kIngestTileRows;
    if (row0 >= A.n) break;
    const int nr = A.n - row0 < kIngestTileRows ? (int)(A.n - row0) : kIngestTileRows;
    if constexpr (KIND == 0) {
      block_sync();  // the previous tile has been read
      const uint64_t* X = (const uint64_t*)A.raw;
      if constexpr (VEC) {  // F, fg0 and nf even: every pair is 16-byte aligned
        const int h = nf >> 1;
        for (int idx = tid; idx < nr * h; idx += kIngestThreads) {
          const int r = idx / h, j = (idx - r * h) * 2;
          const ulonglong2 v = *(const ulonglong2*)(X + (row0 + r) * A.F + fg0 + j);
          tile[r * kIngestPitch + j] = v.x;
          tile[r * kIngestPitch + j + 1] = v.y;
        }
      } else {
        for (int idx = tid; idx < nr * nf; idx += kIngestThreads) {
          const int r = idx / nf, j = idx - r * nf;
          tile[r * kIngestPitch + j] = X[(row0 + r) * A.F + fg0 + j];
        }
      }
      block_sync();
    }
    const bool valid = lane < nr;
    for (int j = wave; j < nf; j += kIngestThreads / 64) {
      const int f = fg0 + j;
      uint64_t bits = 0;
      if (valid) {
        if constexpr (KIND == 0)
          bits = tile[lane * kIngestPitch + j];
        else
          bits = ingest_bits<KIND>(A.raw, A.n, A.F, row0 + lane, f);
      }
      const bool nan = ingest_bits_nan(bits);
      if (__ballot(nan) != 0ull && lane == 0) A.flags[0] = 1;
      const bool wide = __hip_atomic_load(&A.counts[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > kIngestMaxValues;
      if (valid && !nan && !wide) {
        const uint64_t key = ingest_key_bits(bits);
        uint64_t* fs = filter + j * kIngestFilter + (int)((key * 0x9E3779B97F4A7C15ull) >> 58);
        if (*fs != key && ingest_insert(A.sets + (size_t)(f - A.f0) * kIngestSlots, A.counts + f, A.flags, key))
          *fs = key;
      }
    }
  }
}

void launch_ingest_distinct(hipStream_t st, const IngestArgs& a) {
  if (a.n <= 0 || a.f1 <= a.f0) return;
  const int64_t tiles = (a.n + kIngestTileRows - 1) / kIngestTileRows;
  const dim3 grid((unsigned)((tiles + a.tiles_per_wg - 1) / a.tiles_per_wg),
                  (unsigned)ingest_feature_groups(a.f1 - a.f0));
  const size_t lds = ingest_distinct_lds(a.kind == 0);
  const bool vec = a.kind == 0 && (a.F & 1) == 0 && (a.f0 & 1) == 0;
#define SBAG_INGEST_DISTINCT(K, V)                                                         \
  do {                                                                                     \
    ingest_set_max_lds((const void*)k_ingest_distinct<K, V>);                              \
    hipLaunchKernelGGL((k_ingest_distinct<K, V>), grid, dim3(kIngestThreads), lds, st, a); \
  } while (0)
  if (a.kind == 0 && vec)
    SBAG_INGEST_DISTINCT(0, true);
  else if (a.kind == 0)
    SBAG_INGEST_DISTINCT(0, false);
  else if (a.kind == 1)
    SBAG_INGEST_DISTINCT(1, false);
  else if (a.kind == 2)
    SBAG_INGEST_DISTINCT(2, false);
  else
    SBAG_INGEST_DISTINCT(3, false);
#undef SBAG_INGEST_DISTINCT
}

// grid (kIngestSlots / 256, sets): set y's occupied slots to keys[off[y] ...), in any order;
// fill [sets] counts them (zeroed by the caller) and no key is written at or past off[y + 1]
__global__ __launch_bounds__(256) void k_ingest_compact(const uint64_t* __restrict__ sets,
                                                        const int64_t* __restrict__ off, uint32_t* __restrict__ fill,
                                                        uint64_t* __restrict__ keys) {
  const int y = blockIdx.y, lane = threadIdx.x & 63;
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  const uint64_t key = sets[(size_t)y * kIngestSlots + s];
  const bool occ = key != kIngestEmpty;
  const uint64_t mask = __ballot(occ);
  if (mask == 0ull) return;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(&fill[y], (uint32_t)__popcll(mask));
  base = __shfl(base, 0);
  const int64_t pos = off[y] + base + __popcll(mask & ((1ull << lane) - 1ull));
  if (occ && pos < off[y + 1]) keys[pos] = key;
}

void launch_ingest_compact(hipStream_t st, const uint64_t* sets, int nsets, const int64_t* off, uint32_t* fill,
                           uint64_t* keys) {
  if (nsets <= 0) return;
  hipLaunchKernelGGL(k_ingest_compact, dim3(kIngestSlots / 256, (unsigned)nsets), dim3(256), 0, st, sets, off,
                     fill, keys);
}

// grid (blocks of 256 entries, tables): table y is feature feat[y]'s; its sorted entry i (key
// dkeys[meta[f].x + i], i < meta[f].w) is found or put in sets[y] and ranks[y][slot] = i
__global__ __launch_bounds__(256) void k_ingest_rank(const uint64_t* __restrict__ dkeys, const int4* __restrict__ meta,
                                                     const int32_t* __restrict__ feat, uint64_t* __restrict__ sets,
                                                     uint16_t* __restrict__ ranks) {
  const int y = blockIdx.y;
  const int4 m = meta[feat[y]];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m.w) return;
  const uint64_t key = dkeys[(int64_t)m.x + i];
  uint64_t* set = sets + (size_t)y * kIngestSlots;
  uint32_t s = ingest_slot(key);
  for (uint32_t p = 0; p < kIngestSlots; p++, s = (s + 1) & (kIngestSlots - 1)) {
    uint64_t cur = __hip_atomic_load(&set[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kIngestEmpty)
      cur = atomicCAS((unsigned long long*)&set[s], (unsigned long long)kIngestEmpty, (unsigned long long)key);
    if (cur == kIngestEmpty || cur == key) {
      ranks[(size_t)y * kIngestSlots + s] = (uint16_t)i;
      return;
    }
  }
}

void launch_ingest_rank(hipStream_t st, const uint64_t* dkeys, const int4* meta, const int32_t* feat, int ntables,
                        uint64_t* sets, uint16_t* ranks) {
  if (ntables <= 0) return;
  hipLaunchKernelGGL(k_ingest_rank, dim3(kIngestMaxValues / 256, (unsigned)ntables), dim3(256), 0, st, dkeys, meta,
                     feat, sets, ranks);
}

// LDS: out [R][S * sizeof(CT) + 4] (rounded up to 8 bytes), then the arena of padded sorted keys.
// meta[f]: x first key in dkeys, y padded length (0: probe), z arena offset / table, w length.
template <int KIND, typename CT>
__global__ __launch_bounds__(kIngestThreads) void k_ingest_encode(IngestEncodeArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int R = A.R;
  const int rb = A.S * (int)sizeof(CT);  // bytes of a row of codes (a multiple of 16)
  const int pitch = rb + 4;
  unsigned char* out = smem;
  uint64_t* arena = (uint64_t*)(smem + (((size_t)R * pitch + 7) & ~(size_t)7));
  for (int i = tid; i < R * pitch / 4; i += kIngestThreads) ((uint32_t*)out)[i] = 0u;
  const int64_t ntiles = (A.n + R - 1) / R;
  bool staged = false;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * R;
    for (int c = 0; c < A.nchunks; c++) {
      const int2 ch = A.chunks[c];
      if (A.nchunks > 1 || !staged) {
        block_sync();  // the previous chunk's searches are done
        for (int f = ch.x + wave; f < ch.y; f += kIngestThreads / 64) {
          const int4 m = A.meta[f];
          for (int i = lane; i < m.y; i += 64) arena[m.z + i] = i < m.w ? A.dkeys[(int64_t)m.x + i] : kIngestEmpty;
        }
        staged = true;
        block_sync();
      }
      const int nfc = ch.y - ch.x;
      // dense: lanes on consecutive features of a row; columns: on consecutive rows of a feature
      const int j0 = KIND == 0 ? lane : tid / R, dj = KIND == 0 ? 64 : kIngestThreads / R;
      const int r0 = KIND == 0 ? wave : tid & (R - 1), dr = KIND == 0 ? kIngestThreads / 64 : R;
      for (int j = j0; j < nfc; j += dj) {
        const int f = ch.x + j;
        const int4 m = A.meta[f];
        for (int r = r0; r < R; r += dr) {
          if (row0 + r >= A.n) break;
          const uint64_t key = ingest_key_bits(ingest_bits<KIND>(A.raw, A.n, A.F, row0 + r, f));
          uint32_t code = 0;
          if (m.y) {
            const uint64_t* d = arena + m.z;
            for (int step = m.y >> 1; step >= 1; step >>= 1) code += d[code + step - 1] < key ? step : 0;
          } else {
            const uint64_t* set = A.sets + (size_t)m.z * kIngestSlots;
            uint32_t s = ingest_slot(key);
            for (uint32_t p = 0; p < kIngestSlots; p++, s = (s + 1) & (kIngestSlots - 1)) {
              const uint64_t cur = set[s];
              if (cur == key) {
                code = A.ranks[(size_t)m.z * kIngestSlots + s];
                break;
              }
              if (cur == kIngestEmpty) break;  // (not a value of the first pass: the rows changed)
            }
          }
          *(CT*)(out + r * pitch + f * (int)sizeof(CT)) = (CT)code;
        }
      }
    }
    block_sync();  // the tile is assembled
    const int nr = A.n - row0 < R ? (int)(A.n - row0) : R;
    const int vpr = rb >> 4;
    for (int q = tid; q < nr * vpr; q += kIngestThreads) {
      const int r = q / vpr, w = q - r * vpr;
      const uint32_t* s = (const uint32_t*)(out + r * pitch + w * 16);
      *(uint4*)((unsigned char*)A.codes + (row0 + r) * rb + w * 16) = make_uint4(s[0], s[1], s[2], s[3]);
    }
    block_sync();  // written out: the next tile may overwrite it
  }
}

void launch_ingest_encode(hipStream_t st, const IngestEncodeArgs& a, int code_bytes, int num_cus) {
  if (a.n <= 0) return;
  const int64_t ntiles = (a.n + a.R - 1) / a.R;
  const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 8;
  const dim3 grid((unsigned)(ntiles < cap ? ntiles : cap));
  const size_t lds = ingest_encode_lds(a.S, code_bytes, a.R, a.arena_keys) + 8;
#define SBAG_INGEST_ENCODE(K)                                                                       \
  do {                                                                                              \
    if (code_bytes == 1) {                                                                          \
      ingest_set_max_lds((const void*)k_ingest_encode<K, uint8_t>);                                 \
      hipLaunchKernelGGL((k_ingest_encode<K, uint8_t>), grid, dim3(kIngestThreads), lds, st, a);    \
    } else {                                                                                        \
      ingest_set_max_lds((const void*)k_ingest_encode<K, uint16_t>);                                \
      hipLaunchKernelGGL((k_ingest_encode<K, uint16_t>), grid, dim3(kIngestThreads), lds, st, a);   \
    }                                                                                               \
  } while (0)
  if (a.kind == 0)
    SBAG_INGEST_ENCODE(0);
  else if (a.kind == 1)
    SBAG_INGEST_ENCODE(1);
  else if (a.kind == 2)
    SBAG_INGEST_ENCODE(2);
  else
    SBAG_INGEST_ENCODE(3);
#undef SBAG_INGEST_ENCODE
}

}  // namespace sbag
