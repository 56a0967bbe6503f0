// sbag_ingest_plan.h — arithmetic shared by the host and the kernels of the device ingest
// (sbag_host.cpp, sbag_ingest.hip): the order-preserving key of a feature value, the geometry of
// the per-feature sets, the row tiles and the LDS they take, the batch size and the memory the
// raw values may keep.  No HIP in it beyond the host / device marker.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBAG_INGEST_HD __host__ __device__
#else
#define SBAG_INGEST_HD
#endif

namespace sbag {

// ---- keys.  bits(v) with -0.0 canonicalised; negatives have every bit flipped, the others the
// sign bit set: unsigned key order is `<` on the values and key equality is `==`.  The empty
// slot is the key of the NaN pattern 0x7fff...f, which is never inserted (a NaN fails the call).
constexpr uint64_t kIngestEmpty = ~0ull;
constexpr uint64_t kIngestSign = 1ull << 63;

SBAG_INGEST_HD inline uint64_t ingest_key_bits(uint64_t b) {
  if (b == kIngestSign) b = 0;  // -0.0 is 0.0
  return (b & kIngestSign) ? ~b : (b | kIngestSign);
}
SBAG_INGEST_HD inline bool ingest_bits_nan(uint64_t b) { return (b & ~kIngestSign) > 0x7ff0000000000000ull; }
inline uint64_t ingest_key(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return ingest_key_bits(b);
}
inline double ingest_value(uint64_t key) {
  const uint64_t b = (key & kIngestSign) ? (key & ~kIngestSign) : ~key;
  double v;
  std::memcpy(&v, &b, 8);
  return v;
}

// ---- the per-feature set: open addressing over 2^17 slots of 8 bytes (1 MiB), load <= 0.5 at
// the 65 536 values a u16 code can name; a u16 rank table [2^17] beside it for the encode.
constexpr int kIngestSlotBits = 17;
constexpr uint32_t kIngestSlots = 1u << kIngestSlotBits;
constexpr uint32_t kIngestMaxValues = 65536;  // more distinct values: u32 codes, the host ingest
constexpr size_t kIngestSetBytes = (size_t)kIngestSlots * 8;
constexpr size_t kIngestRankBytes = (size_t)kIngestSlots * 2;
constexpr size_t kIngestSetBudget = (size_t)1 << 30;  // sets alive at once: 1024 features a group

SBAG_INGEST_HD inline uint32_t ingest_slot(uint64_t key) {
  // (the keys of nearby doubles differ in their low bits: a multiplicative hash of all 64)
  return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - kIngestSlotBits));
}
inline int ingest_set_group(int F) {
  const int g = (int)(kIngestSetBudget / kIngestSetBytes);
  return F < g ? F : g;
}

// ---- k_ingest_distinct: 256 lanes, a tile of 64 rows x a group of at most 64 features; a wave a
// feature across the 64 rows.  LDS: the transposed tile (dense rows only; pitch 65 doubles) and a
// direct-mapped filter of 64 keys a feature.
constexpr int kIngestThreads = 256;
constexpr int kIngestTileRows = 64;
constexpr int kIngestFeat = 64;
constexpr int kIngestPitch = kIngestFeat + 1;
constexpr int kIngestFilter = 64;
constexpr size_t kIngestLdsCap = 160 * 1024 - 512;

inline size_t ingest_distinct_lds(bool dense) {
  return (size_t)kIngestFeat * kIngestFilter * 8 + (dense ? (size_t)kIngestTileRows * kIngestPitch * 8 : 0);
}
inline int ingest_feature_groups(int F) { return (F + kIngestFeat - 1) / kIngestFeat; }
// row tiles a workgroup of k_ingest_distinct walks (its filter lives that long): about 2048
// workgroups over the batch
inline int64_t ingest_distinct_tiles_per_wg(int64_t rows, int F) {
  const int64_t tiles = (rows + kIngestTileRows - 1) / kIngestTileRows;
  const int64_t want = 2048 / ingest_feature_groups(F) > 0 ? 2048 / ingest_feature_groups(F) : 1;
  const int64_t per = (tiles + want - 1) / want;
  return per > 0 ? per : 1;
}

// ---- k_ingest_encode: a workgroup assembles R rows of codes in LDS at pitch row_bytes + 4 and
// writes them whole.  Dictionaries of at most 256 values are searched in LDS, padded to a power of
// two with the empty key: an arena of 8192 keys, filled once when every such dictionary fits,
// else chunk of features by chunk.
constexpr int kIngestLdsDict = 256;
constexpr int kIngestArenaKeys = 8192;
constexpr size_t kIngestOutLds = 48 * 1024;

inline int ingest_pad(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}
// rows of a tile: the largest of 64, 32, ... 1 whose codes fit kIngestOutLds; 0: none does
inline int ingest_encode_rows(int S, int code_bytes) {
  for (int R = kIngestTileRows; R >= 1; R >>= 1)
    if ((size_t)R * ((size_t)S * code_bytes + 4) <= kIngestOutLds) return R;
  return 0;
}
inline size_t ingest_encode_lds(int S, int code_bytes, int R, int arena_keys) {
  return (size_t)R * ((size_t)S * code_bytes + 4) + (size_t)arena_keys * 8;
}

// ---- batches.  Raw values go up in batches of about 128 MiB (two pinned staging buffers of that
// size); a batch's device image starts at a multiple of 256 bytes.  The raw matrix stays on the
// device between the two passes when it fits beside the codes (assumed u16), the sets and a
// headroom of 1 GiB + 1/16 of the device; else every batch is uploaded twice.
constexpr size_t kIngestBatchBytes = (size_t)128 << 20;

inline int64_t ingest_batch_rows(int64_t N, int F, int elt, int64_t knob) {
  int64_t b = (int64_t)(kIngestBatchBytes / ((size_t)F * elt));
  b = b / kIngestTileRows * kIngestTileRows;
  if (b < kIngestTileRows) b = kIngestTileRows;
  if (knob > 0 && knob < b) b = knob;
  return b < N ? b : N;
}
inline size_t ingest_batch_stride(int64_t batch_rows, int F, int elt) {
  return ((size_t)batch_rows * F * elt + 255) & ~(size_t)255;
}
inline bool ingest_resident(size_t raw_bytes, size_t code_bytes_u16, size_t set_bytes, size_t free_bytes,
                            size_t total_bytes) {
  const size_t headroom = ((size_t)1 << 30) + total_bytes / 16;
  return raw_bytes + code_bytes_u16 + set_bytes + headroom <= free_bytes;
}

}  // namespace sbag
