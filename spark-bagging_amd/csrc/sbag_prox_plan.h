// sbag_prox_plan.h — host arithmetic of the forest proximities (sbag_host.cpp, sbag_prox.hip):
// the width and padding of a row's leaf signature, the row tile of k_leaf_tiled, the block tile
// and K chunk of k_prox_tiled, the query batches and the group-ordered column blocks of the
// moments.  Plain host code with no HIP in it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sbag {

constexpr int kProxMaxTrees = 65535;   // a pair count is a u16
constexpr int kProxMaxLeaves = 65536;  // a leaf code is at most a u16
constexpr int kProxMaxGroups = 16;

// k_prox_tiled: 256 threads as 16 x 16, a thread owns kProxTM x kProxTN pairs (rows ty + 16 a,
// columns tx + 16 b), a block kProxBM x kProxBN pairs; both signature tiles are staged in K
// chunks of kProxKC bytes a row at a pitch of kProxKC + 16 bytes.  The pitch is 36 dwords: the
// 16 consecutive rows a wave reads with one ds_read_b128 start at dword 36 r, that is bank
// group (9 r) mod 16 of the 16 groups of four banks, all distinct, so the read is conflict free
// (at a pitch of 32 dwords rows r and r + 2 would share their banks).
constexpr int kProxThreads = 256;
constexpr int kProxTM = 8, kProxTN = 8;
constexpr int kProxBM = 16 * kProxTM, kProxBN = 16 * kProxTN;
constexpr int kProxKC = 128;
constexpr int kProxPitch = kProxKC + 16;
constexpr size_t kProxTileLds = (size_t)(kProxBM + kProxBN) * kProxPitch;
// counts mode stages the block's u16 counts [kProxBM][kProxBN + 2] in the tiles' place
static_assert((size_t)kProxBM * (kProxBN + 2) * 2 <= kProxTileLds, "the count tile fits the signature tiles");
// moments mode: a lane's sum of counts over its kProxTN columns and a row's sum over the
// block's kProxBN columns are u32; a count is at most kProxMaxTrees.  Sums of squares and
// everything kept across column blocks are u64.
static_assert((uint64_t)kProxBN * kProxMaxTrees < ((uint64_t)1 << 32), "a column block's sum of counts fits a u32");
// a pair's difference count is a u32: at most one per code of the padded signature
static_assert((uint64_t)kProxMaxTrees + 16 < ((uint64_t)1 << 32), "a difference count fits a u32");

constexpr size_t kProxLdsCap = 160 * 1024 - 512;  // = plan_tiled's bound
constexpr size_t kProxMinChunk = 4096;            // = plan_tiled's smallest chunk

// bytes of a leaf code: u8 while code 0xFF is the 256th leaf of the largest tree, else u16
inline int prox_code_bytes(int64_t max_leaves) { return max_leaves <= 256 ? 1 : 2; }
// bytes of a row's signature: the trees' codes and zero padding to 16 bytes
inline int prox_tpad(int L, int code_bytes) { return std::max(16, (L * code_bytes + 15) & ~15); }
// LDS of k_leaf_tiled's signature tile: R rows at tpad + 4 bytes (an odd dword pitch for the
// walk's stores, which run along the rows)
inline size_t prox_sig_lds(int tpad, int R) { return ((size_t)R * (tpad + 4) + 15) & ~(size_t)15; }
// the row tile of k_leaf_tiled: the largest of 512, 256, 128, 64 whose rows (at `pitch` bytes),
// signature tile and a chunk of at least 4 KB fit the LDS; 0: none does
inline int prox_tile_rows(int pitch, int tpad) {
  for (int R = 512; R >= 64; R >>= 1)
    if ((size_t)R * pitch + prox_sig_lds(tpad, R) + kProxMinChunk <= kProxLdsCap) return R;
  return 0;
}

// query rows of a batch.  Counts: each of the two device buffers and the two pinned staging
// buffers holds one batch of u16 [rows][nr], about 16 MB, never less than one block row.
// Moments: 64 MB of signatures at most, 65 536 rows at most (512 block rows).
inline int64_t prox_batch_counts(int64_t nr, int tpad) {
  const int64_t by_out = ((int64_t)16 << 20) / (2 * std::max<int64_t>(nr, 1));
  const int64_t by_sig = ((int64_t)64 << 20) / tpad;
  return std::max<int64_t>(kProxBM, std::min<int64_t>({by_out, by_sig, 65536}) / kProxBM * kProxBM);
}
inline int64_t prox_batch_moments(int tpad) {
  return std::max<int64_t>(kProxBM, std::min<int64_t>(((int64_t)64 << 20) / tpad, 65536) / kProxBM * kProxBM);
}

// ---- top-k mode (k_prox_topk).  A key is cnt << 32 | ~j: larger count first, among equal counts
// the smaller j; j < 2^31, so a key of a pair is never 0 and 0 stands for "no entry".  Beside
// the two signature tiles a block holds, per query row of its tile, a list of k keys (descending),
// a staging area of kTopkStage keys, the area's fill count and the row's filter bound (u32
// each): kProxTileLds + prox_topk_lds(k) bytes, the second part dynamic and sized from k.
//   k <= 26: 36 864 + 44 032 = 80 896 B at most, two blocks a CU (the staging area alone
//            is 16 KB, so no k reaches three)
//   k <= 64: 36 864 + 82 944 = 119 808 B at most, one block a CU
constexpr int kTopkMaxK = 64;
constexpr int kTopkStage = 16;
constexpr size_t prox_topk_lds(int k) { return (size_t)kProxBM * ((size_t)(k + kTopkStage) * 8 + 8); }
static_assert(kProxTileLds + prox_topk_lds(26) <= (160 * 1024) / 2, "k <= 26: two blocks a CU");
static_assert(kProxTileLds + prox_topk_lds(kTopkMaxK) <= kProxLdsCap, "the largest k fits the LDS");
static_assert(kTopkMaxK <= 64 && kTopkStage <= 64, "a merge holds one list entry and one staged key a lane");
static_assert(kProxMaxTrees < (1 << 16), "a key's count is stored as a u16");
// the column blocks one block of k_prox_topk takes in a row: `forced` (SBAG_PROX_TOPK_RUN) if
// positive, else enough runs to fill the device (as moments mode: 2048 blocks a launch)
inline int32_t prox_topk_run(int64_t row_blocks, int64_t nblocks, int64_t forced) {
  if (forced > 0) return (int32_t)std::min<int64_t>(forced, std::max<int64_t>(nblocks, 1));
  const int64_t xs = std::max<int64_t>(1, std::min<int64_t>(nblocks, (2048 + row_blocks - 1) / row_blocks));
  return (int32_t)((nblocks + xs - 1) / xs);
}
// query rows of a batch: 64 MB of signatures at most, 32 768 rows at most (256 block rows), so
// that the partial lists [rows][runs][k] of a launch of at most 2048 + 256 blocks stay below
// 128 x 2304 x 64 x 8 B = 151 MB
inline int64_t prox_batch_topk(int tpad) {
  return std::max<int64_t>(kProxBM, std::min<int64_t>(((int64_t)64 << 20) / tpad, 32768) / kProxBM * kProxBM);
}

struct ProxColBlock {  // columns [col0, col0 + ncols) of the ordered reference rows, ncols <= kProxBN
  int32_t col0, ncols, group, pad;
};

// the reference rows ordered by group (stable), and the column blocks: no block spans two groups
inline void prox_group_blocks(const int32_t* ref_group, int64_t nr, int G, std::vector<int64_t>& perm,
                              std::vector<ProxColBlock>& blocks) {
  std::vector<int64_t> start(G + 1, 0);
  for (int64_t j = 0; j < nr; j++) start[ref_group[j] + 1]++;
  for (int g = 0; g < G; g++) start[g + 1] += start[g];
  perm.assign((size_t)nr, 0);
  std::vector<int64_t> at(start.begin(), start.end() - 1);
  for (int64_t j = 0; j < nr; j++) perm[(size_t)at[ref_group[j]]++] = j;
  blocks.clear();
  for (int g = 0; g < G; g++)
    for (int64_t c = start[g]; c < start[g + 1]; c += kProxBN)
      blocks.push_back(ProxColBlock{(int32_t)c, (int32_t)std::min<int64_t>(kProxBN, start[g + 1] - c), g, 0});
}

}  // namespace sbag
