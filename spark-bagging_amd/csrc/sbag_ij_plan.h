// sbag_ij_plan.h — arithmetic shared by the host and the kernels of the infinitesimal-jackknife
// variance (sbag_host.cpp, sbag_ij.hip): how the bags' Gram matrix is split over workgroups and
// the row tile of k_ij_tiled.  No HIP in it beyond the host / device marker.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBAG_IJ_HD __host__ __device__
#else
#define SBAG_IJ_HD
#endif

namespace sbag {

constexpr int kIjMaxTrees = 1024;
constexpr int kIjTileRows = 256;  // the largest row tile of k_ij_tiled
constexpr int kIjGroup = 4;       // chains s_a a lane keeps in registers
constexpr size_t kIjLdsCap = 160 * 1024 - 512;  // = plan_tiled's bound
constexpr size_t kIjMinChunk = 4096;            // = plan_tiled's smallest chunk

// the fp64 matrix [T][R] of a tile: t_b, then d_b, then d_a * u_a in place
inline size_t ij_matrix_lds(int T, int R) { return (size_t)T * R * 8; }

// the row tile of k_ij_tiled: the largest of 256, 128, 64, 32 whose rows (at `pitch` bytes),
// matrix and a chunk of at least 4 KB fit the LDS; 0: none does
inline int ij_tile_rows(int pitch, int T) {
  for (int R = kIjTileRows; R >= 32; R >>= 1)
    if ((size_t)R * pitch + ij_matrix_lds(T, R) + kIjMinChunk <= kIjLdsCap) return R;
  return 0;
}

// ---- the Gram matrix of the bag counts.  A workgroup stages 256 learner rows of a 256-row
// chunk (pitch 272 bytes as k_hist_mfma's) and owns 32 x 32 learner-tile pairs of the lower
// triangle.  T <= 256: one block of 256 learners, one unit, every pair.  Above: blocks of 128
// learners, a unit per block pair (I, J), I >= J: the diagonal units stage one block (LDS tiles
// 0..3), the others two (block I in tiles 0..3, block J in tiles 4..7).
constexpr int kGramMaxLearners = 1024;
constexpr int kGramChunk = 256;
constexpr int kGramPitch = kGramChunk + 16;
constexpr int kGramLdsRows = 256;
constexpr int kGramWaves = 8;
constexpr int kGramPairs = 5;               // pairs a wave holds: 36 pairs over 8 waves
constexpr int64_t kGramSliceMfma = 65536;   // 127 * 127 * 65536 < 2^31
constexpr int64_t kGramSliceDot = 32768;    // 255 * 255 * 32768 < 2^31

SBAG_IJ_HD inline int gram_block(int T) { return T <= 256 ? 256 : 128; }
SBAG_IJ_HD inline int gram_blocks(int T) { return (T + gram_block(T) - 1) / gram_block(T); }
SBAG_IJ_HD inline int gram_units(int T) { return gram_blocks(T) * (gram_blocks(T) + 1) / 2; }
// unit u -> (I, J), I >= J, row by row of the lower triangle
SBAG_IJ_HD inline void gram_unit(int u, int& I, int& J) {
  I = 0;
  while ((I + 1) * (I + 2) / 2 <= u) I++;
  J = u - I * (I + 1) / 2;
}
// the learner tiles (of 32) block I holds
SBAG_IJ_HD inline int gram_block_tiles(int T, int I) {
  const int left = T - I * gram_block(T), cap = gram_block(T) / 32;
  const int nt = (left + 31) / 32;
  return nt < cap ? nt : cap;
}
// tile pairs of unit (I, J)
SBAG_IJ_HD inline int gram_unit_pairs(int T, int I, int J) {
  const int nx = gram_block_tiles(T, I);
  return I == J ? nx * (nx + 1) / 2 : nx * 4;
}
// pair k of unit (I, J) -> LDS tiles (x, y); x's learners are not below y's
SBAG_IJ_HD inline void gram_pair(int I, int J, int k, int& x, int& y) {
  if (I == J) {
    x = 0;
    while ((x + 1) * (x + 2) / 2 <= k) x++;
    y = k - x * (x + 1) / 2;
  } else {
    x = k >> 2;
    y = 4 + (k & 3);
  }
}
// the first learner of LDS tile x of unit (I, J)
SBAG_IJ_HD inline int gram_tile_learner(int T, int I, int J, int x) {
  return I == J ? I * gram_block(T) + 32 * x : (x < 4 ? I * 128 + 32 * x : J * 128 + 32 * (x - 4));
}

}  // namespace sbag
