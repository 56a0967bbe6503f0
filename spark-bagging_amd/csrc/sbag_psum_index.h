// Which entry of its run a lane of k_fb_psum (sbag_f64s.hip) loads: pure integer arithmetic,
// no HIP, so that tests/c/psum_index_check.cpp can sweep it in a program of its own.
//
// A wave sums R runs side by side.  A step holds kPsumRounds rounds of 64 entries, kPsumRounds
// / R of them per run; round q of a run at step st has lane l at position
// st * 64 * rounds_per_run + 64 * q + l of the run.  Every run of the wave walks as many steps
// as the longest one, so positions at and past a run's length come up all the time, and a run
// (task, partition) may be empty.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBAG_HD __host__ __device__
#else
#define SBAG_HD
#endif

constexpr int kPsumRounds = 8;  // rounds of 64 entries per step

struct PsumSlot {
  int32_t load;  // the run's entry to load (bin word, carried label, entry word), in
                 // [0, len): the position, clamped to the run's last entry so that the load
                 // needs no branch inside a run.  -1: nothing to load (an empty run has no entry
                 // of its own, and its base may be the end of its replica's list)
  bool valid;    // the position is an entry of the run: only then is the loaded entry summed,
                 // and only then may its row index be used to gather a label
};

// len: the run's entries (< 2^31); st < max(1, ceil(len_longest / (64 * rounds_per_run))) with
// len_longest < 2^31 the wave's longest run; q in [0, rounds_per_run); lane in [0, 64).  The
// position then stays below 2^31: the last step ends at len_longest rounded up to the step.
SBAG_HD inline PsumSlot psum_slot(int32_t st, int q, int lane, int32_t len, int rounds_per_run) {
  const int32_t pos = st * (64 * rounds_per_run) + 64 * q + lane;
  PsumSlot s;
  s.valid = pos < len;
  s.load = len > 0 ? (s.valid ? pos : len - 1) : -1;
  return s;
}
