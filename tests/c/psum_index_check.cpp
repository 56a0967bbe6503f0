// Sweep of psum_slot (spark-bagging_amd/csrc/sbag_psum_index.h), the rule by which a lane of
// k_fb_psum picks the entry of its run to load: for every R the kernel is instantiated for, every
// run length 0..1100 and a few near 2^31 - 1, every step (those of the run, and the further ones
// a longer run of the same wave makes it walk), round and lane.
//   * a load index is in [0, len) -- read here from a heap array of exactly len bytes, so that
//     ASan sees a stray index too;
//   * an empty run loads nothing, on any lane;
//   * only a valid lane's entry may be used (its row index gathers a label): a valid lane loads
//     its own position, and the valid (step, round, lane) triples, in that order, load the
//     entries 0, 1, ..., len - 1: each exactly once.
// The runs near 2^31 - 1 take all 64 lanes in the first two steps, the last three and those past
// the end (the rule is affine in the step: clamping and 32-bit overflow can only go wrong at the
// ends; UBSan watches the arithmetic); two of them also walk every step between with lanes 0
// and 63 of every round, the others every 4099th.
// Built and run by tests/test_psum_index_host.py (plain and under ASan/UBSan).
// Exit status 0 and a last line "psum_index_check: N cases (...), 0 failures" when all holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sbag_psum_index.h"

static long long failures = 0, cases = 0, slots = 0, no_loads = 0, clamped = 0;

static void fail(const char* what, int R, int32_t len, int32_t st, int q, int lane, const PsumSlot& s) {
  if (failures++ < 25)
    fprintf(stderr, "FAIL %s: R %d len %d step %d round %d lane %d -> load %d valid %d\n", what, R, len, st,
            q, lane, s.load, (int)s.valid);
}

// the properties of one slot that need no neighbour; returns false when the slot must not be used
static bool check_slot(int R, int32_t len, int32_t st, int q, int lane, const PsumSlot& s) {
  slots++;
  bool ok = true;
  if (len == 0) {
    if (s.load != -1) fail("an empty run loads", R, len, st, q, lane, s), ok = false;
    if (s.valid) fail("an empty run has a valid lane", R, len, st, q, lane, s), ok = false;
    no_loads++;
    return ok;
  }
  if (s.load < 0 || s.load >= len) fail("load index outside [0, len)", R, len, st, q, lane, s), ok = false;
  if (!s.valid) clamped++;
  return ok;
}

// every step, round and lane of a run of len entries walked for `steps` steps
static void sweep_all(int R, int32_t len, int32_t steps) {
  const int kRu = kPsumRounds / R;
  cases++;
  std::vector<uint8_t> entries((size_t)len), seen((size_t)len, 0);  // (len 0: no storage at all)
  for (int32_t i = 0; i < len; i++) entries[(size_t)i] = (uint8_t)(i * 7 + 1);
  int64_t next = 0;  // the entry the next valid triple has to load
  unsigned sink = 0;
  for (int32_t st = 0; st < steps; st++)
    for (int q = 0; q < kRu; q++)
      for (int lane = 0; lane < 64; lane++) {
        const PsumSlot s = psum_slot(st, q, lane, len, kRu);
        if (!check_slot(R, len, st, q, lane, s) || s.load < 0) continue;
        sink += entries.data()[s.load];  // the kernel's unconditional load inside a run
        if (!s.valid) continue;
        if (s.load != next) fail("valid lanes do not load 0, 1, ... in order", R, len, st, q, lane, s);
        seen[(size_t)s.load]++;  // the gather: valid lanes only
        next++;
      }
  for (int32_t i = 0; i < len; i++)
    if (seen[(size_t)i] != 1) {
      PsumSlot none{i, false};
      fail("entry not covered exactly once (load = the entry)", R, len, -1, -1, -1, none);
    }
  if (next != len) {
    PsumSlot none{(int32_t)next, false};
    fail("valid triples != len (load = their number)", R, len, -1, -1, -1, none);
  }
  if (sink == 0xFFFFFFFFu) puts("");  // (keeps the reads)
}

// a run near 2^31 - 1: all lanes at both ends, lanes 0 and 63 of the steps between (every one of
// them, or every 4099th)
static void sweep_long(int R, int32_t len, bool every_step) {
  const int kRu = kPsumRounds / R;
  const int32_t own = (int32_t)(((int64_t)len + 64 * kRu - 1) / (64 * kRu));
  // (the wave's longest run is < 2^31 too: at most one more step when len's last step is full)
  const int32_t steps = (int32_t)(((int64_t)INT32_MAX + 64 * kRu - 1) / (64 * kRu));
  cases++;
  int64_t next = 0;
  for (int32_t st = 0; st < steps; st++) {
    const bool all = st < 2 || st >= own - 3;
    if (!all && !every_step && st % 4099 != 0) {  // (skipped: a whole step inside the run)
      next += 64 * kRu;
      continue;
    }
    for (int q = 0; q < kRu; q++) {
      if (all) {
        for (int lane = 0; lane < 64; lane++) {
          const PsumSlot s = psum_slot(st, q, lane, len, kRu);
          if (!check_slot(R, len, st, q, lane, s) || !s.valid) continue;
          if (s.load != next) fail("valid lanes do not load 0, 1, ... in order", R, len, st, q, lane, s);
          next++;
        }
        continue;
      }
      const PsumSlot a = psum_slot(st, q, 0, len, kRu), b = psum_slot(st, q, 63, len, kRu);
      check_slot(R, len, st, q, 0, a);
      check_slot(R, len, st, q, 63, b);
      // (a middle step lies wholly inside the run)
      if (!a.valid || a.load != next) fail("lane 0 of a middle round", R, len, st, q, 0, a);
      if (!b.valid || b.load != next + 63) fail("lane 63 of a middle round", R, len, st, q, 63, b);
      next += 64;
    }
  }
  if (next != len) {
    PsumSlot none{(int32_t)(next & 0x7fffffff), false};
    fail("valid triples != len (load = their number)", R, len, -1, -1, -1, none);
  }
}

int main() {
  const int Rs[] = {1, 2, 4, 8};
  const int32_t longs[] = {INT32_MAX, INT32_MAX - 1, INT32_MAX - 63, INT32_MAX - 64, INT32_MAX - 511,
                           INT32_MAX - 512, INT32_MAX - 1000};  // (the first and the last: every step)
  for (int R : Rs) {
    const int kRu = kPsumRounds / R;
    for (int32_t len = 0; len <= 1100; len++) {
      const int32_t own = (len + 64 * kRu - 1) / (64 * kRu);
      // its own steps (an all-empty wave walks none), and a longer neighbour's
      const int32_t extra[] = {0, 1, 2, 5};
      for (int32_t e : extra) sweep_all(R, len, own + e);
    }
    for (int32_t len : longs) sweep_long(R, len, len == INT32_MAX || len == INT32_MAX - 1000);
  }
  printf("psum_index_check: %lld cases (%lld slots, %lld of empty runs, %lld clamped), %lld failures\n", cases,
         slots, no_loads, clamped, failures);
  return failures ? 1 : 0;
}
