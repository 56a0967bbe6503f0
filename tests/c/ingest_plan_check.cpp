// Host check of sbag_ingest_plan.h: the key order is `<` on a list of edge doubles and key
// equality is `==`, the transform inverts exactly (-0.0 to 0.0), no value's key is the empty
// slot's, and the tiles' LDS stays within the budget for F in {1, 100, 1000}.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "sbag_ingest_plan.h"

using namespace sbag;

static long cases = 0, failures = 0;
#define CHECK(x)                                            \
  do {                                                      \
    cases++;                                                \
    if (!(x)) {                                             \
      failures++;                                           \
      std::printf("FAILED line %d: %s\n", __LINE__, #x);    \
    }                                                       \
  } while (0)

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  const double den = std::numeric_limits<double>::denorm_min();
  std::vector<double> v = {-inf, -1e308, -2.0, -std::nextafter(1.0, 2.0), -1.0, -2.2250738585072014e-308, -den, -0.0,
                           0.0,  den,    2.2250738585072014e-308, 0.5, 1.0, std::nextafter(1.0, 2.0), 2.0, 1e308, inf};
  for (size_t i = 0; i < v.size(); i++) {
    const uint64_t ki = ingest_key(v[i]);
    CHECK(ki != kIngestEmpty);
    const double back = ingest_value(ki);
    CHECK(back == v[i] && !std::signbit(back) == !(v[i] < 0.0));  // exact; -0.0 comes back as +0.0
    CHECK(ingest_slot(ki) < kIngestSlots);
    uint64_t bits;
    std::memcpy(&bits, &v[i], 8);
    CHECK(!ingest_bits_nan(bits));
    for (size_t j = 0; j < v.size(); j++) {
      CHECK((ki < ingest_key(v[j])) == (v[i] < v[j]));
      CHECK((ki == ingest_key(v[j])) == (v[i] == v[j]));
    }
  }
  for (uint64_t nan : {0x7ff8000000000000ull, 0xfff8000000000000ull, 0x7ff0000000000001ull, 0x7fffffffffffffffull,
                       0xffffffffffffffffull})
    CHECK(ingest_bits_nan(nan));
  CHECK(ingest_key_bits(0x7fffffffffffffffull) == kIngestEmpty);
  for (int F : {1, 100, 1000}) {
    const int S = F <= 64 ? (F + 15) / 16 * 16 : (F + 127) / 128 * 128;  // row_stride
    CHECK(ingest_distinct_lds(true) <= kIngestLdsCap && ingest_distinct_lds(false) <= kIngestLdsCap);
    for (int cb : {1, 2}) {
      const int R = ingest_encode_rows(S, cb);
      CHECK(R >= 1 && (R & (R - 1)) == 0 && R <= kIngestTileRows);
      CHECK(ingest_encode_lds(S, cb, R, kIngestArenaKeys) + 8 <= kIngestLdsCap);
    }
    CHECK(ingest_set_group(F) >= 1 && (size_t)ingest_set_group(F) * kIngestSetBytes <= kIngestSetBudget);
    for (int elt : {1, 4, 8})
      for (int64_t N : {(int64_t)1, (int64_t)4500, (int64_t)10000000}) {
        const int64_t b = ingest_batch_rows(N, F, elt, 0);
        CHECK(b >= 1 && b <= N && (b == N || b % kIngestTileRows == 0));
        CHECK(ingest_batch_stride(b, F, elt) % 256 == 0 && ingest_batch_stride(b, F, elt) >= (size_t)b * F * elt);
        CHECK(ingest_batch_rows(N, F, elt, 1000) == (N < 1000 ? N : b < 1000 ? b : 1000));
        CHECK(ingest_distinct_tiles_per_wg(b, F) >= 1);
      }
  }
  CHECK(ingest_pad(1) == 1 && ingest_pad(5) == 8 && ingest_pad(256) == 256);
  std::printf("ingest_plan_check: %ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
