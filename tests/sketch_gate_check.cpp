// The gate of the sketch tiers (vettore_amd/csrc/host/vt_sketchtiers.h) is plain C++: built here with g++ under
// AddressSanitizer and UBSan.  sketch_tiers_wanted goes by one table row per tier; the reference below states the four
// predicates one by one, each calling the one before it, as the library had them before the table.  The two must agree on
// the full product of metric family, the four settings, every mask of refused columns and of passes that fit, the limits
// either side of every tier's bound and the row bytes either side of every cut -- for a ranked shard with rows of 768
// dimensions, and with each of the gate's other conditions broken one at a time -- and the mask must be nested everywhere.
#include "../vettore_amd/csrc/host/vt_sketchtiers.h"

#include <cstdio>

using namespace vt_host;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (failures < 20) {                                \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__);  \
        std::printf(__VA_ARGS__);                         \
        std::printf("\n");                                \
      }                                                   \
      ++failures;                                         \
    }                                                     \
  } while (0)

static const double kMiB = 1024.0 * 1024.0, kGiB = 1024.0 * kMiB;

static bool w8(const SketchGateShape &s, size_t limit) {
  const bool dot = s.family == kSketchDot, l2 = s.family == kSketchL2;
  if (s.sketch == 0 || s.refused[kTier8] || !(dot || l2) || s.single_nominate) return false;
  if (!s.ranks_clean || s.no_rows || s.dim <= 0 || s.dim > 32768) return false;
  if (limit == 0 || std::max<size_t>(2 * limit, limit + 16) > 256 || !s.pass_fits[kTier8]) return false;
  return s.force_sketch != 0 || s.force_sketch6 != 0 || s.row_bytes >= (l2 ? 1.0 * kGiB : 256.0 * kMiB);
}
static bool w6(const SketchGateShape &s, size_t limit) {
  if (!w8(s, limit) || s.family != kSketchDot || limit > 32 || s.sketch6 == 0 || s.refused[kTier6]) return false;
  if (!s.pass_fits[kTier6]) return false;
  return s.force_sketch6 != 0 || s.row_bytes >= 16.0 * kGiB;
}
static bool w5(const SketchGateShape &s, size_t limit) {
  if (!w6(s, limit) || limit > 10 || s.sketch6 == 2 || s.refused[kTier5]) return false;
  if (!s.pass_fits[kTier5]) return false;
  return s.force_sketch6 >= 2 || s.row_bytes >= 16.0 * kGiB;
}
static bool w4(const SketchGateShape &s, size_t limit) {
  if (!w5(s, limit) || limit > 10 || s.sketch6 == 3 || s.refused[kTier4]) return false;
  if (!s.pass_fits[kTier4]) return false;
  return s.force_sketch6 >= 3 || s.row_bytes >= 16.0 * kGiB;
}

static unsigned long long cases = 0;
static unsigned seen = 0;  // every mask met at least once

// the whole product over one base shape (what `base` sets of rank, single_nominate, rows and dim stays)
static void sweep(const SketchGateShape &base, const char *name) {
  const size_t limits[] = {0, 1, 10, 11, 32, 33, 128, 129};
  const double row_bytes[] = {256.0 * kMiB - 4, 256.0 * kMiB, kGiB - 4, kGiB, 16.0 * kGiB - 4, 16.0 * kGiB};
  for (int family = 0; family < 3; ++family)
    for (long sketch = 0; sketch <= 2; ++sketch)
      for (long sketch6 = 0; sketch6 <= 3; ++sketch6)
        for (long force = 0; force <= 2; ++force)
          for (long force6 = 0; force6 <= 3; ++force6)
            for (unsigned refused = 0; refused < 16; ++refused)
              for (unsigned fits = 0; fits < 16; ++fits)
                for (double bytes : row_bytes) {
                  SketchGateShape s = base;
                  s.family = family == 0 ? kSketchDot : family == 1 ? kSketchL2 : kSketchNoFamily;
                  s.sketch = sketch;
                  s.sketch6 = sketch6;
                  s.force_sketch = force;
                  s.force_sketch6 = force6;
                  s.row_bytes = bytes;
                  for (int t = 0; t < kSketchTierCount; ++t) {
                    s.refused[t] = (refused >> t & 1u) != 0;
                    s.pass_fits[t] = (fits >> t & 1u) != 0;
                  }
                  for (size_t limit : limits) {
                    const unsigned want = (w4(s, limit) ? 1u << kTier4 : 0u) | (w5(s, limit) ? 1u << kTier5 : 0u) |
                                          (w6(s, limit) ? 1u << kTier6 : 0u) | (w8(s, limit) ? 1u << kTier8 : 0u);
                    const unsigned got = sketch_tiers_wanted(s, limit);
                    CHECK(got == want,
                          "%s: family %d sketch %ld sketch6 %ld force %ld force6 %ld refused %x fits %x bytes %.0f limit %zu: mask %x, "
                          "the four predicates say %x",
                          name, family, sketch, sketch6, force, force6, refused, fits, bytes, limit, got, want);
                    // 4 within 5 within 6 within int8
                    CHECK(got == 0u || got == 8u || got == 12u || got == 14u || got == 15u, "%s: mask %x is not nested", name, got);
                    seen |= 1u << got;
                    ++cases;
                  }
                }
}

int main() {
  static_assert(kTier4 == 0 && kTier5 == 1 && kTier6 == 2 && kTier8 == 3 && kSketchTierCount == 4, "narrowest first");
  SketchGateShape base;
  base.ranks_clean = true;
  base.single_nominate = false;
  base.no_rows = false;
  base.dim = 768;
  sweep(base, "ranked, rows of 768");
  CHECK(seen == ((1u << 0) | (1u << 8) | (1u << 12) | (1u << 14) | (1u << 15)), "masks met: %x", seen);
  SketchGateShape s = base;
  s.ranks_clean = false;
  sweep(s, "not ranked");
  s = base;
  s.single_nominate = true;
  sweep(s, "single_nominate");
  s = base;
  s.no_rows = true;
  sweep(s, "no rows");
  s = base;
  s.dim = 0;
  sweep(s, "dim 0");
  s = base;
  s.dim = 32768;
  sweep(s, "dim 32768");
  s = base;
  s.dim = 32769;
  sweep(s, "dim 32769");
  if (failures) {
    std::printf("%d failures in %llu cases\n", failures, cases);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
