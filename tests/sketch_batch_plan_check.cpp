// tests/sketch_batch_plan_check.cpp -- host/vt_sketchbatch.h, the host side of K1qm, against what DESIGN 4.10 says of it: the
// planner (every query once, groups of 2..G of near-equal size), the group the pass's LDS allows per row length, the
// per-query decline and the gate's truth table.  Built by tests/test_sketch_batch_plan.py with g++ under AddressSanitizer
// and UBSan.  Prints "ok".
#include "../vettore_amd/csrc/host/vt_sketchbatch.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace vt_host;

static int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("line %d: %s\n", __LINE__, #c);                  \
      if (++fails > 20) std::exit(1);                              \
    }                                                              \
  } while (0)

static void check_plan() {
  for (uint32_t gmax : {2u, 4u, 8u}) {
    for (size_t nq = 0; nq <= 40; ++nq) {
      const std::vector<uint32_t> sizes = sketch_batch_plan(nq, gmax);
      size_t sum = 0;
      uint32_t lo = ~0u, hi = 0;
      for (uint32_t s : sizes) {
        CHECK(s >= 2 && s <= gmax);
        sum += s;
        lo = std::min(lo, s);
        hi = std::max(hi, s);
      }
      if (nq < 2) {
        CHECK(sizes.empty());
        continue;
      }
      // every query once: the groups are consecutive runs of the queries, so their sizes must add up to all of them --
      // but for an odd count at G = 2, where the last query cannot have a partner
      const bool odd_pairs = gmax == 2 && nq % 2 == 1;
      CHECK(sum == (odd_pairs ? nq - 1 : nq));
      CHECK(sizes.size() == (sum + gmax - 1) / gmax);  // as few passes as G allows
      CHECK(hi - lo <= 1);                             // near-equal
    }
  }
  const std::vector<uint32_t> nine = sketch_batch_plan(9, 8);
  CHECK(nine.size() == 2 && nine[0] == 5 && nine[1] == 4);  // never 8 + 1
  const std::vector<uint32_t> seventeen = sketch_batch_plan(17, 8);
  CHECK(seventeen.size() == 3 && seventeen[0] == 6 && seventeen[1] == 6 && seventeen[2] == 5);
  CHECK(sketch_batch_plan(8, 8).size() == 1 && sketch_batch_plan(8, 8)[0] == 8);
  CHECK(sketch_batch_plan(5, 0).empty() && sketch_batch_plan(5, 1).empty());
}

static void check_lds() {
  // the formula: G images of two levels of ld8 bytes, and four 2-KiB wave buffers per query
  CHECK(sketch_batch_lds_bytes(768, 26, 8) == 8 * 2 * 768 + 8 * 4 * 2048);
  CHECK(sketch_batch_lds_bytes(100, 17, 2) == 2 * 2 * 128 + 2 * 4 * 2048);
  CHECK(sketch_batch_lds_bytes(768, 65, 8) == 0);  // lists past the small wave buffer
  CHECK(sketch_batch_lds_bytes(768, 26, 3) == 0 && sketch_batch_lds_bytes(0, 26, 2) == 0);
  // G shrinks as the rows grow, never grows again, and whatever it is fits half a CU's LDS beside the static words
  uint32_t last = 8;
  for (uint32_t d = 1; d <= 40000; d += (d < 2048 ? 1 : 61)) {
    const uint32_t g = sketch_batch_max_group(d, 64);
    CHECK(g == 0 || g == 2 || g == 4 || g == 8);
    CHECK(g <= last);
    last = g;
    if (g) CHECK(sketch_batch_lds_bytes(d, 64, g) + kSketchBatchLdsStatic <= kSketchBatchLdsLimit);
    if (g && g < 8) CHECK(sketch_batch_lds_bytes(d, 64, 2 * g) == 0);
  }
  CHECK(sketch_batch_max_group(768, 26) == 8);
  CHECK(sketch_batch_max_group(1536, 26) == 4);
  CHECK(sketch_batch_max_group(8192, 26) == 2);
  CHECK(sketch_batch_max_group(12288, 26) == 2);
  CHECK(sketch_batch_max_group(16128, 26) == 2 && sketch_batch_max_group(16129, 26) == 0);
  CHECK(sketch_batch_max_group(896, 64) == 8 && sketch_batch_max_group(897, 64) == 4);
  CHECK(sketch_batch_max_group(32768, 26) == 0);  // the plan declines
  CHECK(sketch_batch_plan(8, sketch_batch_max_group(32768, 26)).empty());
  CHECK(sketch_batch_compiled_group(2) == 2 && sketch_batch_compiled_group(3) == 4 && sketch_batch_compiled_group(4) == 4 &&
        sketch_batch_compiled_group(5) == 8 && sketch_batch_compiled_group(8) == 8);
  CHECK(sketch_batch_list_k(1) == 17 && sketch_batch_list_k(10) == 26 && sketch_batch_list_k(32) == 64 && sketch_batch_list_k(33) == 66);
}

static void check_decline() {
  CHECK(sketch_batch_query_fits(false, 1.0, 1.0) && sketch_batch_query_fits(true, 1.0, 1.0));
  CHECK(!sketch_batch_query_fits(false, 0x1p63, 0x1p63));   // the dot could reach 2^126
  CHECK(sketch_batch_query_fits(false, 0x1p63, 1.0));       // ... against unit rows it cannot
  CHECK(!sketch_batch_query_fits(true, 0x1p63, 1.0));       // the L2 family declines from 2^62 on
  CHECK(sketch_batch_query_fits(true, 0x1p61, 0x1p60) && !sketch_batch_query_fits(true, 0x1p61, 0x1p61));
  CHECK(!sketch_batch_query_fits(false, INFINITY, 1.0) && !sketch_batch_query_fits(true, NAN, 1.0));
}

static void check_gate() {
  for (int family = 0; family < 3; ++family) {  // dot, L2, neither
    for (size_t limit : {(size_t)1, (size_t)32, (size_t)33}) {
      for (int side = 0; side < 2; ++side) {  // just below the family's cut, at it
        for (long sketch : {0L, 1L, 2L}) {
          for (long force : {0L, 1L, 2L}) {
            SketchBatchShape s;
            s.dot_metric = family == 0;
            s.l2_metric = family == 1;
            s.strictly_ranked = true;
            s.dim = 768;
            const double cut = family == 1 ? kSketchBatchL2MinBytes : kSketchBatchMinBytes;
            s.row_bytes = side ? cut : cut - 3072.0;
            s.sketch = sketch;
            s.force = force;
            const bool want = family < 2 && limit <= 32 && sketch == 1 && (side == 1 || force == 2);
            CHECK(sketch_batch_gate(s, 3, limit) == want);
            CHECK(sketch_batch_gate(s, 2, limit) == want);
            CHECK(!sketch_batch_gate(s, 1, limit) && !sketch_batch_gate(s, 0, limit));
            // four queries at any size; five to eight up to the wide bound only; nine and more, and whatever lies past a
            // measured bound, only under the tests' setting
            CHECK(sketch_batch_gate(s, kSketchBatchMaxQueries, limit) == want);
            CHECK(sketch_batch_gate(s, kSketchBatchMaxQueries + 1, limit) == want);
            CHECK(sketch_batch_gate(s, kSketchBatchWideQueries, limit) == want);
            CHECK(sketch_batch_gate(s, kSketchBatchWideQueries + 1, limit) == (want && force == 2));
            SketchBatchShape big = s;
            big.row_bytes = kSketchBatchWideMaxBytes + 3072.0;
            const bool want_big = family < 2 && limit <= 32 && sketch == 1;
            CHECK(sketch_batch_gate(big, kSketchBatchMaxQueries, limit) == want_big);
            CHECK(sketch_batch_gate(big, kSketchBatchMaxQueries + 1, limit) == (want_big && force == 2));
            big.row_bytes = kSketchBatchWideMaxBytes;
            CHECK(sketch_batch_gate(big, kSketchBatchWideQueries, limit) == want_big);
            SketchBatchShape noxx = s;
            noxx.column_lacks_xx = true;  // (an L2 handle's column without ||x||^2 serves nobody; the dot family never looks)
            CHECK(sketch_batch_gate(noxx, 3, limit) == (want && family == 0));
            CHECK(!sketch_batch_gate(s, 2, 0));
            SketchBatchShape t = s;
            t.strictly_ranked = false;
            CHECK(!sketch_batch_gate(t, 2, limit));
            t = s;
            t.single_nominate = true;
            CHECK(!sketch_batch_gate(t, 2, limit));
            t = s;
            t.refused = true;
            CHECK(!sketch_batch_gate(t, 2, limit));
            t = s;
            t.dim = 32768;  // no group fits
            CHECK(!sketch_batch_gate(t, 2, limit));
          }
        }
      }
    }
  }
  CHECK(kSketchBatchMinBytes >= 256.0 * (1 << 20) && kSketchBatchL2MinBytes >= 1024.0 * (1 << 20));  // never below the lone cuts
}

int main() {
  check_plan();
  check_lds();
  check_decline();
  check_gate();
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
