// vt_sketchbatch.h -- the host side of K1qm (vt_sketch_batch.hip): which batches share passes over the int8
// sketch, how their queries are split into groups, how large a group the pass's LDS takes, and which query must stay out.
// Stand-alone on purpose (no HIP, no header of the library): vt_sketchsearch.h and vt_batch.h use it, vt_sketch_batch.hip ties
// its constants to the device side's with static_asserts, and tests/sketch_batch_plan_check.cpp builds it with plain g++
// under AddressSanitizer and UBSan.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vt_host {

// ---- the pass's LDS: G query images of two int8 levels, and a small wave buffer per wave and query ---------------------
constexpr int kSketchBatchMaxGroup = 8;           // G: queries one pass carries at most
constexpr int kSketchBatchWaves = 4;              // waves per block (kWavesPerBlock)
constexpr size_t kSketchBatchWaveBuf = 2048;      // WaveTopK<kCapSmall>: 128 slots of 16 bytes
constexpr uint32_t kSketchBatchListMax = 64;      // k' <= kSmallK: the lists the small buffer holds
constexpr size_t kSketchBatchMaxLimit = 32;       // ... which is limits up to 32 (k' = max(2 k, k + 16))
// A block may take half a CU's 160 KiB: with one block per CU only four waves keep loads in flight there, and the pass is
// a stream.  (1 KiB of each half stays free for the kernel's static words: the queries' scalars and the merge's counts,
// 640 bytes at G = 8 -- vt_sketch_batch.hip asserts that they fit.)
constexpr size_t kSketchBatchLdsLimit = 80 * 1024;
constexpr size_t kSketchBatchLdsStatic = 1024;

constexpr uint32_t sketch_batch_ld8(uint32_t d) { return (d + 127) / 128 * 128; }
constexpr uint32_t sketch_batch_list_k(size_t limit) { return (uint32_t)std::max<size_t>(2 * limit, limit + 16); }

// The group sizes the pass is compiled for.  2, 4 and 8: the pass's cost is the stream's until the 2 G dots per dword
// outweigh it, so a group of 3 loses little as a group of 4 and one of 5..7 little as one of 8, and every further size
// is six more kernels to build and keep.  A group in between runs as the next one up, its unused places zero.
inline uint32_t sketch_batch_compiled_group(uint32_t ng) { return ng <= 2 ? 2u : ng <= 4 ? 4u : 8u; }

// Dynamic LDS of the pass compiled for `group` queries with lists of kp; 0: it does not fit (or no such pass).
inline size_t sketch_batch_lds_bytes(uint32_t d, uint32_t kp, uint32_t group) {
  if (d == 0 || kp == 0 || kp > kSketchBatchListMax) return 0;
  if (group != 2 && group != 4 && group != 8) return 0;
  const size_t bytes = (size_t)group * 2 * sketch_batch_ld8(d) + (size_t)group * kSketchBatchWaves * kSketchBatchWaveBuf;
  return bytes + kSketchBatchLdsStatic <= kSketchBatchLdsLimit ? bytes : 0;
}

// The largest group rows of d dimensions allow: G is lowered until the images fit; 0: not even two queries do.
inline uint32_t sketch_batch_max_group(uint32_t d, uint32_t kp) {
  for (uint32_t g = (uint32_t)kSketchBatchMaxGroup; g >= 2; g /= 2)
    if (sketch_batch_lds_bytes(d, kp, g)) return g;
  return 0;
}

// ---- the planner: nq queries in ceil(nq / gmax) groups of near-equal size, none smaller than two -----------------------
// (nine queries at gmax = 8: 5 + 4, never 8 + 1).  The sizes, in order; their sum is nq, except where no such split exists
// (an odd count at gmax = 2: the last query stays out) and below two queries (no group at all).
inline std::vector<uint32_t> sketch_batch_plan(size_t nq, uint32_t gmax) {
  std::vector<uint32_t> sizes;
  if (gmax < 2) return sizes;
  while (nq >= 2) {
    const size_t groups = (nq + gmax - 1) / gmax;
    if (nq / groups >= 2) {
      for (size_t g = 0; g < groups; ++g) sizes.push_back((uint32_t)(nq / groups + (g < nq % groups ? 1 : 0)));
      break;
    }
    nq -= 1;
  }
  return sizes;
}

// ---- the per-query decline: the lone path's overflow gates (sketch_search), evaluated for one query --------------------
// qn >= ||q||, max_norm >= every row's norm.  Dot family: a dot of these rows could reach the f32 overflow K1 must see for
// itself; L2 family: a squared difference could.  Such a query leaves its group before anything is launched.
inline bool sketch_batch_query_fits(bool l2, double qn, double max_norm) {
  const double up = 1.0 + 0x1p-30;
  return l2 ? (qn + max_norm) * up < 0x1p62 : qn * max_norm * up < 0x1p126;
}

// ---- the gate --------------------------------------------------------------------------------------------------------
// Both bounds are measured (profiles/sketch_batch/): the parent commit's library against this one, alternating,
// three runs each, batches of 2..32 on 768-float rows from 256 MB to 30 GB, cosine and L2; a shape is routed here only
// where its slowest run beat the other route's fastest.
// f32 rows below this cut keep today's routes, in either family.  Not the dot family's lone cut: at 256 MB (87 382 rows)
// a group of four ties with the sweep it replaces (0.123-0.124 ms against 0.124-0.125), from 1 GiB (350 000 rows) on
// every group of two to four is ahead, by 1.25 to 2.4 times.
constexpr double kSketchBatchMinBytes = 1024.0 * (1 << 20);
constexpr double kSketchBatchL2MinBytes = 1024.0 * (1 << 20);
// The largest batch that shares passes at any size.  Four: at 10 M rows a pass for two costs 1.28 ms and a pass for four
// 1.82 against the bf16 shadow pass's 2.26-2.29 -- but the pass compiled for eight costs 2.9-3.2 for five to eight queries
// (its sixteen broadcast LDS reads per chunk, not its dots, are what it waits for) where the matrix cores take 2.28-2.34.
constexpr size_t kSketchBatchMaxQueries = 4;
// Five to eight queries share a pass on rows up to this size only: at 1 GiB and at 3 GB (1 M x 768) the pass for eight is
// ahead of the sweep of the f32 rows such a batch takes today, in both families (0.42-0.49 ms against 0.60-0.75 at 3 GB);
// at 30 GB it loses, and nothing between the two has been measured.  Nine and more lose at every size measured.
constexpr size_t kSketchBatchWideQueries = 8;
constexpr double kSketchBatchWideMaxBytes = 3.0 * 1024 * (1 << 20);

// What the gate looks at, as plain values (vt_sketchsearch.h fills it from the shard and the settings).
struct SketchBatchShape {
  bool dot_metric = false, l2_metric = false;  // the handle's metric family (neither: no sketch serves it)
  bool strictly_ranked = false;                // the rank column is strictly current
  bool single_nominate = false;                // lone searches go through the shadow: so do batches
  bool refused = false;                        // the int8 column could not be had
  uint32_t dim = 0;
  double row_bytes = 0.0;                      // n * ld * 4: the f32 rows
  long sketch = 1;                             // the `sketch` setting: 0 never, 2 lone searches only
  long force = 0;                              // the `force_sketch` setting: 2 lifts the measured bounds (tests)
  bool column_lacks_xx = false;                // an L2 handle's column built without ||x||^2: it never serves the family
};

inline bool sketch_batch_gate(const SketchBatchShape &s, size_t nq, size_t limit) {
  if (s.sketch == 0 || s.sketch == 2) return false;
  if (!(s.dot_metric || s.l2_metric) || !s.strictly_ranked || s.single_nominate || s.refused) return false;
  if (s.l2_metric && s.column_lacks_xx) return false;
  if (limit == 0 || limit > kSketchBatchMaxLimit || nq < 2) return false;
  if (sketch_batch_max_group(s.dim, sketch_batch_list_k(limit)) < 2) return false;
  if (s.force == 2) return true;
  if (nq > kSketchBatchWideQueries) return false;
  if (nq > kSketchBatchMaxQueries && s.row_bytes > kSketchBatchWideMaxBytes) return false;
  return s.row_bytes >= (s.l2_metric ? kSketchBatchL2MinBytes : kSketchBatchMinBytes);
}

}  // namespace vt_host
