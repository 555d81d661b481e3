// vt_hnswplan.h -- the bookkeeping of the HNSW index's slab (vt_hnsw): how large a slab is, when the dead rows of
// deleted nodes are squeezed out, and where every surviving row and its upper-layer lists land when they are.
// Stand-alone (no HIP, no other header of this directory): tests/test_hnsw_plan.py builds it with g++ under the
// sanitizers (tests/hnswplan_check.cpp).  host/vt_hnsw.h acts on the plan, K11c (vt_hnsw.hip) moves the words.
//
// The rule (hnsw_compact_due): an insert compacts first when the dead rows outnumber the live ones and there are at
// least kHnswCompactMinDead of them.  A delete never compacts.  So a compaction of `live` rows is paid for by more
// than `live` erasures, and behind an insert dead <= max(live, kHnswCompactMinDead - 1) + 1 (an upsert's own erasure is
// the + 1); below 64 dead rows the waste is under one traversal tile and a two-node index upserted in a loop keeps its
// buffers.
//
// The plan keeps the survivors in row order, so a row number still orders like the internal id (host/vt_hnsw.h).
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace vt_host {

constexpr uint64_t kHnswCompactMinDead = 64;
constexpr uint64_t kHnswMinRows = 1024;          // the smallest slab
constexpr uint64_t kHnswMinUpper = 4096;         // the smallest array of upper-layer lists, in words
constexpr uint64_t kHnswMaxUpper = 0xFFFFFFF0ull;  // upper-layer offsets are 32 bits (hnsw_insert_one refuses beyond)
constexpr uint64_t kHnswMaxPlanRows = 0xFFFFFFFFull;  // rows are 32 bits and 0xFFFFFFFF names no row

// the slab capacity the growth rule assigns to `rows` rows: 1024 doubled until it fits
inline uint64_t hnsw_capacity_for(uint64_t rows) {
  uint64_t cap = kHnswMinRows;
  while (cap < rows) cap *= 2;
  return cap;
}
// the same for `words` words of upper-layer lists, from 4096
inline uint64_t hnsw_upper_capacity_for(uint64_t words) {
  uint64_t cap = kHnswMinUpper;
  while (cap < words) cap *= 2;
  return cap;
}

inline bool hnsw_compact_due(uint64_t live, uint64_t dead) { return dead > live && dead >= kHnswCompactMinDead; }

// `rows` rows and `upper` words of upper-layer lists are addressable with 32 bits
inline bool hnsw_plan_fits(uint64_t rows, uint64_t upper) { return rows < kHnswMaxPlanRows && upper <= kHnswMaxUpper; }

struct HnswRowLevel {
  uint32_t row, level;
};

struct HnswCompactPlan {
  std::vector<uint32_t> src;    // src[i]: the old row of new row i, ascending
  std::vector<uint32_t> upoff;  // upoff[i]: where new row i's upper-layer lists start
  uint64_t rows_used = 0, upper_used = 0, capacity = 0, upper_capacity = 0;
};

// The plan for the surviving nodes' (old row, level), given in row order (strictly ascending rows), with `m` entries
// per upper-layer list.  false, and *out empty: the rows are not ascending, or the index would not fit in 32 bits.
inline bool hnsw_compact_plan(const std::vector<HnswRowLevel> &live, size_t m, HnswCompactPlan *out) {
  *out = HnswCompactPlan{};
  HnswCompactPlan p;
  if (!hnsw_plan_fits(live.size(), 0)) return false;
  p.src.reserve(live.size());
  p.upoff.reserve(live.size());
  uint64_t upper = 0;
  for (size_t i = 0; i < live.size(); ++i) {
    if (i && live[i].row <= live[i - 1].row) return false;
    p.src.push_back(live[i].row);
    p.upoff.push_back((uint32_t)upper);
    upper += (uint64_t)live[i].level * ((uint64_t)m + 1);  // (level < 2^32, m <= 2^32: no wrap before the check)
    if (!hnsw_plan_fits(live.size(), upper)) return false;
  }
  p.rows_used = live.size();
  p.upper_used = upper;
  p.capacity = hnsw_capacity_for(p.rows_used + 1);  // the insert behind the compaction takes a row at once
  p.upper_capacity = hnsw_upper_capacity_for(upper);
  *out = std::move(p);
  return true;
}

}  // namespace vt_host
