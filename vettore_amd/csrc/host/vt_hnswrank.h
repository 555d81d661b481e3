// vt_hnswrank.h -- the id-rank column of an HNSW slab (host/vt_hnswstage.h keeps it, K15 reads it): for every used row
// the position of its node's external id in the bytewise order of the live ids, kHnswRankNoRow for a row whose node is
// gone.  With it a key orderable(rank) << 32 | id_rank orders like the reference's (rank.total_cmp, id bytes).
// Stand-alone (no HIP, no other header of this directory): tests/test_hnsw_rank.py builds it with g++ under the
// sanitizers (tests/hnswrank_check.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace vt_host {

constexpr uint32_t kHnswRankNoRow = 0xFFFFFFFFu;  // (vt::kHnswNoRow)

// live[i] = (external id, row) of a live node, in any order; rows_used rows in the slab.  out[row] = the id's position
// among the live ids sorted bytewise (std::string's order: unsigned bytes, a prefix first), kHnswRankNoRow for every row no
// node names.  false, and *out empty: a row at or past rows_used, a row named twice, or an id given twice.
inline bool hnsw_id_ranks(const std::vector<std::pair<const std::string *, uint32_t>> &live, size_t rows_used,
                          std::vector<uint32_t> *out) {
  out->clear();
  if (live.size() > rows_used || rows_used >= kHnswRankNoRow) return false;
  std::vector<uint32_t> order(live.size());
  for (size_t i = 0; i < live.size(); ++i) order[i] = (uint32_t)i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return *live[a].first < *live[b].first; });
  std::vector<uint32_t> ranks(rows_used, kHnswRankNoRow);
  for (size_t r = 0; r < order.size(); ++r) {
    const auto &cur = live[order[r]];
    if (r && *live[order[r - 1]].first == *cur.first) return false;
    if (cur.second >= rows_used || ranks[cur.second] != kHnswRankNoRow) return false;
    ranks[cur.second] = (uint32_t)r;
  }
  *out = std::move(ranks);
  return true;
}

}  // namespace vt_host
