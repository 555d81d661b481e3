// vt_fdeplan.h -- what vt_mv_fde_sync (host/vt_fde.h) decides before and between its device steps: which of the listed
// ids are encoded and which leave the index, where the chunks of documents are cut, and which runs of a chunk's rows go
// into the index once the device has said which documents failed.  Stand-alone (no HIP, no other header of this
// directory): tests/fdeplan_check.cpp drives it against a brute-force model.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace vt_host {

// What the store says about an id.
enum FdeDocState : uint8_t {
  kFdeAbsent = 0,  // not a live document
  kFdeEmpty = 1,   // live, without vectors
  kFdeRows = 2,    // live, with at least one vector
};

struct FdeSyncPlan {
  std::vector<uint32_t> unique_of;   // [count] the listed position's place among the distinct ids
  std::vector<uint32_t> first_pos;   // [distinct] where the id stands first in the list
  std::vector<uint8_t> state;        // [distinct] FdeDocState
  std::vector<uint32_t> encode;      // distinct ids that are encoded, in list order (by first occurrence)
  std::vector<uint32_t> remove;      // distinct ids that leave the index, in list order
};

// A duplicate id counts once, at its first place.  state_of(id bytes, length) -> FdeDocState.
template <class StateOf>
void fde_sync_plan(size_t count, const char *ids, const size_t *id_off, StateOf state_of, FdeSyncPlan *plan) {
  FdeSyncPlan p;
  p.unique_of.resize(count);
  std::unordered_map<std::string, uint32_t> seen;
  for (size_t i = 0; i < count; ++i) {
    const char *id = ids + id_off[i];
    const size_t n = id_off[i + 1] - id_off[i];
    auto ins = seen.emplace(std::string(n ? id : "", n), (uint32_t)p.first_pos.size());
    p.unique_of[i] = ins.first->second;
    if (!ins.second) continue;
    const uint8_t st = (uint8_t)state_of(n ? id : "", n);
    p.first_pos.push_back((uint32_t)i);
    p.state.push_back(st);
    (st == kFdeRows ? p.encode : p.remove).push_back(ins.first->second);
  }
  *plan = std::move(p);
}

// Chunks [cut[k], cut[k + 1]) of n documents that each take doc_bytes of scratch: as many as fit the budget, at least one,
// at most max_docs (what one launch addresses).
inline void fde_chunk_cuts(size_t n, size_t doc_bytes, size_t budget, size_t max_docs, std::vector<size_t> *cut) {
  size_t per = doc_bytes ? budget / doc_bytes : n;
  if (per > max_docs) per = max_docs;
  if (per < 1) per = 1;
  cut->assign(1, 0);
  for (size_t i0 = 0; i0 < n;) {
    const size_t i1 = n - i0 < per ? n : i0 + per;
    cut->push_back(i1);
    i0 = i1;
  }
}

// The maximal runs [first, last) of a chunk's documents whose status is 0, in order.
inline void fde_good_runs(const int *status, size_t n, std::vector<std::pair<size_t, size_t>> *runs) {
  runs->clear();
  for (size_t i = 0; i < n;) {
    if (status[i] != 0) {
      ++i;
      continue;
    }
    size_t e = i;
    while (e < n && status[e] == 0) ++e;
    runs->emplace_back(i, e);
    i = e;
  }
}

}  // namespace vt_host
