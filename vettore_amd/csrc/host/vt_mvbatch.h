// vt_mvbatch.h -- packing the query sets of one batched search of a resident multi-vector store (vt_mv_top_k_batch,
// host/vt_mvsearch.h) into the panels K9rb scores (vt_maxsim_batch.hip).  Plain C++, no HIP call: tests/mvbatch_check.cpp
// drives it stand-alone.
//
// A set of c > 0 query vectors takes ceil(c / 8) groups of eight slots, its last group padded, so a lane's eight
// query vectors never belong to two sets.  A panel is a run of whole sets whose groups fit in `capacity` slots (what LDS
// holds beside the wave tiles, cut to whole passes of `pass` slots); a set never straddles two panels.  Sets K9rb does not
// take -- none of the set's vectors, or more groups than one panel holds -- go to the single-set path, in batch order.
// One descriptor per group, in slot order: descriptor g is slots [8 g, 8 g + 8).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace vt_host {

constexpr uint32_t kMvGroupSlots = 8;
constexpr uint32_t kMvGroupFirst = 1u << 8, kMvGroupLast = 1u << 9;  // (kMaxSimBatchFirst / Last, vt_device.h)

struct MvBatchDesc {
  uint32_t set;   // the set the group belongs to
  uint32_t info;  // real slots of the group (1..8) | kMvGroupFirst | kMvGroupLast
};
struct MvBatchPanel {
  uint32_t first_set, sets;  // the panel's first set and how many sets it holds (sets on the single path are not counted)
  uint32_t desc0, ndesc;     // its descriptors: slots [8 desc0, 8 (desc0 + ndesc))
};
struct MvBatchPlan {
  std::vector<MvBatchPanel> panels;
  std::vector<MvBatchDesc> desc;
  std::vector<uint32_t> single;  // sets for the single-set path
};

// `own_panel`: every set is a panel of its own (each has its own document list).
inline void mv_batch_plan(const uint32_t *counts, size_t nsets, uint32_t capacity, uint32_t pass, bool own_panel,
                          MvBatchPlan *out) {
  out->panels.clear();
  out->desc.clear();
  out->single.clear();
  const uint32_t cap_groups = pass ? capacity / pass * pass / kMvGroupSlots : 0;
  bool open = false;
  for (size_t b = 0; b < nsets; ++b) {
    const uint32_t c = counts[b];
    const uint32_t ng = c / kMvGroupSlots + (c % kMvGroupSlots ? 1 : 0);  // (no c + 7: c may be near 2^32)
    if (c == 0 || ng > cap_groups) {
      out->single.push_back((uint32_t)b);
      continue;
    }
    if (!open || own_panel || out->panels.back().ndesc + ng > cap_groups) {
      out->panels.push_back(MvBatchPanel{(uint32_t)b, 0, (uint32_t)out->desc.size(), 0});
      open = true;
    }
    MvBatchPanel &p = out->panels.back();
    p.sets += 1;
    p.ndesc += ng;
    for (uint32_t g = 0; g < ng; ++g) {
      uint32_t info = g + 1 < ng ? kMvGroupSlots : c - g * kMvGroupSlots;
      if (g == 0) info |= kMvGroupFirst;
      if (g + 1 == ng) info |= kMvGroupLast;
      out->desc.push_back(MvBatchDesc{(uint32_t)b, info});
    }
  }
}

}  // namespace vt_host
