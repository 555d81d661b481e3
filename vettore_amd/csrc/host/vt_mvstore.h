// vt_mvstore.h -- the slot table of a resident multi-vector store (vt_mv): which document owns which rows of the
// store's device slab, in the order of the documents' last put.  Stand-alone (no HIP, no other header of this
// directory): tests/test_mv_store.py builds it with g++ and drives it against a Python dict.  The device side --
// the slab, the norm column, the searches -- is host/vt_mvsearch.h.
//
// A put appends: the document's rows go behind the rows in use, its slot behind the slots.  An upsert or a delete
// leaves the old slot dead and its rows dead with it.  Nothing moves until a put finds more dead rows than live ones:
// that put compacts first (the live rows close up in slot order, the dead slots go).  The slab starts at kMvFirstRows
// rows and doubles.  A put is planned before anything changes (plan_put), so that the device side can allocate -- and
// fail -- first, and applied afterwards (apply_put), which cannot fail for lack of rows.
// When the last live row goes the store forgets its dimension and its slab: the next put may bring another dimension.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace vt_host {

constexpr uint64_t kMvFirstRows = 4096;          // rows of a store's first slab
constexpr uint64_t kMvMaxRows = 0xFFFFFFF0ull;   // rows are 32-bit indices on the device

struct MvSlot {
  std::string id;
  uint32_t first_row = 0, rows = 0;
  bool live = false;
};

// What a put is going to do, worked out on the unchanged table.
struct MvPutPlan {
  std::vector<uint32_t> take;   // the call's documents that are stored, in call order: the last of each id
  bool compact = false;         // the live rows close up first ...
  std::vector<uint32_t> src;    // ... row j of the new slab is row src[j] of the old one
  uint64_t capacity = 0;        // rows of the slab afterwards (a new slab when compact or capacity differs)
  uint64_t base = 0;            // the first new row
  uint64_t new_rows = 0;
};

class MvTable {
 public:
  size_t len() const { return by_id_.size(); }
  long dimension() const { return live_rows() ? dim_ : -1; }
  uint64_t used_rows() const { return used_; }
  uint64_t dead_rows() const { return dead_; }
  uint64_t live_rows() const { return used_ - dead_; }
  uint64_t capacity() const { return capacity_; }
  uint64_t compactions() const { return compactions_; }
  const std::vector<MvSlot> &slots() const { return slots_; }

  // false: more rows than the device can index (nothing is planned).  rows[i] = vectors of the call's document i.
  bool plan_put(size_t count, const char *ids, const size_t *id_off, const size_t *rows, MvPutPlan *plan) const {
    MvPutPlan p;
    std::unordered_map<std::string, uint32_t> last;
    for (size_t i = 0; i < count; ++i) last[std::string(ids + id_off[i], id_off[i + 1] - id_off[i])] = (uint32_t)i;
    for (size_t i = 0; i < count; ++i)
      if (last[std::string(ids + id_off[i], id_off[i + 1] - id_off[i])] == i) {
        p.take.push_back((uint32_t)i);
        p.new_rows += rows[i];
      }
    p.compact = dead_ > live_rows();
    p.base = p.compact ? live_rows() : used_;
    if (p.base + p.new_rows > kMvMaxRows) return false;
    if (p.compact)
      for (const MvSlot &s : slots_)
        if (s.live)
          for (uint32_t r = 0; r < s.rows; ++r) p.src.push_back(s.first_row + r);
    p.capacity = capacity_;
    if (p.base + p.new_rows > p.capacity) {
      if (p.capacity == 0) p.capacity = kMvFirstRows;
      while (p.capacity < p.base + p.new_rows) p.capacity *= 2;
    }
    *plan = std::move(p);
    return true;
  }

  // The planned put happens (`dim`: the length of the call's vectors).
  void apply_put(const MvPutPlan &p, const char *ids, const size_t *id_off, const size_t *rows, long dim) {
    if (p.compact) {
      std::vector<MvSlot> kept;
      uint64_t at = 0;
      for (MvSlot &s : slots_)
        if (s.live) {
          s.first_row = (uint32_t)at;
          at += s.rows;
          kept.push_back(std::move(s));
        }
      slots_ = std::move(kept);
      for (uint32_t i = 0; i < slots_.size(); ++i) by_id_[slots_[i].id] = i;
      used_ = at;
      dead_ = 0;
      dead_slots_ = 0;
      ++compactions_;
    }
    capacity_ = p.capacity;
    for (uint32_t i : p.take) {
      std::string id(ids + id_off[i], id_off[i + 1] - id_off[i]);
      kill(id);
      MvSlot s;
      s.first_row = (uint32_t)used_;
      s.rows = (uint32_t)rows[i];
      s.live = true;
      used_ += rows[i];
      by_id_[id] = (uint32_t)slots_.size();
      s.id = std::move(id);
      slots_.push_back(std::move(s));
    }
    if (p.new_rows) dim_ = dim;
    settle();
  }

  // false: no such document
  bool erase(const char *id, size_t n) {
    if (!kill(std::string(id, n))) return false;
    settle();
    return true;
  }

  // The live documents in store order -- the order of their last put -- as slot numbers, and where each slot stands in
  // that list (kNone: dead).
  static constexpr uint32_t kNone = 0xFFFFFFFFu;
  void live_list(std::vector<uint32_t> &list, std::vector<uint32_t> &pos_of_slot) const {
    list.clear();
    pos_of_slot.assign(slots_.size(), kNone);
    for (uint32_t i = 0; i < slots_.size(); ++i)
      if (slots_[i].live) {
        pos_of_slot[i] = (uint32_t)list.size();
        list.push_back(i);
      }
  }
  // rank[k] = how many documents of `list` have smaller id bytes than its k-th (ids of live documents differ)
  void id_ranks(const std::vector<uint32_t> &list, std::vector<uint32_t> &rank) const {
    std::vector<uint32_t> order(list.size());
    for (uint32_t k = 0; k < order.size(); ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return slots_[list[a]].id < slots_[list[b]].id; });
    rank.resize(list.size());
    for (uint32_t k = 0; k < order.size(); ++k) rank[order[k]] = k;
  }
  // the slot of a live document, kNone when there is none
  uint32_t find(const char *id, size_t n) const {
    auto it = by_id_.find(std::string(id, n));
    return it == by_id_.end() ? kNone : it->second;
  }

 private:
  bool kill(const std::string &id) {
    auto it = by_id_.find(id);
    if (it == by_id_.end()) return false;
    MvSlot &s = slots_[it->second];
    s.live = false;
    dead_ += s.rows;
    ++dead_slots_;
    by_id_.erase(it);
    return true;
  }
  // After a change: a store without a live row forgets rows, slab and dimension; dead slots that outnumber the live
  // ones go (their rows stay dead: only a put's compaction moves rows).
  void settle() {
    const bool forget = used_ > 0 && live_rows() == 0;
    if (forget) {
      used_ = dead_ = capacity_ = 0;
      dim_ = -1;
    }
    if (!forget && dead_slots_ <= by_id_.size() + 16) return;
    std::vector<MvSlot> kept;
    for (MvSlot &s : slots_)
      if (s.live) kept.push_back(std::move(s));
    slots_ = std::move(kept);
    for (uint32_t i = 0; i < slots_.size(); ++i) by_id_[slots_[i].id] = i;
    dead_slots_ = 0;
  }

  std::vector<MvSlot> slots_;  // in put order, dead ones included until a compaction or a sweep
  std::unordered_map<std::string, uint32_t> by_id_;  // live documents
  uint64_t used_ = 0, dead_ = 0, capacity_ = 0, compactions_ = 0;
  size_t dead_slots_ = 0;
  long dim_ = -1;
};

}  // namespace vt_host
