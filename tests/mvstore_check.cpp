// Drives vettore_amd/csrc/host/vt_mvstore.h -- the slot table of a resident multi-vector store -- from a script on
// stdin, the way host/vt_mvsearch.h drives it (plan_put, then apply_put; erase), checks its own invariants after every
// step and prints the state a search would see, for tests/test_mv_store.py to compare with a Python dict.
//   P <n> {<id> <rows>}*n   put_many (ids may repeat: the last one counts)      D <id>   delete      S   print the state
#include "../vettore_amd/csrc/host/vt_mvstore.h"

#include <cstdio>
#include <iostream>

using vt_host::MvPutPlan;
using vt_host::MvSlot;
using vt_host::MvTable;

static bool invariants(const MvTable &t, const MvPutPlan *plan) {
  // live rows are disjoint runs inside [0, used), in slot order; the counters add up
  uint64_t live = 0, at = 0;
  size_t docs = 0;
  for (const MvSlot &s : t.slots()) {
    if (!s.live) continue;
    ++docs;
    if (s.rows == 0) continue;
    if (s.first_row < at || (uint64_t)s.first_row + s.rows > t.used_rows()) return false;
    at = (uint64_t)s.first_row + s.rows;
    live += s.rows;
  }
  if (docs != t.len() || live != t.live_rows() || t.used_rows() > t.capacity()) return false;
  if ((t.dimension() < 0) != (live == 0)) return false;
  if (live == 0 && (t.used_rows() || t.capacity())) return false;
  for (const MvSlot &s : t.slots())
    if (s.live && t.find(s.id.data(), s.id.size()) != (uint32_t)(&s - t.slots().data())) return false;
  if (plan && plan->compact && t.live_rows() && plan->src.size() > t.used_rows()) return false;
  return true;
}

int main() {
  MvTable t;
  std::string op;
  long step = 0;
  while (std::cin >> op) {
    ++step;
    if (op == "P") {
      size_t n;
      std::cin >> n;
      std::string blob;
      std::vector<size_t> off{0}, rows;
      for (size_t i = 0; i < n; ++i) {
        std::string id;
        size_t r;
        std::cin >> id >> r;
        blob += id;
        off.push_back(blob.size());
        rows.push_back(r);
      }
      MvPutPlan plan;
      const uint64_t live_before = t.live_rows();
      if (!t.plan_put(n, blob.data(), off.data(), rows.data(), &plan)) { std::printf("plan refused at step %ld\n", step); return 1; }
      // what the device side relies on: the compaction list names every live row once, in order; the new rows fit
      if (plan.compact && plan.src.size() != live_before) { std::printf("src size at step %ld\n", step); return 1; }
      if (plan.base + plan.new_rows > plan.capacity && plan.new_rows) { std::printf("capacity at step %ld\n", step); return 1; }
      t.apply_put(plan, blob.data(), off.data(), rows.data(), 8);
      if (!invariants(t, &plan)) { std::printf("invariants after put, step %ld\n", step); return 1; }
    } else if (op == "D") {
      std::string id;
      std::cin >> id;
      const bool had = t.find(id.data(), id.size()) != MvTable::kNone;
      if (t.erase(id.data(), id.size()) != had) { std::printf("erase at step %ld\n", step); return 1; }
      if (!invariants(t, nullptr)) { std::printf("invariants after delete, step %ld\n", step); return 1; }
    } else if (op == "S") {
      std::vector<uint32_t> list, pos, rank;
      t.live_list(list, pos);
      t.id_ranks(list, rank);
      std::printf("len=%zu dim=%ld used=%llu dead=%llu cap=%llu compactions=%llu :", t.len(), t.dimension(),
                  (unsigned long long)t.used_rows(), (unsigned long long)t.dead_rows(), (unsigned long long)t.capacity(),
                  (unsigned long long)t.compactions());
      for (size_t k = 0; k < list.size(); ++k) {
        const MvSlot &s = t.slots()[list[k]];
        if (pos[list[k]] != k) { std::printf("pos_of_slot at step %ld\n", step); return 1; }
        std::printf(" %s/%u/%u", s.id.c_str(), s.rows, rank[k]);
      }
      std::printf("\n");
    } else {
      std::printf("bad op %s\n", op.c_str());
      return 1;
    }
  }
  std::printf("ok\n");
  return 0;
}
