// Checks vettore_amd/csrc/host/vt_hnswplan.h (when an HNSW slab is compacted and where every survivor lands) and
// HnswGraph::close_rows() (vt_hnswgraph.h) on the CPU: built stand-alone with the sanitizers by tests/test_hnsw_plan.py.
// Prints one line per failed check and returns their number.
#include "../vettore_amd/csrc/host/vt_hnswgraph.h"
#include "../vettore_amd/csrc/host/vt_hnswplan.h"

#include <cstdio>
#include <map>
#include <sstream>

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("line %d: %s\n", __LINE__, #cond);             \
      ++failures;                                                \
    }                                                            \
  } while (0)

using namespace vt_host;

// everything tests/hnswgraph_check.cpp prints of a graph -- next, entry, dimension, size, every level and list -- and the edge count
static std::string dump(const HnswGraph &g) {
  std::map<uint64_t, const HnswNode *> sorted;
  for (const auto &kv : g.nodes()) sorted[kv.first] = &kv.second;
  std::ostringstream o;
  o << g.next() << ' ' << (long long)g.entry() << ' ' << g.dimension() << ' ' << g.len() << ' ' << g.edges();
  for (const auto &kv : sorted) {
    o << " |" << kv.first << ':' << kv.second->level << ':' << kv.second->external_id;
    for (const auto &l : kv.second->conn) {
      o << ';';
      for (size_t i = 0; i < l.size(); ++i) o << (i ? "," : "") << l[i].id << '@' << l[i].dist;
    }
  }
  return o.str();
}

static void check_rule() {
  CHECK(kHnswCompactMinDead == 64);
  // (live, dead) at the boundaries.  The rule as written down -- dead > live && dead >= 64 -- makes (63, 64) due: 64 dead
  // rows outnumber 63 live ones and reach the minimum at the same step.
  CHECK(hnsw_compact_due(63, 64));
  CHECK(!hnsw_compact_due(63, 63));
  CHECK(!hnsw_compact_due(64, 64));
  CHECK(hnsw_compact_due(63, 65));
  CHECK(hnsw_compact_due(0, 64));
  CHECK(!hnsw_compact_due(0, 63));
  CHECK(!hnsw_compact_due(2, 63));
  CHECK(!hnsw_compact_due(1000, 1000));
  CHECK(hnsw_compact_due(1000, 1001));
  // behind an insert that found dead <= max(live, 63) + 1 not due, the next erasure cannot pass the bound by more than itself
  for (uint64_t live = 0; live < 300; ++live)
    for (uint64_t dead = 0; dead < 300; ++dead)
      CHECK(hnsw_compact_due(live, dead) == (dead > std::max<uint64_t>(live, 63)));
}

static void check_capacity() {
  CHECK(hnsw_capacity_for(0) == 1024);
  CHECK(hnsw_capacity_for(1) == 1024);
  CHECK(hnsw_capacity_for(1024) == 1024);
  CHECK(hnsw_capacity_for(1025) == 2048);
  CHECK(hnsw_capacity_for((1ull << 20) + 1) == (1ull << 21));
  CHECK(hnsw_upper_capacity_for(0) == 4096);
  CHECK(hnsw_upper_capacity_for(4096) == 4096);
  CHECK(hnsw_upper_capacity_for(4097) == 8192);
  // the growth rule as hnsw_reserve had it: from the capacity of the moment, doubled until it fits
  for (uint64_t have = 1024; have <= (1u << 16); have *= 2)
    for (uint64_t rows : {have + 1, 2 * have, 2 * have + 1, 5 * have}) {
      uint64_t cap = have;
      while (cap < rows) cap *= 2;
      CHECK(hnsw_capacity_for(rows) == cap);
    }
}

static void check_plan() {
  // rows 0, 1, 4, 9 are dead, 12 rows were handed out; m = 4: an upper-layer list is 5 words
  const std::vector<HnswRowLevel> live = {{2, 0}, {3, 2}, {5, 0}, {6, 1}, {7, 0}, {8, 3}, {10, 0}, {11, 1}};
  HnswCompactPlan p;
  CHECK(hnsw_compact_plan(live, 4, &p));
  CHECK((p.src == std::vector<uint32_t>{2, 3, 5, 6, 7, 8, 10, 11}));
  CHECK((p.upoff == std::vector<uint32_t>{0, 0, 10, 10, 15, 15, 30, 30}));
  CHECK(p.rows_used == 8 && p.upper_used == 35 && p.capacity == 1024 && p.upper_capacity == 4096);
  // the capacity is the growth rule's for the rows and the one the insert behind the compaction takes
  std::vector<HnswRowLevel> many;
  for (uint32_t r = 0; r < 1024; ++r) many.push_back({2 * r + 1, r % 2});
  CHECK(hnsw_compact_plan(many, 16, &p));
  CHECK(p.rows_used == 1024 && p.capacity == 2048 && p.upper_used == 512 * 17 && p.upper_capacity == 16384);
  CHECK(p.src[1023] == 2047 && p.upoff[1023] == 511 * 17 && p.upoff[1] == 0 && p.upoff[2] == 17);
  many.pop_back();
  CHECK(hnsw_compact_plan(many, 16, &p) && p.capacity == 1024);
  // nothing survives: an empty plan (the host never asks: an emptied graph forgets its slab)
  CHECK(hnsw_compact_plan({}, 4, &p) && p.src.empty() && p.rows_used == 0 && p.upper_used == 0 && p.capacity == 1024);
  // rows that do not ascend are no plan
  CHECK(!hnsw_compact_plan({{3, 0}, {3, 1}}, 4, &p) && p.src.empty() && p.upoff.empty() && p.capacity == 0);
  CHECK(!hnsw_compact_plan({{5, 0}, {4, 0}}, 4, &p));
}

static void check_refusal() {
  // 32 bits: a row number below 0xFFFFFFFF (which names no row), upper-layer words up to 0xFFFFFFF0
  CHECK(hnsw_plan_fits(0, 0));
  CHECK(hnsw_plan_fits(0xFFFFFFFEull, 0xFFFFFFF0ull));
  CHECK(!hnsw_plan_fits(0xFFFFFFFFull, 0));
  CHECK(!hnsw_plan_fits(1, 0xFFFFFFF1ull));
  CHECK(!hnsw_plan_fits(1ull << 32, 1ull << 32));
  // levels are the plan's to take as given: three nodes whose lists would need 3 * 2^30 * 2 words, refused at the third
  HnswCompactPlan p;
  CHECK(hnsw_compact_plan({{0, 1u << 30}, {1, (1u << 30) - 8}}, 1, &p) && p.upper_used == 0xFFFFFFF0ull);
  CHECK(p.upper_capacity == (1ull << 32));
  CHECK(!hnsw_compact_plan({{0, 1u << 30}, {1, (1u << 30) - 8}, {2, 1}}, 1, &p));
  CHECK(p.src.empty() && p.upoff.empty() && p.rows_used == 0 && p.capacity == 0);
  CHECK(!hnsw_compact_plan({{7, 0xFFFFFFFFu}}, 1024, &p));
}

static void check_close_rows() {
  HnswGraph g(2, 4, 12);
  uint32_t rows = 0;
  auto insert = [&](const std::string &id, std::vector<std::vector<HnswEdge>> lists) {
    g.erase(id);
    const uint64_t iid = g.take_id();
    g.apply_insert(id, iid, g.level_for(id.data(), id.size()), rows++, 3, std::move(lists));
  };
  // 40 nodes, each linked to up to five earlier ones on every layer it shares with them; then upserts and deletes
  for (int i = 0; i < 40; ++i) {
    const std::string id = "node-" + std::to_string((i * 7919) % 101);
    const uint32_t level = g.level_for(id.data(), id.size());
    std::vector<std::vector<HnswEdge>> lists(level + 1);
    for (const auto &kv : g.nodes())
      for (uint32_t l = 0; l <= level && l <= kv.second.level; ++l)
        if (lists[l].size() < 5) lists[l].push_back(HnswEdge{kv.first, (float)((kv.first * 37 + i) % 11)});
    insert(id, std::move(lists));
  }
  for (int i : {0, 3, 4, 9, 17, 39}) g.erase("node-" + std::to_string((i * 7919) % 101));
  insert("node-" + std::to_string((5 * 7919) % 101), {{HnswEdge{1, 0.5f}, HnswEdge{2, 0.25f}}});  // an upsert: row 40
  {
    const HnswNode *en = g.node(g.entry());
    CHECK(en != nullptr);
    if (en) g.erase(std::string(en->external_id));  // the entry goes
  }
  uint32_t top = 0;
  for (const auto &kv : g.nodes()) top = std::max(top, kv.second.level);
  CHECK(top >= 1 && g.len() == 33 && rows == 41);

  const std::string before = dump(g);
  const auto changed_before = g.changed();
  std::map<uint64_t, uint32_t> old_row;
  for (const auto &kv : g.nodes()) old_row[kv.first] = kv.second.row;
  const std::vector<std::pair<uint32_t, uint32_t>> got = g.close_rows();
  CHECK(dump(g) == before);
  CHECK(g.changed() == changed_before);
  CHECK(got.size() == g.len());
  // rows 0 .. live - 1 in the order of the internal ids; the list names the old rows, ascending, with the levels
  uint32_t i = 0;
  for (const auto &kv : old_row) {  // (a std::map: ascending internal ids)
    const HnswNode *n = g.node(kv.first);
    CHECK(n && n->row == i);
    CHECK(i < got.size() && got[i].first == kv.second && n && got[i].second == n->level);
    CHECK(i == 0 || got[i].first > got[i - 1].first);
    ++i;
  }
  // once more: nothing is dead, nothing moves
  const auto again = g.close_rows();
  CHECK(again.size() == got.size());
  for (size_t k = 0; k < again.size(); ++k) CHECK(again[k].first == k && again[k].second == got[k].second);
  CHECK(dump(g) == before);
  // an empty graph has no rows to close
  HnswGraph e(2, 4, 12);
  CHECK(e.close_rows().empty());
}

int main() {
  check_rule();
  check_capacity();
  check_plan();
  check_refusal();
  check_close_rows();
  if (!failures) std::puts("ok");
  return failures;
}
