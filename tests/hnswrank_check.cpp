// hnswrank_check.cpp -- vettore_amd/csrc/host/vt_hnswrank.h as a program of its own (tests/test_hnsw_rank.py builds it with
// AddressSanitizer and UBSan and runs it): the id-rank column against a plain sort.  Prints "ok" and returns 0, or says
// which check failed.
#include "../vettore_amd/csrc/host/vt_hnswrank.h"

#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

using vt_host::hnsw_id_ranks;
using vt_host::kHnswRankNoRow;
using Live = std::vector<std::pair<const std::string *, uint32_t>>;

static int failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("line %d: %s\n", __LINE__, #cond);              \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// ids[row] (empty optional: dead) -> the column by a plain sort of the live ids
static std::vector<uint32_t> by_sort(const std::vector<std::pair<bool, std::string>> &rows) {
  std::map<std::string, uint32_t> sorted;  // (std::string orders bytewise, as unsigned char)
  for (uint32_t r = 0; r < rows.size(); ++r)
    if (rows[r].first) sorted[rows[r].second] = r;
  std::vector<uint32_t> out(rows.size(), kHnswRankNoRow);
  uint32_t rank = 0;
  for (const auto &kv : sorted) out[kv.second] = rank++;
  return out;
}

static void check_against_sort(const std::vector<std::pair<bool, std::string>> &rows, bool reversed) {
  Live live;
  for (uint32_t r = 0; r < rows.size(); ++r)
    if (rows[r].first) live.emplace_back(&rows[r].second, r);
  if (reversed) live = Live(live.rbegin(), live.rend());  // (the order the live nodes are given in does not matter)
  std::vector<uint32_t> got;
  CHECK(hnsw_id_ranks(live, rows.size(), &got));
  CHECK(got == by_sort(rows));
}

int main() {
  // ids whose byte order differs from row order, ids that are prefixes of one another, bytes above 0x7f, an empty id
  std::vector<std::pair<bool, std::string>> rows;
  for (uint32_t r = 0; r < 300; ++r) rows.emplace_back(true, "k" + std::to_string((r * 7919u) % 1009u) + "/" + std::to_string(r));
  rows.emplace_back(true, "k1");
  rows.emplace_back(true, "k");
  rows.emplace_back(true, "");
  rows.emplace_back(true, "k10");
  rows.emplace_back(true, std::string("k\xff", 2));
  rows.emplace_back(true, std::string("k\x00z", 3));
  rows.emplace_back(true, "k\x7f");
  for (int reversed = 0; reversed < 2; ++reversed) {
    auto t = rows;
    check_against_sort(t, reversed);
    t.front().first = false;  // dead rows first
    t[1].first = false;
    check_against_sort(t, reversed);
    t = rows;
    t.back().first = false;  // ... last
    check_against_sort(t, reversed);
    for (size_t r = 0; r < t.size(); r += 3) t[r].first = false;  // ... in between
    check_against_sort(t, reversed);
    for (auto &x : t) x.first = false;  // ... all
    check_against_sort(t, reversed);
  }
  {
    const auto want = by_sort(rows);
    CHECK(want[302] == 0 && want[301] == 1);  // "" before "k" before everything longer
    CHECK(want[305] < want[300] && want[300] < want[303]);  // "k\0z" < "k1" < "k10"
    CHECK(want[306] < want[304]);  // 0x7f < 0xff: unsigned bytes
  }
  // zero rows
  std::vector<uint32_t> got(3, 7);
  CHECK(hnsw_id_ranks(Live{}, 0, &got) && got.empty());
  // what the input must not hold: a row beyond the slab, a row named twice, an id given twice, more nodes than rows
  const std::string a = "a", b = "b", a2 = "a";
  CHECK(!hnsw_id_ranks(Live{{&a, 2}}, 2, &got) && got.empty());
  CHECK(!hnsw_id_ranks(Live{{&a, 1}, {&b, 1}}, 2, &got) && got.empty());
  CHECK(!hnsw_id_ranks(Live{{&a, 0}, {&a2, 1}}, 2, &got) && got.empty());
  CHECK(!hnsw_id_ranks(Live{{&a, 0}, {&b, 1}}, 1, &got) && got.empty());
  CHECK(hnsw_id_ranks(Live{{&b, 0}, {&a, 1}}, 3, &got) && got == (std::vector<uint32_t>{1, 0, kHnswRankNoRow}));
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
