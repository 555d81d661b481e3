// fdeplan_check.cpp -- vettore_amd/csrc/host/vt_fdeplan.h on its own (no HIP), against a brute-force model: random id
// lists with duplicates, unknown ids and documents without vectors; budgets down to one document a chunk; every pattern
// of failed documents in a chunk of six.  tests/test_fdeplan.py builds it with AddressSanitizer and UBSan and runs it.
#include "../vettore_amd/csrc/host/vt_fdeplan.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>

using namespace vt_host;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

static size_t check_plans(std::mt19937 &rng) {
  size_t dup_lists = 0;
  for (int round = 0; round < 3000; ++round) {
    // the store: ids "d<i>" (some empty-named: the empty id is an id), each absent, empty or with rows
    const size_t universe = 1 + rng() % 12;
    std::vector<std::string> names;
    std::map<std::string, FdeDocState> store;
    for (size_t i = 0; i < universe; ++i) {
      std::string id = i == 0 && rng() % 3 == 0 ? std::string() : "d" + std::to_string(i * (rng() % 2 ? 1 : 11));
      names.push_back(id);
      const unsigned r = rng() % 4;
      if (r != 0) store[id] = r == 1 ? kFdeEmpty : kFdeRows;  // (r == 0: the store does not know it)
    }
    const size_t count = rng() % 25;
    std::string blob;
    std::vector<size_t> off{0};
    std::vector<std::string> listed;
    for (size_t i = 0; i < count; ++i) {
      const std::string &id = names[rng() % names.size()];
      listed.push_back(id);
      blob += id;
      off.push_back(blob.size());
    }
    size_t lookups = 0;
    FdeSyncPlan p;
    fde_sync_plan(count, blob.data(), off.data(), [&](const char *id, size_t n) {
      ++lookups;
      auto it = store.find(std::string(id, n));
      return it == store.end() ? kFdeAbsent : it->second;
    }, &p);

    // the model: distinct ids by first occurrence
    std::vector<std::string> distinct;
    std::vector<size_t> first_pos;
    for (size_t i = 0; i < count; ++i) {
      bool seen = false;
      for (const std::string &d : distinct) seen = seen || d == listed[i];
      if (!seen) {
        distinct.push_back(listed[i]);
        first_pos.push_back(i);
      }
    }
    dup_lists += distinct.size() < count;
    CHECK(lookups == distinct.size());
    CHECK(p.unique_of.size() == count && p.first_pos.size() == distinct.size() && p.state.size() == distinct.size());
    for (size_t u = 0; u < distinct.size(); ++u) {
      CHECK(p.first_pos[u] == first_pos[u]);
      auto it = store.find(distinct[u]);
      CHECK(p.state[u] == (it == store.end() ? kFdeAbsent : it->second));
    }
    for (size_t i = 0; i < count; ++i) CHECK(distinct[p.unique_of[i]] == listed[i]);
    std::vector<uint32_t> encode, remove;
    for (size_t u = 0; u < distinct.size(); ++u) (p.state[u] == kFdeRows ? encode : remove).push_back((uint32_t)u);
    CHECK(p.encode == encode && p.remove == remove);  // each distinct id exactly once, in list order, on one side
  }
  return dup_lists;
}

static void check_cuts(std::mt19937 &rng) {
  for (int round = 0; round < 3000; ++round) {
    const size_t n = rng() % 40;
    const size_t doc_bytes = rng() % 5 == 0 ? 0 : 1 + rng() % 100;
    const size_t budget = rng() % 4 == 0 ? rng() % (doc_bytes + 1) : rng() % 1000;  // (often below one document)
    const size_t max_docs = 1 + rng() % (rng() % 2 ? 3 : 50);
    std::vector<size_t> cut;
    fde_chunk_cuts(n, doc_bytes, budget, max_docs, &cut);
    CHECK(!cut.empty() && cut.front() == 0 && cut.back() == n);
    CHECK(n > 0 || cut.size() == 1);
    for (size_t k = 0; k + 1 < cut.size(); ++k) {
      const size_t docs = cut[k + 1] - cut[k];
      CHECK(docs >= 1 && docs <= max_docs);
      CHECK(docs == 1 || docs * doc_bytes <= budget);  // within the budget, or one document alone
      if (k + 2 < cut.size())                          // greedy: one more would not have fitted
        CHECK(docs == max_docs || (docs + 1) * doc_bytes > budget);
    }
    if (doc_bytes && budget < 2 * doc_bytes) CHECK(cut.size() == n + 1);  // one document per chunk
  }
}

static void check_runs() {
  for (unsigned pattern = 0; pattern < 64; ++pattern) {
    int status[6];
    for (int i = 0; i < 6; ++i) status[i] = (pattern >> i) & 1 ? 28 : 0;
    std::vector<std::pair<size_t, size_t>> runs;
    fde_good_runs(status, 6, &runs);
    std::set<size_t> covered;
    size_t last_end = 0;
    for (size_t r = 0; r < runs.size(); ++r) {
      CHECK(runs[r].first < runs[r].second && runs[r].second <= 6);
      CHECK(r == 0 ? true : runs[r].first > last_end);  // maximal: a failed document lies between two runs
      for (size_t i = runs[r].first; i < runs[r].second; ++i) {
        CHECK(status[i] == 0);
        covered.insert(i);
      }
      last_end = runs[r].second;
    }
    for (size_t i = 0; i < 6; ++i) CHECK((covered.count(i) == 1) == (status[i] == 0));
  }
  std::vector<std::pair<size_t, size_t>> runs{{1, 2}};
  fde_good_runs(nullptr, 0, &runs);
  CHECK(runs.empty());
}

int main() {
  std::mt19937 rng(20261019);
  const size_t dup_lists = check_plans(rng);
  CHECK(dup_lists > 1000);
  check_cuts(rng);
  check_runs();
  std::printf("ok\n");
  return 0;
}
