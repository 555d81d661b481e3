// Drives vettore_amd/csrc/host/vt_mmrplan.h -- the host code of MMR reranking that needs no device -- from a script on
// stdin, one answer per line (tests/test_mmr_host.py compares each with tests/mmr_ref.py and index_flat.result_values).
// Built stand-alone with the sanitizers.  Doubles and floats travel as the hex of their bits.
//   G <alpha bits> <final_k>                  -> 1 | 0                       mmr_guards_ok
//   S <count> <score bits>...                 -> 1 | 0                       mmr_scores_ok
//   H <metric> <raw f32 bits> <score_mode>    -> <score bits>                mmr_hit_score
//   T <count> <id hex | ->...                 (the id table: row i holds id i)
//   E <id hex | ->                            (swap-delete of an id, as shard_delete moves rows)
//   R <count> <id hex | ->...                 -> rows... | bad               mmr_rows_of_ids
//   L <njobs> <n>:<k>...                      -> off:n:kk... total max_n max_kk | bad     mmr_layout
//   C <p> <status> <count> <order>...         -> status: order...            mmr_collect over the last layout (order: all slots)
#include "../vettore_amd/csrc/host/vt_mmrplan.h"

#include <cstdio>
#include <cstring>
#include <iostream>

struct Problem {
  uint32_t off, n, kk, pad;
  double alpha;
};

static std::string unhex(const std::string &h) {
  std::string s;
  if (h == "-") return s;
  for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
  return s;
}
static double f64_of(const std::string &h) {
  const uint64_t u = std::stoull(h, nullptr, 16);
  double d;
  std::memcpy(&d, &u, 8);
  return d;
}
static float f32_of(const std::string &h) {
  const uint32_t u = (uint32_t)std::stoul(h, nullptr, 16);
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

int main() {
  std::vector<std::string> ids;
  vt_host::IdTable table(&ids);
  vt_host::MmrLayout<Problem> lay;
  std::string op;
  while (std::cin >> op) {
    if (op == "G") {
      std::string a;
      size_t k;
      std::cin >> a >> k;
      std::printf("%d\n", vt_host::mmr_guards_ok(f64_of(a), k) ? 1 : 0);
    } else if (op == "S") {
      size_t n;
      std::cin >> n;
      std::vector<double> v(n);
      for (auto &x : v) {
        std::string h;
        std::cin >> h;
        x = f64_of(h);
      }
      std::printf("%d\n", vt_host::mmr_scores_ok(v.data(), n) ? 1 : 0);
    } else if (op == "H") {
      int metric, mode;
      std::string raw;
      std::cin >> metric >> raw >> mode;
      const double s = vt_host::mmr_hit_score(metric, f32_of(raw), mode);
      uint64_t u;
      std::memcpy(&u, &s, 8);
      std::printf("%016llx\n", (unsigned long long)u);
    } else if (op == "T") {
      size_t n;
      std::cin >> n;
      ids.clear();
      table.clear();
      table.reserve(n);
      for (size_t i = 0; i < n; ++i) {
        std::string h;
        std::cin >> h;
        ids.push_back(unhex(h));
        table.insert(vt_host::hash_id(ids.back().data(), ids.back().size()), (uint32_t)i);
      }
    } else if (op == "E") {
      std::string h;
      std::cin >> h;
      const std::string id = unhex(h);
      const uint64_t hash = vt_host::hash_id(id.data(), id.size());
      const uint32_t r = table.find(id.data(), id.size(), hash), last = (uint32_t)ids.size() - 1;
      if (r != vt_host::IdTable::kNone) {
        table.erase(id.data(), id.size(), hash);
        if (r != last) {
          table.move_row(ids[last].data(), ids[last].size(), vt_host::hash_id(ids[last].data(), ids[last].size()), r);
          ids[r] = std::move(ids[last]);
        }
        ids.pop_back();
      }
    } else if (op == "R") {
      size_t n;
      std::cin >> n;
      std::string blob;
      std::vector<size_t> off(n + 1, 0);
      for (size_t i = 0; i < n; ++i) {
        std::string h;
        std::cin >> h;
        blob += unhex(h);
        off[i + 1] = blob.size();
      }
      std::vector<uint32_t> rows;
      std::unordered_set<uint32_t> seen;
      if (!vt_host::mmr_rows_of_ids(table, n, blob.data(), off.data(), rows, seen)) {
        std::printf("bad\n");
      } else {
        for (uint32_t r : rows) std::printf("%u ", r);
        std::printf("\n");
      }
    } else if (op == "L") {
      size_t njobs;
      std::cin >> njobs;
      std::vector<vt_host::MmrJob> jobs(njobs);
      for (auto &j : jobs) {
        std::string spec;
        std::cin >> spec;
        const size_t colon = spec.find(':');
        j = vt_host::MmrJob{nullptr, nullptr, (size_t)std::stoull(spec.substr(0, colon)), (size_t)std::stoull(spec.substr(colon + 1)), 0.5};
      }
      if (!vt_host::mmr_layout(jobs.data(), njobs, &lay)) {
        std::printf("bad\n");
      } else {
        for (const Problem &q : lay.prob) std::printf("%u:%u:%u ", q.off, q.n, q.kk);
        std::printf("%zu %u %u\n", lay.total, lay.max_n, lay.max_kk);
      }
    } else if (op == "C") {
      size_t p;
      int status;
      uint32_t count;
      std::cin >> p >> status >> count;
      std::vector<uint32_t> order(lay.total);
      for (auto &o : order) std::cin >> o;
      std::vector<uint32_t> out;
      const int r = vt_host::mmr_collect(lay.prob[p], status, count, order.data(), &out);
      std::printf("%d:", r);
      for (uint32_t o : out) std::printf(" %u", o);
      std::printf("\n");
    }
  }
  return 0;
}
