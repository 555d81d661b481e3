// Drives vettore_amd/csrc/host/vt_hnswgraph.h from a script on stdin and prints the whole graph after every step
// (tests/test_hnsw_graph.py compares each line with tests/hnsw_ref.py).  Built stand-alone with the sanitizers.
//   P m m0 max_level
//   I <id hex> <dim> <layers>     then per layer, from layer 0 up:   <count> <internal id> <dist bits hex> ...
//   D <id hex>
#include "../vettore_amd/csrc/host/vt_hnswgraph.h"

#include <cstdio>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>

static std::string unhex(const std::string &h) {
  std::string s;
  for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
  return s;
}

int main() {
  std::unique_ptr<vt_host::HnswGraph> g;
  uint32_t rows = 0;
  std::string op;
  while (std::cin >> op) {
    if (op == "P") {
      size_t m, m0, lv;
      std::cin >> m >> m0 >> lv;
      g.reset(new vt_host::HnswGraph(m, m0, lv));
      continue;
    }
    if (op == "I") {
      std::string hex;
      long dim;
      size_t layers;
      std::cin >> hex >> dim >> layers;
      const std::string id = hex == "-" ? std::string() : unhex(hex);
      std::vector<std::vector<vt_host::HnswEdge>> lists(layers);
      for (size_t l = 0; l < layers; ++l) {
        size_t n;
        std::cin >> n;
        for (size_t i = 0; i < n; ++i) {
          uint64_t nid;
          std::string bits;
          std::cin >> nid >> bits;
          const uint32_t u = (uint32_t)std::stoul(bits, nullptr, 16);
          float d;
          std::memcpy(&d, &u, 4);
          lists[l].push_back(vt_host::HnswEdge{nid, d});
        }
      }
      g->erase(id);
      if (g->len() == 0) rows = 0;
      if (!g->ids_left()) return 2;
      const uint64_t iid = g->take_id();
      g->apply_insert(id, iid, g->level_for(id.data(), id.size()), rows++, dim, std::move(lists));
    } else if (op == "D") {
      std::string hex;
      std::cin >> hex;
      g->erase(hex == "-" ? std::string() : unhex(hex));
      if (g->len() == 0) rows = 0;
    } else {
      return 3;
    }
    // every list named as changed must exist or belong to an erased node; the dump is the whole graph
    std::map<uint64_t, const vt_host::HnswNode *> sorted;
    for (const auto &kv : g->nodes()) sorted[kv.first] = &kv.second;
    std::ostringstream o;
    o << g->next() << ' ' << (g->entry() == vt_host::HnswGraph::kNoEntry ? -1 : (long long)g->entry()) << ' ' << g->dimension()
      << ' ' << g->len();
    size_t edges = 0;
    for (const auto &kv : sorted) {
      o << " |" << kv.first << ':' << kv.second->level;
      for (const auto &l : kv.second->conn) {
        o << ';';
        for (size_t i = 0; i < l.size(); ++i) o << (i ? "," : "") << l[i].id;
        edges += l.size();
      }
    }
    if (edges != g->edges()) return 4;
    g->clear_changed();
    std::puts(o.str().c_str());
  }
  return 0;
}
