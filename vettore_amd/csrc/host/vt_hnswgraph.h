// vt_hnswgraph.h -- the authoritative graph of an HNSW index (vt_hnsw): the reference's HnswIndex (hnsw.rs) without its
// distance computations.  Stand-alone (no HIP, no other header of this directory): tests/test_hnsw_graph.py builds it
// with g++ under the sanitizers and drives it against tests/hnsw_ref.py.  The device side -- the slab of rows, the
// mirror of the lists, the traversals (K11, vt_hnsw.hip) -- is host/vt_hnsw.h.
//
// What lives here: `next` (the internal-id counter: internal ids are the reference's and are never reused), per node its
// external id, level, slab row and one adjacency list per layer, external_to_internal, the entry and the dimension.
// A traversal hands over, per layer, the nodes search_layer kept with their rank distances to the new vector
// (hnsw.rs:189-207); apply_insert sorts by (distance, internal id), dedups, truncates to m0 / m, links back and prunes
// (hnsw.rs:224-236, :437-465) and updates the entry (:238-242).
//
// Every edge keeps its rank distance to the list's owner.  The distance prune() needs for the new node in a neighbour's
// list, rank_distance(neighbour, new), is the very value the traversal computed with the same argument order, and the
// f32 chains of L2 / dot are symmetric bit for bit, so the value kept for an edge a -> b serves b -> a as well: a prune
// is a sort by (kept distance, id) and a truncation, no distance is computed twice, and a prune cannot fail once the
// traversal succeeded.
//
// Slab rows: a node's row is handed out by the caller and stays the node's until the caller compacts its slab
// (host/vt_hnswplan.h says when): close_rows() then renumbers the live nodes 0 .. len() - 1 in the order of their old
// rows, which is the order of the internal ids, and that is all it changes.  Rows also come back when the last node
// goes and the slab with it.
//
// Out of scope, on purpose: an internal-id counter that reaches 2^32 refuses further inserts (VT_ERR_NOMEM at the
// C ABI): the device addresses nodes with 32 bits.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace vt_host {

struct HnswEdge {
  uint64_t id;
  float dist;  // rank distance to the owner of the list
};

// f32::total_cmp as an order-preserving u32
inline uint32_t hnsw_orderable(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline bool hnsw_edge_less(const HnswEdge &a, const HnswEdge &b) {
  const uint32_t ka = hnsw_orderable(a.dist), kb = hnsw_orderable(b.dist);
  return ka != kb ? ka < kb : a.id < b.id;
}

struct HnswNode {
  std::string external_id;
  uint32_t level = 0;
  uint32_t row = 0;                           // the node's row of the device slab
  std::vector<std::vector<HnswEdge>> conn;    // [level + 1], each sorted by (dist, id)
};

class HnswGraph {
 public:
  static constexpr uint64_t kNoEntry = ~0ull;
  static constexpr uint64_t kMaxIds = 1ull << 32;

  HnswGraph(size_t m, size_t m0, size_t max_level) : m_(m), m0_(m0), max_level_(max_level) {}

  size_t len() const { return nodes_.size(); }
  long dimension() const { return dim_; }
  uint64_t next() const { return next_; }
  uint64_t entry() const { return entry_; }
  size_t edges() const { return edges_; }
  const std::unordered_map<uint64_t, HnswNode> &nodes() const { return nodes_; }
  const HnswNode *node(uint64_t id) const {
    auto it = nodes_.find(id);
    return it == nodes_.end() ? nullptr : &it->second;
  }
  // the internal id of a live external id, kNoEntry when there is none
  uint64_t find(const std::string &external_id) const {
    auto it = by_ext_.find(external_id);
    return it == by_ext_.end() ? kNoEntry : it->second;
  }

  // hnsw.rs:473-497: FNV-1a of the id's bytes, one level per pair of zero bits from the bottom
  uint32_t level_for(const char *id, size_t n) const {
    uint64_t hash = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) {
      hash ^= (uint64_t)(unsigned char)id[i];
      hash *= 0x00000100000001B3ull;
    }
    uint32_t level = 0;
    while (level < max_level_ && (hash & 3u) == 0) {
      ++level;
      hash >>= 2;
    }
    return level;
  }

  bool ids_left() const { return next_ < kMaxIds; }
  // hnsw.rs:159-160: the insert's internal id (taken whether or not the insert's traversal succeeds later)
  uint64_t take_id() { return next_++; }

  // hnsw.rs:163-177 (an empty graph: lists.empty()) and :187-242.  lists[layer]: what search_layer returned on that
  // layer, in any order, for layer <= min(level, top layer); missing layers are empty.
  void apply_insert(const std::string &external_id, uint64_t id, uint32_t level, uint32_t row, long dim,
                    std::vector<std::vector<HnswEdge>> lists) {
    HnswNode n;
    n.external_id = external_id;
    n.level = level;
    n.row = row;
    n.conn.resize((size_t)level + 1);
    for (size_t layer = 0; layer < lists.size() && layer <= level; ++layer) {
      std::vector<HnswEdge> &c = lists[layer];
      std::sort(c.begin(), c.end(), hnsw_edge_less);
      c.erase(std::unique(c.begin(), c.end(), [](const HnswEdge &a, const HnswEdge &b) { return a.id == b.id; }), c.end());
      const size_t limit = layer == 0 ? m0_ : m_;
      if (c.size() > limit) c.resize(limit);
      n.conn[layer] = std::move(c);
      edges_ += n.conn[layer].size();
    }
    const bool first = nodes_.empty();
    auto &stored = nodes_[id] = std::move(n);
    by_ext_[external_id] = id;
    dim_ = dim;
    for (uint32_t layer = 0; layer <= level; ++layer) touch(id, layer);
    if (first) {
      entry_ = id;
      return;
    }
    for (uint32_t layer = 0; layer <= level; ++layer) {
      const std::vector<HnswEdge> mine = stored.conn[layer];  // (a copy: reciprocal_connections)
      for (const HnswEdge &e : mine) {
        auto it = nodes_.find(e.id);
        if (it == nodes_.end()) continue;
        HnswNode &nb = it->second;
        if (layer >= nb.conn.size()) continue;
        std::vector<HnswEdge> &l = nb.conn[layer];
        bool present = false;
        for (const HnswEdge &x : l) present = present || x.id == id;
        if (!present) {
          l.push_back(HnswEdge{id, e.dist});
          ++edges_;
        }
        prune(l, layer);
        touch(e.id, layer);
      }
    }
    if (entry_ != kNoEntry && level > nodes_[entry_].level) entry_ = id;
  }

  // hnsw.rs:263-289; false: no such id
  bool erase(const std::string &external_id) {
    auto bi = by_ext_.find(external_id);
    if (bi == by_ext_.end()) return false;
    const uint64_t id = bi->second;
    by_ext_.erase(bi);
    for (const auto &l : nodes_[id].conn) edges_ -= l.size();
    nodes_.erase(id);
    for (auto &kv : nodes_) {
      HnswNode &n = kv.second;
      for (uint32_t layer = 0; layer < n.conn.size(); ++layer) {
        std::vector<HnswEdge> &l = n.conn[layer];
        const size_t before = l.size();
        l.erase(std::remove_if(l.begin(), l.end(), [&](const HnswEdge &e) { return e.id == id; }), l.end());
        if (l.size() != before) {
          edges_ -= before - l.size();
          touch(kv.first, layer);
        }
      }
    }
    if (entry_ == id) {
      // the maximum of (layer, reversed external id): the highest layer, among those the smallest id bytes
      entry_ = kNoEntry;
      const HnswNode *best = nullptr;
      for (const auto &kv : nodes_) {
        const HnswNode &n = kv.second;
        if (!best || n.level > best->level || (n.level == best->level && n.external_id < best->external_id)) {
          best = &n;
          entry_ = kv.first;
        }
      }
    }
    if (nodes_.empty()) {
      dim_ = -1;
      changed_.clear();  // (the mirror goes with the slab)
    }
    return true;
  }

  // The slab was compacted: every live node's (old row, level) in row order, and node.row = its place in that list.
  // Levels, lists, entry, ids and the changed lists stay as they are.
  std::vector<std::pair<uint32_t, uint32_t>> close_rows() {
    std::vector<std::pair<uint32_t, HnswNode *>> by_row;
    by_row.reserve(nodes_.size());
    for (auto &kv : nodes_) by_row.emplace_back(kv.second.row, &kv.second);
    std::sort(by_row.begin(), by_row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    std::vector<std::pair<uint32_t, uint32_t>> out;
    out.reserve(by_row.size());
    for (size_t i = 0; i < by_row.size(); ++i) {
      out.emplace_back(by_row[i].first, by_row[i].second->level);
      by_row[i].second->row = (uint32_t)i;
    }
    return out;
  }

  // The adjacency lists that changed since the last clear_changed(), as (internal id, layer): the device mirror is
  // patched, not uploaded again.  A list may be named more than once; lists of erased nodes may be named too.
  const std::vector<std::pair<uint64_t, uint32_t>> &changed() const { return changed_; }
  void clear_changed() { changed_.clear(); }

 private:
  void touch(uint64_t id, uint32_t layer) { changed_.emplace_back(id, layer); }
  // hnsw.rs:437-465 with the kept distances
  void prune(std::vector<HnswEdge> &l, uint32_t layer) {
    const size_t limit = layer == 0 ? m0_ : m_;
    std::sort(l.begin(), l.end(), hnsw_edge_less);
    if (l.size() > limit) {
      edges_ -= l.size() - limit;
      l.resize(limit);
    }
  }

  size_t m_, m0_, max_level_;
  std::unordered_map<uint64_t, HnswNode> nodes_;
  std::unordered_map<std::string, uint64_t> by_ext_;
  std::vector<std::pair<uint64_t, uint32_t>> changed_;
  uint64_t entry_ = kNoEntry, next_ = 0;
  size_t edges_ = 0;
  long dim_ = -1;
};

}  // namespace vt_host
