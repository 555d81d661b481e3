// vt_hnswstage.h -- quantized_search, funnel_search and hybrid_search (collection.ex:232-348) on the HNSW index: the
// stages of host/vt_quantized.h, vt_search.h (funnel_rows / funnel_stage) and vt_hybrid.h over the slab where it lies,
// scored by K15 (vt_hnsw_stage.hip), selected by K3 through collect_from_keys.
// Part of vt_index.cpp's translation unit (included there, in this order, exactly once).
//
// Nothing here depends on the graph but the hybrid search's VT_GEN_SEARCH generator (the handle's own traversal with
// limit = candidates, its rows in result order): binary_top_k and vector_top_k order by (rank.total_cmp, id bytes)
// whatever order their candidates arrive in, and the slab holds the vectors as they were given.  So over the same
// (id, vector) pairs the answers are the flat handle's, bit for bit.  Validation order, status codes and the rules for an
// empty answer are those of quantized_ready, funnel_ready and hybrid_ready, with the live node count for ix->n.
//
// The id-rank column (host/vt_hnswrank.h) is rebuilt -- (id, row) of every live node, one sort, one upload -- by the first
// staged call after the row set changed: an insert, an upsert, a delete, a compaction, the last node's going
// (vt_hnsw::epoch counts them).  A plain search never pays for it.  The caller holds the handle's mutex for the whole call.
#pragma once

namespace {

// The three staged entry points of the C ABI (vt_flat_quantized_search, vt_flat_funnel_search, vt_flat_hybrid_search)
// take an HNSW handle in the flat one's place (VT_HNSW_STAGED, include/vettore_flat.h: the set of exported symbols is
// pinned).  Every live vt_hnsw is known here, so a pointer is told apart without looking at what it points to; while no
// HNSW handle lives the flat path pays one relaxed load.
std::mutex g_hnsw_live_mu;
std::unordered_set<const void *> g_hnsw_live;
std::atomic<size_t> g_hnsw_live_count{0};

void hnsw_staged_register(vt_hnsw *h) {
  std::lock_guard<std::mutex> g(g_hnsw_live_mu);
  g_hnsw_live.insert(h);
  g_hnsw_live_count.store(g_hnsw_live.size(), std::memory_order_release);
}
void hnsw_staged_unregister(vt_hnsw *h) {
  std::lock_guard<std::mutex> g(g_hnsw_live_mu);
  g_hnsw_live.erase(h);
  g_hnsw_live_count.store(g_hnsw_live.size(), std::memory_order_release);
}
vt_hnsw *hnsw_staged_handle(const void *p) {
  if (g_hnsw_live_count.load(std::memory_order_acquire) == 0) return nullptr;
  std::lock_guard<std::mutex> g(g_hnsw_live_mu);
  return g_hnsw_live.count(p) ? static_cast<vt_hnsw *>(const_cast<void *>(p)) : nullptr;
}

// dIdRank as the row set is now
int hnsw_stage_ranks(vt_hnsw *h) {
  if (h->rank_epoch == h->epoch && h->dIdRank.p) return VT_OK;
  std::vector<std::pair<const std::string *, uint32_t>> live;
  live.reserve(h->graph.len());
  for (uint64_t r = 0; r < h->rows_used; ++r) {
    const vt_host::HnswNode *n = h->graph.node(h->row_id[(size_t)r]);
    if (n && n->row == r) live.emplace_back(&n->external_id, (uint32_t)r);
  }
  std::vector<uint32_t> ranks;
  if (live.size() != h->graph.len() || !vt_host::hnsw_id_ranks(live, (size_t)h->rows_used, &ranks))
    return fail(VT_ERR_DEVICE, "hnsw index: the slab's rows and the graph's nodes do not match");
  VT_TRY(h->hStageWords.ensure(ranks.size()));
  VT_TRY(h->dIdRank.ensure(ranks.size()));
  std::memcpy(h->hStageWords.p, ranks.data(), ranks.size() * sizeof(uint32_t));
  hipStream_t s = h->ctx.stream;
  VT_HIP(hipMemcpyAsync(h->dIdRank.p, h->hStageWords.p, ranks.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  VT_HIP(hipStreamSynchronize(s));  // (the pinned block carries a stage's row list next)
  h->rank_epoch = h->epoch;
  return VT_OK;
}

// What every staged call does first once it has something to score: the device, the rank column, and the query -- its
// floats padded to the slab's stride, behind them its sign bits in K15b's order -- in one copy.
int hnsw_stage_begin(vt_hnsw *h, const float *query) {
  VT_TRY(h->ctx.bind());
  if (h->rows_used >= vt::kHnswNoRow) return fail(VT_ERR_UNSUPPORTED, "hnsw index: more than 2^32 - 2 rows");
  VT_TRY(hnsw_stage_ranks(h));
  const uint32_t d = h->d, qs = h->stride;
  const size_t total = (size_t)qs + 2 * vt::hnsw_stage_qword_count(d);  // (qs is a multiple of 4: the words are 16-byte aligned)
  VT_TRY(h->hStageQ.ensure(total));
  VT_TRY(h->dStageQ.ensure(total));
  std::memcpy(h->hStageQ.p, query, (size_t)d * sizeof(float));
  for (uint32_t e = d; e < qs; ++e) h->hStageQ.p[e] = 0.0f;
  vt::hnsw_stage_qwords(query, d, reinterpret_cast<uint64_t *>(h->hStageQ.p + qs));
  VT_HIP(hipMemcpyAsync(h->dStageQ.p, h->hStageQ.p, total * sizeof(float), hipMemcpyHostToDevice, h->ctx.stream));
  return VT_OK;
}

int hnsw_stage_collect(vt_hnsw *h, uint32_t m, size_t want, std::vector<vt::Entry> &out) {
  const int rc = collect_from_keys(h->ctx, h->dStageKeys.p, h->dStagePay.p, m, want, out);
  if (rc == kRetryInternal) return fail(VT_ERR_DEVICE, "hnsw index: the selection of a staged search did not come back");
  return rc;
}

// binary_top_k (search.rs:76-92) over every live row: the `want` nearest by sign-bit Hamming distance, ascending
int hnsw_stage_bits(vt_hnsw *h, size_t want, std::vector<vt::Entry> &out) {
  const uint32_t rows = (uint32_t)h->rows_used;
  VT_TRY(h->dStageKeys.ensure(rows));
  VT_TRY(h->dStagePay.ensure(rows));
  vt::HnswStageBitsArgs a{};
  a.X = h->X.p;
  a.stride = h->stride;
  a.d = h->d;
  a.rows = rows;
  a.id_rank = h->dIdRank.p;
  a.qwords = reinterpret_cast<const uint64_t *>(h->dStageQ.p + h->stride);
  a.keys = h->dStageKeys.p;
  a.pay = h->dStagePay.p;
  VT_HIP(vt::launch_hnsw_stage_bits(a, h->ctx.stream));
  return hnsw_stage_collect(h, rows, want, out);
}

// One vector_top_k stage (search.rs:38-73): prefix length p, over every live row (`rows` null) or over the rows of the
// previous stage; keeps `want` >= 1 hits, ascending.
int hnsw_stage_score(vt_hnsw *h, const float *query, uint32_t p, const std::vector<uint32_t> *rows, size_t want,
                     std::vector<vt::Entry> &out) {
  hipStream_t s = h->ctx.stream;
  const uint32_t n = rows ? (uint32_t)rows->size() : (uint32_t)h->rows_used;
  if (rows) {
    for (uint32_t r : *rows)
      if (r >= h->rows_used) return fail(VT_ERR_DEVICE, "hnsw index: a stage named a row that is not there");
    VT_TRY(h->hStageWords.ensure(n));
    VT_TRY(h->dStageRows.ensure(n));
    std::memcpy(h->hStageWords.p, rows->data(), (size_t)n * sizeof(uint32_t));
    // (pinned: the block is written again only behind the wait that ends this stage)
    VT_HIP(hipMemcpyAsync(h->dStageRows.p, h->hStageWords.p, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  }
  VT_TRY(h->dStageKeys.ensure(n));
  VT_TRY(h->dStagePay.ensure(n));
  vt::HnswStageScoreArgs a{};
  a.X = h->X.p;
  a.stride = h->stride;
  a.d = h->d;
  a.rows = (uint32_t)h->rows_used;
  a.p = p;
  a.q = h->dStageQ.p;
  if (h->metric == VT_COSINE)  // f64_dot(q, q) over the prefix (distances.rs:179-185)
    for (uint32_t j = 0; j < p; ++j) a.qq += (double)query[j] * (double)query[j];
  a.id_rank = h->dIdRank.p;
  a.list = rows ? h->dStageRows.p : nullptr;
  a.n = n;
  a.metric = h->metric;
  a.order = h->order;
  a.keys = h->dStageKeys.p;
  a.pay = h->dStagePay.p;
  a.status = h->ctx.dStatus.p;
  VT_HIP(vt::launch_hnsw_stage_score(a, s));
  return hnsw_stage_collect(h, n, want, out);
}

void hnsw_rows_of(const std::vector<vt::Entry> &entries, std::vector<uint32_t> &rows) {
  rows.resize(entries.size());
  for (size_t i = 0; i < entries.size(); ++i) rows[i] = entries[i].row;
}

// Candidate rows of one funnel pass (collection.ex:674-691) without the final rerank: funnel_rows on the slab.
int hnsw_funnel_rows(vt_hnsw *h, const float *query, const size_t *stages, size_t nstages, size_t candidates,
                     std::vector<uint32_t> &rows) {
  rows.clear();
  std::vector<vt::Entry> kept;
  for (size_t i = 0; i < nstages; ++i) {
    kept.clear();
    VT_TRY(hnsw_stage_score(h, query, (uint32_t)stages[i], i == 0 ? nullptr : &rows, candidates, kept));
    hnsw_rows_of(kept, rows);
    if (rows.empty()) break;
  }
  return VT_OK;
}

// the hit list of `entries`: the id bytes from the graph
int hnsw_stage_hits(vt_hnsw *h, const std::vector<vt::Entry> &entries, vt_hits **out) {
  auto hits = std::make_unique<vt_hits>();
  for (const vt::Entry &e : entries) {
    const vt_host::HnswNode *n = e.row < h->rows_used ? h->graph.node(h->row_id[e.row]) : nullptr;
    if (!n || n->row != e.row) return fail(VT_ERR_DEVICE, "hnsw index: a stage named a row that is not there");
    hits->ids.push_back(n->external_id);
    hits->raw.push_back(e.raw);
    hits->rank_key.push_back(rank_key_of(e.key));
  }
  *out = hits.release();
  return VT_OK;
}

// exact_rerank on the full vectors (collection.ex:821-851), cut to `limit`
int hnsw_stage_rerank(vt_hnsw *h, const float *query, const std::vector<uint32_t> &rows, size_t limit, vt_hits **out) {
  if (rows.empty()) return empty_hits(out);
  std::vector<vt::Entry> entries;
  VT_TRY(hnsw_stage_score(h, query, h->d, &rows, limit, entries));
  return hnsw_stage_hits(h, entries, out);
}

// collection.ex:276-295 (quantized_ready)
int hnsw_quantized(vt_hnsw *h, const float *query, size_t n, size_t candidates, size_t limit, vt_hits **out) {
  if (h->poisoned) return VT_ERR_HNSW_POISONED;
  VT_TRY(validate_vector(query, n, h->graph.dimension()));
  const size_t live = h->graph.len();
  if (live == 0 || candidates == 0 || limit == 0) return empty_hits(out);
  VT_TRY(hnsw_stage_begin(h, query));
  std::vector<vt::Entry> cand;
  VT_TRY(hnsw_stage_bits(h, std::min(candidates, live), cand));
  std::vector<uint32_t> rows;
  hnsw_rows_of(cand, rows);
  return hnsw_stage_rerank(h, query, rows, limit, out);
}

// collection.ex:245-260 (funnel_ready)
int hnsw_funnel(vt_hnsw *h, const float *query, size_t n, const size_t *stages, size_t nstages, size_t candidates, size_t limit,
                vt_hits **out) {
  if (h->poisoned) return VT_ERR_HNSW_POISONED;
  VT_TRY(validate_vector(query, n, h->graph.dimension()));
  if (nstages == 0) return VT_ERR_PREFIX;
  for (size_t i = 0; i < nstages; ++i)
    if (stages[i] == 0 || stages[i] > n) return VT_ERR_PREFIX;
  if (h->graph.len() == 0 || candidates == 0 || limit == 0) return empty_hits(out);
  VT_TRY(hnsw_stage_begin(h, query));
  std::vector<uint32_t> rows;
  VT_TRY(hnsw_funnel_rows(h, query, stages, nstages, candidates, rows));
  return hnsw_stage_rerank(h, query, rows, limit, out);
}

// collection.ex:325-345 (hybrid_ready)
int hnsw_hybrid(vt_hnsw *h, const float *query, size_t n, const int *kinds, const size_t *candidates, const size_t *stage_off,
                const size_t *stages, size_t ngen, size_t limit, vt_hits **out) {
  if (h->poisoned) return VT_ERR_HNSW_POISONED;
  VT_TRY(validate_vector(query, n, h->graph.dimension()));
  if (ngen == 0) return VT_ERR_ARGUMENT;
  for (size_t i = 0; i < ngen; ++i) {
    if (kinds[i] < VT_GEN_FUNNEL || kinds[i] > VT_GEN_SEARCH || candidates[i] == 0) return VT_ERR_ARGUMENT;
    if (kinds[i] == VT_GEN_FUNNEL) {
      if (stage_off[i + 1] <= stage_off[i]) return VT_ERR_PREFIX;
      for (size_t j = stage_off[i]; j < stage_off[i + 1]; ++j)
        if (stages[j] == 0 || stages[j] > n) return VT_ERR_PREFIX;
    }
  }
  const size_t live = h->graph.len();
  if (live == 0 || limit == 0) return empty_hits(out);
  VT_TRY(hnsw_stage_begin(h, query));
  // hybrid_candidates (collection.ex:515-532): every generator's candidates, first occurrence wins
  std::vector<uint32_t> all, rows;
  std::unordered_set<uint32_t> seen;
  std::vector<vt::Entry> kept;
  for (size_t i = 0; i < ngen; ++i) {
    if (kinds[i] == VT_GEN_FUNNEL) {
      VT_TRY(hnsw_funnel_rows(h, query, stages + stage_off[i], stage_off[i + 1] - stage_off[i], candidates[i], rows));
    } else if (kinds[i] == VT_GEN_QUANTIZED) {
      kept.clear();
      VT_TRY(hnsw_stage_bits(h, std::min(candidates[i], live), kept));
      hnsw_rows_of(kept, rows);
    } else {  // hnsw_candidates (collection.ex:594-600): the index's own search with limit = candidates, in result order
      vt_hits *found = nullptr;
      int status = VT_OK;
      VT_TRY(hnsw_search_many(h, query, 1, n, candidates[i], &found, &status));
      std::unique_ptr<vt_hits> own(found);
      if (status != VT_OK) return status;
      rows.clear();
      for (const std::string &id : own->ids) {
        const vt_host::HnswNode *node = h->graph.node(h->graph.find(id));
        if (!node) return fail(VT_ERR_DEVICE, "hnsw index: a search named a node that is not there");
        rows.push_back(node->row);
      }
    }
    for (uint32_t r : rows)
      if (seen.insert(r).second) all.push_back(r);
  }
  // hybrid_rerank :exact == exact_rerank (collection.ex:627-630, :821-851)
  return hnsw_stage_rerank(h, query, all, limit, out);
}

}  // namespace
