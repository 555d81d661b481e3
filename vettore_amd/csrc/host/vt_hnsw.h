// vt_hnsw.h -- the HNSW index (vt_hnsw): the reference's HnswIndex (hnsw.rs) with its traversals on the device.
// The authoritative graph is host/vt_hnswgraph.h; here are the slab of rows, the device mirror of the lists, the
// traversal launches (K11, vt_hnsw.hip) and what the host does around them: validation in the reference's order,
// the sort of a search's results by (rank, external id bytes), the rerun of a traversal that outgrew its scratch.
// Part of vt_index.cpp's translation unit (included there, in this order, exactly once).
//
// The contract: after any inserts and deletes the graph -- levels, entry, every list -- is the reference's, and a search
// returns the reference's ids in its order with the raw values' bits.  One mutex per handle, every call exclusive.
// Rows are handed out in insertion order and never reused while a node lives, so a row number orders like the internal
// id and the device names nodes by rows.  The row of a deleted node stays dead until an insert finds more dead rows
// than live ones (host/vt_hnswplan.h: the rule, never on a delete): then the survivors are gathered in row order into
// a fresh slab and mirror with every list entry renumbered (K11c), and the buffers may shrink.  The slab doubles by
// allocate + copy; when the last node goes the slab and the dimension go too (`next` keeps counting).
#pragma once

struct vt_hnsw {
  std::mutex mu;
  Ctx ctx;  // (first: its stream goes last)
  int metric = 0, order = 0;
  size_t m = 0, m0 = 0, ef_construction = 0, ef_search = 0;
  vt_host::HnswGraph graph;
  bool poisoned = false;
  // the slab and the mirror: [capacity] rows
  DevBuf<float> X;
  DevBuf<uint32_t> dAdj0, dLevel, dUpoff, dUpper;
  uint32_t stride = 0, d = 0;
  uint64_t capacity = 0, rows_used = 0, dead_rows = 0, upper_used = 0;
  std::vector<uint64_t> row_id;      // the internal id each used row was handed to
  std::vector<uint32_t> row_upoff;   // where each used row's upper-layer lists start in dUpper
  // staging and scratch
  PinnedBuf<float> hRows;
  PinnedBuf<vt::HnswPatch> hPatch;
  DevBuf<vt::HnswPatch> dPatch;
  DevBuf<float> dQ;
  DevBuf<uint64_t> dScratch;
  DevBuf<uint32_t> dOut, dQmap;
  PinnedBuf<uint32_t> hOut;
  // vt_hnsw_counters: launches of the traversal kernel, traversals asked for, traversals run again with full scratch
  uint64_t launches = 0, traversals = 0, reruns = 0;
  // the staged searches (host/vt_hnswstage.h): `epoch` counts the changes of the row set -- an insert, a delete, a
  // compaction, the last node's going --, rank_epoch is the one dIdRank was built at; the query (floats, then its sign bits
  // in K15b's order), a stage's row list, and its key and payload columns
  uint64_t epoch = 1, rank_epoch = 0;
  DevBuf<uint32_t> dIdRank, dStageRows;
  PinnedBuf<uint32_t> hStageWords;
  DevBuf<float> dStageQ;
  PinnedBuf<float> hStageQ;
  DevBuf<uint64_t> dStageKeys;
  DevBuf<vt::Payload> dStagePay;

  vt_hnsw(size_t m_, size_t m0_, size_t max_level) : graph(m_, m0_, max_level) {}
};

namespace {

// HnswParams::validate (hnsw.rs:25-49), in its order
int hnsw_check_params(size_t m, size_t m0, size_t ef_construction, size_t ef_search, size_t max_level) {
  if (m == 0) return VT_ERR_HNSW_M;
  if (m0 == 0) return VT_ERR_HNSW_M0;
  if (m > 1024 || m0 > 2048 || m0 < m) return VT_ERR_HNSW_DEGREE;
  if (ef_construction < m) return VT_ERR_HNSW_EF_CONSTRUCTION;
  if (ef_construction > 1000000) return VT_ERR_HNSW_EF_LIMIT;
  if (ef_search == 0 || ef_search > 1000000) return VT_ERR_HNSW_EF_SEARCH;
  if (max_level == 0 || max_level > 64) return VT_ERR_HNSW_MAX_LEVEL;
  return VT_OK;
}

template <typename T>
int hnsw_alloc(DevBuf<T> &b, size_t want) {
  b.release();
  const hipError_t e = hipMalloc(reinterpret_cast<void **>(&b.p), std::max<size_t>(want, 1) * sizeof(T));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    b.p = nullptr;
    return fail(e == hipErrorOutOfMemory ? VT_ERR_NOMEM : VT_ERR_DEVICE, std::string("hnsw index: ") + hipGetErrorString(e));
  }
  b.count = std::max<size_t>(want, 1);
  return VT_OK;
}

inline uint64_t hnsw_pow2(uint64_t v) {
  uint64_t p = 2;
  while (p < v) p <<= 1;
  return p;
}

// the last node went: slab, mirror and dimension with it
void hnsw_forget(vt_hnsw *h) {
  h->X.release();
  h->dAdj0.release();
  h->dLevel.release();
  h->dUpoff.release();
  h->dUpper.release();
  h->stride = h->d = 0;
  h->capacity = h->rows_used = h->dead_rows = h->upper_used = 0;
  h->row_id.clear();
  h->row_upoff.clear();
  ++h->epoch;
}

// room for `rows` rows and `upper` words of upper-layer lists: nothing changes when an allocation fails
int hnsw_reserve(vt_hnsw *h, uint64_t rows, uint64_t upper) {
  hipStream_t s = h->ctx.stream;
  if (rows > h->capacity) {
    const uint64_t cap = vt_host::hnsw_capacity_for(rows);
    DevBuf<float> nX;
    DevBuf<uint32_t> nAdj, nLevel, nUpoff;
    VT_TRY(hnsw_alloc(nX, (size_t)cap * h->stride));
    VT_TRY(hnsw_alloc(nAdj, (size_t)cap * (h->m0 + 1)));
    VT_TRY(hnsw_alloc(nLevel, (size_t)cap));
    VT_TRY(hnsw_alloc(nUpoff, (size_t)cap));
    if (h->rows_used) {
      const size_t u = (size_t)h->rows_used;
      VT_HIP(hipMemcpyAsync(nX.p, h->X.p, u * h->stride * sizeof(float), hipMemcpyDeviceToDevice, s));
      VT_HIP(hipMemcpyAsync(nAdj.p, h->dAdj0.p, u * (h->m0 + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
      VT_HIP(hipMemcpyAsync(nLevel.p, h->dLevel.p, u * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
      VT_HIP(hipMemcpyAsync(nUpoff.p, h->dUpoff.p, u * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
      VT_HIP(hipStreamSynchronize(s));
    }
    mv_swap(h->X, nX);
    mv_swap(h->dAdj0, nAdj);
    mv_swap(h->dLevel, nLevel);
    mv_swap(h->dUpoff, nUpoff);
    h->capacity = cap;
  }
  if (upper > h->dUpper.count || !h->dUpper.p) {
    const uint64_t cap = vt_host::hnsw_upper_capacity_for(upper);
    DevBuf<uint32_t> nUp;
    VT_TRY(hnsw_alloc(nUp, (size_t)cap));
    if (h->upper_used) {
      VT_HIP(hipMemcpyAsync(nUp.p, h->dUpper.p, (size_t)h->upper_used * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
      VT_HIP(hipStreamSynchronize(s));
    }
    mv_swap(h->dUpper, nUp);
  }
  return VT_OK;
}

// The lists the graph says changed, and `extra`, into the mirror: one copy and one launch.
int hnsw_patch_mirror(vt_hnsw *h, std::vector<vt::HnswPatch> &extra) {
  std::vector<std::pair<uint64_t, uint32_t>> ch = h->graph.changed();
  h->graph.clear_changed();
  std::sort(ch.begin(), ch.end());
  ch.erase(std::unique(ch.begin(), ch.end()), ch.end());
  std::vector<vt::HnswPatch> &p = extra;
  for (const auto &c : ch) {
    const vt_host::HnswNode *n = h->graph.node(c.first);
    if (!n || c.second >= n->conn.size()) continue;  // (erased since)
    const std::vector<vt_host::HnswEdge> &l = n->conn[c.second];
    const uint32_t target = c.second == 0 ? 0u : 1u;
    const uint64_t base = c.second == 0 ? (uint64_t)n->row * (h->m0 + 1)
                                        : (uint64_t)h->row_upoff[n->row] + (uint64_t)(c.second - 1) * (h->m + 1);
    p.push_back(vt::HnswPatch{base, (uint32_t)l.size(), target});
    for (size_t i = 0; i < l.size(); ++i) p.push_back(vt::HnswPatch{base + 1 + i, h->graph.node(l[i].id)->row, target});
  }
  if (p.empty()) return VT_OK;
  VT_TRY(h->hPatch.ensure(p.size()));
  VT_TRY(h->dPatch.ensure(p.size()));
  std::memcpy(h->hPatch.p, p.data(), p.size() * sizeof(vt::HnswPatch));
  hipStream_t s = h->ctx.stream;
  VT_HIP(hipMemcpyAsync(h->dPatch.p, h->hPatch.p, p.size() * sizeof(vt::HnswPatch), hipMemcpyHostToDevice, s));
  VT_HIP(vt::launch_hnsw_patch(h->dPatch.p, (uint32_t)p.size(), h->dAdj0.p, h->dUpper.p, h->dLevel.p, h->dUpoff.p, s));
  VT_HIP(hipStreamSynchronize(s));
  return VT_OK;
}

// `nq` traversals in one launch (more only when their scratch would not fit in kHnswScratchBytes), the ones that
// outgrew their scratch once more with full-size scratch.  The output blocks land in h->hOut, `out_stride` words each.
constexpr size_t kHnswScratchBytes = (size_t)2 << 30;
int hnsw_traverse(vt_hnsw *h, int mode, uint32_t nq, const float *Q, uint32_t q_stride, uint32_t ef, uint32_t node_level,
                  uint32_t out_stride) {
  Ctx &c = h->ctx;
  hipStream_t s = c.stream;
  const vt_host::HnswNode *en = h->graph.node(h->graph.entry());
  if (!en) return fail(VT_ERR_DEVICE, "hnsw index: missing entry");
  if (h->rows_used + 64 > (1ull << 30)) return fail(VT_ERR_UNSUPPORTED, "hnsw index: more than 2^30 rows");
  vt::HnswTravArgs a{};
  a.g.X = h->X.p;
  a.g.stride = h->stride;
  a.g.d = h->d;
  a.g.adj0 = h->dAdj0.p;
  a.g.level = h->dLevel.p;
  a.g.upoff = h->dUpoff.p;
  a.g.upper = h->dUpper.p;
  a.g.m = (uint32_t)h->m;
  a.g.m0 = (uint32_t)h->m0;
  a.metric = h->metric;
  a.order = h->order;
  a.mode = mode;
  a.Q = Q;
  a.q_stride = q_stride;
  a.entry = en->row;
  a.top = en->level;
  a.node_level = node_level;
  a.ef = ef;
  a.out_stride = out_stride;
  vt::hnsw_tile_plan(h->d, h->stride, &a.tt, &a.ld);

  // scratch for the common case -- a few thousand visited nodes --, never more than what no traversal outgrows
  const uint64_t full = hnsw_pow2(h->rows_used + 64);
  long forced = 0;
#ifdef VT_TEST_HOOKS
  forced = vt::env::get(vt::env::TEST_HNSW_SCRATCH_CAP);  // (tests: the rerun at small shapes)
#endif
  uint64_t cap = forced > 0 ? hnsw_pow2((uint64_t)forced) : std::max<uint64_t>(4096, hnsw_pow2(8ull * ef));
  cap = std::min(cap, full);

  VT_TRY(h->dOut.ensure((size_t)nq * out_stride));
  VT_TRY(h->hOut.ensure((size_t)nq * out_stride));
  auto run = [&](uint32_t first, uint32_t count, const uint32_t *qmap, uint64_t cap_now) -> int {
    const size_t per_slot = (size_t)3 * cap_now * sizeof(uint64_t);
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(count, kHnswScratchBytes / per_slot));
    VT_TRY(h->dScratch.ensure((size_t)chunk * 3 * cap_now));
    a.cap = (uint32_t)cap_now;
    a.hshift = 32;
    for (uint64_t v = 2 * cap_now; v > 1; v >>= 1) --a.hshift;
    a.scratch = h->dScratch.p;
    a.out = h->dOut.p;
    for (uint32_t at = 0; at < count; at += chunk) {
      const uint32_t now = std::min(chunk, count - at);
      // (without a map slot t is query first + at + t: the query and output pointers move instead)
      vt::HnswTravArgs b = a;
      if (qmap) {
        b.qmap = qmap + at;
      } else {
        b.Q = Q + (size_t)(first + at) * q_stride;
        b.out = h->dOut.p + (size_t)(first + at) * out_stride;
      }
      VT_HIP(vt::launch_hnsw_traverse(b, now, s));
      ++h->launches;
    }
    return VT_OK;
  };
  h->traversals += nq;
  VT_TRY(run(0, nq, nullptr, cap));
  VT_HIP(hipMemcpyAsync(h->hOut.p, h->dOut.p, (size_t)nq * out_stride * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  VT_HIP(hipStreamSynchronize(s));
  std::vector<uint32_t> again;
  for (uint32_t i = 0; i < nq; ++i)
    if (h->hOut.p[(size_t)i * out_stride] == (uint32_t)vt::kHnswRetry) again.push_back(i);
  if (again.empty()) return VT_OK;
  if (cap >= full) return fail(VT_ERR_DEVICE, "hnsw index: a traversal outgrew full-size scratch");
  h->reruns += again.size();
  VT_TRY(h->dQmap.ensure(again.size()));
  VT_HIP(hipMemcpyAsync(h->dQmap.p, again.data(), again.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  VT_TRY(run(0, (uint32_t)again.size(), h->dQmap.p, full));
  VT_HIP(hipMemcpyAsync(h->hOut.p, h->dOut.p, (size_t)nq * out_stride * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  VT_HIP(hipStreamSynchronize(s));
  for (uint32_t i : again)
    if (h->hOut.p[(size_t)i * out_stride] == (uint32_t)vt::kHnswRetry)
      return fail(VT_ERR_DEVICE, "hnsw index: a traversal outgrew full-size scratch");
  return VT_OK;
}

// hnsw.rs:263-289 and what the mirror needs afterwards (an unknown id: nothing)
int hnsw_erase(vt_hnsw *h, const std::string &id, bool *mutated) {
  if (h->graph.find(id) == vt_host::HnswGraph::kNoEntry) return VT_OK;
  h->graph.erase(id);
  *mutated = true;
  ++h->dead_rows;
  ++h->epoch;
  if (h->graph.len() == 0) {
    hnsw_forget(h);
    return VT_OK;
  }
  std::vector<vt::HnswPatch> none;
  return hnsw_patch_mirror(h, none);
}

// hipMalloc into an empty buffer without a word in the call's error text; false: refused (the HIP error is cleared)
template <typename T>
bool hnsw_try_alloc(DevBuf<T> &b, size_t want) {
  b.release();
  want = std::max<size_t>(want, 1);
  if (hipMalloc(reinterpret_cast<void **>(&b.p), want * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    b.p = nullptr;
    return false;
  }
  b.count = want;
  return true;
}

// An insert into a graph with nodes, behind its erase: when the dead rows outnumber the live ones (vt_hnswplan.h) the
// survivors move, in row order, into a fresh slab and mirror (K11c).  Everything is allocated before anything changes,
// and a card without room for the second set of buffers means no compaction this time: no error, the handle as it
// was.  A HIP error leaves the handle as it was too.  A guard of the kernel that fired means the mirror had parted from
// the graph before: nothing is swapped, the handle is poisoned.
int hnsw_compact_if_due(vt_hnsw *h) {
  const uint64_t live = h->graph.len();
  if (live == 0 || !vt_host::hnsw_compact_due(live, h->dead_rows)) return VT_OK;
  std::vector<vt_host::HnswRowLevel> rl;
  rl.reserve((size_t)live);
  for (uint64_t r = 0; r < h->rows_used; ++r) {
    const vt_host::HnswNode *n = h->graph.node(h->row_id[(size_t)r]);
    if (n && n->row == r) rl.push_back(vt_host::HnswRowLevel{(uint32_t)r, n->level});
  }
  vt_host::HnswCompactPlan plan;
  if (rl.size() != live || !vt_host::hnsw_compact_plan(rl, h->m, &plan)) return VT_OK;  // (what fits now fits with fewer rows)

  DevBuf<float> nX;
  DevBuf<uint32_t> nAdj, nLevel, nUpoff, nUpper, dRemap, dPlan, dStatus;
  const size_t n = (size_t)plan.rows_used;
  if (!hnsw_try_alloc(nX, (size_t)plan.capacity * h->stride) || !hnsw_try_alloc(nAdj, (size_t)plan.capacity * (h->m0 + 1)) ||
      !hnsw_try_alloc(nLevel, (size_t)plan.capacity) || !hnsw_try_alloc(nUpoff, (size_t)plan.capacity) ||
      !hnsw_try_alloc(nUpper, (size_t)plan.upper_capacity) || !hnsw_try_alloc(dRemap, (size_t)h->rows_used) ||
      !hnsw_try_alloc(dPlan, 2 * n) || !hnsw_try_alloc(dStatus, vt::kHnswCompactGuards))
    return VT_OK;

  hipStream_t s = h->ctx.stream;
  VT_HIP(hipMemcpyAsync(dPlan.p, plan.src.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  VT_HIP(hipMemcpyAsync(dPlan.p + n, plan.upoff.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  vt::HnswCompactArgs a{};
  a.X = h->X.p;
  a.adj0 = h->dAdj0.p;
  a.level = h->dLevel.p;
  a.upoff = h->dUpoff.p;
  a.upper = h->dUpper.p;
  a.old_rows = (uint32_t)h->rows_used;
  a.old_upper = h->upper_used;
  a.stride = h->stride;
  a.m = (uint32_t)h->m;
  a.m0 = (uint32_t)h->m0;
  a.src = dPlan.p;
  a.new_upoff = dPlan.p + n;
  a.rows = (uint32_t)n;
  a.new_upper = plan.upper_used;
  a.remap = dRemap.p;
  a.outX = nX.p;
  a.out_adj0 = nAdj.p;
  a.out_level = nLevel.p;
  a.out_upoff = nUpoff.p;
  a.out_upper = nUpper.p;
  a.status = dStatus.p;
  VT_HIP(vt::launch_hnsw_compact(a, s));
  uint32_t fired[vt::kHnswCompactGuards] = {};
  VT_HIP(hipMemcpyAsync(fired, dStatus.p, sizeof fired, hipMemcpyDeviceToHost, s));
  VT_HIP(hipStreamSynchronize(s));
  static const char *const kGuard[vt::kHnswCompactGuards] = {"a list names a row beyond the slab", "a list names a dead row",
                                                            "a list is longer than its degree",
                                                            "a level or list offset is not the graph's"};
  for (uint32_t g = 0; g < vt::kHnswCompactGuards; ++g)
    if (fired[g]) {
      h->poisoned = true;
      return fail(VT_ERR_DEVICE, std::string("hnsw index: compaction found the device mirror apart from the graph: ") + kGuard[g]);
    }

  mv_swap(h->X, nX);
  mv_swap(h->dAdj0, nAdj);
  mv_swap(h->dLevel, nLevel);
  mv_swap(h->dUpoff, nUpoff);
  mv_swap(h->dUpper, nUpper);
  h->graph.close_rows();
  std::vector<uint64_t> ids(n);
  for (size_t i = 0; i < n; ++i) ids[i] = h->row_id[plan.src[i]];
  h->row_id = std::move(ids);
  h->row_upoff = std::move(plan.upoff);
  h->rows_used = plan.rows_used;
  h->dead_rows = 0;
  h->upper_used = plan.upper_used;
  h->capacity = plan.capacity;
  ++h->epoch;
  return VT_OK;
}

}  // namespace


namespace {

inline float hnsw_rank_value(int metric, float raw) {  // distances.rs:113-119
  if (metric == VT_COSINE) return 1.0f - raw;
  if (metric == VT_INNER_PRODUCT) return -raw;
  return raw;
}

// hnsw.rs:152-245 behind its validation.  `mutated`: the graph changed (a failure afterwards poisons the handle).
int hnsw_insert_one(vt_hnsw *h, const char *id, size_t id_len, const float *vec, size_t n, bool *mutated) {
  if (n > 0x7ffffff0u) return fail(VT_ERR_UNSUPPORTED, "vector dimension exceeds what the HNSW kernel addresses");
  VT_TRY(h->ctx.bind());
  const std::string ext(id_len ? id : "", id_len);
  VT_TRY(hnsw_erase(h, ext, mutated));  // an existing id goes first, whatever happens to the insert
  VT_TRY(hnsw_compact_if_due(h));       // (an emptied graph went through hnsw_forget; a delete never compacts)
  if (!h->graph.ids_left()) return fail(VT_ERR_NOMEM, "hnsw index: the internal id counter reached 2^32");
  const uint64_t iid = h->graph.take_id();
  const uint32_t level = h->graph.level_for(ext.data(), ext.size());
  const bool first = h->graph.len() == 0;
  if (first) {
    h->d = (uint32_t)n;
    h->stride = round_up_u32((uint32_t)n, 4);
  }
  const uint64_t upper_need = h->upper_used + (uint64_t)level * (h->m + 1);
  if (upper_need > 0xFFFFFFF0ull) return fail(VT_ERR_UNSUPPORTED, "hnsw index: upper-layer lists beyond 2^32 words");
  VT_TRY(hnsw_reserve(h, h->rows_used + 1, upper_need));
  hipStream_t s = h->ctx.stream;
  const uint32_t row = (uint32_t)h->rows_used;
  // the new vector goes to its slab row first and is the traversal's query; a row past rows_used belongs to nobody
  VT_TRY(h->hRows.ensure(h->stride));
  std::memcpy(h->hRows.p, vec, n * sizeof(float));
  for (uint32_t e = (uint32_t)n; e < h->stride; ++e) h->hRows.p[e] = 0.0f;
  float *at = h->X.p + (size_t)row * h->stride;
  VT_HIP(hipMemcpyAsync(at, h->hRows.p, (size_t)h->stride * sizeof(float), hipMemcpyHostToDevice, s));

  std::vector<std::vector<vt_host::HnswEdge>> lists;
  if (!first) {
    const vt_host::HnswNode *en = h->graph.node(h->graph.entry());
    const uint32_t top = en ? en->level : 0;
    const uint32_t nl = std::min(level, top) + 1;
    const uint32_t ef = (uint32_t)std::min<uint64_t>(h->ef_construction, h->graph.len());
    const uint32_t block = 1 + 2 * ef;
    VT_TRY(hnsw_traverse(h, 1, 1, at, h->stride, ef, level, 2 + nl * block));
    const uint32_t *o = h->hOut.p;
    if (o[0] == (uint32_t)VT_ERR_OVERFLOW) return VT_ERR_OVERFLOW;
    if (o[0] != 0 || o[1] != nl) return fail(VT_ERR_DEVICE, "hnsw index: the insert's traversal did not come back");
    lists.resize(nl);
    for (uint32_t l = 0; l < nl; ++l) {
      const uint32_t *b = o + 2 + (size_t)l * block;
      const uint32_t cnt = std::min(b[0], ef);
      for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t r = b[1 + 2 * i];
        if (r >= h->rows_used) return fail(VT_ERR_DEVICE, "hnsw index: a traversal named a row that is not there");
        float dist;
        std::memcpy(&dist, &b[2 + 2 * i], 4);
        lists[l].push_back(vt_host::HnswEdge{h->row_id[r], dist});
      }
    }
  }
  h->graph.apply_insert(ext, iid, level, row, (long)n, std::move(lists));
  *mutated = true;
  h->row_id.push_back(iid);
  h->row_upoff.push_back((uint32_t)h->upper_used);
  std::vector<vt::HnswPatch> p;
  p.push_back(vt::HnswPatch{row, level, 2});
  p.push_back(vt::HnswPatch{row, (uint32_t)h->upper_used, 3});
  h->upper_used = upper_need;
  ++h->rows_used;
  ++h->epoch;
  return hnsw_patch_mirror(h, p);
}

// a mutation's status: a failure after the graph changed leaves host and device apart
int hnsw_settle(vt_hnsw *h, int st, bool mutated) {
  if (st != VT_OK && st != VT_ERR_OVERFLOW && mutated) h->poisoned = true;
  return st;
}

int hnsw_insert_many(vt_hnsw *h, size_t count, const char *ids, const size_t *id_off, const float *values,
                     const size_t *value_off) {
  if (h->poisoned) return VT_ERR_HNSW_POISONED;
  // hnsw.rs:249-260: everything against the index's dimension, or the first vector's length, before anything changes
  long expected = h->graph.dimension();
  if (expected < 0 && count) expected = (long)(value_off[1] - value_off[0]);
  for (size_t i = 0; i < count; ++i) VT_TRY(validate_vector(values + value_off[i], value_off[i + 1] - value_off[i], expected));
  for (size_t i = 0; i < count; ++i) {
    bool mutated = false;
    const size_t n = value_off[i + 1] - value_off[i];
    // (insert validates again against the dimension of the moment: hnsw.rs:153)
    int st = validate_vector(values + value_off[i], n, h->graph.dimension());
    if (st == VT_OK) st = no_throw([&]() { return hnsw_insert_one(h, ids + id_off[i], id_off[i + 1] - id_off[i], values + value_off[i], n, &mutated); });
    VT_TRY(hnsw_settle(h, st, mutated));
  }
  return VT_OK;
}

int hnsw_delete(vt_hnsw *h, const char *id, size_t id_len) {
  if (h->poisoned) return VT_ERR_HNSW_POISONED;
  VT_TRY(h->ctx.bind());
  bool mutated = false;
  const int st = no_throw([&]() { return hnsw_erase(h, std::string(id_len ? id : "", id_len), &mutated); });
  return hnsw_settle(h, st, mutated);
}

// hnsw.rs:292-333 for nq queries of d floats in one launch; status[i] and out[i] per query
int hnsw_search_many(vt_hnsw *h, const float *queries, size_t nq, size_t d, size_t limit, vt_hits **out, int *status) {
  if (h->poisoned) return VT_ERR_HNSW_POISONED;
  for (size_t i = 0; i < nq; ++i) {
    out[i] = nullptr;
    status[i] = VT_OK;
  }
  if (limit == 0) {  // before the query is looked at
    for (size_t i = 0; i < nq; ++i) VT_TRY(empty_hits(&out[i]));
    return VT_OK;
  }
  std::vector<uint32_t> valid;
  for (size_t i = 0; i < nq; ++i) {
    status[i] = validate_vector(queries + i * d, d, h->graph.dimension());
    if (status[i] == VT_OK) valid.push_back((uint32_t)i);
  }
  if (h->graph.len() == 0) {
    for (uint32_t i : valid) VT_TRY(empty_hits(&out[i]));
    return VT_OK;
  }
  if (valid.empty()) return VT_OK;
  if (valid.size() > 0x7fffffffu) return fail(VT_ERR_UNSUPPORTED, "hnsw index: too many queries in one call");
  VT_TRY(h->ctx.bind());
  hipStream_t s = h->ctx.stream;
  const uint32_t nv = (uint32_t)valid.size(), qs = h->stride;
  VT_TRY(h->hRows.ensure((size_t)nv * qs));
  VT_TRY(h->dQ.ensure((size_t)nv * qs));
  for (uint32_t k = 0; k < nv; ++k) {
    float *dst = h->hRows.p + (size_t)k * qs;
    std::memcpy(dst, queries + (size_t)valid[k] * d, d * sizeof(float));
    for (uint32_t e = (uint32_t)d; e < qs; ++e) dst[e] = 0.0f;
  }
  VT_HIP(hipMemcpyAsync(h->dQ.p, h->hRows.p, (size_t)nv * qs * sizeof(float), hipMemcpyHostToDevice, s));
  const uint32_t ef = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(h->ef_search, limit), h->graph.len());
  const uint32_t out_stride = 2 + 2 * ef;
  if ((uint64_t)nv * out_stride > (1ull << 32)) return fail(VT_ERR_UNSUPPORTED, "hnsw index: the call's result lists exceed 16 GiB");
  VT_TRY(hnsw_traverse(h, 0, nv, h->dQ.p, qs, ef, 0, out_stride));
  struct Item {
    uint32_t key;
    float raw;
    const std::string *id;
  };
  std::vector<Item> items;
  for (uint32_t k = 0; k < nv; ++k) {
    const uint32_t *o = h->hOut.p + (size_t)k * out_stride;
    const uint32_t qi = valid[k];
    if (o[0] == (uint32_t)VT_ERR_OVERFLOW) {
      status[qi] = VT_ERR_OVERFLOW;
      continue;
    }
    if (o[0] != 0 || o[1] > ef) return fail(VT_ERR_DEVICE, "hnsw index: a search's traversal did not come back");
    items.clear();
    for (uint32_t i = 0; i < o[1]; ++i) {
      const uint32_t r = o[2 + 2 * i];
      if (r >= h->rows_used) return fail(VT_ERR_DEVICE, "hnsw index: a traversal named a row that is not there");
      const vt_host::HnswNode *n = h->graph.node(h->row_id[r]);
      if (!n) return fail(VT_ERR_DEVICE, "hnsw index: a traversal named a deleted node");
      float raw;
      std::memcpy(&raw, &o[3 + 2 * i], 4);
      items.push_back(Item{vt_host::hnsw_orderable(hnsw_rank_value(h->metric, raw)), raw, &n->external_id});
    }
    // (rank by total_cmp, external id bytes), then `limit` of them
    std::sort(items.begin(), items.end(), [](const Item &a, const Item &b) { return a.key != b.key ? a.key < b.key : *a.id < *b.id; });
    if (items.size() > limit) items.resize(limit);
    auto hits = std::make_unique<vt_hits>();
    for (const Item &it : items) {
      hits->ids.push_back(*it.id);
      hits->raw.push_back(it.raw);
      hits->rank_key.push_back(it.key);
    }
    out[qi] = hits.release();
  }
  return VT_OK;
}

}  // namespace
