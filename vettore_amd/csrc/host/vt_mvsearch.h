// vt_mvsearch.h -- the resident multi-vector store (vt_mv): documents put once, kept in device memory, searched by
// MaxSim without another upload.  The slot table is host/vt_mvstore.h; here are the slab, the norm column, the device
// mirror of the live list and the searches (K9r, vt_maxsim_resident.hip; K9 over the slab where K9r does not serve).
// Part of vt_index.cpp's translation unit (included there, in this order, exactly once).
//
// The contract: after any puts and deletes a search returns what vt_multi_vector_top_k returns for the live documents
// handed over in the order of their last put -- ids, order, score bits and status, the earliest failing document's
// status included (the slot list IS that order, and the kernels report (list position << 8 | status) by atomicMin).
// One mutex per handle, every call exclusive; the handle has its own stream and scratch and takes nothing from the
// stateless session.  The slab is one hipMalloc that doubles by allocate + copy + free (no mapped chunks).
//
// A batched search (vt_mv_top_k_batch / vt_mv_top_k_ids_batch, mv_search_batch below) answers every set with what the
// single-set search returns for it, under one hold of the mutex: host/vt_mvbatch.h packs the sets K9rb serves into
// panels (vt_maxsim_batch.hip), one select launch cuts all their lists and one read-back brings hits and error words;
// every other set goes through mv_search itself.
#pragma once

struct vt_mv {
  std::mutex mu;
  Ctx ctx;  // (first: its stream goes last)
  vt_host::MvTable table;
  DevBuf<float> X;        // [capacity][stride] token rows, stride = round_up(d, 4), the pad zero and never read
  DevBuf<double> norms;   // [capacity] sqrt(f64 t.t) of each row, computed once when the row is put
  uint32_t stride = 0;
  uint64_t uploaded_bytes = 0;
  // the live list, rebuilt by the first search after a mutation: per position the document's first row, row count and id rank
  bool list_current = false;
  std::vector<uint32_t> list, pos_of_slot, first, cnt, rank;
  DevBuf<uint32_t> dFirstRow, dCnt, dRank;
  // a put's staging and a compaction's row list
  PinnedBuf<float> hRows;
  DevBuf<uint32_t> dSrc;
  // a search's scratch (MaxSimState, slot 0 only) and a subset search's own list
  MaxSimState P;
  DevBuf<uint32_t> dSubFirstRow, dSubCnt, dSubRank;
  // a batched search's own scratch (mv_search_batch): slot matrix and norms, descriptors / groups / lists in one block,
  // keys and payloads [set][key_stride], one error word per set, the select's result blocks and their pinned copies
  DevBuf<float> dBQ;
  DevBuf<double> dBQNorm;
  DevBuf<uint32_t> dBMeta;
  DevBuf<uint64_t> dBKeys;
  DevBuf<vt::Payload> dBPay;
  DevBuf<unsigned long long> dBFirst;
  DevBuf<unsigned char> dBOut;
  PinnedBuf<unsigned char> hBOut;
  PinnedBuf<unsigned long long> hBFirst;
  // vt_mv_counters: launches of a MaxSim scoring kernel (K9, K9r, K9rb) and query sets scored by K9rb, since vt_mv_new
  uint64_t scoring_launches = 0, batched_sets = 0;
  // the documents' MUVERA encodings (host/vt_fde.h): a call's table and slot lists, a chunk's rows, first rows and counts
  MuveraState F;
  DevBuf<uint32_t> dFdeDoc;
};

namespace {

// hipMalloc into an empty buffer; a card without room is VT_ERR_NOMEM, not a device error
template <typename T>
int mv_alloc(DevBuf<T> &b, size_t want) {
  b.release();
  const hipError_t e = hipMalloc(reinterpret_cast<void **>(&b.p), std::max<size_t>(want, 1) * sizeof(T));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    b.p = nullptr;
    return fail(e == hipErrorOutOfMemory ? VT_ERR_NOMEM : VT_ERR_DEVICE, std::string("resident store: ") + hipGetErrorString(e));
  }
  b.count = std::max<size_t>(want, 1);
  return VT_OK;
}

template <typename T>
void mv_swap(DevBuf<T> &a, DevBuf<T> &b) {
  std::swap(a.p, b.p);
  std::swap(a.count, b.count);
}

void mv_after_mutation(vt_mv *s) {
  s->list_current = false;
  if (s->table.capacity() == 0) {  // the last live row went: slab and dimension with it
    s->X.release();
    s->norms.release();
    s->stride = 0;
  }
}

int mv_put_many(vt_mv *s, size_t count, const char *ids, const size_t *id_off, const size_t *doc_vec_off,
                const float *values, const size_t *value_off) {
  if (count == 0) return VT_OK;
  // every row is checked before anything changes: empty, then dimension, then finiteness, the first bad row's status
  const size_t v0 = doc_vec_off[0], v1 = doc_vec_off[count];
  long dim = s->table.dimension();
  if (dim < 0 && v1 > v0) dim = (long)(value_off[v0 + 1] - value_off[v0]);
  for (size_t v = v0; v < v1; ++v) {
    const size_t len = value_off[v + 1] - value_off[v];
    if (len == 0) return VT_ERR_EMPTY_VECTORS;
    if (len != (size_t)dim) return VT_ERR_DIMENSION;
    VT_TRY(validate_finite(values + value_off[v], len));
  }
  if (v1 > v0 && (size_t)dim > 0x7ffffff0u) return fail(VT_ERR_UNSUPPORTED, "vector dimension exceeds what the MaxSim kernels address");
  std::vector<size_t> rows(count);
  for (size_t i = 0; i < count; ++i) rows[i] = doc_vec_off[i + 1] - doc_vec_off[i];
  vt_host::MvPutPlan plan;
  if (!s->table.plan_put(count, ids, id_off, rows.data(), &plan)) return fail(VT_ERR_UNSUPPORTED, "more than 2^32-16 vectors in one store");

  // allocate before mutating: the new slab (compaction, growth), the staging block
  VT_TRY(s->ctx.bind());
  hipStream_t stream = s->ctx.stream;
  const uint32_t d = plan.new_rows ? (uint32_t)dim : 0;
  const uint32_t stride = plan.new_rows ? round_up_u32(d, 4) : s->stride;
  const bool move = plan.compact || plan.capacity != s->table.capacity();
  DevBuf<float> nX;
  DevBuf<double> nNorms;
  if (move && plan.capacity) {
    VT_TRY(mv_alloc(nX, (size_t)plan.capacity * stride));
    VT_TRY(mv_alloc(nNorms, (size_t)plan.capacity));
    if (plan.compact && !plan.src.empty()) {
      VT_TRY(s->dSrc.ensure(plan.src.size()));
      VT_HIP(hipMemcpyAsync(s->dSrc.p, plan.src.data(), plan.src.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
      VT_HIP(vt::launch_mv_compact(s->X.p, s->norms.p, s->dSrc.p, (uint32_t)plan.src.size(), stride, nX.p, nNorms.p, stream));
    } else if (!plan.compact && s->table.used_rows()) {
      const size_t used = (size_t)s->table.used_rows();
      VT_HIP(hipMemcpyAsync(nX.p, s->X.p, used * stride * sizeof(float), hipMemcpyDeviceToDevice, stream));
      VT_HIP(hipMemcpyAsync(nNorms.p, s->norms.p, used * sizeof(double), hipMemcpyDeviceToDevice, stream));
    }
  }
  float *X = move ? nX.p : s->X.p;
  double *norms = move ? nNorms.p : s->norms.p;
  if (plan.new_rows) {
    // the stored documents' rows in store order, each padded with zeros to the row stride; rows past `used` of a slab
    // belong to nobody, so a failure from here on leaves the store as it was
    const size_t floats = (size_t)plan.new_rows * stride;
    VT_TRY(s->hRows.ensure(floats));
    float *dst = s->hRows.p;
    for (uint32_t i : plan.take)
      for (size_t v = doc_vec_off[i]; v < doc_vec_off[i + 1]; ++v, dst += stride) {
        std::memcpy(dst, values + value_off[v], (size_t)d * sizeof(float));
        for (uint32_t e = d; e < stride; ++e) dst[e] = 0.0f;
      }
    float *at = X + (size_t)plan.base * stride;
    VT_HIP(hipMemcpyAsync(at, s->hRows.p, floats * sizeof(float), hipMemcpyHostToDevice, stream));
    VT_HIP(vt::launch_maxsim_norms(at, stride, (uint32_t)plan.new_rows, d, norms + plan.base, stream));
  }
  VT_HIP(hipStreamSynchronize(stream));
  if (move) {
    mv_swap(s->X, nX);
    mv_swap(s->norms, nNorms);
  }
  if (plan.new_rows) s->stride = stride;
  s->uploaded_bytes += (uint64_t)plan.new_rows * stride * sizeof(float);
  s->table.apply_put(plan, ids, id_off, rows.data(), dim);
  mv_after_mutation(s);
  return VT_OK;
}

// The live list and its device mirror, after a mutation.
int mv_refresh_list(vt_mv *s) {
  if (s->list_current) return VT_OK;
  s->table.live_list(s->list, s->pos_of_slot);
  s->table.id_ranks(s->list, s->rank);
  const size_t n = s->list.size();
  s->first.resize(n);
  s->cnt.resize(n);
  for (size_t k = 0; k < n; ++k) {
    const vt_host::MvSlot &slot = s->table.slots()[s->list[k]];
    s->first[k] = slot.first_row;
    s->cnt[k] = slot.rows;
  }
  if (n) {
    VT_TRY(s->dFirstRow.ensure(n));
    VT_TRY(s->dCnt.ensure(n));
    VT_TRY(s->dRank.ensure(n));
    VT_HIP(hipMemcpyAsync(s->dFirstRow.p, s->first.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s->ctx.stream));
    VT_HIP(hipMemcpyAsync(s->dCnt.p, s->cnt.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s->ctx.stream));
    VT_HIP(hipMemcpyAsync(s->dRank.p, s->rank.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s->ctx.stream));
    VT_HIP(hipStreamSynchronize(s->ctx.stream));
  }
  s->list_current = true;
  return VT_OK;
}

// vt_mv_top_k (subset == false) and vt_mv_top_k_ids: maxsim_top_k (vt_maxsim.h) over documents that are already there.
int mv_search(vt_mv *s, bool subset, size_t count, const char *ids, const size_t *id_off, const float *query,
              const size_t *query_off, size_t nquery, int metric_code, size_t limit, vt_hits **out) {
  if (metric_code < VT_L2 || metric_code > VT_JACCARD) return VT_ERR_UNKNOWN_METRIC;
  VT_TRY(maxsim_validate_standalone(query, query_off, 0, nquery));
  const size_t dim = nquery ? query_off[1] - query_off[0] : 0;
  if (nquery && s->table.dimension() >= 0 && (size_t)s->table.dimension() != dim) return VT_ERR_DIMENSION;
  if (dim > 0x7ffffff0u || nquery > 0xFFFFFFF0ull) return fail(VT_ERR_UNSUPPORTED, "query dimension or count exceeds what the MaxSim kernels address");
  Ctx &c = s->ctx;
  VT_TRY(c.bind());
  VT_TRY(mv_refresh_list(s));
  MaxSimState &P = s->P;

  // the documents to score: the live list, or the listed live documents in store order (a duplicate once, unknown ids skipped)
  std::vector<uint32_t> pos;
  const uint32_t *dFirstRow = s->dFirstRow.p, *dCnt = s->dCnt.p, *dRank = s->dRank.p;
  uint32_t n = (uint32_t)s->list.size();
  if (subset) {
    for (size_t i = 0; i < count; ++i) {
      const uint32_t slot = s->table.find(ids + id_off[i], id_off[i + 1] - id_off[i]);
      if (slot != vt_host::MvTable::kNone) pos.push_back(s->pos_of_slot[slot]);
    }
    std::sort(pos.begin(), pos.end());
    pos.erase(std::unique(pos.begin(), pos.end()), pos.end());
    n = (uint32_t)pos.size();
    if (n) {
      std::vector<uint32_t> sub(3 * (size_t)n);
      for (uint32_t k = 0; k < n; ++k) {
        sub[k] = s->first[pos[k]];
        sub[n + k] = s->cnt[pos[k]];
        sub[2 * (size_t)n + k] = s->rank[pos[k]];  // (ranks within the store order the subset as well)
      }
      VT_TRY(s->dSubFirstRow.ensure(3 * (size_t)n));
      VT_HIP(hipMemcpyAsync(s->dSubFirstRow.p, sub.data(), sub.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
      VT_HIP(hipStreamSynchronize(c.stream));  // (sub leaves scope)
      dFirstRow = s->dSubFirstRow.p;
      dCnt = dFirstRow + n;
      dRank = dFirstRow + 2 * (size_t)n;
    }
  }
  if (n == 0) return empty_hits(out);

  const uint32_t nq = (uint32_t)nquery, d = (uint32_t)dim;
  vt::MaxSimResidentPlan plan{};
  bool resident = nq && vt::maxsim_resident_plan(d, nq, metric_code, &plan);
#ifdef VT_TEST_HOOKS
  if (vt::env::on(vt::env::TEST_MV_K9)) resident = false;
#endif
  uint32_t q_stride = plan.q_stride;
  const uint32_t panel = !nq ? 1 : resident ? plan.panel : vt::maxsim_panel_rows(d, &q_stride);
  if (panel == 0) return fail(VT_ERR_UNSUPPORTED, "vector dimension exceeds what the MaxSim kernel stages in LDS");

  VT_TRY(P.dKeys.ensure(n));
  VT_TRY(P.dPay.ensure(n));
  VT_TRY(P.dFirst.ensure(1));
  VT_TRY(P.hFirst.ensure(1));
  VT_HIP(hipMemsetAsync(P.dFirst.p, 0xFF, sizeof(unsigned long long), c.stream));
  if (nq) {  // the query vectors, zero-padded to q_stride, and (cosine) their norms
    std::vector<float> qpad((size_t)nq * q_stride, 0.0f);
    for (uint32_t i = 0; i < nq; ++i) std::memcpy(&qpad[(size_t)i * q_stride], query + query_off[i], (size_t)d * sizeof(float));
    VT_TRY(P.dQ.ensure(qpad.size()));
    VT_HIP(hipMemcpyAsync(P.dQ.p, qpad.data(), qpad.size() * sizeof(float), hipMemcpyHostToDevice, c.stream));
    if (metric_code == VT_COSINE) {
      VT_TRY(P.dQNorm.ensure(nq));
      VT_HIP(vt::launch_maxsim_norms(P.dQ.p, q_stride, nq, d, P.dQNorm.p, c.stream));
    }
    VT_HIP(hipStreamSynchronize(c.stream));  // (qpad leaves scope)
  }

  vt::MaxSimArgs a{};
  a.X = s->X.p;
  a.stride = s->stride ? s->stride : round_up_u32(d, 4);  // (a store without a row: no document reads X)
  a.doc_off = dFirstRow;
  a.doc_cnt = dCnt;
  a.ndoc = n;
  a.Q = P.dQ.p;
  a.q_stride = q_stride;
  a.nq = nq;
  a.d = d;
  a.metric = metric_code;
  a.order = default_order();
  a.qnorm = P.dQNorm.p;
  a.tnorm = s->norms.p;
  a.id_rank = dRank;
  a.keys = P.dKeys.p;
  a.pay = P.dPay.p;
  a.first_error = P.dFirst.p;
  if (nq > panel) {  // query vectors in several panels: the running sums wait in device memory in between
    VT_TRY(P.dTotal[0].ensure(n));
    VT_TRY(P.dStatus[0].ensure(n));
    a.total = P.dTotal[0].p;
    a.status = P.dStatus[0].p;
  }
  const size_t by_doc = ((size_t)n + vt::kWavesPerBlock - 1) / vt::kWavesPerBlock;
  // (K9r's documents differ in length and a block's waves wait for its longest: more, shorter-lived blocks even that out)
  const uint32_t blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>(by_doc, (size_t)c.num_cus * (resident ? 16 : 4)));
  do {
    a.panel_qn = nq ? std::min(panel, nq - a.panel_q0) : 0;
    if (resident) VT_HIP(vt::launch_maxsim_resident(a, plan, blocks, c.stream));
    else VT_HIP(vt::launch_maxsim(a, blocks, c.stream));
    s->scoring_launches += 1;
    a.panel_q0 += a.panel_qn;
  } while (a.panel_q0 < nq);

  // limit == 0 still scores everything (errors surface): select one
  std::vector<vt::Entry> entries;
  VT_TRY(collect_from_keys(c, P.dKeys.p, P.dPay.p, n, std::max<size_t>(limit, 1), entries));
  if (limit == 0) entries.clear();
  VT_HIP(hipMemcpyAsync(P.hFirst.p, P.dFirst.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
  VT_HIP(hipStreamSynchronize(c.stream));
  const unsigned long long fe = *P.hFirst.p;
  if (fe != ~0ull) return (int)(fe & 0xFF);  // the earliest document, in store order, that failed on the device
  auto h = std::make_unique<vt_hits>();
  for (const auto &e : entries) {
    const uint32_t at = subset ? pos[e.row] : e.row;
    h->ids.push_back(s->table.slots()[s->list[at]].id);
    h->raw.push_back(e.raw);
    h->rank_key.push_back(rank_key_of(e.key));
  }
  *out = h.release();
  return VT_OK;
}

constexpr size_t kMvBatchPanelLds = 52 * 1024;  // LDS of a whole-store panel's block: three blocks share a CU's 160 KiB
constexpr size_t kMvBatchMaxSets = 65535;       // sets one call hands to K9rb: a launch's gridDim.y
constexpr uint64_t kMvBatchMaxKeys = 1ull << 26;  // keys + payloads [set][key_stride] of a batch: 1 GiB of scratch at most

// vt_mv_top_k_batch (subset == false) and vt_mv_top_k_ids_batch: out[b] / status[b] are mv_search's for set b.  A status
// other than VT_OK returned from here is the call's own (the device failed under the batch).
int mv_search_batch(vt_mv *s, bool subset, size_t nsets, const size_t *set_id_off, const char *ids, const size_t *id_off,
                    const size_t *set_vec_off, const float *query, const size_t *query_off, int metric_code, size_t limit,
                    vt_hits **out, int *status) {
  auto single = [&](size_t b) {
    const size_t v0 = set_vec_off[b], nv = set_vec_off[b + 1] - v0;
    const size_t i0 = subset ? set_id_off[b] : 0, ni = subset ? set_id_off[b + 1] - i0 : 0;
    status[b] = mv_search(s, subset, ni, ids, ni ? id_off + i0 : nullptr, query, nv ? query_off + v0 : nullptr, nv, metric_code,
                          limit, &out[b]);
  };
  auto all_single = [&](const std::vector<uint32_t> &sets) {
    for (uint32_t b : sets) single(b);
    return VT_OK;
  };
  // Sets K9rb may take: valid on the host, of the store's dimension, with a vector.  Every other set -- the ones mv_search
  // refuses among them -- takes mv_search, so its status is the single call's by construction.  Two bounds of the device
  // side send sets there as well (DESIGN 4.13 lists them): a set's vectors are counted in 32 bits, as in mv_search, and
  // one call batches at most kMvBatchMaxSets sets (gridDim.y of K9rb and of the select launch); the rest go one by one.
  const long sdim = s->table.dimension();
  std::vector<uint32_t> cand, rest;
  for (size_t b = 0; b < nsets; ++b) {
    const size_t v0 = set_vec_off[b], v1 = set_vec_off[b + 1];
    const bool ok = nsets >= 2 && v1 > v0 && v1 - v0 <= 0xFFFFFFF0ull && sdim >= 0 && cand.size() < kMvBatchMaxSets &&
                    maxsim_validate_standalone(query, query_off, v0, v1) == VT_OK &&
                    query_off[v0 + 1] - query_off[v0] == (size_t)sdim;
    (ok ? cand : rest).push_back((uint32_t)b);
  }
  all_single(rest);
  if (cand.empty()) return VT_OK;
  Ctx &c = s->ctx;
  VT_TRY(c.bind());
  VT_TRY(mv_refresh_list(s));

  // each set's documents: the live list, or the listed live documents in store order (as in mv_search)
  const uint32_t nlive = (uint32_t)s->list.size();
  std::vector<std::vector<uint32_t>> pos(subset ? cand.size() : 0);
  for (size_t k = 0; k < pos.size(); ++k) {  // (a list without a live document stays in the batch: its set's answer is empty)
    std::vector<uint32_t> &p = pos[k];
    for (size_t i = set_id_off[cand[k]]; i < set_id_off[cand[k] + 1]; ++i) {
      const uint32_t slot = s->table.find(ids + id_off[i], id_off[i + 1] - id_off[i]);
      if (slot != vt_host::MvTable::kNone) p.push_back(s->pos_of_slot[slot]);
    }
    std::sort(p.begin(), p.end());
    p.erase(std::unique(p.begin(), p.end()), p.end());
  }
  const uint32_t d = (uint32_t)sdim;
  bool served = (subset || nlive) && metric_code != VT_HAMMING && metric_code != VT_JACCARD;
#ifdef VT_TEST_HOOKS
  if (vt::env::on(vt::env::TEST_MV_K9)) served = false;
#endif
  // the tile and a panel's slots, asked for the largest panel wanted: all sets together, or -- each set its own panel -- the longest
  std::vector<uint32_t> counts(cand.size());
  uint64_t want = 0;
  for (size_t k = 0; k < cand.size(); ++k) {
    counts[k] = (uint32_t)(set_vec_off[cand[k] + 1] - set_vec_off[cand[k]]);
    const uint64_t padded = ((uint64_t)counts[k] + 7) / 8 * 8;
    want = subset ? std::max(want, padded) : want + padded;
  }
  vt::MaxSimResidentPlan plan{};
  served = served && !cand.empty() && vt::maxsim_resident_plan(d, (uint32_t)std::min<uint64_t>(want, 0xFFFFFF00u), metric_code, &plan);
  vt_host::MvBatchPlan bp;
  if (served) {
    const uint32_t pass = 8u * (64u >> plan.tile_log2);
    uint32_t capacity = plan.panel;
    if (!subset) {
      // Over the whole store the kernel, not the launch chain, is the time, and a panel that fills LDS leaves one block
      // a CU: 8 sets of 32 vectors over 20 000 documents took 22.4 ms in panels of five sets against 11.0 ms for eight
      // single calls (profiles/maxsim_resident_batch_full_lds.json).  A panel stays within a third of a CU's LDS -- K9r's
      // own footprint at that shape --, or one pass where the tiles alone leave less: 10.0 ms against 10.6 ms
      // (profiles/maxsim_resident_batch.json).
      const size_t tiles = vt::maxsim_resident_lds_bytes(0, plan.q_stride, plan), qrow = (size_t)plan.q_stride * sizeof(float);
      const size_t room = kMvBatchPanelLds > tiles ? (kMvBatchPanelLds - tiles) / qrow / pass * pass : 0;
      capacity = (uint32_t)std::min<size_t>(capacity, std::max<size_t>(room, pass));
    }
    vt_host::mv_batch_plan(counts.data(), counts.size(), capacity, pass, subset, &bp);
  }
  const size_t nb = served ? cand.size() - bp.single.size() : 0;
  uint32_t key_stride = nlive;
  if (subset) {
    key_stride = 0;
    for (const auto &p : pos) key_stride = std::max<uint32_t>(key_stride, (uint32_t)p.size());
  }
  // (a batch of one takes the single path; so does one whose key matrix [set][key_stride] would pass kMvBatchMaxKeys)
  if (nb < 2 || key_stride == 0 || (uint64_t)nb * key_stride > kMvBatchMaxKeys) return all_single(cand);
  {
    std::vector<uint32_t> alone;
    for (uint32_t k : bp.single) alone.push_back(cand[k]);
    all_single(alone);
  }

  // ---- the device's view: descriptors (set = the set's place among the nb batched ones), groups, list lengths, lists
  const uint32_t kNone = 0xFFFFFFFFu;
  std::vector<uint32_t> ord(cand.size(), kNone), set_of, desc0_of;
  const size_t ndesc = bp.desc.size(), ngroups = bp.panels.size();
  size_t ndocs = 0;
  for (const auto &p : pos) ndocs += p.size();  // (sets on the single path included: their lists are simply not used)
  const size_t oDesc = 0, oGroups = oDesc + 2 * ndesc, oM = oGroups + 4 * ngroups, oList = oM + nb;
  std::vector<uint32_t> meta(oList + 3 * ndocs);
  for (size_t g = 0; g < ndesc; ++g) {
    const uint32_t k = bp.desc[g].set;
    if (ord[k] == kNone) {
      ord[k] = (uint32_t)set_of.size();
      set_of.push_back(k);
      desc0_of.push_back((uint32_t)g);
    }
    meta[oDesc + 2 * g] = ord[k];
    meta[oDesc + 2 * g + 1] = bp.desc[g].info;
  }
  uint32_t max_ndesc = 0, list0 = 0;
  for (size_t p = 0; p < ngroups; ++p) {
    const vt_host::MvBatchPanel &pn = bp.panels[p];
    uint32_t *g = &meta[oGroups + 4 * p];
    g[0] = pn.desc0;
    g[1] = pn.ndesc;
    g[2] = 0;
    g[3] = nlive;
    if (subset) {  // (a panel is one set, with its own list: first row / count / rank, as mv_search builds them)
      const std::vector<uint32_t> &ps = pos[pn.first_set];
      g[2] = list0;
      g[3] = (uint32_t)ps.size();
      for (size_t i = 0; i < ps.size(); ++i) {
        meta[oList + list0 + i] = s->first[ps[i]];
        meta[oList + ndocs + list0 + i] = s->cnt[ps[i]];
        meta[oList + 2 * ndocs + list0 + i] = s->rank[ps[i]];
      }
      list0 += (uint32_t)ps.size();
    }
    max_ndesc = std::max(max_ndesc, pn.ndesc);
  }
  for (size_t o = 0; o < nb; ++o) meta[oM + o] = subset ? (uint32_t)pos[set_of[o]].size() : nlive;
  // the slot matrix: every set's vectors from its first slot on, rows zero-padded to q_stride, pad slots zero
  const uint32_t q_stride = plan.q_stride;
  const size_t slots = ndesc * vt_host::kMvGroupSlots;
  std::vector<float> qpad(slots * q_stride, 0.0f);
  for (size_t o = 0; o < nb; ++o) {
    const size_t v0 = set_vec_off[cand[set_of[o]]];
    for (uint32_t i = 0; i < counts[set_of[o]]; ++i)
      std::memcpy(&qpad[((size_t)desc0_of[o] * vt_host::kMvGroupSlots + i) * q_stride], query + query_off[v0 + i], (size_t)d * sizeof(float));
  }
  const size_t nkeys = nb * (size_t)key_stride;
  VT_TRY(s->dBMeta.ensure(meta.size()));
  VT_TRY(s->dBQ.ensure(qpad.size()));
  VT_TRY(s->dBKeys.ensure(nkeys));
  VT_TRY(s->dBPay.ensure(nkeys));
  VT_TRY(s->dBFirst.ensure(nb));
  VT_TRY(s->hBFirst.ensure(nb));
  VT_HIP(hipMemcpyAsync(s->dBMeta.p, meta.data(), meta.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
  VT_HIP(hipMemcpyAsync(s->dBQ.p, qpad.data(), qpad.size() * sizeof(float), hipMemcpyHostToDevice, c.stream));
  VT_HIP(hipMemsetAsync(s->dBFirst.p, 0xFF, nb * sizeof(unsigned long long), c.stream));
  if (metric_code == VT_COSINE) {
    VT_TRY(s->dBQNorm.ensure(slots));
    VT_HIP(vt::launch_maxsim_norms(s->dBQ.p, q_stride, (uint32_t)slots, d, s->dBQNorm.p, c.stream));
  }

  static_assert(sizeof(vt::MaxSimBatchDesc) == 8 && sizeof(vt::MaxSimBatchGroup) == 16 && sizeof(vt_host::MvBatchDesc) == 8 &&
                    vt_host::kMvGroupFirst == vt::kMaxSimBatchFirst && vt_host::kMvGroupLast == vt::kMaxSimBatchLast,
                "the words of `meta` are the kernel's descriptors and groups");
  vt::MaxSimBatchArgs a{};
  a.X = s->X.p;
  a.stride = s->stride;
  a.Q = s->dBQ.p;
  a.q_stride = q_stride;
  a.d = d;
  a.metric = metric_code;
  a.order = default_order();
  a.qnorm = s->dBQNorm.p;
  a.tnorm = s->norms.p;
  a.groups = reinterpret_cast<const vt::MaxSimBatchGroup *>(s->dBMeta.p + oGroups);
  a.desc = reinterpret_cast<const vt::MaxSimBatchDesc *>(s->dBMeta.p + oDesc);
  a.doc_first = subset ? s->dBMeta.p + oList : s->dFirstRow.p;
  a.doc_cnt = subset ? s->dBMeta.p + oList + ndocs : s->dCnt.p;
  a.doc_rank = subset ? s->dBMeta.p + oList + 2 * ndocs : s->dRank.p;
  a.ngroups = subset ? (uint32_t)ngroups : 1;  // (whole store: one launch per panel, its LDS sized by that panel)
  a.key_stride = key_stride;
  a.keys = s->dBKeys.p;
  a.pay = s->dBPay.p;
  a.first_error = s->dBFirst.p;
  const size_t by_doc = ((size_t)key_stride + vt::kWavesPerBlock - 1) / vt::kWavesPerBlock;
  const uint32_t blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>(by_doc, std::max<size_t>(1, (size_t)c.num_cus * 16 / a.ngroups)));
  for (size_t p = 0; p < (subset ? 1 : ngroups); ++p) {
    a.max_ndesc = subset ? max_ndesc : bp.panels[p].ndesc;
    VT_HIP(vt::launch_maxsim_batch(a, plan, blocks, c.stream));
    s->scoring_launches += 1;
    a.groups += 1;
  }
  s->batched_sets += nb;

  // ---- every list cut in one launch, hits and error words in one read-back (limits above kMaxFusedK: set by set)
  const bool fused = limit <= (size_t)vt::kMaxFusedK;
  const uint32_t k = (uint32_t)std::max<size_t>(std::min<size_t>(limit, vt::kMaxFusedK), 1);  // (limit == 0 still scores: select one)
  const uint32_t out_stride = 16 + k * (uint32_t)sizeof(vt::Entry);
  if (fused) {
    VT_TRY(s->dBOut.ensure(nb * (size_t)out_stride));
    VT_TRY(s->hBOut.ensure(nb * (size_t)out_stride));
    if (subset)
      VT_HIP(vt::launch_select_lists(s->dBKeys.p, s->dBPay.p, (uint32_t)nb, key_stride, s->dBMeta.p + oM, k, s->dBOut.p, out_stride,
                                     c.stream, false));
    else VT_HIP(vt::launch_select_queries(s->dBKeys.p, s->dBPay.p, (uint32_t)nb, key_stride, k, s->dBOut.p, out_stride, c.stream));
    VT_HIP(hipMemcpyAsync(s->hBOut.p, s->dBOut.p, nb * (size_t)out_stride, hipMemcpyDeviceToHost, c.stream));
  }
  VT_HIP(hipMemcpyAsync(s->hBFirst.p, s->dBFirst.p, nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
  VT_HIP(hipStreamSynchronize(c.stream));
  std::vector<vt::Entry> entries;
  for (size_t o = 0; o < nb; ++o) {
    const uint32_t b = cand[set_of[o]];
    const unsigned long long fe = s->hBFirst.p[o];
    if (fe != ~0ull) {
      status[b] = (int)(fe & 0xFF);  // the set's earliest document, in store order, that failed on the device
      continue;
    }
    const vt::Entry *e = nullptr;
    size_t ne = 0;
    if (fused) {
      const auto *blk = reinterpret_cast<const vt::ResultBlock *>(s->hBOut.p + o * (size_t)out_stride);
      e = blk->e;
      ne = limit ? std::min<size_t>(blk->count, k) : 0;
    } else {
      entries.clear();
      VT_TRY(collect_from_keys(c, s->dBKeys.p + o * (size_t)key_stride, s->dBPay.p + o * (size_t)key_stride, meta[oM + o], limit, entries));
      e = entries.data();
      ne = entries.size();
    }
    auto h = std::make_unique<vt_hits>();
    for (size_t i = 0; i < ne; ++i) {
      const uint32_t at = subset ? pos[set_of[o]][e[i].row] : e[i].row;
      h->ids.push_back(s->table.slots()[s->list[at]].id);
      h->raw.push_back(e[i].raw);
      h->rank_key.push_back(rank_key_of(e[i].key));
    }
    out[b] = h.release();
    status[b] = VT_OK;
  }
  return VT_OK;
}

}  // namespace
