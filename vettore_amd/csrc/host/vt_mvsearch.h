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

}  // namespace
