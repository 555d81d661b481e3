// vt_maxsim.h -- multi_vector_top_k / multi_vector_score (multi_vector.rs:40-132): validation on the host in the
// reference's order, scoring on the device (K9, vt_maxsim.hip) in bounded chunks of documents.
// Part of vt_index.cpp's translation unit (included there, in this order, exactly once).
//
// A chunk's document vectors are one contiguous run of the caller's `values` (every scored vector has the query's
// length), copied into one of the upload ring's two staging blocks (UploadRing, vt_stateless.h) and uploaded into one
// of its two device buffers while the previous chunk is scored: chunk k + 1's upload overlaps chunk k's kernel, and
// the host's copy into staging overlaps both.  Keys accumulate over the whole call; one select at the end.
#pragma once

namespace {

constexpr size_t kMaxSimChunkBytes = 64u << 20;  // default upload chunk (vt_debug_set maxsim_chunk_bytes)

// validate_vectors (multi_vector.rs:152-160) over vectors [v0, v1) against `dim`
int maxsim_validate(const float *values, const size_t *value_off, size_t v0, size_t v1, size_t dim) {
  for (size_t v = v0; v < v1; ++v) {
    if (value_off[v + 1] - value_off[v] != dim) return VT_ERR_DIMENSION;
    VT_TRY(validate_finite(values + value_off[v], dim));
  }
  return VT_OK;
}
// validate_standalone_vectors (multi_vector.rs:142-150)
int maxsim_validate_standalone(const float *values, const size_t *value_off, size_t v0, size_t v1) {
  if (v0 == v1) return VT_OK;
  const size_t dim = value_off[v0 + 1] - value_off[v0];
  if (dim == 0) return VT_ERR_EMPTY_VECTORS;
  return maxsim_validate(values, value_off, v0, v1, dim);
}

// multi_vector.rs:90-132 top_k: the `limit` best of the documents into `entries` (row = document index; no answer on a failure).
int maxsim_top_k(int device, size_t count, const char *ids, const size_t *id_off, const size_t *doc_vec_off,
                 const float *values, const size_t *value_off, const float *query, const size_t *query_off,
                 size_t nquery, int metric_code, size_t limit, std::vector<vt::Entry> &entries) {
  // nifs.rs:196-197: the metric is decoded first
  if (metric_code < VT_L2 || metric_code > VT_JACCARD) return VT_ERR_UNKNOWN_METRIC;
  VT_TRY(maxsim_validate_standalone(query, query_off, 0, nquery));
  const size_t dim = nquery ? query_off[1] - query_off[0] : 0;
  // the reference walks the documents in order and stops at the first error; documents before the first
  // invalid one are scored and may fail first ("metric overflow", "score overflow")
  auto check_doc = [&](size_t i) {
    const size_t v0 = doc_vec_off[i], v1 = doc_vec_off[i + 1];
    return nquery == 0 ? maxsim_validate_standalone(values, value_off, v0, v1) : maxsim_validate(values, value_off, v0, v1, dim);
  };
  int first_error = VT_OK;
  const size_t good = first_refused(count, check_doc, &first_error);
  if (good == 0) return first_error;
  uint32_t q_stride = 0;
  const uint32_t panel = nquery ? vt::maxsim_panel_rows((uint32_t)std::min<size_t>(dim, 0x7fffffffu), &q_stride) : 1;
  if (dim > 0x7fffffffu || panel == 0)
    return fail(VT_ERR_UNSUPPORTED, "vector dimension exceeds what the MaxSim kernel stages in LDS");
  if (good > 0xFFFFFFF0ull || nquery > 0xFFFFFFF0ull) return fail(VT_ERR_UNSUPPORTED, "more than 2^32-16 documents or query vectors");
  StatelessLease lease;
  VT_TRY(stateless_lease(device, &lease));
  Ctx &c = lease.s->ctx;
  UploadRing &ring = lease.s->ring;
  MaxSimState &P = lease.s->maxsim;
  VT_TRY(ring.open());
  const uint32_t n = (uint32_t)good, nq = (uint32_t)nquery, d = (uint32_t)dim;

  std::vector<uint32_t> rank;
  ranks_for_ids(ids, id_off, good, rank);
  VT_TRY(P.dRank.ensure(n));
  VT_TRY(P.dKeys.ensure(n));
  VT_TRY(P.dPay.ensure(n));
  VT_TRY(P.dFirst.ensure(1));
  VT_TRY(P.hFirst.ensure(1));
  VT_HIP(hipMemcpyAsync(P.dRank.p, rank.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
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
  a.Q = P.dQ.p;
  a.q_stride = q_stride;
  a.nq = nq;
  a.d = d;
  a.metric = metric_code;
  a.order = default_order();
  a.qnorm = P.dQNorm.p;
  a.first_error = P.dFirst.p;
  auto launch_chunk = [&](uint32_t row0, uint32_t ndoc, int b) -> int {
    a.row0 = row0;
    a.ndoc = ndoc;
    a.id_rank = P.dRank.p + row0;
    a.keys = P.dKeys.p + row0;
    a.pay = P.dPay.p + row0;
    const uint32_t blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>((ndoc + vt::kWavesPerBlock - 1) / vt::kWavesPerBlock,
                                                                           (size_t)c.num_cus * 4));
    if (nq > panel) {  // query vectors in several panels: the running sums wait in device memory in between
      VT_TRY(P.dTotal[b].ensure(ndoc));
      VT_TRY(P.dStatus[b].ensure(ndoc));
      a.total = P.dTotal[b].p;
      a.status = P.dStatus[b].p;
    }
    a.panel_q0 = 0;
    do {
      a.panel_qn = std::min(panel, nq - a.panel_q0);
      VT_HIP(vt::launch_maxsim(a, blocks, c.stream));
      a.panel_q0 += a.panel_qn;
    } while (a.panel_q0 < nq);
    return VT_OK;
  };

  if (nq == 0) {
    VT_TRY(launch_chunk(0, n, 0));  // no pair to score: every document 0.0, no vector uploaded
  } else {
    const long forced = vt::env::get(vt::env::MAXSIM_CHUNK_BYTES);
    const size_t chunk_bytes = forced > 0 ? (size_t)forced : kMaxSimChunkBytes;
    const size_t row_bytes = (size_t)d * sizeof(float);
    const size_t chunk_rows = std::max<size_t>(1, std::min<size_t>(chunk_bytes / row_bytes, 0xFFFFFFF0ull));
    size_t i0 = 0;
    for (int k = 0; i0 < good; ++k) {
      // documents [i0, i1): as many as fit in chunk_rows vectors, at least one
      size_t i1 = i0 + 1;
      while (i1 < good && doc_vec_off[i1 + 1] - doc_vec_off[i0] <= chunk_rows) ++i1;
      const size_t v0 = doc_vec_off[i0], v1 = doc_vec_off[i1];
      const size_t rows = v1 - v0, ndoc = i1 - i0;
      if (rows > 0xFFFFFFF0ull) return fail(VT_ERR_UNSUPPORTED, "more than 2^32-16 vectors in one document");
      const int b = k & 1;
      VT_TRY(ring.reserve(b, rows * d, ndoc + 1));
      const float *src = values + value_off[v0];  // every vector of a scored document has length d: one run
      float *dst = ring.hX[b].p;
      parallel_for(rows * d, (size_t)1 << 20, [&](size_t lo, size_t hi) { std::memcpy(dst + lo, src + lo, (hi - lo) * sizeof(float)); });
      for (size_t i = 0; i <= ndoc; ++i) ring.hOff[b].p[i] = (uint32_t)(doc_vec_off[i0 + i] - v0);
      VT_TRY(ring.send(b, rows * d, ndoc + 1));
      VT_TRY(ring.wait_ready(b, c.stream));
      a.X = ring.dX[b].p;
      a.stride = d;
      a.doc_off = ring.dOff[b].p;
      if (metric_code == VT_COSINE) {
        VT_TRY(P.dNorm[b].ensure(std::max<size_t>(rows, 1)));
        VT_HIP(vt::launch_maxsim_norms(a.X, d, (uint32_t)rows, d, P.dNorm[b].p, c.stream));
        a.tnorm = P.dNorm[b].p;
      }
      VT_TRY(launch_chunk((uint32_t)i0, (uint32_t)ndoc, b));
      VT_TRY(ring.mark_consumed(b, c.stream));
      i0 = i1;
    }
  }
  // limit == 0 still scores everything (errors surface): select one
  VT_TRY(collect_from_keys(c, P.dKeys.p, P.dPay.p, n, std::max<size_t>(limit, 1), entries));
  if (limit == 0) entries.clear();
  VT_HIP(hipMemcpyAsync(P.hFirst.p, P.dFirst.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
  VT_HIP(hipStreamSynchronize(c.stream));
  const unsigned long long fe = *P.hFirst.p;
  if (fe != ~0ull) return (int)(fe & 0xFF);  // the earliest document that failed on the device: before the host's first error
  return first_error;
}

}  // namespace
