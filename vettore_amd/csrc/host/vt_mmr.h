// vt_mmr.h -- MMR reranking (Vettore.Distance.mmr_rerank/5, lib/vettore_distance.ex:334-519; Vettore.rerank/4,
// lib/vettore.ex:622-640): the argument checks, a call's problems laid out for K12 (vt_mmr.hip) and its launch chain, the
// stateless call over uploaded rows, and the three handle calls over resident rows -- rerank by ids, and the exact search
// followed by MMR over its hits under one lease.  What needs no device is host/vt_mmrplan.h.
// Part of vt_index.cpp's translation unit (included there, in this order, exactly once).
#pragma once

namespace {

using vt_host::mmr_guards_ok;
using vt_host::mmr_scores_ok;
using vt_host::mmr_hit_score;
using vt_host::mmr_rows_of_ids;
using vt_host::MmrJob;
using MmrLayout = vt_host::MmrLayout<vt::MmrProblem>;

// ------------------------------------------------------------------ the launch chain
// `njobs` problems over one row matrix on the context's stream: max_p(kk_p) + 1 step launches back to back, one wait at
// the end.  status[p]: VT_OK or VT_ERR_OVERFLOW; orders[p]: the chosen candidates of problem p.
int mmr_run(Ctx &c, const float *X, size_t stride, uint32_t d, int metric, int order, const MmrJob *jobs, size_t njobs,
            std::vector<std::vector<uint32_t>> *orders, std::vector<int> *status) {
  orders->assign(njobs, {});
  status->assign(njobs, VT_OK);
  if (njobs == 0) return VT_OK;
  if (njobs > 65535) return fail(VT_ERR_UNSUPPORTED, "more than 65 535 MMR problems in one call");
  MmrLayout lay;
  if (!vt_host::mmr_layout(jobs, njobs, &lay)) return fail(VT_ERR_UNSUPPORTED, "more than 2^32-16 MMR candidates in one call");
  if (lay.total == 0) return VT_OK;
  const size_t P = njobs, total = lay.total;
  VT_TRY(c.dMmrProb.ensure(P));
  VT_TRY(c.dMmrRows.ensure(total));
  VT_TRY(c.dMmrRel.ensure(total));
  VT_TRY(c.dMmrRed.ensure(total));
  VT_TRY(c.dMmrNorm.ensure(total));
  VT_TRY(c.dMmrLive.ensure(total));
  VT_TRY(c.dMmrOrder.ensure(total));
  VT_TRY(c.dMmrCount.ensure(P));
  VT_TRY(c.dMmrStatus.ensure(P));
  const uint32_t block_rows = mmr_block_rows();
  const uint32_t blocks = std::min<uint32_t>(vt::kMmrMaxBlocks, (lay.max_n + block_rows - 1) / block_rows);
  VT_TRY(c.dMmrPartial.ensure((size_t)2 * P * blocks));
  const vt::MmrArgs a = mmr_args(RowSet{X, stride, nullptr, 0, metric, order}, c, d, block_rows);  // (after the last ensure)
  // up: {problems, relevance, rows}; down: {status, count, order}
  const size_t up_rel = round_up_u32((uint32_t)(P * sizeof(vt::MmrProblem)), 8), up_rows = up_rel + total * sizeof(double);
  VT_TRY(c.hMmrUp.ensure(up_rows + total * sizeof(uint32_t)));
  std::memcpy(c.hMmrUp.p, lay.prob.data(), P * sizeof(vt::MmrProblem));
  for (size_t p = 0; p < P; ++p) {
    if (!jobs[p].n) continue;
    std::memcpy(c.hMmrUp.p + up_rel + (size_t)lay.prob[p].off * sizeof(double), jobs[p].rel, jobs[p].n * sizeof(double));
    std::memcpy(c.hMmrUp.p + up_rows + (size_t)lay.prob[p].off * sizeof(uint32_t), jobs[p].rows, jobs[p].n * sizeof(uint32_t));
  }
  VT_HIP(hipMemcpyAsync(c.dMmrProb.p, c.hMmrUp.p, P * sizeof(vt::MmrProblem), hipMemcpyHostToDevice, c.stream));
  VT_HIP(hipMemcpyAsync(c.dMmrRel.p, c.hMmrUp.p + up_rel, total * sizeof(double), hipMemcpyHostToDevice, c.stream));
  VT_HIP(hipMemcpyAsync(c.dMmrRows.p, c.hMmrUp.p + up_rows, total * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
  for (uint32_t t = 0; t <= lay.max_kk; ++t) VT_HIP(vt::launch_mmr_step(a, t, blocks, (uint32_t)P, c.stream));
  const size_t dn_count = P * sizeof(int), dn_order = dn_count + P * sizeof(uint32_t);
  VT_TRY(c.hMmrDown.ensure(dn_order + total * sizeof(uint32_t)));
  VT_HIP(hipMemcpyAsync(c.hMmrDown.p, c.dMmrStatus.p, P * sizeof(int), hipMemcpyDeviceToHost, c.stream));
  VT_HIP(hipMemcpyAsync(c.hMmrDown.p + dn_count, c.dMmrCount.p, P * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
  VT_HIP(hipMemcpyAsync(c.hMmrDown.p + dn_order, c.dMmrOrder.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
  VT_HIP(hipStreamSynchronize(c.stream));
  const int *st = reinterpret_cast<const int *>(c.hMmrDown.p);
  const uint32_t *cnt = reinterpret_cast<const uint32_t *>(c.hMmrDown.p + dn_count);
  const uint32_t *ord = reinterpret_cast<const uint32_t *>(c.hMmrDown.p + dn_order);
  for (size_t p = 0; p < P; ++p) {
    const int r = vt_host::mmr_collect(lay.prob[p], st[p], cnt[p], ord, &(*orders)[p]);
    if (r < 0) return fail(VT_ERR_DEVICE, "internal: an MMR chain ended before its last round");
    if (r != VT_OK && r != VT_ERR_OVERFLOW) return r;
    (*status)[p] = r;
  }
  return VT_OK;
}

// ------------------------------------------------------------------ vt_mmr_rerank: rows that come with the call
int mmr_rerank_stateless(int device, int metric_code, size_t count, size_t d, const float *values, const double *scores,
                         double alpha, size_t final_k, uint32_t *order, size_t *order_len) {
  // mmr_rerank/5's guards and validate_mmr_initial's finite scores are one status here; then the metric, the vectors
  if (!mmr_guards_ok(alpha, final_k) || !mmr_scores_ok(scores, count)) return VT_ERR_MMR_ARGS;
  if (metric_code < VT_L2 || metric_code > VT_JACCARD) return VT_ERR_UNKNOWN_METRIC;
  if (d == 0) return VT_ERR_EMPTY;
  VT_TRY(validate_finite(values, count * d));
  *order_len = 0;
  if (count == 0) return VT_OK;
  if (count > 0x7fffffffu || d > 0x7ffffff0u) return fail(VT_ERR_UNSUPPORTED, "MMR batch too large");
  StatelessLease lease;
  VT_TRY(stateless_lease(device, &lease));
  Ctx &c = lease.s->ctx;
  UploadRing &ring = lease.s->ring;
  const uint32_t ld = round_up_u32((uint32_t)d, 4);
  VT_TRY(ring.open());
  VT_TRY(ring.reserve(0, count * ld, 1));
  float *hX = ring.hX[0].p;
  for (size_t i = 0; i < count; ++i) {
    std::memcpy(hX + i * ld, values + i * d, d * sizeof(float));
    for (size_t j = d; j < ld; ++j) hX[i * ld + j] = 0.0f;
  }
  ring.hOff[0].p[0] = 0;
  VT_TRY(ring.send(0, count * ld, 1));
  VT_TRY(ring.wait_ready(0, c.stream));
  std::vector<uint32_t> rows(count);
  for (size_t i = 0; i < count; ++i) rows[i] = (uint32_t)i;
  const MmrJob job{rows.data(), scores, count, final_k, alpha};
  std::vector<std::vector<uint32_t>> orders;
  std::vector<int> status;
  const int rc = mmr_run(c, ring.dX[0].p, ld, (uint32_t)d, metric_code, default_order(), &job, 1, &orders, &status);
  VT_TRY(ring.mark_consumed(0, c.stream));
  VT_TRY(rc);
  VT_TRY(status[0]);
  std::copy(orders[0].begin(), orders[0].end(), order);
  *order_len = orders[0].size();
  return VT_OK;
}

// ------------------------------------------------------------------ the handle calls
// (a read like a search: read_single's shared lock and leased context; no derived column is needed)
int mmr_refuse_sharded(const vt_flat *h) {
  return h->multi() ? fail(VT_ERR_UNSUPPORTED, "MMR reranking runs on a one-shard handle: a sharded handle's rows live on several devices")
                    : VT_OK;
}

int flat_mmr_rerank(vt_flat *h, size_t count, const char *ids, const size_t *id_off, const double *scores, double alpha,
                    size_t final_k, uint32_t *order, size_t *order_len) {
  if (!mmr_guards_ok(alpha, final_k) || !mmr_scores_ok(scores, count)) return VT_ERR_MMR_ARGS;
  VT_TRY(mmr_refuse_sharded(h));
  *order_len = 0;
  return read_single(h, 0, 1, [&](Shard *ix, Ctx &c) -> int {
    std::vector<uint32_t> rows;
    std::unordered_set<uint32_t> seen;
    if (!mmr_rows_of_ids(ix->row_of, count, ids, id_off, rows, seen)) return VT_ERR_MMR_ARGS;
    if (count == 0) return VT_OK;
    const MmrJob job{rows.data(), scores, count, final_k, alpha};
    std::vector<std::vector<uint32_t>> orders;
    std::vector<int> status;
    VT_TRY(mmr_run(c, ix->dX, ix->ld, (uint32_t)ix->dim, ix->metric, ix->order, &job, 1, &orders, &status));
    VT_TRY(status[0]);
    std::copy(orders[0].begin(), orders[0].end(), order);
    *order_len = orders[0].size();
    return VT_OK;
  });
}

// Several rerank problems over the resident rows in one launch chain: problem p owns entries [prob_off[p], prob_off[p + 1])
// of ids / scores / order, with its own alpha[p] and final_k[p].  A problem's own error -- its arguments, its ids,
// "metric overflow" -- is its status; the problems that stand go to the device together.
int flat_mmr_rerank_batch(vt_flat *h, size_t nprob, const size_t *prob_off, const char *ids, const size_t *id_off,
                          const double *scores, const double *alpha, const size_t *final_k, uint32_t *order, size_t *order_len,
                          int *prob_status) {
  VT_TRY(mmr_refuse_sharded(h));
  std::vector<int> status(nprob, VT_OK);
  for (size_t p = 0; p < nprob; ++p) {
    order_len[p] = 0;
    if (!mmr_guards_ok(alpha[p], final_k[p]) || !mmr_scores_ok(scores + prob_off[p], prob_off[p + 1] - prob_off[p]))
      status[p] = VT_ERR_MMR_ARGS;
  }
  const int st = read_single(h, 0, 1, [&](Shard *ix, Ctx &c) -> int {
    std::vector<std::vector<uint32_t>> rows(nprob);
    std::unordered_set<uint32_t> seen;
    std::vector<MmrJob> jobs;
    std::vector<size_t> which;
    for (size_t p = 0; p < nprob; ++p) {
      if (status[p] != VT_OK) continue;
      const size_t n = prob_off[p + 1] - prob_off[p];
      if (!mmr_rows_of_ids(ix->row_of, n, ids, id_off + prob_off[p], rows[p], seen)) {
        status[p] = VT_ERR_MMR_ARGS;
        continue;
      }
      jobs.push_back(MmrJob{rows[p].data(), scores + prob_off[p], n, final_k[p], alpha[p]});
      which.push_back(p);
    }
    std::vector<std::vector<uint32_t>> orders;
    std::vector<int> run;
    VT_TRY(mmr_run(c, ix->dX, ix->ld, ix->dim > 0 ? (uint32_t)ix->dim : 1u, ix->metric, ix->order, jobs.data(), jobs.size(), &orders, &run));
    for (size_t j = 0; j < which.size(); ++j) {
      const size_t p = which[j];
      status[p] = run[j];
      if (run[j] != VT_OK) continue;
      std::copy(orders[j].begin(), orders[j].end(), order + prob_off[p]);
      order_len[p] = orders[j].size();
    }
    return VT_OK;
  });
  VT_TRY(st);
  // without prob_status the first failing problem, in batch order, fails the call (vt_hnsw_search_batch's convention)
  for (size_t p = 0; p < nprob; ++p) {
    if (prob_status) prob_status[p] = status[p];
    else if (status[p] != VT_OK) return status[p];
  }
  return VT_OK;
}

// MMR over the hit lists of nq searches that have just run on (ix, c), still under their lease: the hits' rows through
// the id table, their scores by result_values, all queries one launch chain.  Query i's order lands at order + i * cap
// (cap = min(final_k, candidates)), its length in order_len[i], its own status in status[i].
int mmr_over_hits(Shard *ix, Ctx &c, vt_hits *const *hits, size_t nq, double alpha, size_t final_k, int score_mode, size_t cap,
                  uint32_t *order, size_t *order_len, int *status) {
  std::vector<std::vector<uint32_t>> rows(nq);
  std::vector<std::vector<double>> rel(nq);
  std::vector<MmrJob> jobs(nq);
  for (size_t i = 0; i < nq; ++i) {
    const vt_hits *h = hits[i];
    const size_t n = h ? h->ids.size() : 0;
    rows[i].resize(n);
    rel[i].resize(n);
    for (size_t j = 0; j < n; ++j) {
      const std::string &id = h->ids[j];
      const uint32_t r = ix->row_of.find(id.data(), id.size(), vt_host::hash_id(id.data(), id.size()));
      if (r == vt_host::IdTable::kNone) return fail(VT_ERR_DEVICE, "internal: a hit's id is not in the index it came from");
      rows[i][j] = r;
      rel[i][j] = mmr_hit_score(ix->metric, h->raw[j], score_mode);
    }
    jobs[i] = MmrJob{rows[i].data(), rel[i].data(), n, final_k, alpha};
  }
  std::vector<std::vector<uint32_t>> orders;
  std::vector<int> st;
  VT_TRY(mmr_run(c, ix->dX, ix->ld, ix->dim > 0 ? (uint32_t)ix->dim : 1u, ix->metric, ix->order, jobs.data(), nq, &orders, &st));
  for (size_t i = 0; i < nq; ++i) {
    status[i] = st[i];
    order_len[i] = std::min(orders[i].size(), cap);
    std::copy(orders[i].begin(), orders[i].begin() + order_len[i], order + i * cap);
  }
  return VT_OK;
}

int flat_mmr_search(vt_flat *h, const float *query, size_t n, size_t candidates, size_t final_k, double alpha, int score_mode,
                    vt_hits **out, uint32_t *order, size_t *order_len) {
  if (!mmr_guards_ok(alpha, final_k) || (score_mode != 0 && score_mode != 1)) return VT_ERR_MMR_ARGS;
  VT_TRY(mmr_refuse_sharded(h));
  *order_len = 0;
  // the search is search_direct's (vt_multi.h), what vt_flat_search runs behind its queue: the hits are its hits
  int mmr_status = VT_OK;
  const int st = search_direct(h, query, n, candidates, out, [&](Shard *ix, Ctx &c) -> int {
    return mmr_over_hits(ix, c, out, 1, alpha, final_k, score_mode, std::min(final_k, candidates), order, order_len, &mmr_status);
  });
  if (st == VT_OK && mmr_status == VT_OK) return VT_OK;
  delete *out;
  *out = nullptr;
  *order_len = 0;
  return st != VT_OK ? st : mmr_status;
}

int flat_mmr_search_batch(vt_flat *h, const float *queries, size_t nq, size_t d, size_t candidates, size_t final_k, double alpha,
                          int score_mode, vt_hits **out, uint32_t *order, size_t *order_len, int *query_status) {
  if (!mmr_guards_ok(alpha, final_k) || (score_mode != 0 && score_mode != 1)) return VT_ERR_MMR_ARGS;
  VT_TRY(mmr_refuse_sharded(h));
  for (size_t i = 0; i < nq; ++i) {
    out[i] = nullptr;
    order_len[i] = 0;
  }
  if (nq == 0) return VT_OK;
  auto drop = [&]() {
    for (size_t i = 0; i < nq; ++i) {
      delete out[i];
      out[i] = nullptr;
      order_len[i] = 0;
    }
  };
  // the search is batch_direct's (vt_multi.h), what vt_flat_search_batch runs: the hits are its hits; it leaves every
  // out[i] NULL when it fails
  std::vector<int> status(nq, VT_OK);
  int st = batch_direct(h, queries, nq, d, candidates, out, [&](Shard *ix, Ctx &c) -> int {
    return mmr_over_hits(ix, c, out, nq, alpha, final_k, score_mode, std::min(final_k, candidates), order, order_len, status.data());
  });
  // without query_status the first failing query, in batch order, fails the call (vt_hnsw_search_batch's convention)
  for (size_t i = 0; i < nq && st == VT_OK && !query_status; ++i) st = status[i];
  if (st != VT_OK) {
    drop();
    return st;
  }
  for (size_t i = 0; i < nq; ++i) {
    if (status[i] != VT_OK) {  // a query's own error: no hits, no order
      delete out[i];
      out[i] = nullptr;
      order_len[i] = 0;
    }
    if (query_status) query_status[i] = status[i];
  }
  return VT_OK;
}

}  // namespace
