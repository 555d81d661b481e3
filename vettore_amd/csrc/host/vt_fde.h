// vt_fde.h -- the MUVERA retrieval flow over a resident multi-vector store (vt_mv) and a flat index of its documents'
// fixed-dimensional encodings: encode every document (K10s, vt_muvera.hip, straight from the store's slab), keep the
// encodings in a flat inner-product handle (vt_mv_fde_sync), search that handle with the query's encoding and rerank the
// candidates with exact MaxSim (vt_mv_fde_top_k, vt_mv_fde_top_k_batch).  The sync's planning is host/vt_fdeplan.h.
// Part of vt_index.cpp's translation unit (included there, in this order, exactly once).
//
// Locks: the store's mutex is held for a whole call; the index is used through its own entry points (vt_flat_*), each
// under the index's own lock, always taken after the store's.  The stateless session (the query's encoding) likewise.
#pragma once

namespace {

struct FdeShape {
  size_t out_size = 0, fde = 0;
};

// What every call asks of `index` (fde == 0: the configuration is not valid, its own status comes later).
int fde_check_index(const vt_mv *s, const vt_flat *index, size_t fde) {
  if (vt_flat_shard_count(index) != 1) return fail(VT_ERR_UNSUPPORTED, "the FDE index of a resident store must be a single-shard handle");
  if (vt_flat_shard_device(index, 0) != s->ctx.device) return fail(VT_ERR_ARGUMENT, "the FDE index is not on the store's device");
  if (vt_flat_metric(index) != VT_INNER_PRODUCT) return fail(VT_ERR_ARGUMENT, "the FDE index must be an inner-product handle");
  if (fde && vt_flat_len(index) > 0 && vt_flat_dimension(index) != (long)fde) return VT_ERR_DIMENSION;
  return VT_OK;
}

// The call-level checks of the two encoding calls, behind the NULL checks.
int fde_check_call(const vt_mv *s, const MuveraConfig &m, FdeShape *shape) {
  VT_TRY(muvera_check_config(m));
  VT_TRY(muvera_check_sizes(m, &shape->out_size, &shape->fde));
  if (s->table.dimension() >= 0 && (size_t)s->table.dimension() != m.d) return VT_ERR_DIMENSION;
  return VT_OK;
}

// Document-mode encodings of n resident documents (document i: cnt[i] > 0 rows from first[i] on of the slab), chunk by
// chunk under muvera_chunk_bytes.  After each chunk -- the stream synchronized -- sink(i0, n, rows, status) sees its
// dense device rows [n][fde] and the device's statuses; the buffers are reused once it returns.
template <class Sink>
int fde_encode_resident(vt_mv *s, const MuveraConfig &m, const FdeShape &shape, const uint32_t *first, const uint32_t *cnt,
                        size_t n, Sink sink) {
  if (n == 0) return VT_OK;
  const size_t out_size = shape.out_size, fde = shape.fde;
  if (m.d > vt::kMuveraMaxDim) return fail(VT_ERR_UNSUPPORTED, "vector dimension exceeds what the MUVERA kernel stages in LDS");
  const bool identity = m.pd == m.d;
  const size_t C = m.k + (identity ? 0 : m.pd);
  const size_t table_floats = m.R * m.d * C;
  if (table_floats > kMuveraMaxTable) return fail(VT_ERR_UNSUPPORTED, "MUVERA weight table exceeds 1 GiB");
  Ctx &c = s->ctx;
  VT_TRY(c.bind());
  MuveraState &P = s->F;

  vt::MuveraSlabArgs sa{};
  sa.a = muvera_args(m.d, m.R, m.k, m.pd, 1, out_size);
  vt::MuveraArgs &a = sa.a;
  sa.stride = s->stride;
  const bool global_counts = ((size_t)1 << m.k) > vt::kMuveraLdsPartitions;
  if (table_floats) {
    VT_TRY(P.dTable.ensure(table_floats));
    VT_HIP(vt::launch_muvera_table(m.seed, a.R, a.d, a.k, a.C, P.dTable.p, c.stream));
    a.table = P.dTable.p;
  }
  std::vector<uint32_t> slot_off, slot_list;
  if (m.final_some) {
    muvera_slot_lists(m.seed, out_size, m.final_dim, slot_off, slot_list);
    VT_TRY(P.dSlotOff.ensure(slot_off.size()));
    VT_TRY(P.dSlotList.ensure(std::max<size_t>(slot_list.size(), 1)));
    VT_HIP(hipMemcpyAsync(P.dSlotOff.p, slot_off.data(), slot_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
    VT_HIP(hipMemcpyAsync(P.dSlotList.p, slot_list.data(), slot_list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
    VT_HIP(hipStreamSynchronize(c.stream));
  }

  // chunks of documents: the intermediate rows, the final rows and the counts within the budget (the vectors are there)
  const long forced = vt::env::get(vt::env::MUVERA_CHUNK_BYTES);
  const size_t budget = std::min<size_t>(forced > 0 ? (size_t)forced : kMuveraChunkBytes, (size_t)4 << 30);
  const size_t doc_bytes =
      (out_size + (m.final_some ? fde : 0) + (global_counts ? out_size / m.pd : 0)) * sizeof(float) + 2 * sizeof(uint32_t);
  std::vector<size_t> cut;
  vt_host::fde_chunk_cuts(n, doc_bytes, budget, std::max<size_t>(1, 0x7fffffffull / a.groups), &cut);

  for (size_t k = 0; k + 1 < cut.size(); ++k) {
    const size_t i0 = cut[k], nd = cut[k + 1] - i0;
    VT_TRY(P.dFull.ensure(nd * out_size));
    VT_TRY(P.dStatus.ensure(nd));
    VT_TRY(P.hStatus.ensure(nd));
    VT_TRY(s->dFdeDoc.ensure(2 * nd));
    VT_HIP(hipMemsetAsync(P.dFull.p, 0, nd * out_size * sizeof(float), c.stream));
    VT_HIP(hipMemsetAsync(P.dStatus.p, 0, nd * sizeof(int), c.stream));
    VT_HIP(hipMemcpyAsync(s->dFdeDoc.p, first + i0, nd * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
    VT_HIP(hipMemcpyAsync(s->dFdeDoc.p + nd, cnt + i0, nd * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
    a.counts = nullptr;
    if (global_counts) {
      const size_t words = nd * (out_size / m.pd);
      VT_TRY(P.dCounts.ensure(words));
      VT_HIP(hipMemsetAsync(P.dCounts.p, 0, words * sizeof(uint32_t), c.stream));
      a.counts = P.dCounts.p;
    }
    a.X = s->X.p;
    a.set_off = nullptr;
    a.nsets = (uint32_t)nd;
    a.full = P.dFull.p;
    a.status = P.dStatus.p;
    sa.doc_first = s->dFdeDoc.p;
    sa.doc_cnt = s->dFdeDoc.p + nd;
    if (vt::muvera_slab_lds_bytes(sa) > 160u * 1024) return fail(VT_ERR_UNSUPPORTED, "MUVERA: the vector and the partition counts exceed the LDS");
    VT_HIP(vt::launch_muvera_encode_slab(sa, c.stream));
    const float *rows = P.dFull.p;
    if (m.final_some) {
      VT_TRY(P.dFinal.ensure(nd * fde));
      VT_HIP(vt::launch_muvera_sketch(P.dFull.p, out_size, a.nsets, (uint32_t)fde, P.dSlotOff.p, P.dSlotList.p, P.dFinal.p, P.dStatus.p,
                                      c.stream));
      rows = P.dFinal.p;
    }
    VT_HIP(hipMemcpyAsync(P.hStatus.p, P.dStatus.p, nd * sizeof(int), hipMemcpyDeviceToHost, c.stream));
    VT_HIP(hipStreamSynchronize(c.stream));  // the rows are complete before anybody else's stream reads them
    VT_TRY(sink(i0, nd, rows, P.hStatus.p));
    VT_TRY(c.bind());  // (the sink may have bound another context of this device)
  }
  return VT_OK;
}

// the first failing document in list order, where the caller has no place for statuses (vt_muvera_encode's convention)
int fde_report(const std::vector<int> &st, size_t count, int *doc_status) {
  if (doc_status && count) std::memcpy(doc_status, st.data(), count * sizeof(int));
  if (doc_status && count != 1) return VT_OK;
  for (size_t i = 0; i < count; ++i)
    if (st[i] != VT_OK) return st[i];
  return VT_OK;
}

int mv_encode_documents(vt_mv *s, size_t count, const char *ids, const size_t *id_off, const MuveraConfig &m, float *out,
                        int *doc_status) {
  FdeShape shape;
  VT_TRY(fde_check_call(s, m, &shape));
  if (count == 0) return VT_OK;
  if (!out) return VT_ERR_ARGUMENT;
  const size_t fde = shape.fde;
  std::vector<int> st(count, VT_OK);
  std::vector<uint32_t> where, first, cnt;  // the documents that are encoded: place in the list, rows
  for (size_t i = 0; i < count; ++i) {
    const size_t n = id_off[i + 1] - id_off[i];
    const uint32_t slot = s->table.find(n ? ids + id_off[i] : "", n);
    if (slot == vt_host::MvTable::kNone || s->table.slots()[slot].rows == 0) {
      st[i] = VT_ERR_EMPTY_SET;
      std::memset(out + i * fde, 0, fde * sizeof(float));
      continue;
    }
    where.push_back((uint32_t)i);
    first.push_back(s->table.slots()[slot].first_row);
    cnt.push_back(s->table.slots()[slot].rows);
  }
  std::vector<float> host;
  VT_TRY(fde_encode_resident(s, m, shape, first.data(), cnt.data(), where.size(),
                             [&](size_t i0, size_t n, const float *rows, const int *status) -> int {
    host.resize(n * fde);
    VT_HIP(hipMemcpy(host.data(), rows, n * fde * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
      float *dst = out + (size_t)where[i0 + i] * fde;
      if (status[i] != 0) {
        st[where[i0 + i]] = status[i];
        std::memset(dst, 0, fde * sizeof(float));
      } else {
        std::memcpy(dst, &host[i * fde], fde * sizeof(float));
      }
    }
    return VT_OK;
  }));
  return fde_report(st, count, doc_status);
}

int mv_fde_sync(vt_mv *s, vt_flat *index, size_t count, const char *ids, const size_t *id_off, const MuveraConfig &m,
                int *doc_status) {
  FdeShape shape;
  VT_TRY(fde_check_call(s, m, &shape));
  VT_TRY(fde_check_index(s, index, shape.fde));
  const size_t fde = shape.fde;

  // count == 0 without ids: every live document, in store order
  std::string all_ids;
  std::vector<size_t> all_off;
  if (count == 0 && !ids) {
    all_off.push_back(0);
    for (const vt_host::MvSlot &slot : s->table.slots())
      if (slot.live) {
        all_ids += slot.id;
        all_off.push_back(all_ids.size());
      }
    count = all_off.size() - 1;
    ids = all_ids.data();
    id_off = all_off.data();
    doc_status = nullptr;  // (nobody listed anything: the first failing document, in store order, is the call's status)
  }
  if (count == 0) return VT_OK;
  if (count > 0xFFFFFFF0ull) return fail(VT_ERR_UNSUPPORTED, "more than 2^32-16 ids");

  vt_host::FdeSyncPlan plan;
  vt_host::fde_sync_plan(count, ids, id_off, [&](const char *id, size_t n) {
    const uint32_t slot = s->table.find(id, n);
    if (slot == vt_host::MvTable::kNone) return vt_host::kFdeAbsent;
    return s->table.slots()[slot].rows ? vt_host::kFdeRows : vt_host::kFdeEmpty;
  }, &plan);
  auto id_of = [&](uint32_t u) { return ids + id_off[plan.first_pos[u]]; };
  auto len_of = [&](uint32_t u) { return id_off[plan.first_pos[u] + 1] - id_off[plan.first_pos[u]]; };

  std::vector<int> ust(plan.state.size(), VT_OK);  // per distinct id
  for (uint32_t u : plan.remove) {
    VT_TRY(vt_flat_delete(index, id_of(u), len_of(u)));
    if (plan.state[u] == vt_host::kFdeEmpty) ust[u] = VT_ERR_EMPTY_SET;
  }

  // the documents to encode, their ids packed in the same order: a run of a chunk's rows is a run of these offsets
  const size_t ne = plan.encode.size();
  std::vector<uint32_t> first(ne), cnt(ne);
  std::string enc_ids;
  std::vector<size_t> enc_off(ne + 1, 0);
  for (size_t i = 0; i < ne; ++i) {
    const uint32_t u = plan.encode[i];
    const vt_host::MvSlot &slot = s->table.slots()[s->table.find(id_of(u), len_of(u))];
    first[i] = slot.first_row;
    cnt[i] = slot.rows;
    enc_ids.append(id_of(u), len_of(u));
    enc_off[i + 1] = enc_ids.size();
  }
  std::vector<std::pair<size_t, size_t>> runs;
  VT_TRY(fde_encode_resident(s, m, shape, first.data(), cnt.data(), ne,
                             [&](size_t i0, size_t n, const float *rows, const int *status) -> int {
    vt_host::fde_good_runs(status, n, &runs);
    for (const auto &r : runs)
      VT_TRY(vt_flat_load_device_matrix(index, r.second - r.first, fde, enc_ids.data(), enc_off.data() + i0 + r.first,
                                        rows + r.first * fde));
    for (size_t i = 0; i < n; ++i)
      if (status[i] != 0) {
        const uint32_t u = plan.encode[i0 + i];
        ust[u] = status[i];
        VT_TRY(vt_flat_delete(index, id_of(u), len_of(u)));
      }
    return VT_OK;
  }));

  std::vector<int> st(count);
  for (size_t i = 0; i < count; ++i) st[i] = ust[plan.unique_of[i]];
  return fde_report(st, count, doc_status);
}

// Steps 3 and 4 of vt_mv_fde_top_k's statuses for the query vectors [v0, v1): vt_mv_top_k's validation up to the
// device, then vt_muvera_encode(mode 0, count 1)'s on the host.
int fde_check_query(const vt_mv *s, const MuveraConfig &m, const float *query, const size_t *query_off, size_t v0, size_t v1) {
  VT_TRY(maxsim_validate_standalone(query, query_off, v0, v1));
  const size_t dim = v1 > v0 ? query_off[v0 + 1] - query_off[v0] : 0;
  if (v1 > v0 && s->table.dimension() >= 0 && (size_t)s->table.dimension() != dim) return VT_ERR_DIMENSION;
  if (v0 == v1) return VT_ERR_EMPTY_SET;
  VT_TRY(muvera_check_config(m));
  VT_TRY(muvera_check_set(query, query_off, v0, v1, m.d));
  size_t out_size = 0, fde = 0;
  return muvera_check_sizes(m, &out_size, &fde);
}

size_t fde_dimension_or_zero(const MuveraConfig &m) {
  size_t out_size = 0, fde = 0;
  if (muvera_check_config(m) != VT_OK || muvera_check_sizes(m, &out_size, &fde) != VT_OK) return 0;
  return fde;
}

// ids of a hit list as one blob with offsets
void fde_pack_ids(const vt_hits *h, std::string &blob, std::vector<size_t> &off) {
  for (const std::string &id : h->ids) {
    blob += id;
    off.push_back(blob.size());
  }
}

int mv_fde_top_k(vt_mv *s, vt_flat *index, const MuveraConfig &m, const float *query, const size_t *query_off, size_t nquery,
                 size_t candidates, int metric_code, size_t limit, vt_hits **out) {
  const size_t fde = fde_dimension_or_zero(m);
  VT_TRY(fde_check_index(s, index, fde));
  if (metric_code < VT_L2 || metric_code > VT_JACCARD) return VT_ERR_UNKNOWN_METRIC;
  VT_TRY(fde_check_query(s, m, query, query_off, 0, nquery));
  std::vector<float> qfde(fde);
  const size_t one_set[2] = {0, nquery};
  VT_TRY(muvera_encode(s->ctx.device, 0, 1, one_set, query, query_off, m, qfde.data(), nullptr));
  if (candidates == 0 || vt_flat_len(index) == 0) return empty_hits(out);
  vt_hits *found = nullptr;
  VT_TRY(vt_flat_search(index, qfde.data(), fde, candidates, &found));
  std::unique_ptr<vt_hits> H(found);
  std::string blob;
  std::vector<size_t> off{0};
  fde_pack_ids(H.get(), blob, off);
  return mv_search(s, true, off.size() - 1, blob.data(), off.data(), query, query_off, nquery, metric_code, limit, out);
}

// out[b] / status[b]: mv_fde_top_k's for set b.  A status other than VT_OK returned from here is the call's own.
int mv_fde_top_k_sets(vt_mv *s, vt_flat *index, const MuveraConfig &m, size_t nsets, const size_t *set_vec_off, const float *query,
                      const size_t *query_off, size_t candidates, int metric_code, size_t limit, vt_hits **out, int *status) {
  const size_t fde = fde_dimension_or_zero(m);
  // the valid sets, their vectors packed one behind the other
  std::vector<uint32_t> valid;
  std::vector<float> q2;
  std::vector<size_t> qoff2{0}, svo2{0};
  for (size_t b = 0; b < nsets; ++b) {
    const size_t v0 = set_vec_off[b], v1 = set_vec_off[b + 1];
    status[b] = fde_check_query(s, m, query, query_off, v0, v1);
    if (status[b] != VT_OK) continue;
    valid.push_back((uint32_t)b);
    for (size_t v = v0; v < v1; ++v) {
      q2.insert(q2.end(), query + query_off[v], query + query_off[v + 1]);
      qoff2.push_back(q2.size());
    }
    svo2.push_back(qoff2.size() - 1);
  }
  size_t nv = valid.size();
  if (nv == 0) return VT_OK;

  // one encoding call for all of them; a set that overflows keeps its status and leaves
  std::vector<float> qfde(nv * fde);
  std::vector<int> est(nv, VT_OK);
  const int erc = muvera_encode(s->ctx.device, 0, nv, svo2.data(), q2.data(), qoff2.data(), m, qfde.data(), est.data());
  if (nv == 1) est[0] = erc;  // (one set: the call is the NIF, its status the set's)
  else if (erc != VT_OK) return erc;
  std::vector<uint32_t> keep;  // places among the valid sets
  for (size_t k = 0; k < nv; ++k) {
    if (est[k] != VT_OK) status[valid[k]] = est[k];
    else keep.push_back((uint32_t)k);
  }
  if (keep.empty()) return VT_OK;
  if (candidates == 0 || vt_flat_len(index) == 0) {
    for (uint32_t k : keep) VT_TRY(empty_hits(&out[valid[k]]));
    return VT_OK;
  }
  if (keep.size() != nv) {  // close the rows and the vectors up
    std::vector<float> f2, q3;
    std::vector<size_t> qoff3{0}, svo3{0};
    for (uint32_t k : keep) {
      f2.insert(f2.end(), qfde.begin() + (size_t)k * fde, qfde.begin() + (size_t)(k + 1) * fde);
      for (size_t v = svo2[k]; v < svo2[k + 1]; ++v) {
        q3.insert(q3.end(), q2.begin() + qoff2[v], q2.begin() + qoff2[v + 1]);
        qoff3.push_back(q3.size());
      }
      svo3.push_back(qoff3.size() - 1);
    }
    qfde.swap(f2);
    q2.swap(q3);
    qoff2.swap(qoff3);
    svo2.swap(svo3);
  }
  std::vector<uint32_t> set_of(keep.size());
  for (size_t k = 0; k < keep.size(); ++k) set_of[k] = valid[keep[k]];
  nv = keep.size();

  // one search of the index for all of them
  std::vector<vt_hits *> found(nv, nullptr);
  struct Drop {
    std::vector<vt_hits *> &h;
    ~Drop() { for (vt_hits *p : h) delete p; }
  } drop{found};
  const int src = vt_flat_search_batch(index, qfde.data(), nv, fde, candidates, found.data());
  if (src != VT_OK) {  // (what every lone call's search would have answered)
    for (size_t k = 0; k < nv; ++k) status[set_of[k]] = src;
    return VT_OK;
  }
  std::string blob;
  std::vector<size_t> off{0}, set_id_off{0};
  for (size_t k = 0; k < nv; ++k) {
    fde_pack_ids(found[k], blob, off);
    set_id_off.push_back(off.size() - 1);
  }

  // one pass through the batched rerank
  std::vector<vt_hits *> ranked(nv, nullptr);
  std::vector<int> rst(nv, VT_OK);
  Drop drop2{ranked};
  VT_TRY(mv_search_batch(s, true, nv, set_id_off.data(), blob.data(), off.data(), svo2.data(), q2.data(), qoff2.data(), metric_code,
                         limit, ranked.data(), rst.data()));
  for (size_t k = 0; k < nv; ++k) {
    status[set_of[k]] = rst[k];
    if (rst[k] == VT_OK) std::swap(out[set_of[k]], ranked[k]);
  }
  return VT_OK;
}

// vt_mv_fde_top_k_batch behind its argument checks: vt_mv_top_k_ids_batch's conventions (mv_batch_call)
int mv_fde_batch_call(vt_mv *s, vt_flat *index, const MuveraConfig &m, size_t nsets, const size_t *set_vec_off, const float *query,
                      const size_t *query_off, size_t candidates, int metric_code, size_t limit, vt_hits **out, int *set_status) {
  for (size_t b = 0; b < nsets; ++b) out[b] = nullptr;
  std::lock_guard<std::mutex> g(s->mu);
  VT_TRY(fde_check_index(s, index, fde_dimension_or_zero(m)));
  if (metric_code < VT_L2 || metric_code > VT_JACCARD) return VT_ERR_UNKNOWN_METRIC;
  if (nsets == 0) return VT_OK;
  std::vector<int> status(nsets, VT_OK);
  auto drop = [&]() {  // a call that fails leaves every out[b] NULL
    for (size_t b = 0; b < nsets; ++b) {
      delete out[b];
      out[b] = nullptr;
    }
  };
  int rc;
  try {
    rc = mv_fde_top_k_sets(s, index, m, nsets, set_vec_off, query, query_off, candidates, metric_code, limit, out, status.data());
  } catch (...) {
    drop();
    throw;
  }
  for (size_t b = 0; b < nsets && rc == VT_OK && !set_status; ++b) rc = status[b];
  if (rc != VT_OK) {
    drop();
    return rc;
  }
  for (size_t b = 0; b < nsets && set_status; ++b) {
    set_status[b] = status[b];
    if (status[b] != VT_OK && out[b]) {
      delete out[b];
      out[b] = nullptr;
    }
  }
  return VT_OK;
}

}  // namespace
