// vt_sketchsearch.h -- the sketch searches of a shard: what tells the tiers apart on the device side, the gate's
// shape filled from a shard, the three chains (sketch_search, sketch_group_search, nibble_search) and the columns' upkeep.
// The tiers' constants and the gate itself are plain C++ in vt_sketchtiers.h.
// Part of vt_index.cpp's translation unit (included there, in this order, exactly once): the host
// side is one TU on purpose -- everything below the C ABI lives in an anonymous namespace.
#pragma once

namespace {

static_assert(vt::kSketch6Levels == vt_host::kSketch6Levels, "one number of query levels on both sides");
static_assert(vt::kSketchMaxDim == vt_host::kSketchGateMaxDim, "one largest dimension on both sides");
static_assert(vt::kMaxFusedK == (int)vt_host::kSketchListMax, "one longest list on both sides");
static_assert(vt::kSketch4BlockLists == vt_host::kSketchTiers[vt_host::kTier4].block_lists, "one number of lists a block of K1n's pass leaves");
static_assert(vt_host::sketch_batch_list_k(10) == vt_host::sketch_list_k(10) && vt_host::sketch_batch_list_k(32) == vt_host::sketch_list_k(32),
              "K1qm's lists are K1q's");

using vt_host::sketch_list_k;

bool sketch_dot_metric(int metric) { return metric == VT_COSINE || metric == VT_INNER_PRODUCT || metric == VT_NEG_INNER_PRODUCT; }
bool sketch_l2_metric(int metric) { return metric == VT_L2 || metric == VT_L2_SQUARED; }

// What tells the sketch columns apart on the device side, by tier (vt_sketchtiers.h holds the rest of the row): the column's
// size, its builders and pass, the bound of a query level its pass keeps off a plane, its counters and its refusal hook.
// index_ensure_sketch, nibble_search and every walk over the tiers go by this one table and that one.
struct SketchKind {
  size_t (*bytes)(uint32_t rows, uint32_t d);
  hipError_t (*build)(const float *, size_t, uint32_t, uint32_t, uint32_t, void *, unsigned long long *, hipStream_t);
  hipError_t (*rows)(const float *, size_t, const uint32_t *, uint32_t, uint32_t, uint32_t, void *, unsigned long long *, hipStream_t);
  // (the same two for a column with xx_r, Shard::sketch_xx; null: the tier has none)
  hipError_t (*build_xx)(const float *, size_t, uint32_t, uint32_t, uint32_t, void *, unsigned long long *, hipStream_t);
  hipError_t (*rows_xx)(const float *, size_t, const uint32_t *, uint32_t, uint32_t, uint32_t, void *, unsigned long long *, hipStream_t);
  size_t (*scan_lds)(uint32_t d, uint32_t k);
  hipError_t (*scan)(const vt::Sketch6ScanArgs &, uint32_t, hipStream_t);  // (null: K1q's pass takes other arguments)
  // c3, w3 of the query's last level (null: one plane, every level meets every bit -- both are zero)
  void (*level_bound)(const uint32_t *level, uint32_t lw, float t, double *c, double *w);
  uint64_t vt_profile::*launches;
  double vt_profile::*ms;
  uint64_t vt_profile::*bytes_read, vt_profile::*candidates, vt_profile::*fallbacks, vt_profile::*builds, vt_profile::*patched_rows;
  uint64_t vt_profile::*tail_words;  // (null: not counted)
  vt::env::Key refuse_hook;
  size_t elems(const Shard *ix) const { return bytes((uint32_t)std::max<size_t>(ix->cap, ix->n), (uint32_t)ix->dim); }
};
const SketchKind &sketch_kind(int tier) {
  static const SketchKind kinds[vt_host::kSketchTierCount] = {
      {vt::sketch4_bytes, vt::launch_sketch4_build, vt::launch_sketch4_rows, nullptr, nullptr, vt::sketch4_scan_lds_bytes,
       vt::launch_sketch4_scan, nullptr, &vt_profile::sketch4_launches, &vt_profile::sketch4_ms, &vt_profile::sketch4_bytes,
       &vt_profile::sketch4_candidates, &vt_profile::sketch4_fallbacks, &vt_profile::sketch4_builds, &vt_profile::sketch4_patched_rows,
       nullptr, vt::env::TEST_REFUSE_SKETCH4},
      {vt::sketch5_bytes, vt::launch_sketch5_build, vt::launch_sketch5_rows, nullptr, nullptr, vt::sketch5_scan_lds_bytes,
       vt::launch_sketch5_scan, vt_host::sketch5_level_bound, &vt_profile::sketch5_launches, &vt_profile::sketch5_ms,
       &vt_profile::sketch5_bytes, &vt_profile::sketch5_candidates, &vt_profile::sketch5_fallbacks, &vt_profile::sketch5_builds,
       &vt_profile::sketch5_patched_rows, nullptr, vt::env::TEST_REFUSE_SKETCH5},
      {vt::sketch6_bytes, vt::launch_sketch6_build, vt::launch_sketch6_rows, nullptr, nullptr, vt::sketch6_scan_lds_bytes,
       vt::launch_sketch6_scan, vt_host::sketch6_level_bound, &vt_profile::sketch6_launches, &vt_profile::sketch6_ms,
       &vt_profile::sketch6_bytes, &vt_profile::sketch6_candidates, &vt_profile::sketch6_fallbacks, &vt_profile::sketch6_builds,
       &vt_profile::sketch6_patched_rows, &vt_profile::sketch6_tail_words, vt::env::TEST_REFUSE_SKETCH6},
      {vt::sketch_bytes, vt::launch_sketch_build, vt::launch_sketch_rows, vt::launch_sketch_build_xx, vt::launch_sketch_rows_xx,
       vt::sketch_scan_lds_bytes, nullptr, nullptr, &vt_profile::sketch_launches, &vt_profile::sketch_ms, &vt_profile::sketch_bytes,
       &vt_profile::sketch_candidates, &vt_profile::sketch_fallbacks, &vt_profile::sketch_builds, &vt_profile::sketch_patched_rows,
       nullptr, vt::env::TEST_REFUSE_SKETCH},
  };
  return kinds[tier];
}

// ---- the gate ------------------------------------------------------------------------------------------------------------
// The tiers a lone search of `limit` hits on this shard wants (a mask of 1 << tier, vt_host::sketch_tiers_wanted): the
// shard and the settings as the gate's plain values.  NEED_SKETCH asks for those columns, NEED_SKETCH8 for the int8 one
// alone, and both mean nothing where this says no.
unsigned sketch_tiers(const Shard *ix, size_t limit) {
  vt_host::SketchGateShape s;
  s.family = sketch_dot_metric(ix->metric) ? vt_host::kSketchDot : sketch_l2_metric(ix->metric) ? vt_host::kSketchL2 : vt_host::kSketchNoFamily;
  if (s.family == vt_host::kSketchNoFamily) return 0;
  s.ranks_clean = ix->ranks_clean;
  s.single_nominate = ix->single_nominate != 0;
  s.no_rows = ix->n == 0;
  s.dim = ix->dim;
  s.row_bytes = (double)ix->n * ix->ld * 4.0;
  s.sketch = vt::env::get(vt::env::SKETCH);
  s.sketch6 = vt::env::get(vt::env::SKETCH6);
  s.force_sketch = vt::env::get(vt::env::FORCE_SKETCH);
  s.force_sketch6 = vt::env::get(vt::env::FORCE_SKETCH6);
  const bool dim_ok = ix->dim > 0 && ix->dim <= (long)vt::kSketchMaxDim;
  for (int t = 0; t < vt_host::kSketchTierCount; ++t) {
    const uint32_t list_k = vt_host::kSketchTiers[t].list_k ? vt_host::kSketchTiers[t].list_k : sketch_list_k(limit);
    s.refused[t] = ix->sketches[t].col.refused;
    s.pass_fits[t] = dim_ok && sketch_kind(t).scan_lds((uint32_t)ix->dim, list_k) != 0;
  }
  return vt_host::sketch_tiers_wanted(s, limit);
}

// K1qm (vt_sketch_batch.hip): a batch -- or callers that met -- of 2..kSketchBatchMaxQueries queries with limits up
// to 32 shares passes over the int8 sketch, eight queries a pass, where a lone search of the handle would read it and
// the f32 rows reach the batch cut (host/vt_sketchbatch.h holds the gate, the cuts and the planner as plain C++).
// force_sketch = 2 lifts the cut and the query bound (tests); sketch = 2 keeps batches off the sketch.
bool sketch_batch_wanted(const Shard *ix, size_t nq, size_t limit) {
  if (!(sketch_tiers(ix, limit) >> vt_host::kTier8 & 1u)) return false;
  vt_host::SketchBatchShape s;
  s.dot_metric = sketch_dot_metric(ix->metric);
  s.l2_metric = sketch_l2_metric(ix->metric);
  s.strictly_ranked = ix->ranks_clean;
  s.single_nominate = ix->single_nominate;
  s.refused = ix->sketches[vt_host::kTier8].col.refused;
  s.dim = (uint32_t)ix->dim;
  s.row_bytes = (double)ix->n * ix->ld * 4.0;
  s.sketch = vt::env::get(vt::env::SKETCH);
  s.force = vt::env::get(vt::env::FORCE_SKETCH);
  s.column_lacks_xx = ix->sketches[vt_host::kTier8].col.valid && !ix->sketch_xx;
  return vt_host::sketch_batch_gate(s, nq, limit);
}

// ---- what the chains share -----------------------------------------------------------------------------------------------
// max |q_i|, ||q||^2 as an f64 sum in index order, and ||q|| rounded up: these decide certification.
constexpr double kSketchUp = 1.0 + 0x1p-30;
struct SketchQuery {
  float m1;
  double qq, qn;
};
SketchQuery sketch_query(const float *query, uint32_t d) {
  float m1 = 0.0f;
  double qq = 0.0;
  for (uint32_t i = 0; i < d; ++i) {
    m1 = std::max(m1, std::fabs(query[i]));
    qq += (double)query[i] * (double)query[i];
  }
  return {m1, qq, std::sqrt(qq) * kSketchUp};
}

// The int8 pass's scalars for one query, and its image: the query in two int8 levels behind its f32 copy in c.hQ (padded to
// ld), q = t1 Q1 + t2 Q2 + eta.  The integers are chosen with a reciprocal; the residuals r = q - t1 Q1 and eta = r - t2 Q2
// are then formed from the chosen integers in f64 (t Q has at most 31 significant bits: exact), so the bound holds for any
// |Q| <= 127 and only its tightness depends on the rounding.  The lone pass takes the bounds as they are, K1qm's pass as
// slot g of its arrays.
struct SketchBounds {
  float t1, t2;
  double qn, eta, kerr, qq_lo, qq_hi;
};
SketchBounds sketch_query_image(Ctx &c, const float *query, const SketchQuery &sq, uint32_t d, uint32_t ld, uint32_t ld8, bool l2) {
  float *hq = c.hQ.p;
  std::memcpy(hq, query, (size_t)d * sizeof(float));
  for (uint32_t i = d; i < ld; ++i) hq[i] = 0.0f;
  int8_t *q1 = reinterpret_cast<int8_t *>(hq + ld), *q2 = q1 + ld8;
  std::memset(q1 + d, 0, ld8 - d);
  std::memset(q2 + d, 0, ld8 - d);
  float t1 = sq.m1 / 127.0f, t2 = 0.0f;
  if (!(t1 > 0.0f) || !std::isfinite(127.0f / sq.m1)) t1 = 0.0f;
  double *r = c.hSkResid.data();
  constexpr double kRound = 0x1.8p52;  // (v + kRound) - kRound: v to the nearest integer, |v| < 2^51, no library call
  const double t1d = (double)t1, inv1 = t1 > 0.0f ? 1.0 / t1d : 0.0;
  double m2 = 0.0;
  for (uint32_t i = 0; i < d; ++i) {
    const double x = (double)query[i];
    const int v = (int)std::max(-127.0, std::min(127.0, (x * inv1 + kRound) - kRound));
    q1[i] = (int8_t)v;
    r[i] = x - t1d * v;
    m2 = std::max(m2, std::fabs(r[i]));
  }
  t2 = (float)(m2 / 127.0);
  if (!(t2 > 0.0f) || !std::isfinite(127.0 / (double)t2)) t2 = 0.0f;
  const double t2d = (double)t2, inv2 = t2 > 0.0f ? 1.0 / t2d : 0.0;
  double ee = 0.0;  // sum eta_i^2
  for (uint32_t i = 0; i < d; ++i) {
    const int v = (int)std::max(-127.0, std::min(127.0, (r[i] * inv2 + kRound) - kRound));
    q2[i] = (int8_t)v;
    const double e = r[i] - t2d * v;
    ee += e * e;
  }
  // ||eta|| from an f64 sum rounded up.  kerr: K1's summation error per unit of ||q|| ||x_r|| (DESIGN_APPENDIX A.5); the L2
  // family bounds the real dot and carries K1's rounding as a relative term of the distance (A.5b)
  return {t1, t2, sq.qn, std::sqrt(ee) * kSketchUp, l2 ? 0.0 : 8.0 * d * 0x1p-24, sq.qq / kSketchUp, sq.qq * kSketchUp};
}

// K1q's tail over `lists` lists of kp from the int8 pass, for a lone search on `c` (the group chain overrides q, status
// and out: block g takes its own slice).
vt::SketchTailArgs sketch_tail_args(const Shard *ix, Ctx &c, uint32_t lists, uint32_t kp, uint32_t k, uint32_t *info) {
  vt::SketchTailArgs ta{};
  ta.keys = c.dSkKeys.p;
  ta.pay = c.dSkPay.p;
  ta.lists = lists;
  ta.kp = kp;
  ta.k = k;
  ta.cap = vt_host::kSketchTiers[vt_host::kTier8].cand_cap;
  ta.rows = c.dSkRows[vt_host::kTier8].p;
  ta.count = c.dSkCount.p;
  ta.info = info;
  ta.X = ix->dX;
  ta.stride = ix->ld;
  ta.q = c.qsrc;
  ta.id_rank = ix->dRank.p;
  ta.d = (uint32_t)ix->dim;
  ta.metric = ix->metric;
  ta.order = ix->order;
  ta.status = c.dStatus.p;
  ta.out = c.dResMapped;
  return ta;
}

// The gathered K1 over a tier's candidate list (GENERAL, the count read on the device), then its select into the pinned
// result block, and the wait for them.  (c.ensure_part_lists(blocks * k) is the caller's.)
vt::ScanArgs gathered_args(Shard *ix, Ctx &c, const uint32_t *rows, uint32_t cap, uint32_t k) {
  vt::ScanArgs sa = scan_args(ix, c, (uint32_t)ix->dim);
  set_gather(sa, gather_of(rows), cap);  // (the list's room: the count is batch_counts[0])
  sa.k = k;
  use_part_lists(sa, c);
  sa.batch_counts = c.dSkCount.p;
  sa.batch_cap = cap;
  return sa;
}
int rescore_gathered(Shard *ix, Ctx &c, const uint32_t *rows, uint32_t cap, uint32_t blocks, uint32_t k) {
  VT_HIP(vt::launch_scan_batch(gathered_args(ix, c, rows, cap, k), blocks, 1, c.stream));
  VT_HIP(vt::launch_select(c.dPartKeys.p, c.dPartPay.p, blocks * k, k, 0, 0, c.dStatus.p, c.dResMapped, c.dSelKeys.p, c.dSelPay.p,
                           c.stream));
  VT_HIP(hipStreamSynchronize(c.stream));
  return VT_OK;
}

// The end of a lone chain over a tier's column: the pass booked (the tier's own counters and a scan of the rows' sketch);
// not certified: a fallback, and one more miss of the shard's on that tier; certified: the misses start over, the hits in the
// pinned result block are the answer and *done is set.
int sketch_settle(Shard *ix, Ctx &c, int tier, bool certified, bool *done, vt_hits **out) {
  const SketchKind &kind = sketch_kind(tier);
  std::atomic<uint32_t> &misses = ix->sketches[tier].misses;  // (the int8 tier's are counted and never read: it has no limit)
  if (c.profiling) {
    float ms = 0.f;
    VT_TRY(c.span_ms(&ms));
    const uint64_t bytes = (uint64_t)kind.bytes(ix->n, (uint32_t)ix->dim);
    c.prof.*kind.launches += 1;
    c.prof.*kind.ms += ms;
    c.prof.*kind.bytes_read += bytes;
    c.prof.*kind.candidates += c.hSkInfo.p[1];
    VT_TRY(c.book_scan(1, ix->n, bytes));
  }
  if (!certified) {
    c.prof.*kind.fallbacks += 1;
    misses.fetch_add(1, std::memory_order_relaxed);
    return VT_OK;
  }
  misses.store(0, std::memory_order_relaxed);
  std::vector<vt::Entry> entries(c.hRes.p->e, c.hRes.p->e + c.hRes.p->count);
  VT_TRY(make_hits(ix, entries, out));
  *done = true;
  return VT_OK;
}

// Room for a lone pass's lists (`slots` entries) and the tier's candidate list; *info: the status words the chain's kernels
// write through the host mapping.
int sketch_lists_ensure(Ctx &c, int tier, size_t slots, uint32_t **info) {
  VT_TRY(c.dSkKeys.ensure(slots));
  VT_TRY(c.dSkPay.ensure(slots));
  VT_TRY(c.dSkRows[tier].ensure(vt_host::kSketchTiers[tier].cand_cap));
  VT_TRY(c.dSkCount.ensure(1));
  VT_TRY(c.hSkInfo.ensure(4));
  *info = c.hSkInfo.mapped();
  return *info ? VT_OK : fail(VT_ERR_DEVICE, "hipHostGetDevicePointer (sketch status)");
}

// ---- K1q -----------------------------------------------------------------------------------------------------------------
// K1q and its tail, one host wait: the pass, then one block that certifies and -- the usual case, a few
// dozen candidates -- rescores them with K1's arithmetic and fills the pinned result block.  A candidate list too long
// for that block (up to the tier's cand_cap) goes through the gathered K1 and its select after a second wait.  *done: the
// hits in *out are the exact top `limit`; otherwise the caller scans the f32 rows -- the bound could not certify
// (counted), or it declined before any launch because a dot of these rows could reach the f32 overflow K1 must see for
// itself.  The L2 family: the same chain over the column with xx (the pass's L2 epilogue, kerr = 0, ||q||^2 between its two
// ends), declined where a squared difference could overflow f32.
int sketch_search(Shard *ix, Ctx &c, const float *query, size_t limit, bool *done, vt_hits **out) {
  *done = false;
  const vt_host::SketchTierRow &row = vt_host::kSketchTiers[vt_host::kTier8];
  const SketchTier &st = ix->sketches[vt_host::kTier8];
  const uint32_t d = (uint32_t)ix->dim, ld = ix->ld, ld8 = vt::sketch_ld8(d), nch = ld8 / 16;
  const SketchQuery sq = sketch_query(query, d);
  const bool l2 = sketch_l2_metric(ix->metric);
  // (L2: ||q - x|| <= ||q|| + ||x||: below 2^62 no square of K1's can overflow; at or past it the plain scan recomputes in
  // f64 or reports "metric overflow" for itself.  A column built without xx never serves the family.  Dot: K1's overflow
  // flag depends on every row: its scan decides.)
  if (l2 && !ix->sketch_xx) return VT_OK;
  if (!vt_host::sketch_batch_query_fits(l2, sq.qn, st.max_norm)) return VT_OK;
  const size_t total = (size_t)ld + 2 * (size_t)ld8 / 4;
  VT_TRY(c.dQ.ensure(total));
  VT_TRY(c.hQ.ensure(total));
  if (c.hSkResid.size() < d) c.hSkResid.resize(d);
  const SketchBounds b = sketch_query_image(c, query, sq, d, ld, ld8, l2);
  c.qbits_kind = 0;
  c.qsrc = c.dQ.p;
  VT_HIP(hipMemcpyAsync(c.dQ.p, c.hQ.p, total * sizeof(float), hipMemcpyHostToDevice, c.stream));

  const uint32_t kp = sketch_list_k(limit), k = (uint32_t)limit;
  const uint32_t blocks = (uint32_t)c.num_cus * (kp <= (uint32_t)vt::kSmallK ? 4u : 2u);
  uint32_t *info = nullptr;
  VT_TRY(sketch_lists_ensure(c, vt_host::kTier8, (size_t)blocks * kp, &info));
  vt::SketchScanArgs a{};
  a.img = st.col.buf.p;
  a.id_rank = ix->dRank.p;
  a.qimg = reinterpret_cast<const int8_t *>(c.dQ.p + ld);
  a.n = ix->n;
  a.d = d;
  a.nch = nch;
  a.metric = ix->metric;
  a.t1 = b.t1;
  a.t2 = b.t2;
  a.qn = b.qn;
  a.eta = b.eta;
  a.kerr = b.kerr;
  a.qq_lo = b.qq_lo;
  a.qq_hi = b.qq_hi;
  a.k = kp;
  a.part_keys = c.dSkKeys.p;
  a.part_pay = c.dSkPay.p;
  VT_TRY(c.mark_begin());
  VT_HIP(vt::launch_sketch_scan(a, blocks, c.stream));
  VT_TRY(c.mark_end());
  VT_HIP(vt::launch_sketch_tail(sketch_tail_args(ix, c, blocks, kp, k, info), c.stream));
  VT_HIP(hipStreamSynchronize(c.stream));
  if (c.hSkInfo.p[0] == 2u) {
    // more candidates than the tail's block takes: K1 itself, then its select
    VT_TRY(c.ensure_part_lists((size_t)row.rescore_blocks * k));
    VT_TRY(rescore_gathered(ix, c, c.dSkRows[vt_host::kTier8].p, row.cand_cap, row.rescore_blocks, k));
  }
  if (c.profiling) c.prof.sketch_tail_rescored += c.hSkInfo.p[0] == 1u ? 1 : 0;
  return sketch_settle(ix, c, vt_host::kTier8, c.hSkInfo.p[0] != 0u && c.hRes.p->status == 0, done, out);
}

// ---- K1qm ----------------------------------------------------------------------------------------------------------------
// K1qm, one host wait: the queries `which` (2..8 rows of `queries`, none of which sketch_batch_query_fits
// turned away; sq[i]: query i's norms) in ONE pass over the int8 sketch, then one launch of K1q's tail with a block per
// query -- blit, pass, tail, wait, as a lone K1q search.  Each query's levels, bounds and lists are the ones sketch_search
// would form for it, so a query whose block certified and rescored (outcome 1) gets flat_search's hits and
// done[which[g]] = 1.  A query whose candidate list is too long for the block (outcome 2), or not certified (0), or whose
// rescoring raised K1's overflow flag, stays unanswered for what batch_ready does with left-over queries, and counts as a
// fallback: no second chain here.
int sketch_group_search(Shard *ix, Ctx &c, const float *queries, const std::vector<SketchQuery> &sq, const std::vector<size_t> &which,
                        size_t limit, vt_hits **out, std::vector<char> &done) {
  const uint32_t ng = (uint32_t)which.size();
  const uint32_t d = (uint32_t)ix->dim, ld = ix->ld, ld8 = vt::sketch_ld8(d), nch = ld8 / 16;
  const uint32_t kp = sketch_list_k(limit), k = (uint32_t)limit;
  const uint32_t group = vt::sketch_scan_multi_group(ng);
  const size_t lds = vt::sketch_scan_multi_lds_bytes(d, kp, group);
  if (ng < 2 || ng > (uint32_t)vt::kSketchMultiMax || !lds) return fail(VT_ERR_DEVICE, "internal: a sketch group the pass does not take");
  const bool l2 = sketch_l2_metric(ix->metric);
  const uint32_t cand_cap = vt_host::kSketchTiers[vt_host::kTier8].cand_cap;
  // one upload: the ng f32 queries (the tail's), then `group` images of two levels (the pass's; the places past ng zero)
  const size_t img_floats = 2 * (size_t)ld8 / 4;
  const size_t total = (size_t)ng * ld + (size_t)group * img_floats;
  VT_TRY(c.dBQ.ensure(total));
  VT_TRY(c.hBQ.ensure(total));
  VT_TRY(c.hQ.ensure((size_t)ld + img_floats));
  if (c.hSkResid.size() < d) c.hSkResid.resize(d);
  vt::SketchScanMultiArgs a{};
  for (uint32_t g = 0; g < ng; ++g) {
    const SketchBounds b = sketch_query_image(c, queries + which[g] * d, sq[which[g]], d, ld, ld8, l2);
    std::memcpy(c.hBQ.p + (size_t)g * ld, c.hQ.p, (size_t)ld * sizeof(float));
    std::memcpy(c.hBQ.p + (size_t)ng * ld + (size_t)g * img_floats, c.hQ.p + ld, img_floats * sizeof(float));
    a.t1[g] = b.t1;
    a.t2[g] = b.t2;
    a.qn[g] = b.qn;
    a.eta[g] = b.eta;
    a.kerr[g] = b.kerr;
    a.qq_lo[g] = b.qq_lo;
    a.qq_hi[g] = b.qq_hi;
  }
  if (group > ng) std::memset(c.hBQ.p + (size_t)ng * ld + (size_t)ng * img_floats, 0, (size_t)(group - ng) * img_floats * sizeof(float));
  c.qbits_kind = 0;  // (c.hQ no longer holds the query last uploaded)
  VT_HIP(hipMemcpyAsync(c.dBQ.p, c.hBQ.p, total * sizeof(float), hipMemcpyHostToDevice, c.stream));

  // (two to four blocks a CU, as many as its LDS holds of them: K1q's grid where the group is small)
  const uint32_t per_cu = (uint32_t)std::min<size_t>(4, (160 * 1024) / (lds + vt_host::kSketchBatchLdsStatic));
  const uint32_t blocks = (uint32_t)c.num_cus * std::max(1u, per_cu);
  VT_TRY(c.dSkKeys.ensure((size_t)ng * blocks * kp));
  VT_TRY(c.dSkPay.ensure((size_t)ng * blocks * kp));
  VT_TRY(c.dSkRows[vt_host::kTier8].ensure((size_t)vt::kSketchMultiMax * cand_cap));
  VT_TRY(c.dSkCount.ensure(vt::kSketchMultiMax));
  VT_TRY(c.hSkInfo.ensure(4 * vt::kSketchMultiMax));
  VT_TRY(c.hSkgRes.ensure(vt::kSketchMultiMax));
  if (c.dSkgStatus.count < (size_t)vt::kSketchMultiMax) {
    VT_TRY(c.dSkgStatus.ensure(vt::kSketchMultiMax));
    VT_HIP(hipMemsetAsync(c.dSkgStatus.p, 0, vt::kSketchMultiMax * sizeof(int), c.stream));
  }
  uint32_t *info = c.hSkInfo.mapped();
  vt::ResultBlock *res = c.hSkgRes.mapped();
  if (!info || !res) return fail(VT_ERR_DEVICE, "hipHostGetDevicePointer (sketch group status)");
  a.img = ix->sketches[vt_host::kTier8].col.buf.p;
  a.id_rank = ix->dRank.p;
  a.qimg = reinterpret_cast<const int8_t *>(c.dBQ.p + (size_t)ng * ld);
  a.n = ix->n;
  a.d = d;
  a.nch = nch;
  a.ng = ng;
  a.metric = ix->metric;
  a.k = kp;
  a.part_keys = c.dSkKeys.p;
  a.part_pay = c.dSkPay.p;
  VT_TRY(c.mark_begin());
  VT_HIP(vt::launch_sketch_scan_multi(a, blocks, c.stream));
  VT_TRY(c.mark_end());
  vt::SketchTailArgs ta = sketch_tail_args(ix, c, blocks, kp, k, info);  // (query 0's: block g takes its own slice)
  ta.q = c.dBQ.p;
  ta.status = c.dSkgStatus.p;
  ta.out = res;
  VT_HIP(vt::launch_sketch_tail_group(ta, ng, ld, c.stream));
  VT_HIP(hipStreamSynchronize(c.stream));
  if (c.profiling) {
    float ms = 0.f;
    VT_TRY(c.span_ms(&ms));
    c.prof.sketch_batch_launches += 1;
    c.prof.sketch_batch_queries += ng;
    c.prof.sketch_batch_ms += ms;
    c.prof.sketch_batch_bytes += (uint64_t)vt::sketch_bytes(ix->n, d);
    VT_TRY(c.book_scan(1, ix->n, (uint64_t)vt::sketch_bytes(ix->n, d)));  // (a pass over the rows' sketch: a scan, as K1q's counts)
  }
  for (uint32_t g = 0; g < ng; ++g) {
    const uint32_t *gi = c.hSkInfo.p + 4 * g;
    const vt::ResultBlock &rb = c.hSkgRes.p[g];
    if (c.profiling) c.prof.sketch_batch_candidates += gi[1];
    if (gi[0] != 1u || rb.status != 0) {
      if (c.profiling) c.prof.sketch_batch_fallbacks += 1;
      continue;
    }
    if (c.profiling) c.prof.sketch_batch_tail_rescored += 1;
    std::vector<vt::Entry> entries(rb.e, rb.e + std::min<uint32_t>(rb.count, k));
    VT_TRY(make_hits(ix, entries, &out[which[g]]));
    done[which[g]] = 1;
  }
  return VT_OK;
}

// ---- K1s, K1f, K1n -------------------------------------------------------------------------------------------------------
// The query's signed-nibble levels behind its f32 copy, uploaded in one blit, and what the pass takes from them: *a's
// qimg, t, qn, eta, kerr and the bound of the last level, which stays off the L plane -- its share there is c3 -+ w3 per
// unit of s_r (none where the tier has one plane).  `chain_zeros` (K1n): zero words ride behind the image in the same blit
// -- the filtered K1's count, overflow and ticket words (4 KiB: a line per ticket; *chain_words, ScanArgs::fsync) start
// every call from zero whatever the last one did, at no launch's cost.
int nibble_query_upload(Ctx &c, const SketchKind &kind, const float *query, const SketchQuery &sq, uint32_t d, uint32_t ld,
                        bool chain_zeros, vt::Sketch6ScanArgs *a, uint32_t **chain_words) {
  const uint32_t lw = vt_host::sketch6_level_words(d);
  const size_t qwords = (size_t)ld + (size_t)vt::kSketch6Levels * lw;
  const size_t total = qwords + (chain_zeros ? vt::kScanFilterSyncWords : 0);
  VT_TRY(c.dQ.ensure(total));
  VT_TRY(c.hQ.ensure(total));
  if (c.hSkResid.size() < d) c.hSkResid.resize(d);
  float *hq = c.hQ.p;
  std::memcpy(hq, query, (size_t)d * sizeof(float));
  for (uint32_t i = d; i < ld; ++i) hq[i] = 0.0f;
  uint32_t *levels = reinterpret_cast<uint32_t *>(hq + ld);
  double ee = 0.0;
  vt_host::sketch6_query_levels(query, d, levels, c.hSkResid.data(), a->t, &ee);
  if (kind.level_bound) kind.level_bound(levels + (size_t)(vt::kSketch6Levels - 1) * lw, lw, a->t[vt::kSketch6Levels - 1], &a->c3, &a->w3);
  a->qimg = reinterpret_cast<const uint32_t *>(c.dQ.p + ld);
  a->qn = sq.qn;
  a->eta = std::sqrt(ee) * kSketchUp;
  a->kerr = 8.0 * d * 0x1p-24;  // K1's summation error per unit of ||q|| ||x_r|| (DESIGN_APPENDIX A.5)
  if (chain_zeros) std::memset(hq + qwords, 0, vt::kScanFilterSyncWords * sizeof(float));
  *chain_words = reinterpret_cast<uint32_t *>(c.dQ.p + qwords);
  c.qbits_kind = 0;
  c.qsrc = c.dQ.p;
  VT_HIP(hipMemcpyAsync(c.dQ.p, c.hQ.p, total * sizeof(float), hipMemcpyHostToDevice, c.stream));
  return VT_OK;
}

// What the threshold and collect kernels take over the `lists` lists a nibble pass left on `c`.
vt::SketchSpreadArgs nibble_spread_args(Ctx &c, int tier, uint32_t lists, uint32_t k, uint32_t *info) {
  const uint32_t kp = vt_host::kSketchNibbleListK, thresh_blocks = vt::sketch_thresh_blocks(lists, kp);
  vt::SketchSpreadArgs ta{};
  ta.lo_words = c.dSkLoWords.p;
  ta.hi_words = c.dSkHiWords.p;
  ta.pay = c.dSkPay.p;
  ta.lists = lists;
  ta.kp = kp;
  ta.k = k;
  ta.cap = vt_host::kSketchTiers[tier].cand_cap;
  ta.parts = c.dSkParts.p;
  ta.live = c.dSkParts.p + (size_t)thresh_blocks * k;
  ta.sync = c.dSkSync.p;
  ta.rows = c.dSkRows[tier].p;
  ta.count = c.dSkCount.p;
  ta.info = info;
  return ta;
}

// The certification spread over the card: the threshold kernel over the pass's lists and, where the tier takes its
// threshold from exact keys (K1n), launch_sketch_refine behind it.  *ta: what the collect kernel takes, kt_word set where
// the refine ran.
int nibble_threshold(Shard *ix, Ctx &c, int tier, uint32_t lists, uint32_t k, uint32_t *info, vt::SketchSpreadArgs *ta_out) {
  const vt_host::SketchTierRow &row = vt_host::kSketchTiers[tier];
  vt::SketchSpreadArgs ta = nibble_spread_args(c, tier, lists, k, info);
  const uint32_t thresh_blocks = vt::sketch_thresh_blocks(lists, ta.kp);
  if (row.exact_threshold) ta.slots = ta.live + thresh_blocks;
  VT_HIP(vt::launch_sketch_thresh(ta, c.stream));
  if (row.exact_threshold) {
    vt::SketchRefineArgs ra{};
    ra.parts = ta.parts;
    ra.slots = ta.slots;
    ra.live = ta.live;
    ra.thresh_blocks = thresh_blocks;
    ra.k = k;
    ra.pay = c.dSkPay.p;
    ra.slots_total = lists * ta.kp;
    ra.X = ix->dX;
    ra.stride = ix->ld;
    ra.q = c.qsrc;
    ra.d = (uint32_t)ix->dim;
    ra.metric = ix->metric;
    ra.order = ix->order;
    ra.kt_out = ta.slots + (size_t)thresh_blocks * k;
    VT_HIP(vt::launch_sketch_refine(ra, c.stream));
    ta.kt_word = ra.kt_out;
  }
  *ta_out = ta;
  return VT_OK;
}

// Whether launch_sketch4_rescore takes the shard's rows: K1n's candidates are then rescored straight from the pass's lists.
bool nibble_from_lists(const Shard *ix, uint32_t k, uint32_t kp) {
  return sketch_dot_metric(ix->metric) && k <= (uint32_t)vt::kSmallK && vt::sketch4_rescore_lds_bytes((uint32_t)ix->dim, kp) != 0;
}

// Whether K1n takes its exact threshold from each list's best rows, rescored inside the pass: blit, pass,
// rescore, wait -- no threshold and no refine launch.  The tier says so, the rescoring kernel takes the rows and the words
// (two a list, a select of k <= kSketch4BestMaxK over at most kSketch4BestMaxWords in every block's head), the rows' chunk
// sums fit the pass's wave buffers, a list's slots number at most the storing wave's 64 lanes, and every wave of the pass
// owns a tile, so that the lists have rows to rescore.  Smaller corpora keep the chain they had, launch for launch.
bool nibble_best_rows(const Shard *ix, int tier, uint32_t k, uint32_t kp, uint32_t blocks, uint32_t lists) {
  const uint32_t ntiles = (ix->n + vt::kSketchTileRows - 1) / vt::kSketchTileRows;
  return vt_host::kSketchTiers[tier].best_rows && nibble_from_lists(ix, k, kp) && k <= vt::kSketch4BestMaxK &&
         (size_t)lists * vt::kSketch4BestRows <= vt::kSketch4BestMaxWords && kp <= 64u &&
         vt::padded_dim((uint32_t)ix->dim) / 8 + 12 <= vt::kSketch4BestRowFloats && ntiles >= blocks * (uint32_t)vt::kWavesPerBlock;
}

// K1n's finish behind the exact threshold, and its one host wait: the rows whose rank word is <= Kt' are kept -- the k hits
// and what ties the k-th -- and the last block sorts them into the result block: no lists, no select (the survivors lie
// where the lists would).  Wherever its launcher takes the shape the candidates are rescored straight from the pass's lists
// by one kernel (launch_sketch4_rescore) that certifies as the collect does and finishes as the filtered K1 does, no
// candidate array (*from_lists); otherwise the collect with that threshold and the gathered K1 in filter mode.
// best_words (nibble_best_rows said yes, the pass left them: best_count words): the rescoring kernel takes its threshold from
// them in its head and publishes it in *ta.kt_word, which no launch has written -- nothing ran between the pass and it.
int nibble_finish_exact(Shard *ix, Ctx &c, int tier, const vt::SketchSpreadArgs &ta, uint32_t *chain_words, uint32_t blocks,
                        const uint32_t *best_words, uint32_t best_count, bool *from_lists, bool *delivered) {
  const vt_host::SketchTierRow &row = vt_host::kSketchTiers[tier];
  *from_lists = ta.kt_word && nibble_from_lists(ix, ta.k, ta.kp);
  if (best_words && !*from_lists) return fail(VT_ERR_DEVICE, "internal: best rows without the rescoring kernel");
  if (!*from_lists) VT_HIP(vt::launch_sketch_collect(ta, c.stream));
  vt::ScanArgs fa = gathered_args(ix, c, ta.rows, row.cand_cap, ta.k);
  fa.hi_word = ta.kt_word;
  fa.surv_keys = c.dPartKeys.p;
  fa.surv_pay = c.dPartPay.p;
  fa.surv_cap = vt::kScanFilterCap;
  fa.fsync = chain_words;
  fa.out = c.dResMapped;
  fa.info = ta.info;
  if (*from_lists) {
    vt::Sketch4RescoreArgs ra{};
    ra.s = fa;
    ra.s.gather = nullptr;
    ra.s.batch_counts = nullptr;
    ra.hi_words = ta.hi_words;
    ra.pay = ta.pay;
    ra.kp = ta.kp;
    ra.cap = row.cand_cap;
    if (best_words) {
      ra.s.hi_word = nullptr;
      ra.best_words = best_words;
      ra.best_count = best_count;
      ra.kt_out = const_cast<uint32_t *>(ta.kt_word);
    }
    VT_HIP(vt::launch_sketch4_rescore(ra, blocks, c.stream));
  } else {
    VT_HIP(vt::launch_scan_filter(fa, row.rescore_blocks, c.stream));
  }
  VT_HIP(hipStreamSynchronize(c.stream));
  *delivered = c.hSkInfo.p[0] == vt::kScanFilterDelivered;
  return VT_OK;
}

// K1s, K1f or K1n by `tier`, one host wait: blit, the tier's pass, the certification spread over the card (the threshold
// kernel, the collect kernel), the gathered K1 over the candidate rows they left (the count read on the device: none when
// the pass did not certify) and K1's select, all queued before the wait.  K1n ends behind its exact threshold instead
// (nibble_finish_exact); a search of its whose survivors overflow the short list queues the collect, the lists and the
// select behind a second wait.  Where nibble_best_rows says so K1n's chain is blit, pass, rescore, wait: the pass leaves
// the exact keys of each list's two best rows and the rescoring kernel takes its threshold from them (sketch4_best counts
// these searches).
// *done as sketch_search has it; a pass that does not certify counts towards the shard's miss limit.
int nibble_search(Shard *ix, Ctx &c, const float *query, size_t limit, bool *done, vt_hits **out, int tier) {
  const SketchKind &kind = sketch_kind(tier);
  const vt_host::SketchTierRow &row = vt_host::kSketchTiers[tier];
  SketchTier &st = ix->sketches[tier];
  *done = false;
  const uint32_t d = (uint32_t)ix->dim;
  const SketchQuery sq = sketch_query(query, d);
  if (!vt_host::sketch_batch_query_fits(false, sq.qn, st.max_norm)) return VT_OK;  // (K1's overflow flag depends on every row: its scan decides)
  vt::Sketch6ScanArgs a{};
  uint32_t *chain_words = nullptr, *info = nullptr;
  VT_TRY(nibble_query_upload(c, kind, query, sq, d, ix->ld, row.exact_threshold, &a, &chain_words));

  const uint32_t kp = vt_host::kSketchNibbleListK, k = (uint32_t)limit;
  const uint32_t blocks = (uint32_t)c.num_cus * 4u, lists = blocks * row.block_lists;
  VT_TRY(sketch_lists_ensure(c, tier, (size_t)lists * kp, &info));
  VT_TRY(c.dSkLoWords.ensure((size_t)lists * kp));
  VT_TRY(c.dSkHiWords.ensure((size_t)lists * kp));
  // (parts[thresh_blocks][k] | live[thresh_blocks] | K1n: slots[thresh_blocks][k] | the exact threshold's word)
  // (K1n from its lists' best rows: best_words[lists][2] | the threshold's word, in the same room)
  const bool best = nibble_best_rows(ix, tier, k, kp, blocks, lists);
  const size_t best_count = (size_t)lists * vt::kSketch4BestRows;
  VT_TRY(c.dSkParts.ensure(std::max((size_t)vt::sketch_thresh_blocks(lists, kp) * (2 * k + 1) + 1, best_count + 1)));
  VT_TRY(c.dSkSync.ensure(4));
  VT_TRY(c.ensure_part_lists(std::max<size_t>((size_t)row.rescore_blocks * k, vt::kScanFilterCap)));  // (K1n: the survivors lie there)
  a.img = st.col.buf.p;
  a.id_rank = ix->dRank.p;
  a.n = ix->n;
  a.d = d;
  a.ld8 = vt::sketch_ld8(d);
  a.metric = ix->metric;
  a.k = kp;
  a.part_keys = c.dSkKeys.p;
  a.part_pay = c.dSkPay.p;
  a.lo_words = c.dSkLoWords.p;
  a.hi_words = c.dSkHiWords.p;
  if (best) {
    a.best_words = c.dSkParts.p;
    a.X = ix->dX;
    a.stride = ix->ld;
    a.q = c.qsrc;  // (the blit in front of the pass carries it)
    a.order = ix->order;
  }
  VT_TRY(c.mark_begin());
  VT_HIP(kind.scan(a, blocks, c.stream));
  VT_TRY(c.mark_end());
  vt::SketchSpreadArgs ta{};
  if (best) {
    ta = nibble_spread_args(c, tier, lists, k, info);
    ta.kt_word = c.dSkParts.p + best_count;  // (the rescoring kernel's block 0 writes it)
  } else {
    VT_TRY(nibble_threshold(ix, c, tier, lists, k, info, &ta));
  }
  bool from_lists = false, delivered = false;
  if (row.exact_threshold)
    VT_TRY(nibble_finish_exact(ix, c, tier, ta, chain_words, blocks, best ? c.dSkParts.p : nullptr, (uint32_t)best_count, &from_lists, &delivered));
  else VT_HIP(vt::launch_sketch_collect(ta, c.stream));
  if (!delivered && (!row.exact_threshold || c.hSkInfo.p[0] == 2u)) {
    // (K1n, certified but not delivered -- more survivors than the short list holds: thousands of rows tie the k-th key,
    // or the refine kept the sketch's own Kt: the lists and their select over the candidates, behind a second wait.  The
    // rescoring kernel left no candidate array: the collect, over the lists still on the device, goes first -- with the
    // word that kernel published where the best rows gave it, and its three shared words zeroed here, where no threshold
    // kernel ran to zero them.  Not a fallback.)
    if (best) VT_HIP(hipMemsetAsync(c.dSkSync.p, 0, 4 * sizeof(uint32_t), c.stream));
    if (from_lists) VT_HIP(vt::launch_sketch_collect(ta, c.stream));
    VT_TRY(rescore_gathered(ix, c, ta.rows, row.cand_cap, row.rescore_blocks, k));
  }
  const bool certified = (delivered || c.hSkInfo.p[0] == 2u) && c.hRes.p->status == 0;
  if (best) c.prof.sketch4_best += 1;
  if (delivered && certified) c.prof.sketch4_finished += 1;
  if (c.profiling && kind.tail_words) c.prof.*kind.tail_words += c.hSkInfo.p[3] == 1u ? 1 : 0;
  return sketch_settle(ix, c, tier, certified, done, out);
}

// A lone search through the sketches (flat_search; the single searches a batch leaves over do not come here): the tiers it
// wants whose column is current, the narrowest first -- K1n, then K1f, then K1s, then K1q: a tier that is not taken or
// does not certify leaves it to the next.  *done false: the caller scans the f32 rows.
int sketch_lone_search(Shard *ix, Ctx &c, const float *query, size_t limit, bool *done, vt_hits **out) {
  *done = false;
  const unsigned tiers = sketch_tiers(ix, limit);
  for (int t = 0; t < vt_host::kSketchTierCount && !*done; ++t) {
    const uint32_t miss_limit = vt_host::kSketchTiers[t].miss_limit;
    SketchTier &st = ix->sketches[t];
    if (!(tiers >> t & 1u) || !st.col.current(sketch_kind(t).elems(ix))) continue;
    if (miss_limit && st.misses.load(std::memory_order_relaxed) >= miss_limit) continue;
    if (t == vt_host::kTier8) VT_TRY(sketch_search(ix, c, query, limit, done, out));
    else VT_TRY(nibble_search(ix, c, query, limit, done, out, t));
  }
  return VT_OK;
}

// A tier's column brought up to date (exclusive access; primary context), on the shadow's terms: the rows mutated since
// its last use are re-quantised in place; a first use, a slab that outgrew it or more than kMaxDerivedDirty mutations
// rebuild it (one pass over the rows); without room for it -- a quarter of the card must stay free -- it is refused and
// lone searches go on to the next tier, the last to the f32 rows.  The bound on every row's norm comes back with it (the
// overflow guard); a whole build starts its misses over.  The int8 column of an L2 / squared-L2 handle is built and patched
// with xx_r in the metadata run's fourth dword (Shard::sketch_xx); every other column's image is what it was.
int index_ensure_sketch(Shard *ix, size_t bytes, int tier) {
  Ctx &c = ix->ctx;
  const SketchKind &kind = sketch_kind(tier);
  SketchTier &st = ix->sketches[tier];
  DerivedColumn<unsigned char> &col = st.col;
  if (col.current(bytes)) return VT_OK;
  const uint32_t d = (uint32_t)ix->dim;
  const size_t tile_bytes = kind.bytes(vt::kSketchTileRows, d);
  VT_TRY(c.dBNorm.ensure(1));
  unsigned long long bits = 0;
  if (col.patchable(bytes)) {
    const bool with_xx = kind.rows_xx && ix->sketch_xx;  // (the patch writes what the build wrote)
    uint32_t count = 0;
    VT_TRY(upload_row_list(ix, col.dirty, &count));
    std::memcpy(&bits, &st.max_norm, sizeof(double));
    VT_HIP(hipMemcpyAsync(c.dBNorm.p, &bits, sizeof(bits), hipMemcpyHostToDevice, c.stream));
    const uint32_t rows_img = (uint32_t)(col.buf.count / tile_bytes * vt::kSketchTileRows);
    VT_HIP((with_xx ? kind.rows_xx : kind.rows)(ix->dX, ix->ld, c.dRankPairs.p, count, rows_img, d, col.buf.p, c.dBNorm.p, c.stream));
    c.prof.*kind.patched_rows += count;
  } else {
    col.forget();
    if (col.buf.count < bytes) {
      col.buf.release();
      size_t free_b = 0, total_b = 0;
      VT_HIP(hipMemGetInfo(&free_b, &total_b));
      bool refused = free_b < bytes || free_b - bytes < total_b / 4;
      // (geometric head room, as the shadow keeps: a corpus that arrives in appends would otherwise rebuild at every growth)
      size_t want = bytes;
      if (!refused) {
        const size_t roomy = (bytes + bytes / 4 + tile_bytes - 1) / tile_bytes * tile_bytes;
        if (free_b >= roomy && free_b - roomy >= total_b / 4) want = roomy;
        refused = col.buf.ensure(want) != VT_OK;
      }
#ifdef VT_TEST_HOOKS
      // (libvettore_hip_hooks.so only: the allocation "fails", tests/test_gpu_sketch.py checks what follows)
      refused = refused || vt::env::on(kind.refuse_hook);
#endif
      if (refused) {
        col.refuse();
        return VT_OK;
      }
    }
    const uint32_t rows_img = (uint32_t)(bytes / tile_bytes * vt::kSketchTileRows);
    VT_HIP(hipMemsetAsync(c.dBNorm.p, 0, sizeof(unsigned long long), c.stream));
    if (kind.build_xx) ix->sketch_xx = sketch_l2_metric(ix->metric);  // (a handle's metric never changes: fixed with the column)
    const bool with_xx = kind.build_xx && ix->sketch_xx;
    VT_HIP((with_xx ? kind.build_xx : kind.build)(ix->dX, ix->ld, ix->n, rows_img, d, col.buf.p, c.dBNorm.p, c.stream));
    c.prof.*kind.builds += 1;
    st.misses.store(0, std::memory_order_relaxed);
  }
  VT_HIP(hipMemcpyAsync(&bits, c.dBNorm.p, sizeof(bits), hipMemcpyDeviceToHost, c.stream));
  // current from here on, for readers on other streams too: the build has finished before the exclusive lock can drop
  VT_HIP(hipStreamSynchronize(c.stream));
  std::memcpy(&st.max_norm, &bits, sizeof(double));
  col.mark_current();
  return VT_OK;
}

}  // namespace
