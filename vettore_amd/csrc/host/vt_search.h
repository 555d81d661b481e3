// vt_search.h -- what a reader needs current, flat search on a shard, the f64 cosine scan, funnel stages, sign bits, norms.
// Part of vt_index.cpp's translation unit (included there, in this order, exactly once): the host
// side is one TU on purpose -- everything below the C ABI lives in an anonymous namespace.
#pragma once

namespace {

// ---- what a reader needs up to date before it may run under the shared lock ----------
enum : unsigned { NEED_RANKS = 1, NEED_STRICT_RANKS = 2, NEED_BITS = 4, NEED_NORMS = 8, NEED_NZBITS = 16, NEED_SKETCH = 32, NEED_SKETCH8 = 64 };
// Internal: only the true id order can decide (a tie at the boundary of a lazy search).
constexpr int kEscalate = -101;

// Ids inserted out of order since the last ranking keep one shared sentinel rank; a search
// that wants `limit` hits may run on that column if it can ask for one hit more (see
// search_ready).  Past ~1/8 of the rows unranked the eventual rebuild would have to sort
// too many ids at once: rebuild now, while it is still cheap.
bool lazy_ranks_ok(const Shard *ix, size_t limit) {
  const size_t lazy_want = std::min<size_t>(limit, ix->n) + (limit < ix->n ? 1 : 0);
  // (one select pass only: very wide rows leave LDS for the small candidate buffer alone)
  const size_t kmax = vt::scan_lds_bytes((uint32_t)ix->dim, vt::kMaxFusedK) ? (size_t)vt::kMaxFusedK : (size_t)vt::kSmallK;
  return !ix->ranks_clean && !ix->external_ranks && lazy_want <= kmax &&
         ix->unranked <= std::max<size_t>(65536, ix->n / 8);
}

// Float hamming and jaccard compare which coordinates are non-zero and nothing else
// (distances.rs:319-347), so on a collection under one of them flat_search is K4 over a column of
// non-zero bits -- d / 8 bytes per row instead of 4 d, the same integers, the same f32 score, the
// same keys -- once the corpus is big enough for the column to pay for its upkeep and as long as
// the hits fit a few K4 passes (K1's one-pass threshold path serves the larger limits).
// NEED_NZBITS asks for that column and means nothing where this says no.
constexpr size_t kPatternMinRows = 16384, kPatternMaxWant = 8 * (size_t)vt::kMaxFusedK;
bool pattern_metric(int metric) {
  return metric == VT_HAMMING || metric == VT_JACCARD;
}
bool pattern_search_applies(const Shard *ix, size_t limit) {
  return pattern_metric(ix->metric) && !ix->nz_bits.refused && ix->n >= kPatternMinRows &&
         std::min<size_t>(limit, ix->n) + 1 <= kPatternMaxWant;
}

// The bf16 shadow of the rows (K2s, vt_batch_shadow.hip) travels with NEED_NORMS: both are what a
// matrix-core batch wants current, and nothing else reads either.
bool shadow_metric(int metric) {
  return metric == VT_COSINE || metric == VT_INNER_PRODUCT || metric == VT_NEG_INNER_PRODUCT || metric == VT_L2 ||
         metric == VT_L2_SQUARED;
}
bool shadow_wanted(const Shard *ix) {
  return ix->shadow_mode == VT_SHADOW_AUTO && !ix->shadow.refused && ix->nominate == VT_NOMINATE_BF16 && shadow_metric(ix->metric) &&
         ix->n > 0 && ix->dim > 0;
}
size_t shadow_elems(const Shard *ix) { return vt::shadow_elems((uint32_t)std::max<size_t>(ix->cap, ix->n), ix->ld); }
bool shadow_current(const Shard *ix) { return ix->shadow.current(shadow_elems(ix)); }

// K1q (vt_sketch.hip): a lone cosine / inner-product / L2 search over rows of at least kSketchMinBytes reads the
// int8 sketch -- a quarter of the bytes -- and the exact K1 rescores the rows it cannot rule out.  Only on strictly
// ranked shards (lazy searches after trickle inserts keep K1), and only while each block's list of k' = max(2k, k + 16)
// fits one wave buffer.  NEED_SKETCH asks for the column and means nothing where this says no.
// f32 rows below this take K1.  (With the pass's tail in one kernel the two paths meet near 130 MB of f32 rows, DESIGN 5;
// the cut stays where the suite's launch counters on mid-size corpora were written against it.)
constexpr double kSketchMinBytes = 256.0 * (1 << 20);
// The L2 family's own cut.  The family has been measured at 5 M and 10 M rows of d = 768 and in a sweep down to 256 MB
// (DESIGN 5); the cut does not sit at the measured meeting point but at 1 GiB, above the 461-MB shards whose lone L2
// searches the two-rank rehearsal of config 4 prices as scans of the f32 rows.  L2 rows below it are served as before.
constexpr double kSketchL2MinBytes = 1024.0 * (1 << 20);
constexpr uint32_t kSketchCandCap = 4096;              // candidates the gathered K1 rescores at most (more: not certified)
constexpr uint32_t kSketchRescoreBlocks = 32;
inline uint32_t sketch_list_k(size_t limit) { return (uint32_t)std::max<size_t>(2 * limit, limit + 16); }
// The L2 family (L2, squared L2) reads the int8 sketch alone -- its column keeps ||x_r||^2 beside the dot's bounds (DESIGN
// 4.10); the 6-, 5- and 4-bit tiers stay with the dot family (sketch_dot_metric: their passes have no such epilogue).
bool sketch_dot_metric(int metric) { return metric == VT_COSINE || metric == VT_INNER_PRODUCT || metric == VT_NEG_INNER_PRODUCT; }
bool sketch_l2_metric(int metric) { return metric == VT_L2 || metric == VT_L2_SQUARED; }
bool sketch_metric(int metric) { return sketch_dot_metric(metric) || sketch_l2_metric(metric); }
bool sketch_wanted(const Shard *ix, size_t limit) {
  if (!vt::env::on(vt::env::SKETCH) || ix->sketch.refused || !sketch_metric(ix->metric) || ix->single_nominate) return false;
  if (!ix->ranks_clean || ix->n == 0 || ix->dim <= 0 || (uint32_t)ix->dim > vt::kSketchMaxDim) return false;
  if (limit == 0 || sketch_list_k(limit) > (size_t)vt::kMaxFusedK || vt::sketch_scan_lds_bytes((uint32_t)ix->dim, sketch_list_k(limit)) == 0)
    return false;
  // (force_sketch6 brings the int8 sketch with it: it is the 6-bit pass's fallback, and serves the limits that pass declines)
  const double cut = sketch_l2_metric(ix->metric) ? kSketchL2MinBytes : kSketchMinBytes;
  return vt::env::on(vt::env::FORCE_SKETCH) || vt::env::on(vt::env::FORCE_SKETCH6) || (double)ix->n * ix->ld * 4.0 >= cut;
}
size_t sketch_elems(const Shard *ix) { return vt::sketch_bytes((uint32_t)std::max<size_t>(ix->cap, ix->n), (uint32_t)ix->dim); }

// K1qm (vt_sketch_batch.hip): a batch -- or callers that met -- of 2..kSketchBatchMaxQueries queries with limits up
// to 32 shares passes over the int8 sketch, eight queries a pass, where a lone search of the handle would read it and
// the f32 rows reach the batch cut (host/vt_sketchbatch.h holds the gate, the cuts and the planner as plain C++).
// force_sketch = 2 lifts the cut and the query bound (tests); sketch = 2 keeps batches off the sketch.  NEED_SKETCH8 asks
// for the int8 column alone and means nothing where sketch_wanted says no.
bool sketch_batch_wanted(const Shard *ix, size_t nq, size_t limit) {
  if (!sketch_wanted(ix, limit)) return false;
  vt_host::SketchBatchShape s;
  s.dot_metric = sketch_dot_metric(ix->metric);
  s.l2_metric = sketch_l2_metric(ix->metric);
  s.strictly_ranked = ix->ranks_clean;
  s.single_nominate = ix->single_nominate;
  s.refused = ix->sketch.refused;
  s.dim = (uint32_t)ix->dim;
  s.row_bytes = (double)ix->n * ix->ld * 4.0;
  s.sketch = vt::env::get(vt::env::SKETCH);
  s.force = vt::env::get(vt::env::FORCE_SKETCH);
  s.column_lacks_xx = ix->sketch.valid && !ix->sketch_xx;
  return vt_host::sketch_batch_gate(s, nq, limit);
}

// K1s (vt_sketch_nibble.hip; its tail: vt_sketch.hip): where K1q applies, limits up to kSketch6MaxLimit over f32 rows of at least
// kSketch6MinBytes read the 6-bit sketch instead -- 0.755 of the int8 sketch's bytes -- with block lists of kSketch6ListK
// entries; its wider intervals leave hundreds of candidates, which always go through the gathered K1.  The int8 pass is
// its fallback: a pass that does not certify is followed by K1q, and after kSketch6MissLimit such passes in a row the
// shard stops taking K1s until the column is built anew (spiky rows never certify: DESIGN 4.10).  force_sketch alone
// never selects it.
// kSketch6MinBytes: the chain behind the pass (certify-only tail 40 us, gathered K1 16, select 8.5 against K1q's tail of
// 26: +39 us in the headline's trace) is paid back at 26 ps per row (592 B at 6.63 TB/s against 784 B at 6.79 TB/s), i.e.
// near 1.5 M rows of d = 768 = 4.6 GB of f32 rows.  That is an estimate from two traces: the sweep over sizes that would
// place the meeting point has not been run, so the cut stays where the path has been measured to win.  Rows
// below it are served exactly as before.
constexpr double kSketch6MinBytes = 16.0 * 1024 * (1 << 20);
constexpr size_t kSketch6MaxLimit = 32;
constexpr uint32_t kSketch6ListK = 64;
constexpr uint32_t kSketch6CandCap = 32768;       // ~100 MB of f32 rows at d = 768
constexpr uint32_t kSketch6RescoreBlocks = 256;
constexpr uint32_t kSketch6MissLimit = 4;
bool sketch6_wanted(const Shard *ix, size_t limit) {
  if (!sketch_wanted(ix, limit) || !sketch_dot_metric(ix->metric) || limit > kSketch6MaxLimit || !vt::env::on(vt::env::SKETCH6) ||
      ix->sketch6.refused)
    return false;
  if (vt::sketch6_scan_lds_bytes((uint32_t)ix->dim, kSketch6ListK) == 0) return false;
  return vt::env::on(vt::env::FORCE_SKETCH6) || (double)ix->n * ix->ld * 4.0 >= kSketch6MinBytes;
}

// K1f (vt_sketch_nibble.hip; its tail: vt_sketch.hip): where K1s applies, limits up to kSketch5MaxLimit over f32 rows
// of at least kSketch5MinBytes read the 5-bit sketch first -- 0.838 of the 6-bit sketch's bytes.  Its intervals are twice as
// wide and leave thousands of candidates (about 19 000 of 10 M uniform unit rows at d = 768), so its candidate list has a
// row for every retained slot of the block lists and the gathered K1 behind it runs on kSketch5RescoreBlocks blocks (8-row
// tiles, a wave each: 2 048 waves keep 16 MB in flight over a list of some 58 MB).  K1s is its fallback, on K1s's own terms;
// after kSketch5MissLimit passes in a row that did not certify the shard stops taking K1f until the column is built anew.
// The settings are K1s's, one value further (the product's list of settings stays as long as it was): VT_SKETCH6=2 keeps
// K1s and switches K1f off (0: both); force_sketch6 = 1 never selects K1f, force_sketch6 = 2 forces both.
// kSketch5MaxLimit: on the headline corpus 300 queries at limit 10 left 12 147 ... 38 087 candidates (mean 22 758) and none
// missed; at limit 16 (mean 30 267, up to 40 685: the lists saturate) 7 missed, over the 1 % a miss's extra pass may cost
// (profiles/sketch5/candidates.json).
// kSketch5MinBytes: the sweep over sizes has not been run; the cut stays at the one size the path has been measured at
// (DESIGN 5), which is K1s's.
constexpr double kSketch5MinBytes = 16.0 * 1024 * (1 << 20);
constexpr size_t kSketch5MaxLimit = 10;
constexpr uint32_t kSketch5CandCap = 65536;       // every retained slot: 1 024 lists of 64
constexpr uint32_t kSketch5RescoreBlocks = 512;
constexpr uint32_t kSketch5MissLimit = 4;
bool sketch5_wanted(const Shard *ix, size_t limit) {
  if (!sketch6_wanted(ix, limit) || limit > kSketch5MaxLimit || vt::env::get(vt::env::SKETCH6) == 2 || ix->sketch5.refused) return false;
  if (vt::sketch5_scan_lds_bytes((uint32_t)ix->dim, kSketch6ListK) == 0) return false;
  return vt::env::get(vt::env::FORCE_SKETCH6) >= 2 || (double)ix->n * ix->ld * 4.0 >= kSketch5MinBytes;
}

// K1n (vt_sketch_nibble.hip; its tail: vt_sketch.hip): where K1f applies, limits up to kSketch4MaxLimit over f32 rows
// of at least kSketch4MinBytes read the 4-bit sketch first -- 0.806 of the 5-bit sketch's bytes.  Its intervals are twice
// K1f's again: under the sketch's own threshold Kt a quarter of the corpus would be a candidate.  The threshold is therefore
// taken from the exact keys of the k rows with the smallest key(lo) (launch_sketch_refine, between the threshold and the
// collect kernels): the band is then one interval wide, not two, and leaves what K1f leaves behind Kt (tens of thousands
// of 10 M uniform unit rows at d = 768), over a wider spread -- so the pass leaves two lists a block, the candidate list
// has a row for every slot of those and the gathered K1 runs on kSketch4RescoreBlocks blocks.  K1f is its fallback, on
// K1f's own terms; after kSketch4MissLimit passes in a row that did not certify the shard stops taking K1n until the
// column is built anew.  The settings are K1s's, one value further still (the product's list of settings stays as long
// as it was): VT_SKETCH6=3 keeps K1s and K1f and switches K1n off -- the chain as it was without this column --;
// force_sketch6 = 1 / 2 select what they did, force_sketch6 = 3 forces all three.
// kSketch4MinBytes: the sweep over sizes has not been run for any of the three cuts; this one stays at the one size the
// path has been measured at, which is K1s's and K1f's.
constexpr double kSketch4MinBytes = 16.0 * 1024 * (1 << 20);
constexpr size_t kSketch4MaxLimit = 10;
constexpr uint32_t kSketch4CandCap = 131072;      // every retained slot: 2 048 lists of 64
constexpr uint32_t kSketch4RescoreBlocks = 1024;
constexpr uint32_t kSketch4MissLimit = 4;
bool sketch4_wanted(const Shard *ix, size_t limit) {
  if (!sketch5_wanted(ix, limit) || limit > kSketch4MaxLimit || vt::env::get(vt::env::SKETCH6) == 3 || ix->sketch4.refused) return false;
  if (vt::sketch4_scan_lds_bytes((uint32_t)ix->dim, kSketch6ListK) == 0) return false;
  return vt::env::get(vt::env::FORCE_SKETCH6) >= 3 || (double)ix->n * ix->ld * 4.0 >= kSketch4MinBytes;
}

// What tells the sketch columns apart, by bits per element (8: K1q, 6: K1s, 5: K1f, 4: K1n): the column and what is kept
// beside it, its builders and pass, its counters, the shape of the chain behind the pass, and when a search takes it.
// index_ensure_sketch, nibble_search and every walk over the nibble tiers (kNibbleTiers) go by this one table.
struct SketchKind {
  DerivedColumn<unsigned char> Shard::*col;
  double Shard::*max_norm;
  std::atomic<uint32_t> Shard::*misses;  // (null: K1q counts none)
  size_t (*bytes)(uint32_t rows, uint32_t d);
  hipError_t (*build)(const float *, size_t, uint32_t, uint32_t, uint32_t, void *, unsigned long long *, hipStream_t);
  hipError_t (*rows)(const float *, size_t, const uint32_t *, uint32_t, uint32_t, uint32_t, void *, unsigned long long *, hipStream_t);
  hipError_t (*scan)(const vt::Sketch6ScanArgs &, uint32_t, hipStream_t);  // (null: K1q's pass takes other arguments)
  uint64_t vt_profile::*launches;
  double vt_profile::*ms;
  uint64_t vt_profile::*bytes_read, vt_profile::*candidates, vt_profile::*fallbacks, vt_profile::*builds, vt_profile::*patched_rows;
  vt::env::Key refuse_hook;
  uint32_t block_lists, cand_cap, rescore_blocks;  // lists a block of the pass leaves; the candidate list; the gathered K1's grid
  DevBuf<uint32_t> Ctx::*cand_rows;
  bool exact_threshold;  // Kt' from launch_sketch_refine
  bool (*wanted)(const Shard *, size_t limit);
  uint32_t miss_limit;  // passes in a row that did not certify before the shard stops taking the tier (K1q: none counted)
  size_t elems(const Shard *ix) const { return bytes((uint32_t)std::max<size_t>(ix->cap, ix->n), (uint32_t)ix->dim); }
};
// The nibble tiers by bits per element, in the order a lone search tries them: the narrowest first, each the fallback of
// the one before it (and each wanted only where the next is: sketch4_wanted / sketch5_wanted above).
constexpr int kNibbleTiers[] = {4, 5, 6};
constexpr size_t kNibbleTierCount = sizeof(kNibbleTiers) / sizeof(kNibbleTiers[0]);
const SketchKind &sketch_kind(int bits) {
  static const SketchKind k8{&Shard::sketch, &Shard::sketch_max_norm, nullptr, vt::sketch_bytes, vt::launch_sketch_build, vt::launch_sketch_rows,
                             nullptr, &vt_profile::sketch_launches, &vt_profile::sketch_ms, &vt_profile::sketch_bytes,
                             &vt_profile::sketch_candidates, &vt_profile::sketch_fallbacks, &vt_profile::sketch_builds,
                             &vt_profile::sketch_patched_rows, vt::env::TEST_REFUSE_SKETCH, 1, kSketchCandCap, kSketchRescoreBlocks,
                             &Ctx::dSkRows, false, sketch_wanted, 0};
  static const SketchKind k6{&Shard::sketch6, &Shard::sketch6_max_norm, &Shard::sketch6_misses, vt::sketch6_bytes, vt::launch_sketch6_build,
                             vt::launch_sketch6_rows, vt::launch_sketch6_scan, &vt_profile::sketch6_launches, &vt_profile::sketch6_ms,
                             &vt_profile::sketch6_bytes, &vt_profile::sketch6_candidates, &vt_profile::sketch6_fallbacks,
                             &vt_profile::sketch6_builds, &vt_profile::sketch6_patched_rows, vt::env::TEST_REFUSE_SKETCH6, 1,
                             kSketch6CandCap, kSketch6RescoreBlocks, &Ctx::dSk6Rows, false, sketch6_wanted, kSketch6MissLimit};
  static const SketchKind k5{&Shard::sketch5, &Shard::sketch5_max_norm, &Shard::sketch5_misses, vt::sketch5_bytes, vt::launch_sketch5_build,
                             vt::launch_sketch5_rows, vt::launch_sketch5_scan, &vt_profile::sketch5_launches, &vt_profile::sketch5_ms,
                             &vt_profile::sketch5_bytes, &vt_profile::sketch5_candidates, &vt_profile::sketch5_fallbacks,
                             &vt_profile::sketch5_builds, &vt_profile::sketch5_patched_rows, vt::env::TEST_REFUSE_SKETCH5, 1,
                             kSketch5CandCap, kSketch5RescoreBlocks, &Ctx::dSk5Rows, false, sketch5_wanted, kSketch5MissLimit};
  static const SketchKind k4{&Shard::sketch4, &Shard::sketch4_max_norm, &Shard::sketch4_misses, vt::sketch4_bytes, vt::launch_sketch4_build,
                             vt::launch_sketch4_rows, vt::launch_sketch4_scan, &vt_profile::sketch4_launches, &vt_profile::sketch4_ms,
                             &vt_profile::sketch4_bytes, &vt_profile::sketch4_candidates, &vt_profile::sketch4_fallbacks,
                             &vt_profile::sketch4_builds, &vt_profile::sketch4_patched_rows, vt::env::TEST_REFUSE_SKETCH4,
                             vt::kSketch4BlockLists, kSketch4CandCap, kSketch4RescoreBlocks, &Ctx::dSk4Rows, true, sketch4_wanted,
                             kSketch4MissLimit};
  return bits == 4 ? k4 : bits == 5 ? k5 : bits == 6 ? k6 : k8;
}

// The derived columns a reader with `need` / `limit` wants current, as the elements each must hold (0: not wanted).
// shard_stale and shard_prepare both go by this one answer.  (A shard with rows.)
struct ColumnsWanted {
  size_t bits = 0, nz_bits = 0, norms = 0, shadow = 0, sketch = 0;
  size_t nibble[kNibbleTierCount] = {};  // by kNibbleTiers
};
ColumnsWanted columns_wanted(const Shard *ix, unsigned need, size_t limit) {
  ColumnsWanted w;
  const size_t rows = std::max<size_t>(ix->cap, ix->n);
  const size_t bwords = vt::hamming_matrix_words((uint32_t)rows, ((uint32_t)ix->dim + 63) / 64);
  if (need & NEED_BITS) w.bits = bwords;
  if ((need & NEED_NZBITS) && pattern_search_applies(ix, limit)) w.nz_bits = bwords;
  if (need & NEED_NORMS) w.norms = rows;
  if ((need & NEED_NORMS) && shadow_wanted(ix)) w.shadow = shadow_elems(ix);
  if ((need & (NEED_SKETCH | NEED_SKETCH8)) && sketch_wanted(ix, limit)) w.sketch = sketch_elems(ix);
  for (size_t t = 0; t < kNibbleTierCount; ++t) {
    const SketchKind &kind = sketch_kind(kNibbleTiers[t]);
    if ((need & NEED_SKETCH) && kind.wanted(ix, limit)) w.nibble[t] = kind.elems(ix);
  }
  return w;
}

bool shard_stale(const Shard *ix, unsigned need, size_t limit) {
  if (ix->n == 0) return false;
  const size_t rows = std::max<size_t>(ix->cap, ix->n);
  if ((need & (NEED_RANKS | NEED_STRICT_RANKS)) && !ix->ranks_clean) {
    if ((need & NEED_STRICT_RANKS) || !lazy_ranks_ok(ix, limit)) return true;
    if (!ix->rank_dirty.empty() || ix->rank_dirty_all || ix->dRank.count < rows) return true;
  }
  const ColumnsWanted w = columns_wanted(ix, need, limit);
  for (size_t t = 0; t < kNibbleTierCount; ++t)
    if (w.nibble[t] && !(ix->*sketch_kind(kNibbleTiers[t]).col).current(w.nibble[t])) return true;
  return (w.bits && !ix->bits.current(w.bits)) || (w.nz_bits && !ix->nz_bits.current(w.nz_bits)) ||
         (w.norms && !ix->norms.current(w.norms)) || (w.shadow && !ix->shadow.current(w.shadow)) ||
         (w.sketch && !ix->sketch.current(w.sketch));
}

int index_ensure_bits(Shard *ix, bool nonzero, size_t bwords);
int index_ensure_norms(Shard *ix, size_t rows);
int index_ensure_shadow(Shard *ix, size_t elems);
int index_ensure_sketch(Shard *ix, size_t bytes, int bits = 8);

// Brings the derived columns a reader needs up to date (exclusive access; primary context).
int shard_prepare(Shard *ix, unsigned need, size_t limit) {
  if (ix->n == 0) return VT_OK;
  if (need & (NEED_RANKS | NEED_STRICT_RANKS)) {
    if (!(need & NEED_STRICT_RANKS) && lazy_ranks_ok(ix, limit)) VT_TRY(index_lazy_ranks(ix));
    else VT_TRY(index_sync_ranks(ix, false));
  }
  const ColumnsWanted w = columns_wanted(ix, need, limit);
  if (w.bits) VT_TRY(index_ensure_bits(ix, false, w.bits));
  if (w.nz_bits) VT_TRY(index_ensure_bits(ix, true, w.nz_bits));
  if (w.norms) VT_TRY(index_ensure_norms(ix, w.norms));
  if (w.shadow) VT_TRY(index_ensure_shadow(ix, w.shadow));
  if (w.sketch) VT_TRY(index_ensure_sketch(ix, w.sketch));
  for (size_t t = kNibbleTierCount; t-- > 0;)  // (the widest first: where the card runs out of room, the narrowest goes without)
    if (w.nibble[t]) VT_TRY(index_ensure_sketch(ix, w.nibble[t], kNibbleTiers[t]));
  return VT_OK;
}

int batch_group(Shard *ix, Ctx &c, const float *queries, size_t nq, size_t limit, vt_hits **out, std::vector<char> &done,
                bool bf16, const float *tau_given, std::vector<float> *retry_tau);

// A lone search as a batch of one through the bf16 shadow (vt_flat_set_single_nominate): applies when everything the
// batch path wants is current already -- a reader under the shared lock never waits for a build.
bool single_nominate_applies(const Shard *ix, size_t limit) {
  return ix->single_nominate && ix->ranks_clean && limit >= 1 && limit <= (size_t)vt::kMaxFusedK && ix->n >= 4096 &&
         shadow_wanted(ix) && !shard_stale(ix, NEED_NORMS, limit);
}

// The query in two int8 levels behind its f32 copy in c.hQ: q = t1 Q1 + t2 Q2 + eta.  The integers are chosen with
// a reciprocal; the residuals r = q - t1 Q1 and eta = r - t2 Q2 are then formed from the chosen integers in f64
// (t Q has at most 31 significant bits: exact), so the bound holds for any |Q| <= 127 and only its tightness depends on
// the rounding.  *ee = sum eta_i^2.
void sketch_query_image(Ctx &c, const float *query, uint32_t d, uint32_t ld, uint32_t ld8, float m1, float *t1_out, float *t2_out,
                        double *ee_out) {
  float *hq = c.hQ.p;
  std::memcpy(hq, query, (size_t)d * sizeof(float));
  for (uint32_t i = d; i < ld; ++i) hq[i] = 0.0f;
  int8_t *q1 = reinterpret_cast<int8_t *>(hq + ld), *q2 = q1 + ld8;
  std::memset(q1 + d, 0, ld8 - d);
  std::memset(q2 + d, 0, ld8 - d);
  float t1 = m1 / 127.0f, t2 = 0.0f;
  if (!(t1 > 0.0f) || !std::isfinite(127.0f / m1)) t1 = 0.0f;
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
  double ee = 0.0;
  for (uint32_t i = 0; i < d; ++i) {
    const int v = (int)std::max(-127.0, std::min(127.0, (r[i] * inv2 + kRound) - kRound));
    q2[i] = (int8_t)v;
    const double e = r[i] - t2d * v;
    ee += e * e;
  }
  *t1_out = t1;
  *t2_out = t2;
  *ee_out = ee;
}

// K1q and its tail, one host wait: the pass, then one block that certifies and -- the usual case, a few
// dozen candidates -- rescores them with K1's arithmetic and fills the pinned result block.  A candidate list too long
// for that block (up to kSketchCandCap) goes through the gathered K1 and its select after a second wait.  *done: the
// hits in *out are the exact top `limit`; otherwise the caller scans the f32 rows -- the bound could not certify
// (counted), or it declined before any launch because a dot of these rows could reach the f32 overflow K1 must see for
// itself.  The L2 family: the same chain over the column with xx (the pass's L2 epilogue, kerr = 0, ||q||^2 between its two
// ends), declined where a squared difference could overflow f32.
int sketch_search(Shard *ix, Ctx &c, const float *query, size_t limit, bool *done, vt_hits **out) {
  *done = false;
  const uint32_t d = (uint32_t)ix->dim, ld = ix->ld, ld8 = vt::sketch_ld8(d), nch = ld8 / 16;
  // ||q|| and ||eta|| from f64 sums rounded up
  float m1 = 0.0f;
  double qq = 0.0;
  for (uint32_t i = 0; i < d; ++i) {
    m1 = std::max(m1, std::fabs(query[i]));
    qq += (double)query[i] * (double)query[i];
  }
  const double up = 1.0 + 0x1p-30;
  const double qn = std::sqrt(qq) * up;
  const bool l2 = sketch_l2_metric(ix->metric);
  if (l2) {
    // (||q - x|| <= ||q|| + ||x||: below 2^62 no square of K1's can overflow; at or past it the plain scan recomputes in
    // f64 or reports "metric overflow" for itself.  A column built without xx never serves the family.)
    if (!ix->sketch_xx || !((qn + ix->sketch_max_norm) * up < 0x1p62)) return VT_OK;
  } else if (!(qn * ix->sketch_max_norm * up < 0x1p126)) {
    return VT_OK;  // (K1's overflow flag depends on every row: its scan decides)
  }
  const size_t total = (size_t)ld + 2 * (size_t)ld8 / 4;
  VT_TRY(c.dQ.ensure(total));
  VT_TRY(c.hQ.ensure(total));
  if (c.hSkResid.size() < d) c.hSkResid.resize(d);
  float t1 = 0.0f, t2 = 0.0f;
  double ee = 0.0;
  sketch_query_image(c, query, d, ld, ld8, m1, &t1, &t2, &ee);
  c.qbits_kind = 0;
  c.qsrc = c.dQ.p;
  VT_HIP(hipMemcpyAsync(c.dQ.p, c.hQ.p, total * sizeof(float), hipMemcpyHostToDevice, c.stream));

  const uint32_t kp = sketch_list_k(limit), k = (uint32_t)limit;
  const uint32_t blocks = (uint32_t)c.num_cus * (kp <= (uint32_t)vt::kSmallK ? 4u : 2u);
  VT_TRY(c.dSkKeys.ensure((size_t)blocks * kp));
  VT_TRY(c.dSkPay.ensure((size_t)blocks * kp));
  VT_TRY(c.dSkRows.ensure(kSketchCandCap));
  VT_TRY(c.dSkCount.ensure(1));
  VT_TRY(c.hSkInfo.ensure(4));
  uint32_t *info = c.hSkInfo.mapped();
  if (!info) return fail(VT_ERR_DEVICE, "hipHostGetDevicePointer (sketch status)");
  vt::SketchScanArgs a{};
  a.img = ix->sketch.buf.p;
  a.id_rank = ix->dRank.p;
  a.qimg = reinterpret_cast<const int8_t *>(c.dQ.p + ld);
  a.n = ix->n;
  a.d = d;
  a.nch = nch;
  a.metric = ix->metric;
  a.t1 = t1;
  a.t2 = t2;
  a.qn = qn;
  a.eta = std::sqrt(ee) * up;
  // K1's summation error per unit of ||q|| ||x_r|| (DESIGN_APPENDIX A.5); the L2 family bounds the real dot and carries
  // K1's rounding as a relative term of the distance (A.5b)
  a.kerr = l2 ? 0.0 : 8.0 * d * 0x1p-24;
  a.qq_lo = qq / up;
  a.qq_hi = qq * up;
  a.k = kp;
  a.part_keys = c.dSkKeys.p;
  a.part_pay = c.dSkPay.p;
  VT_TRY(c.mark_begin());
  VT_HIP(vt::launch_sketch_scan(a, blocks, c.stream));
  VT_TRY(c.mark_end());
  vt::SketchTailArgs ta{};
  ta.keys = c.dSkKeys.p;
  ta.pay = c.dSkPay.p;
  ta.lists = blocks;
  ta.kp = kp;
  ta.k = k;
  ta.cap = kSketchCandCap;
  ta.rows = c.dSkRows.p;
  ta.count = c.dSkCount.p;
  ta.info = info;
  ta.X = ix->dX;
  ta.stride = ld;
  ta.q = c.qsrc;
  ta.id_rank = ix->dRank.p;
  ta.d = d;
  ta.metric = ix->metric;
  ta.order = ix->order;
  ta.status = c.dStatus.p;
  ta.out = c.dResMapped;
  VT_HIP(vt::launch_sketch_tail(ta, c.stream));
  VT_HIP(hipStreamSynchronize(c.stream));
  if (c.hSkInfo.p[0] == 2u) {
    // more candidates than the tail's block takes: K1 itself (GENERAL, the count read on the device), then its select
    VT_TRY(c.ensure_part_lists((size_t)kSketchRescoreBlocks * k));
    vt::ScanArgs sa = scan_args(ix, c, d);
    set_gather(sa, gather_of(c.dSkRows.p), kSketchCandCap);  // (the list's room: the count is batch_counts[0])
    sa.k = k;
    use_part_lists(sa, c);
    sa.batch_counts = c.dSkCount.p;
    sa.batch_cap = kSketchCandCap;
    VT_HIP(vt::launch_scan_batch(sa, kSketchRescoreBlocks, 1, c.stream));
    VT_HIP(vt::launch_select(c.dPartKeys.p, c.dPartPay.p, kSketchRescoreBlocks * k, k, 0, 0, c.dStatus.p, c.dResMapped,
                             c.dSelKeys.p, c.dSelPay.p, c.stream));
    VT_HIP(hipStreamSynchronize(c.stream));
  }
  const bool certified = c.hSkInfo.p[0] != 0u && c.hRes.p->status == 0;
  if (c.profiling) {
    float ms = 0.f;
    VT_TRY(c.span_ms(&ms));
    const uint64_t bytes = (uint64_t)vt::sketch_bytes(ix->n, d);
    c.prof.sketch_launches += 1;
    c.prof.sketch_ms += ms;
    c.prof.sketch_bytes += bytes;
    c.prof.sketch_candidates += c.hSkInfo.p[1];
    c.prof.sketch_tail_rescored += c.hSkInfo.p[0] == 1u ? 1 : 0;
    VT_TRY(c.book_scan(1, ix->n, bytes));
  }
  if (!certified) {
    c.prof.sketch_fallbacks += 1;
    return VT_OK;
  }
  std::vector<vt::Entry> entries(c.hRes.p->e, c.hRes.p->e + c.hRes.p->count);
  VT_TRY(make_hits(ix, entries, out));
  *done = true;
  return VT_OK;
}

// ||q||^2 in f64 and max |q_i|, as sketch_search forms them
void sketch_query_norms(const float *query, uint32_t d, float *m1_out, double *qq_out) {
  float m1 = 0.0f;
  double qq = 0.0;
  for (uint32_t i = 0; i < d; ++i) {
    m1 = std::max(m1, std::fabs(query[i]));
    qq += (double)query[i] * (double)query[i];
  }
  *m1_out = m1;
  *qq_out = qq;
}

// K1qm, one host wait: the queries `which` (2..8 rows of `queries`, none of which sketch_batch_query_fits
// turned away) in ONE pass over the int8 sketch, then one launch of K1q's tail with a block per query -- blit, pass, tail,
// wait, as a lone K1q search.  Each query's levels, bounds and lists are the ones sketch_search would form for it, so a
// query whose block certified and rescored (outcome 1) gets flat_search's hits and done[which[g]] = 1.  A query whose
// candidate list is too long for the block (outcome 2), or not certified (0), or whose rescoring raised K1's overflow
// flag, stays unanswered for what batch_ready does with left-over queries, and counts as a fallback: no second chain here.
int sketch_group_search(Shard *ix, Ctx &c, const float *queries, const std::vector<size_t> &which, size_t limit, vt_hits **out,
                        std::vector<char> &done) {
  const uint32_t ng = (uint32_t)which.size();
  const uint32_t d = (uint32_t)ix->dim, ld = ix->ld, ld8 = vt::sketch_ld8(d), nch = ld8 / 16;
  const uint32_t kp = sketch_list_k(limit), k = (uint32_t)limit;
  const uint32_t group = vt::sketch_scan_multi_group(ng);
  const size_t lds = vt::sketch_scan_multi_lds_bytes(d, kp, group);
  if (ng < 2 || ng > (uint32_t)vt::kSketchMultiMax || !lds) return fail(VT_ERR_DEVICE, "internal: a sketch group the pass does not take");
  const bool l2 = sketch_l2_metric(ix->metric);
  const double up = 1.0 + 0x1p-30;
  // one upload: the ng f32 queries (the tail's), then `group` images of two levels (the pass's; the places past ng zero)
  const size_t img_floats = 2 * (size_t)ld8 / 4;
  const size_t total = (size_t)ng * ld + (size_t)group * img_floats;
  VT_TRY(c.dBQ.ensure(total));
  VT_TRY(c.hBQ.ensure(total));
  VT_TRY(c.hQ.ensure((size_t)ld + img_floats));
  if (c.hSkResid.size() < d) c.hSkResid.resize(d);
  vt::SketchScanMultiArgs a{};
  for (uint32_t g = 0; g < ng; ++g) {
    const float *query = queries + which[g] * d;
    float m1 = 0.0f, t1 = 0.0f, t2 = 0.0f;
    double qq = 0.0, ee = 0.0;
    sketch_query_norms(query, d, &m1, &qq);
    sketch_query_image(c, query, d, ld, ld8, m1, &t1, &t2, &ee);  // (into c.hQ: the query padded to ld, its two levels behind)
    std::memcpy(c.hBQ.p + (size_t)g * ld, c.hQ.p, (size_t)ld * sizeof(float));
    std::memcpy(c.hBQ.p + (size_t)ng * ld + (size_t)g * img_floats, c.hQ.p + ld, img_floats * sizeof(float));
    a.t1[g] = t1;
    a.t2[g] = t2;
    a.qn[g] = std::sqrt(qq) * up;
    a.eta[g] = std::sqrt(ee) * up;
    a.kerr[g] = l2 ? 0.0 : 8.0 * d * 0x1p-24;  // (as sketch_search)
    a.qq_lo[g] = qq / up;
    a.qq_hi[g] = qq * up;
  }
  if (group > ng) std::memset(c.hBQ.p + (size_t)ng * ld + (size_t)ng * img_floats, 0, (size_t)(group - ng) * img_floats * sizeof(float));
  c.qbits_kind = 0;  // (c.hQ no longer holds the query last uploaded)
  VT_HIP(hipMemcpyAsync(c.dBQ.p, c.hBQ.p, total * sizeof(float), hipMemcpyHostToDevice, c.stream));

  // (two to four blocks a CU, as many as its LDS holds of them: K1q's grid where the group is small)
  const uint32_t per_cu = (uint32_t)std::min<size_t>(4, (160 * 1024) / (lds + vt_host::kSketchBatchLdsStatic));
  const uint32_t blocks = (uint32_t)c.num_cus * std::max(1u, per_cu);
  VT_TRY(c.dSkKeys.ensure((size_t)ng * blocks * kp));
  VT_TRY(c.dSkPay.ensure((size_t)ng * blocks * kp));
  VT_TRY(c.dSkRows.ensure((size_t)vt::kSketchMultiMax * kSketchCandCap));
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
  a.img = ix->sketch.buf.p;
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
  vt::SketchTailArgs ta{};  // (query 0's: block g takes its own slice)
  ta.keys = c.dSkKeys.p;
  ta.pay = c.dSkPay.p;
  ta.lists = blocks;
  ta.kp = kp;
  ta.k = k;
  ta.cap = kSketchCandCap;
  ta.rows = c.dSkRows.p;
  ta.count = c.dSkCount.p;
  ta.info = info;
  ta.X = ix->dX;
  ta.stride = ld;
  ta.q = c.dBQ.p;
  ta.id_rank = ix->dRank.p;
  ta.d = d;
  ta.metric = ix->metric;
  ta.order = ix->order;
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

// K1s, one host wait: blit, the 6-bit pass, the certification spread over the card (the threshold kernel, the collect
// kernel), the gathered K1 over the candidate rows they left (the count read on the device: none when the pass did not
// certify) and K1's select, all queued before the wait.
// *done as sketch_search has it; a pass that does not certify counts towards the shard's miss limit.
// `bits` 5: K1f, the same chain over the 5-bit sketch (its pass, its bound of the level kept off the L plane, its longer
// candidate list, more blocks for the gathered K1, its own counters and misses).  `bits` 4: K1n, over the 4-bit sketch
// (one plane: no such level bound; two lists a block), with launch_sketch_refine behind the threshold kernel and one kernel
// behind that (launch_sketch4_rescore): it takes the candidates under the exact threshold straight from the pass's lists,
// rescores them, keeps the rows under that threshold and writes the sorted result itself, no select behind it.  (Rows too
// long for its block: the collect with that threshold and the gathered K1 in filter mode, launch_scan_filter, as before.)
// A search whose survivors overflow its short list queues the collect, the lists and the select behind a second wait.
int nibble_search(Shard *ix, Ctx &c, const float *query, size_t limit, bool *done, vt_hits **out, int bits) {
  const SketchKind &kind = sketch_kind(bits);
  const bool five = bits == 5;
  *done = false;
  const uint32_t d = (uint32_t)ix->dim, ld = ix->ld, ld8 = vt::sketch_ld8(d);
  double qq = 0.0;
  for (uint32_t i = 0; i < d; ++i) qq += (double)query[i] * (double)query[i];
  const double up = 1.0 + 0x1p-30;
  const double qn = std::sqrt(qq) * up;
  if (!(qn * ix->*kind.max_norm * up < 0x1p126)) return VT_OK;  // (K1's overflow flag depends on every row: its scan decides)
  const uint32_t lw = vt_host::sketch6_level_words(d);
  const size_t qwords = (size_t)ld + (size_t)vt::kSketch6Levels * lw;
  // K1n: zero words ride behind the query's image in the same blit -- the filtered K1's count, overflow and ticket words
  // (4 KiB: a line per ticket) start every call from zero whatever the last one did, at no launch's cost
  const size_t chain_zeros = vt::kScanFilterSyncWords;
  const size_t total = qwords + (kind.exact_threshold ? chain_zeros : 0);
  VT_TRY(c.dQ.ensure(total));
  VT_TRY(c.hQ.ensure(total));
  if (c.hSkResid.size() < d) c.hSkResid.resize(d);
  float *hq = c.hQ.p;
  std::memcpy(hq, query, (size_t)d * sizeof(float));
  for (uint32_t i = d; i < ld; ++i) hq[i] = 0.0f;
  float t[vt::kSketch6Levels];
  double ee = 0.0;
  static_assert(vt::kSketch6Levels == vt_host::kSketch6Levels, "one number of query levels on both sides");
  vt_host::sketch6_query_levels(query, d, reinterpret_cast<uint32_t *>(hq + ld), c.hSkResid.data(), t, &ee);
  if (kind.exact_threshold) std::memset(hq + qwords, 0, chain_zeros * sizeof(float));
  uint32_t *chain_words = reinterpret_cast<uint32_t *>(c.dQ.p + qwords);  // (ScanArgs::fsync)
  c.qbits_kind = 0;
  c.qsrc = c.dQ.p;
  VT_HIP(hipMemcpyAsync(c.dQ.p, c.hQ.p, total * sizeof(float), hipMemcpyHostToDevice, c.stream));

  const uint32_t kp = kSketch6ListK, k = (uint32_t)limit;
  const uint32_t blocks = (uint32_t)c.num_cus * 4u, lists = blocks * kind.block_lists;
  VT_TRY(c.dSkKeys.ensure((size_t)lists * kp));
  VT_TRY(c.dSkPay.ensure((size_t)lists * kp));
  VT_TRY(c.dSkLoWords.ensure((size_t)lists * kp));
  VT_TRY(c.dSkHiWords.ensure((size_t)lists * kp));
  const uint32_t cand_cap = kind.cand_cap, rescore_blocks = kind.rescore_blocks;
  DevBuf<uint32_t> &cand_rows = c.*kind.cand_rows;
  VT_TRY(cand_rows.ensure(cand_cap));
  VT_TRY(c.dSkCount.ensure(1));
  const uint32_t thresh_blocks = vt::sketch_thresh_blocks(lists, kp);
  // (parts[thresh_blocks][k] | live[thresh_blocks] | K1n: slots[thresh_blocks][k] | the exact threshold's word)
  VT_TRY(c.dSkParts.ensure((size_t)thresh_blocks * (2 * k + 1) + 1));
  VT_TRY(c.dSkSync.ensure(4));
  VT_TRY(c.hSkInfo.ensure(4));
  VT_TRY(c.ensure_part_lists(std::max<size_t>((size_t)rescore_blocks * k, vt::kScanFilterCap)));  // (K1n: the survivors lie there)
  uint32_t *info = c.hSkInfo.mapped();
  if (!info) return fail(VT_ERR_DEVICE, "hipHostGetDevicePointer (sketch status)");
  vt::Sketch6ScanArgs a{};
  a.img = (ix->*kind.col).buf.p;
  a.id_rank = ix->dRank.p;
  a.qimg = reinterpret_cast<const uint32_t *>(c.dQ.p + ld);
  a.n = ix->n;
  a.d = d;
  a.ld8 = ld8;
  a.metric = ix->metric;
  for (int j = 0; j < vt::kSketch6Levels; ++j) a.t[j] = t[j];
  a.qn = qn;
  a.eta = std::sqrt(ee) * up;
  a.kerr = 8.0 * d * 0x1p-24;  // K1's summation error per unit of ||q|| ||x_r|| (DESIGN_APPENDIX A.5)
  {  // the last level stays off the L plane: its share there is c3 -+ w3 per unit of s_r (exact: 25 bits times 19)
    int64_t pos = 0, neg = 0, l1 = 0;
    const uint32_t *last = reinterpret_cast<const uint32_t *>(hq + ld) + (size_t)(vt::kSketch6Levels - 1) * lw;
    if (bits == 4) {  // (one plane: every level meets every bit)
      a.c3 = a.w3 = 0.0;
    } else if (five) {  // (0 <= L <= 1: half of t3 where the 6-bit plane has 1.5)
      vt_host::sketch5_level_bound(last, lw, t[vt::kSketch6Levels - 1], &a.c3, &a.w3);
    } else {
      vt_host::sketch6_level_sums(last, lw, &pos, &neg, &l1);
      const double t3 = 1.5 * (double)t[vt::kSketch6Levels - 1];
      a.c3 = t3 * (double)(pos + neg);
      a.w3 = t3 * (double)l1;
    }
  }
  a.k = kp;
  a.part_keys = c.dSkKeys.p;
  a.part_pay = c.dSkPay.p;
  a.lo_words = c.dSkLoWords.p;
  a.hi_words = c.dSkHiWords.p;
  VT_TRY(c.mark_begin());
  VT_HIP(kind.scan(a, blocks, c.stream));
  VT_TRY(c.mark_end());
  vt::SketchSpreadArgs ta{};
  ta.lo_words = c.dSkLoWords.p;
  ta.hi_words = c.dSkHiWords.p;
  ta.pay = c.dSkPay.p;
  ta.lists = lists;
  ta.kp = kp;
  ta.k = k;
  ta.cap = cand_cap;
  ta.parts = c.dSkParts.p;
  ta.live = c.dSkParts.p + (size_t)thresh_blocks * k;
  ta.sync = c.dSkSync.p;
  ta.rows = cand_rows.p;
  ta.count = c.dSkCount.p;
  ta.info = info;
  if (kind.exact_threshold) ta.slots = ta.live + thresh_blocks;
  VT_HIP(vt::launch_sketch_thresh(ta, c.stream));
  if (kind.exact_threshold) {
    vt::SketchRefineArgs ra{};
    ra.parts = ta.parts;
    ra.slots = ta.slots;
    ra.live = ta.live;
    ra.thresh_blocks = thresh_blocks;
    ra.k = k;
    ra.pay = c.dSkPay.p;
    ra.slots_total = lists * kp;
    ra.X = ix->dX;
    ra.stride = ld;
    ra.q = c.qsrc;
    ra.d = d;
    ra.metric = ix->metric;
    ra.order = ix->order;
    ra.kt_out = ta.slots + (size_t)thresh_blocks * k;
    VT_HIP(vt::launch_sketch_refine(ra, c.stream));
    ta.kt_word = ra.kt_out;
  }
  // K1n, wherever its launcher takes the shape: the candidates are rescored straight from the pass's lists by one kernel
  // (launch_sketch4_rescore) that certifies as the collect does and finishes as the filtered K1 does; no candidate array
  const bool dot_metric = ix->metric == VT_COSINE || ix->metric == VT_INNER_PRODUCT || ix->metric == VT_NEG_INNER_PRODUCT;
  const bool from_lists = kind.exact_threshold && dot_metric && k <= (uint32_t)vt::kSmallK && ta.kt_word &&
                          vt::sketch4_rescore_lds_bytes(d, kp) != 0;
  if (!from_lists) VT_HIP(vt::launch_sketch_collect(ta, c.stream));
  vt::ScanArgs sa = scan_args(ix, c, d);
  set_gather(sa, gather_of(cand_rows.p), cand_cap);  // (the list's room: the count is batch_counts[0])
  sa.k = k;
  use_part_lists(sa, c);
  sa.batch_counts = c.dSkCount.p;
  sa.batch_cap = cand_cap;
  bool delivered = false;
  if (kind.exact_threshold) {
    // K1n: the rows whose rank word is <= Kt' are kept -- the k hits and what ties the k-th -- and the last block sorts
    // them into the result block: no lists, no select (the survivors lie where the lists would)
    vt::ScanArgs fa = sa;
    fa.hi_word = ta.kt_word;
    fa.surv_keys = c.dPartKeys.p;
    fa.surv_pay = c.dPartPay.p;
    fa.surv_cap = vt::kScanFilterCap;
    fa.fsync = chain_words;
    fa.out = c.dResMapped;
    fa.info = info;
    if (from_lists) {
      vt::Sketch4RescoreArgs ra{};
      ra.s = fa;
      ra.s.gather = nullptr;
      ra.s.batch_counts = nullptr;
      ra.hi_words = ta.hi_words;
      ra.pay = ta.pay;
      ra.kp = kp;
      ra.cap = cand_cap;
      VT_HIP(vt::launch_sketch4_rescore(ra, blocks, c.stream));
    } else {
      VT_HIP(vt::launch_scan_filter(fa, rescore_blocks, c.stream));
    }
    VT_HIP(hipStreamSynchronize(c.stream));
    delivered = c.hSkInfo.p[0] == vt::kScanFilterDelivered;
  }
  if (!delivered && (!kind.exact_threshold || c.hSkInfo.p[0] == 2u)) {
    // (K1n, certified but not delivered -- more survivors than the short list holds: thousands of rows tie the k-th key,
    // or the refine kept the sketch's own Kt: the lists and their select over the candidates, behind a second wait.  The
    // rescoring kernel left no candidate array: the collect, over the lists still on the device, goes first.  Not a
    // fallback.)
    if (from_lists) VT_HIP(vt::launch_sketch_collect(ta, c.stream));
    VT_HIP(vt::launch_scan_batch(sa, rescore_blocks, 1, c.stream));
    VT_HIP(vt::launch_select(c.dPartKeys.p, c.dPartPay.p, rescore_blocks * k, k, 0, 0, c.dStatus.p, c.dResMapped,
                             c.dSelKeys.p, c.dSelPay.p, c.stream));
    VT_HIP(hipStreamSynchronize(c.stream));
  }
  const bool certified = (delivered || c.hSkInfo.p[0] == 2u) && c.hRes.p->status == 0;
  if (delivered && certified) c.prof.sketch4_finished += 1;
  if (c.profiling) {
    float ms = 0.f;
    VT_TRY(c.span_ms(&ms));
    const uint64_t bytes = (uint64_t)kind.bytes(ix->n, d);
    c.prof.*kind.launches += 1;
    c.prof.*kind.ms += ms;
    c.prof.*kind.bytes_read += bytes;
    c.prof.*kind.candidates += c.hSkInfo.p[1];
    if (bits == 6) c.prof.sketch6_tail_words += c.hSkInfo.p[3] == 1u ? 1 : 0;
    VT_TRY(c.book_scan(1, ix->n, bytes));
  }
  std::atomic<uint32_t> &misses = ix->*kind.misses;
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

// flat.rs:96-124 on a shard whose rank column shard_prepare has brought up to date --
// strictly (ranks_clean) or lazily (newcomers share kUnranked).  Read-only on the shard.
// `lone`: a search on its own (flat_search), which takes K1q when the sketch is current; the single searches a batch
// leaves over do not.
int search_ready(Shard *ix, Ctx &c, const float *query, size_t n, size_t limit, vt_hits **out, bool lone = false) {
  if (limit == 0) return empty_hits(out);
  VT_TRY(validate_vector(query, n, ix->dim));
  if (ix->n == 0) return empty_hits(out);
  for (int bits : kNibbleTiers) {  // (K1n, then K1f, then K1s: a tier that is not taken or does not certify leaves it to the next)
    const SketchKind &kind = sketch_kind(bits);
    if (!lone || !kind.wanted(ix, limit) || !(ix->*kind.col).current(kind.elems(ix)) ||
        (ix->*kind.misses).load(std::memory_order_relaxed) >= kind.miss_limit)
      continue;
    bool done = false;
    VT_TRY(nibble_search(ix, c, query, limit, &done, out, bits));
    if (done) return VT_OK;
  }
  if (lone && sketch_wanted(ix, limit) && ix->sketch.current(sketch_elems(ix))) {
    bool done = false;
    VT_TRY(sketch_search(ix, c, query, limit, &done, out));
    if (done) return VT_OK;
  }
  if (single_nominate_applies(ix, limit)) {
    std::vector<char> done(1, 0);
    vt_hits *one = nullptr;
    VT_TRY(batch_group(ix, c, query, 1, limit, &one, done, true, nullptr, nullptr));
    if (done[0]) {
      *out = one;
      return VT_OK;
    }
    delete one;  // (not certified: the exact scan decides)
    c.prof.batch_fallbacks += 1;
  }
  const bool lazy = !ix->ranks_clean;
  const size_t lazy_want = std::min<size_t>(limit, ix->n) + (limit < ix->n ? 1 : 0);
  // (a non-zero-bit column that is not current is simply not used: the rows always are)
  const bool by_pattern = pattern_search_applies(ix, limit) && !shard_stale(ix, NEED_NZBITS, limit);
  uint32_t qnz = 0;
  VT_TRY(upload_query(c, query, n, &qnz, by_pattern ? 2 : 0));
  vt::ScanArgs j = scan_args(ix, c, (uint32_t)ix->dim);
  j.q_nonzero = qnz;
  std::vector<vt::Entry> entries;
  auto best_rows = [&](size_t want) -> int {
    if (by_pattern)
      return run_hamming(c, ix->nz_bits.buf.p, c.dQbits, ix->dRank.p, ix->n, j.d, want, entries, true, ix->metric == VT_JACCARD);
    return run_scan(c, j, want, entries, true);
  };
  if (lazy) {
    // one hit more than asked for: if it does not tie with the last wanted one, the set is
    // exact whatever the unranked rows' id order is, and equal-rank runs are put in id order here
    VT_TRY(best_rows(lazy_want));
    const bool ambiguous = limit < ix->n && entries.size() == lazy_want &&
                           rank_key_of(entries[limit - 1].key) == rank_key_of(entries[limit].key);
    if (ambiguous) return kEscalate;  // a tie across the boundary: only the true id order can cut it
    if (entries.size() > limit) entries.resize(limit);
    for (size_t i = 0; i < entries.size();) {
      size_t e = i + 1;
      while (e < entries.size() && rank_key_of(entries[e].key) == rank_key_of(entries[i].key)) ++e;
      if (e - i > 1)
        std::sort(entries.begin() + i, entries.begin() + e,
                  [&](const vt::Entry &a, const vt::Entry &b) { return ix->ids[a.row] < ix->ids[b.row]; });
      i = e;
    }
    return make_hits(ix, entries, out);
  }
  VT_TRY(best_rows(limit));
  return make_hits(ix, entries, out);
}

// The same for a caller that owns the shard outright (a shard worker, or any caller under
// the exclusive lock): prepare, run on the primary context, settle a boundary tie.
int search_owner(Shard *ix, const float *query, size_t n, size_t limit, vt_hits **out) {
  const unsigned need = NEED_RANKS | NEED_NZBITS | NEED_SKETCH;
  if (shard_stale(ix, need, limit)) VT_TRY(shard_prepare(ix, need, limit));
  int st = search_ready(ix, ix->ctx, query, n, limit, out, true);
  if (st == kEscalate) {
    VT_TRY(shard_prepare(ix, NEED_STRICT_RANKS, limit));
    st = search_ready(ix, ix->ctx, query, n, limit, out, true);
  }
  return st;
}

// Exact f64-cosine scan of the first `d` coordinates of every row (K6b), passes
// of <= kMaxFusedK until `want` hits are collected.  Query already in c.dQ.
int run_cosine_scan(Ctx &c, Shard *ix, uint32_t d, double qq, size_t want, std::vector<vt::Entry> &out) {
  const size_t kmax = vt::cosine_scan_lds_bytes(d, vt::kMaxFusedK) ? (size_t)vt::kMaxFusedK : (size_t)vt::kSmallK;
  if (vt::cosine_scan_lds_bytes(d, 1) == 0) return fail(VT_ERR_UNSUPPORTED, "prefix too long for the cosine scan kernel");
  uint64_t lo = 0;
  bool has_lo = false;
  const size_t total = std::min<size_t>(want, ix->n);
  // (a prefix-cosine pass costs ~90 us before its first byte: f64 sums, its own select and wait)
  if (out.empty() && threshold_applies(total, ix->n, (double)ix->n * vt::padded_dim(d) * 4.0, 90e-6)) {
    const uint32_t k = (uint32_t)total;
    VT_TRY(c.dKeyCol.ensure(((size_t)ix->n + 1) / 2 * 2));
    VT_TRY(c.ensure_part_lists(kThresholdListCap));  // (threshold_rows' list: the scan's own lists are shorter)
    vt::CosineScanArgs a = cosine_scan_args(ix, c, d, qq);
    a.k = 1;
    a.key_out = c.dKeyCol.p;
    uint32_t blocks = 0;
    VT_TRY(cosine_scan_all(c, a, &blocks));
    VT_TRY(threshold_rows(c, ix->n, k));
    VT_TRY(c.ensure_cand_lists(k));
    vt::CosineRerankArgs g = cosine_rerank_args(ix, c, d);
    set_gather(g, gather_of(c.dListPay.p), k);
    VT_HIP(vt::launch_cosine_rerank(g, c.stream));
    const int rc = collect_sorted_list(c, c.dCandKeys.p, c.dCandPay.p, k, out);
    if (c.profiling && rc != kRetryInternal) VT_TRY(c.book_prefix((uint64_t)ix->n * d * 4));
    if (rc != kRetryInternal) return rc;
    out.clear();
  }
  while (out.size() < total) {
    const uint32_t k = (uint32_t)std::min<size_t>(kmax, total - out.size());
    vt::CosineScanArgs a = cosine_scan_args(ix, c, d, qq);
    a.k = k;
    a.lo_key = lo;
    a.has_lo = has_lo ? 1 : 0;
    uint32_t blocks = 0;
    VT_TRY(cosine_scan_all(c, a, &blocks));
    VT_TRY(select_pass(c, c.dPartKeys.p, c.dPartPay.p, blocks * k, k, 0, false));
    if (c.profiling) VT_TRY(c.book_prefix((uint64_t)ix->n * d * 4));
    if (c.hRes.p->status == VT_ERR_OVERFLOW) return VT_ERR_OVERFLOW;
    const uint32_t got = c.hRes.p->count;
    for (uint32_t i = 0; i < got; ++i) out.push_back(c.hRes.p->e[i]);
    if (got < k) break;
    lo = c.hRes.p->e[got - 1].key;
    has_lo = true;
  }
  return VT_OK;
}

// A stage over ALL rows of a float hamming / jaccard collection -- vector_top_k on the first d coordinates
// (search.rs:38-73; distances.rs:319-347 look at nothing but which coordinates are non-zero) -- reads the
// first ceil(d / 64) words of every row's non-zero bits instead of the rows: K4 with a prefix mask, 1/32 of the
// bytes.  Applies when the column is current (a reader never waits for it) and the query's non-zero bits are
// what c.dQbits holds (upload_query with_bits = 2).
bool pattern_stage_applies(const Shard *ix, const Ctx &c, size_t want) {
  return c.qbits_kind == 2 && want >= 1 && want <= (size_t)vt::kMaxFusedK && pattern_search_applies(ix, want) &&
         !shard_stale(ix, NEED_NZBITS, want);
}

// One vector_top_k stage (search.rs:38-73) on the resident corpus: prefix length
// `d`, over all rows (`rows` empty) or over the candidate rows of the previous
// stage; keeps `want` hits.
int funnel_stage(Shard *ix, Ctx &c, const float *query, uint32_t d, const std::vector<uint32_t> &rows, bool all_rows,
                 size_t want, uint32_t qnz, std::vector<vt::Entry> &out) {
  if (!all_rows) {
    VT_TRY(c.dRows.ensure(rows.size()));
    VT_HIP(hipMemcpyAsync(c.dRows.p, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
    VT_HIP(hipStreamSynchronize(c.stream));
  }
  if (ix->metric == VT_COSINE) {
    double qq = 0.0;  // f64_dot(q, q) over the prefix (distances.rs:179-185)
    for (uint32_t j = 0; j < d; ++j) qq += (double)query[j] * (double)query[j];
    if (all_rows) return run_cosine_scan(c, ix, d, qq, want, out);
    VT_TRY(c.ensure_cand_lists(rows.size()));
    vt::CosineRerankArgs a = cosine_rerank_args(ix, c, d);
    set_gather(a, gather_of(c.dRows.p), (uint32_t)rows.size());
    VT_HIP(vt::launch_cosine_rerank(a, c.stream));
    return collect_from_keys(c, c.dCandKeys.p, c.dCandPay.p, (uint32_t)rows.size(), want, out);
  }
  if (all_rows && pattern_stage_applies(ix, c, want))
    return run_hamming(c, ix->nz_bits.buf.p, c.dQbits, ix->dRank.p, ix->n, d, want, out, true, ix->metric == VT_JACCARD,
                       (((uint32_t)ix->dim + 63) / 64 + 1) / 2);
  vt::ScanArgs j = scan_args(ix, c, d);
  if (!all_rows) set_gather(j, gather_of(c.dRows.p), (uint32_t)rows.size());
  j.q_nonzero = qnz;
  return run_scan(c, j, want, out, false);
}

// The index's own metric (K1 arithmetic: for a cosine index the f32 dot of normalised rows, like
// flat_search) over the first `d` coordinates of `count` rows -- all rows, or the Entry.row column
// of `src` -- on the device: the `want` <= kMaxFusedK best, sorted, into `dst`.  Nothing is waited
// for; an overflow flag stays in c.dStatus until a select with `last` moves it into its block.
int scan_stage_dev(Shard *ix, Ctx &c, uint32_t d, const ResultBlock *src, uint32_t count, uint32_t want, uint32_t qnz,
                   ResultBlock *dst, bool last) {
  int *status = last ? c.dStatus.p : nullptr;
  if (!src && pattern_stage_applies(ix, c, want)) {
    // all rows under float hamming / jaccard: the non-zero bits of the prefix (K4) instead of the rows
    const uint32_t hblocks = c.grid_for((ix->n + 63) / 64, vt::hamming_lds_bytes(want), c.hamming_blocks_per_cu);
    const uint32_t hlists = vt::scan_lists(hblocks);
    VT_TRY(c.ensure_part_lists((size_t)hlists * want));
    vt::HammingArgs h = pattern_prefix_args(ix, c, d);
    h.k = want;
    use_part_lists(h, c);
    VT_TRY(c.mark_begin());
    VT_HIP(vt::launch_hamming(h, hblocks, c.stream));
    VT_TRY(c.mark_end());
    c.defer_prefix(c.profiling, (uint64_t)ix->n * h.words * 8);
    VT_HIP(vt::launch_select(c.dPartKeys.p, c.dPartPay.p, hlists * want, want, 0, 0, status, dst, c.dSelKeys.p, c.dSelPay.p, c.stream));
    return VT_OK;
  }
  vt::ScanArgs a = scan_args(ix, c, d);  // (all rows: count == ix->n)
  if (src) set_gather(a, gather_of(src), count);
  a.q_nonzero = qnz;
  const bool timed = c.profiling && !src && d < (uint32_t)ix->dim;  // a sweep of every row's prefix: priced like the cosine one
  VT_TRY(scan_to_block(c, a, want, timed, status, dst));
  c.defer_prefix(timed, (uint64_t)ix->n * d * 4);
  return VT_OK;
}

// One funnel / rerank stage that never leaves the device: scores `count` rows
// (all rows, or the Entry.row column of the previous stage's block), keeps
// `want` <= kMaxFusedK of them in `dst`.  Nothing is waited for; an overflow
// flag raised by any stage stays in c.dStatus until a select with `last` moves
// it into its block.
int funnel_stage_dev(Shard *ix, Ctx &c, const float *query, uint32_t d, const ResultBlock *src, uint32_t count,
                     uint32_t want, uint32_t qnz, ResultBlock *dst, bool last) {
  if (ix->metric != VT_COSINE) return scan_stage_dev(ix, c, d, src, count, want, qnz, dst, last);
  int *status = last ? c.dStatus.p : nullptr;
  double qq = 0.0;  // f64_dot(q, q) over the prefix (distances.rs:179-185)
  for (uint32_t j = 0; j < d; ++j) qq += (double)query[j] * (double)query[j];
  if (!src) {
    vt::CosineScanArgs a = cosine_scan_args(ix, c, d, qq);
    a.k = want;
    uint32_t blocks = 0;
    VT_TRY(cosine_scan_all(c, a, &blocks));
    c.defer_prefix(c.profiling, (uint64_t)ix->n * d * 4);
    VT_HIP(vt::launch_select(c.dPartKeys.p, c.dPartPay.p, blocks * want, want, 0, 0, status, dst, c.dSelKeys.p,
                             c.dSelPay.p, c.stream));
    return VT_OK;
  }
  VT_TRY(c.ensure_cand_lists(count));
  vt::CosineRerankArgs a = cosine_rerank_args(ix, c, d);
  set_gather(a, gather_of(src), count);
  VT_HIP(vt::launch_cosine_rerank(a, c.stream));
  VT_HIP(vt::launch_select(c.dCandKeys.p, c.dCandPay.p, count, want, 0, 0, status, dst, c.dSelKeys.p, c.dSelPay.p,
                           c.stream));
  return VT_OK;
}

// True when every stage of a funnel fits one fused pass on the device.
bool funnel_fits_device(const Shard *ix, const size_t *stages, size_t nstages, size_t candidates, size_t limit) {
  if (candidates > (size_t)vt::kMaxFusedK || limit > (size_t)vt::kMaxFusedK) return false;
  if (ix->metric == VT_JACCARD && ix->dim >= 4096) return false;
  auto fits = [&](uint32_t d, uint32_t k, bool all_rows) {
    if (ix->metric == VT_COSINE) return all_rows ? vt::cosine_scan_lds_bytes(d, k) != 0 : (size_t)2 * d * 4 + 64 <= 160 * 1024;
    return vt::scan_lds_bytes(d, k) != 0;
  };
  for (size_t i = 0; i < nstages; ++i)
    if (!fits((uint32_t)stages[i], (uint32_t)std::min<size_t>(candidates, ix->n), i == 0)) return false;
  return fits((uint32_t)ix->dim, (uint32_t)std::min<size_t>(limit, ix->n), false);
}

// Candidate rows of one funnel pass (collection.ex:674-691) without the final rerank.
int funnel_rows(Shard *ix, Ctx &c, const float *query, const size_t *stages, size_t nstages, size_t candidates,
                std::vector<uint32_t> &rows, std::vector<vt::Entry> *first = nullptr) {
  rows.clear();
  if (first) first->clear();
  bool all_rows = true;
  for (size_t i = 0; i < nstages; ++i) {
    uint32_t nz = 0;
    for (size_t j = 0; j < stages[i]; ++j) nz += query[j] != 0.0f ? 1u : 0u;
    std::vector<vt::Entry> kept;
    VT_TRY(funnel_stage(ix, c, query, (uint32_t)stages[i], rows, all_rows, candidates, nz, kept));
    if (first && i == 0) *first = kept;  // the only stage that cuts: later ones re-score the same set
    rows.resize(kept.size());
    for (size_t r = 0; r < kept.size(); ++r) rows[r] = kept[r].row;
    all_rows = false;
    if (rows.empty()) break;
  }
  return VT_OK;
}

// Sign bits of every stored row in K4's layout -- compress_sign_bits (collection.ex:926) kept in HBM, `bwords` words --
// built on first use (`nonzero`: the column of non-zero bits that flat_search under float hamming / jaccard reads
// instead of the rows).
int index_ensure_bits(Shard *ix, bool nonzero, size_t bwords) {
  Ctx &c = ix->ctx;
  const uint32_t d = (uint32_t)ix->dim;
  DerivedColumn<uint64_t> &col = nonzero ? ix->nz_bits : ix->bits;
  if (col.current(bwords)) return VT_OK;
  if (col.patchable(bwords)) {
    // only the rows mutated since the last use
    uint32_t count = 0;
    VT_TRY(upload_row_list(ix, col.dirty, &count));
    VT_HIP(vt::launch_sign_pack_rows(ix->dX, ix->ld, c.dRankPairs.p, count, d, col.buf.p, c.stream, nonzero ? 1 : 0));
    if (count) VT_HIP(hipStreamSynchronize(c.stream));  // the pinned list is reused by the next caller
    col.mark_current();
    return VT_OK;
  }
  col.forget();
  if (nonzero) {
    // (an accelerator, not a requirement: on a card too full for d / 8 more bytes per row the
    // searches keep reading the rows)
    bool refused = col.buf.ensure(bwords) != VT_OK;
#ifdef VT_TEST_HOOKS
    // (libvettore_hip_hooks.so only: the allocation "fails", tests/test_gpu_parity.py checks what follows)
    refused = refused || vt::env::on(vt::env::TEST_REFUSE_NZBITS);
#endif
    if (refused) {
      col.refuse();
      return VT_OK;
    }
  } else {
    VT_TRY(col.buf.ensure(bwords));
  }
  VT_HIP(hipMemsetAsync(col.buf.p, 0, bwords * sizeof(uint64_t), c.stream));
  VT_HIP(vt::launch_sign_pack(ix->dX, ix->ld, ix->n, d, col.buf.p, 1, c.stream, nonzero ? 1 : 0));
  // The column counts as current from here on, for readers on OTHER streams too (leased contexts
  // under the shared lock): the build must have finished before the exclusive lock can drop, also on
  // the paths that return without touching this stream again (limit == 0, a query that fails
  // validation) -- ADVICE r3.
  VT_HIP(hipStreamSynchronize(c.stream));
  col.mark_current();
  return VT_OK;
}

// The bf16 shadow of the rows brought up to date (exclusive access; primary context): the rows
// mutated since its last use are re-rounded in place; a first use, a slab that outgrew it or more
// than kMaxDerivedDirty mutations rebuild the whole image (one pass over the rows: ~10 ms per
// 30 GB).  An accelerator, not a requirement: without room for it -- after the allocation at least
// a quarter of the card must still be free, the rows will want to grow -- the shard is marked
// refused and its batches keep streaming the f32 rows (until the index is emptied).
int index_ensure_shadow(Shard *ix, size_t elems) {
  Ctx &c = ix->ctx;
  DerivedColumn<uint16_t> &col = ix->shadow;
  if (col.current(elems)) return VT_OK;
  if (col.patchable(elems)) {
    uint32_t count = 0;
    VT_TRY(upload_row_list(ix, col.dirty, &count));
    VT_HIP(vt::launch_shadow_rows(ix->dX, ix->ld, c.dRankPairs.p, count, ix->ld, col.buf.p, c.stream));
    if (count) VT_HIP(hipStreamSynchronize(c.stream));  // the pinned list is reused by the next caller; readers on other streams follow
    c.prof.shadow_patched_rows += count;
    col.mark_current();
    return VT_OK;
  }
  col.forget();
  if (col.buf.count < elems) {
    col.buf.release();
    size_t free_b = 0, total_b = 0;
    VT_HIP(hipMemGetInfo(&free_b, &total_b));
    bool refused = free_b < elems * sizeof(uint16_t) || free_b - elems * sizeof(uint16_t) < total_b / 4;
    // (geometric head room: a corpus that arrives in appends would otherwise re-allocate at every growth of the slab)
    size_t want = elems;
    if (!refused) {
      const size_t roomy = elems + elems / 4;
      if (free_b >= roomy * sizeof(uint16_t) && free_b - roomy * sizeof(uint16_t) >= total_b / 4) want = roomy;
      refused = col.buf.ensure(want) != VT_OK;
    }
#ifdef VT_TEST_HOOKS
    // (libvettore_hip_hooks.so only: the allocation "fails", tests/test_gpu_shadow.py checks what follows)
    refused = refused || vt::env::on(vt::env::TEST_REFUSE_SHADOW);
#endif
    if (refused) {
      col.refuse();
      return VT_OK;
    }
  }
  // (the slab's rows [0, cap) -> the whole image)
  const uint32_t rows_img = (uint32_t)(elems / ix->ld);
  VT_TRY(c.mark_begin());
  VT_HIP(vt::launch_shadow_build(ix->dX, ix->ld, ix->cap, rows_img, ix->ld, col.buf.p, c.stream));
  VT_TRY(c.mark_end());
  // current from here on, for readers on other streams too: the build has finished before the
  // exclusive lock can drop
  VT_HIP(hipStreamSynchronize(c.stream));
  if (c.profiling) {
    float ms = 0.f;
    VT_TRY(c.span_ms(&ms));
    c.prof.shadow_builds += 1;
    c.prof.shadow_build_ms += ms;
  }
  col.mark_current();
  return VT_OK;
}

// The int8 sketch brought up to date (exclusive access; primary context), on the shadow's terms: the rows mutated since
// its last use are re-quantised in place; a first use, a slab that outgrew it or more than kMaxDerivedDirty mutations
// rebuild it (one pass over the rows); without room for it -- a quarter of the card must stay free -- it is refused and
// lone searches keep scanning the f32 rows.  The bound on every row's norm comes back with it (the overflow guard).
// `bits` 6 / 5 / 4: the 6-bit / 5-bit / 4-bit sketch on the same terms (its own bound, its own counters: sketch_kind); a
// whole build starts its misses over.  The int8 column of an L2 / squared-L2 handle is built and patched with xx_r in the
// metadata run's fourth dword (Shard::sketch_xx); every other column's image is what it was.
int index_ensure_sketch(Shard *ix, size_t bytes, int bits_per) {
  Ctx &c = ix->ctx;
  const SketchKind &kind = sketch_kind(bits_per);
  DerivedColumn<unsigned char> &col = ix->*kind.col;
  double &max_norm = ix->*kind.max_norm;
  if (col.current(bytes)) return VT_OK;
  const uint32_t d = (uint32_t)ix->dim;
  const size_t tile_bytes = kind.bytes(vt::kSketchTileRows, d);
  VT_TRY(c.dBNorm.ensure(1));
  unsigned long long bits = 0;
  if (col.patchable(bytes)) {
    const bool with_xx = bits_per == 8 && ix->sketch_xx;  // (the patch writes what the build wrote)
    uint32_t count = 0;
    VT_TRY(upload_row_list(ix, col.dirty, &count));
    std::memcpy(&bits, &max_norm, sizeof(double));
    VT_HIP(hipMemcpyAsync(c.dBNorm.p, &bits, sizeof(bits), hipMemcpyHostToDevice, c.stream));
    const uint32_t rows_img = (uint32_t)(col.buf.count / tile_bytes * vt::kSketchTileRows);
    VT_HIP((with_xx ? vt::launch_sketch_rows_xx : kind.rows)(ix->dX, ix->ld, c.dRankPairs.p, count, rows_img, d, col.buf.p, c.dBNorm.p,
                                                             c.stream));
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
    if (bits_per == 8) ix->sketch_xx = sketch_l2_metric(ix->metric);  // (a handle's metric never changes: fixed with the column)
    const bool with_xx = bits_per == 8 && ix->sketch_xx;
    VT_HIP((with_xx ? vt::launch_sketch_build_xx : kind.build)(ix->dX, ix->ld, ix->n, rows_img, d, col.buf.p, c.dBNorm.p, c.stream));
    c.prof.*kind.builds += 1;
    if (kind.misses) (ix->*kind.misses).store(0, std::memory_order_relaxed);
  }
  VT_HIP(hipMemcpyAsync(&bits, c.dBNorm.p, sizeof(bits), hipMemcpyDeviceToHost, c.stream));
  // current from here on, for readers on other streams too: the build has finished before the exclusive lock can drop
  VT_HIP(hipStreamSynchronize(c.stream));
  std::memcpy(&max_norm, &bits, sizeof(double));
  col.mark_current();
  return VT_OK;
}

// binary_top_k candidates (search.rs:76-92) of the query already in c.dQ.
int quantized_rows(Shard *ix, Ctx &c, size_t candidates, std::vector<uint32_t> &rows, std::vector<vt::Entry> *entries = nullptr) {
  const uint32_t d = (uint32_t)ix->dim;
  std::vector<vt::Entry> local;
  std::vector<vt::Entry> &cand = entries ? *entries : local;
  cand.clear();
  VT_TRY(run_hamming(c, ix->bits.buf.p, c.dQbits, ix->dRank.p, ix->n, d, candidates, cand, false));
  rows.resize(cand.size());
  for (size_t i = 0; i < cand.size(); ++i) rows[i] = cand[i].row;
  return VT_OK;
}

// Per-row squared norms and their maximum (the error margin of the batched path), brought
// up to date: all rows on first use, afterwards only the rows mutated since.
int index_ensure_norms(Shard *ix, size_t rows) {
  Ctx &c = ix->ctx;
  const uint32_t d = (uint32_t)ix->dim, n = ix->n;
  DerivedColumn<float> &col = ix->norms;
  if (col.current(rows)) return VT_OK;
  VT_TRY(c.dBNorm.ensure(1));
  unsigned long long bits = 0;
  if (col.patchable(rows)) {
    // norms of the rows mutated since the last batch; the maximum can only be kept or raised
    // (a stale larger bound only widens the acceptance margin)
    uint32_t count = 0;
    VT_TRY(upload_row_list(ix, col.dirty, &count));
    std::memcpy(&bits, &ix->max_sqnorm, sizeof(double));
    VT_HIP(hipMemcpyAsync(c.dBNorm.p, &bits, sizeof(bits), hipMemcpyHostToDevice, c.stream));
    VT_HIP(vt::launch_row_sqnorms_rows(ix->dX, ix->ld, c.dRankPairs.p, count, d, col.buf.p, c.dBNorm.p, c.stream));
  } else {
    // all rows: a first use, more than kMaxDerivedDirty mutations since, or a slab that grew past the column
    col.forget();
    VT_TRY(col.buf.ensure(rows));
    VT_HIP(hipMemsetAsync(c.dBNorm.p, 0, sizeof(unsigned long long), c.stream));
    VT_HIP(vt::launch_row_sqnorms(ix->dX, ix->ld, n, d, col.buf.p, c.dBNorm.p, c.stream));
  }
  VT_HIP(hipMemcpyAsync(&bits, c.dBNorm.p, sizeof(bits), hipMemcpyDeviceToHost, c.stream));
  VT_HIP(hipStreamSynchronize(c.stream));
  std::memcpy(&ix->max_sqnorm, &bits, sizeof(double));
  col.mark_current();
  return VT_OK;
}

}  // namespace
