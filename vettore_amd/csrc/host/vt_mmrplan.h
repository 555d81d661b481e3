// vt_mmrplan.h -- the part of MMR reranking (host/vt_mmr.h) that needs no device: the argument checks of
// Vettore.Distance.mmr_rerank/5 (lib/vettore_distance.ex:334-345, :407-414), result_values/3's score of a hit (:525-546),
// the rows of a list of ids, a call's problems laid out for K12, and what comes back read into orders.
// Stand-alone (no HIP): tests/mmr_check.cpp drives it under AddressSanitizer and UBSan.
#pragma once
#include "../../../include/vettore_flat.h"
#include "vt_idtable.h"

#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <string>
#include <unordered_set>
#include <vector>

namespace vt_host {

// the guards of mmr_rerank/5 (:334-336): alpha a number in [0, 1] (a NaN is neither), final_k positive
inline bool mmr_guards_ok(double alpha, size_t final_k) { return alpha >= 0.0 && alpha <= 1.0 && final_k > 0; }
// finite_number? (:407-414): within the f32 range, which a NaN or an infinity is not
inline bool mmr_score_ok(double v) { return v >= -(double)FLT_MAX && v <= (double)FLT_MAX; }
inline bool mmr_scores_ok(const double *scores, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!mmr_score_ok(scores[i])) return false;
  return true;
}

// result_values/3 (:525-546), the score of a hit: f64 from the f32 raw value.  score_mode 0: raw, 1: similarity.
inline double mmr_hit_score(int metric, float raw32, int score_mode) {
  const double raw = (double)raw32;
  if (metric == VT_NEG_INNER_PRODUCT) return -raw;
  const bool similarity_metric = metric == VT_COSINE || metric == VT_INNER_PRODUCT;
  if (score_mode == 0) return similarity_metric ? raw : -raw;
  if (similarity_metric) return metric == VT_COSINE ? (raw + 1.0) / 2.0 : raw;
  return 1.0 / (1.0 + raw);
}

// The rows of a list of ids in an id table: false when an id is not there or occurs twice (`seen` is scratch).
inline bool mmr_rows_of_ids(const IdTable &table, size_t count, const char *ids, const size_t *id_off,
                            std::vector<uint32_t> &rows, std::unordered_set<uint32_t> &seen) {
  rows.resize(count);
  seen.clear();
  for (size_t i = 0; i < count; ++i) {
    const char *id = ids + id_off[i];
    const size_t len = id_off[i + 1] - id_off[i];
    const uint32_t r = table.find(len ? id : "", len, hash_id(len ? id : "", len));
    if (r == IdTable::kNone || !seen.insert(r).second) return false;
    rows[i] = r;
  }
  return true;
}

// One problem of a call: n candidates (rows of the call's matrix, their relevance), alpha, final_k.
struct MmrJob {
  const uint32_t *rows;
  const double *rel;
  size_t n, k;
  double alpha;
};
// Where everything of a call sits: problem p's candidates at off[p] of the per-candidate arrays.
template <class Problem>
struct MmrLayout {
  std::vector<Problem> prob;
  size_t total = 0;
  uint32_t max_n = 0, max_kk = 0;
};
template <class Problem>
inline bool mmr_layout(const MmrJob *jobs, size_t njobs, MmrLayout<Problem> *out) {
  out->prob.resize(njobs);
  size_t total = 0;
  for (size_t p = 0; p < njobs; ++p) {
    if (jobs[p].n > 0x7fffffffu || total + jobs[p].n > 0xfffffff0u) return false;
    Problem &q = out->prob[p];
    q.off = (uint32_t)total;
    q.n = (uint32_t)jobs[p].n;
    q.kk = (uint32_t)std::min<size_t>(jobs[p].k, jobs[p].n);
    q.pad = 0;
    q.alpha = jobs[p].alpha;
    total += jobs[p].n;
    out->max_n = std::max(out->max_n, q.n);
    out->max_kk = std::max(out->max_kk, q.kk);
  }
  out->total = total;
  return true;
}
// What a call brings back for problem p: its status, and the candidates chosen, in order of choice.
// (-1: the chain ended before the problem's last round -- an internal error the caller names)
template <class Problem>
inline int mmr_collect(const Problem &q, int status, uint32_t count, const uint32_t *order, std::vector<uint32_t> *out) {
  out->clear();
  if (status != 0) return status;
  if (count != q.kk) return -1;
  out->assign(order + q.off, order + q.off + count);
  return VT_OK;
}

}  // namespace vt_host
