// vt_launch.h -- what every launch site repeats, said once: the kernels' argument structs filled from a shard and a context,
// gather lists by name, the context's list buffers handed to a launch, K1 into a device block, the all-rows f64 cosine scan.
// Part of vt_index.cpp's translation unit (included there, in this order, exactly once): the host
// side is one TU on purpose -- everything below the C ABI lives in an anonymous namespace.
#pragma once

namespace {

// ------------------------------------------------------------------ argument builders
// Every field a builder does not name stays zero; a site then says only what is particular to it (its gather list, k,
// q_nonzero, a query block of its own).  A field left out does not fail, it returns other hits for some metric at some
// size: the fields common to all sites are filled here and nowhere else.

// The rows a kernel reads, as its arguments name them: a shard's slab, or rows a stateless call has just uploaded.
struct RowSet {
  const float *X;
  size_t stride;
  const uint32_t *id_rank;
  uint32_t n;
  int metric, order;
};
inline RowSet rows_of(const Shard *ix) { return RowSet{ix->dX, ix->ld, ix->dRank.p, ix->n, ix->metric, ix->order}; }

// K1 over the first d coordinates of all n rows, the query where upload_query left it.
inline vt::ScanArgs scan_args(const RowSet &r, Ctx &c, uint32_t d) {
  vt::ScanArgs a{};
  a.X = r.X;
  a.stride = r.stride;
  a.q = c.qsrc;
  a.id_rank = r.id_rank;
  a.n = r.n;
  a.d = d;
  a.metric = r.metric;
  a.order = r.order;
  a.status = c.dStatus.p;
  return a;
}
inline vt::ScanArgs scan_args(const Shard *ix, Ctx &c, uint32_t d) { return scan_args(rows_of(ix), c, d); }

// K6b: qq = f64_dot(q, q) over the first d coordinates (sequential, host).
inline vt::CosineScanArgs cosine_scan_args(const Shard *ix, Ctx &c, uint32_t d, double qq) {
  vt::CosineScanArgs a{};
  a.X = ix->dX;
  a.stride = ix->ld;
  a.q = c.qsrc;
  a.qq = qq;
  a.id_rank = ix->dRank.p;
  a.n = ix->n;
  a.d = d;
  a.status = c.dStatus.p;
  return a;
}

// The exact cosine rerank: one candidate per row until set_gather names a list; keys and payloads into c.dCandKeys /
// c.dCandPay as they are NOW (ensure_cand_lists comes first).
inline vt::CosineRerankArgs cosine_rerank_args(const RowSet &r, Ctx &c, uint32_t d) {
  vt::CosineRerankArgs a{};
  a.X = r.X;
  a.stride = r.stride;
  a.q = c.qsrc;
  a.id_rank = r.id_rank;
  a.n = r.n;
  a.d = d;
  a.out_keys = c.dCandKeys.p;
  a.out_pay = c.dCandPay.p;
  a.status = c.dStatus.p;
  return a;
}
inline vt::CosineRerankArgs cosine_rerank_args(const Shard *ix, Ctx &c, uint32_t d) { return cosine_rerank_args(rows_of(ix), c, d); }

// K4 over the first d bits of n rows of a bit column in its tiled layout ...
inline vt::HammingArgs hamming_args(const uint64_t *bits, const uint64_t *qbits, const uint32_t *id_rank, uint32_t n, uint32_t d) {
  vt::HammingArgs a{};
  a.bits = bits;
  a.qbits = qbits;
  a.id_rank = id_rank;
  a.n = n;
  a.words = (d + 63) / 64;
  a.pairs = (a.words + 1) / 2;
  a.d = d;
  return a;
}
// ... one of the shard's columns (sign bits, non-zero bits) against the query bits upload_query packed.
inline vt::HammingArgs hamming_args(const uint64_t *bits, Ctx &c, const Shard *ix, uint32_t d) {
  return hamming_args(bits, c.dQbits, ix->dRank.p, ix->n, d);
}
// ... a PREFIX of the non-zero bits (funnel stages under float hamming / jaccard, HammingArgs.tile_pairs): the tiles
// hold the whole rows' word pairs.
inline vt::HammingArgs pattern_prefix_args(const Shard *ix, Ctx &c, uint32_t d) {
  vt::HammingArgs a = hamming_args(ix->nz_bits.buf.p, c, ix, d);
  a.jaccard = ix->metric == VT_JACCARD ? 1 : 0;
  a.tile_pairs = (((uint32_t)ix->dim + 63) / 64 + 1) / 2;
  return a;
}

// K10 for one configuration (validated: every size fits its field): the shape of a wave's work.  The chunk's buffers
// (X, set_off, nsets, full, counts, status) and the table are the caller's to name.
inline vt::MuveraArgs muvera_args(size_t d, size_t R, size_t k, size_t pd, int mode, size_t out_size) {
  vt::MuveraArgs a{};
  a.d = (uint32_t)d;
  a.R = (uint32_t)R;
  a.k = (uint32_t)k;
  a.pd = (uint32_t)pd;
  a.identity = pd == d ? 1 : 0;
  a.C = (uint32_t)(k + (a.identity ? 0 : pd));
  a.mode = mode;
  a.rg = vt::muvera_reps_per_wave(a.R, a.k, a.C, mode);
  a.groups = (a.R + a.rg - 1) / a.rg;
  a.rep_size = ((size_t)1 << k) * pd;
  a.out_size = out_size;
  return a;
}

// K12 over the rows of `r` (d coordinates used), the context's MMR buffers as they are NOW (every ensure comes first).
// The two test hooks are read here and nowhere else: candidates per block and pass, and the staging limit.
inline uint32_t mmr_block_rows() {
  const long v = vt::env::get(vt::env::TEST_MMR_BLOCK_ROWS);
  return v >= 1 && v <= (long)vt::kMmrBlockRows ? (uint32_t)v : vt::kMmrBlockRows;
}
inline vt::MmrArgs mmr_args(const RowSet &r, Ctx &c, uint32_t d, uint32_t block_rows) {
  vt::MmrArgs a{};
  a.X = r.X;
  a.stride = r.stride;
  a.d = d;
  a.metric = r.metric;
  a.order = r.order;
  a.prob = c.dMmrProb.p;
  a.rows = c.dMmrRows.p;
  a.rel = c.dMmrRel.p;
  a.red = c.dMmrRed.p;
  a.norm = c.dMmrNorm.p;
  a.live = c.dMmrLive.p;
  a.partial = c.dMmrPartial.p;
  a.order_out = c.dMmrOrder.p;
  a.count = c.dMmrCount.p;
  a.status = c.dMmrStatus.p;
  a.block_rows = block_rows;
  const long ldim = vt::env::get(vt::env::TEST_MMR_LDS_DIM);
  a.lds_dim = ldim >= 1 && ldim <= (long)vt::kMmrLdsDim ? (uint32_t)ldim : vt::kMmrLdsDim;
  return a;
}

// ------------------------------------------------------------------ gather lists
// One stage's output as the next stage's gather list: the first row index and the u32 words from one to the next.
struct GatherList {
  const uint32_t *rows;
  uint32_t stride;
};
inline GatherList gather_of(const uint32_t *rows) { return GatherList{rows, 1}; }
inline GatherList gather_of(const ResultBlock *b) { return GatherList{&b->e[0].row, sizeof(vt::Entry) / sizeof(uint32_t)}; }
inline GatherList gather_of(const vt::Payload *p) { return GatherList{&p->row, sizeof(vt::Payload) / sizeof(uint32_t)}; }
inline GatherList gather_of(const vt::BatchCand *p) { return GatherList{&p->row, sizeof(vt::BatchCand) / sizeof(uint32_t)}; }
// Batch mode over one ResultBlock per query: the words from a block's list to the next block's.
constexpr uint32_t kBlockGatherWords = (uint32_t)(sizeof(ResultBlock) / sizeof(uint32_t));
// `count` rows of the list instead of all rows (ScanArgs, CosineRerankArgs).
template <class Args>
inline void set_gather(Args &a, GatherList g, uint32_t count) {
  a.gather = g.rows;
  a.gather_stride = g.stride;
  a.n = count;
}

// The context's partial lists as a launch's output (any Args with part_keys / part_pay), as they are NOW:
// ensure_part_lists comes first.
template <class Args>
inline void use_part_lists(Args &a, Ctx &c) {
  a.part_keys = c.dPartKeys.p;
  a.part_pay = c.dPartPay.p;
}

// ------------------------------------------------------------------ launches more than one path shares
// K1 with `a` (scan_args plus the caller's gather list and q_nonzero) on a fully resident grid, then the select that
// leaves the `want` <= kMaxFusedK best, sorted, in the device block `dst`.  Nothing is waited for.  `timed`: ev0 / ev1
// around the scan -- the caller books the span under its own counters.  sel_status: the status word the select moves
// into the block (null: a raised flag stays in c.dStatus for a later select).
int scan_to_block(Ctx &c, vt::ScanArgs a, uint32_t want, bool timed, int *sel_status, ResultBlock *dst) {
  a.tile_rows = vt::scan_tile_rows(a.n, a.d, c.resident_waves());
  const uint32_t blocks = c.grid_for((a.n + a.tile_rows - 1) / a.tile_rows, vt::scan_lds_bytes(a.d, want));
  const uint32_t lists = vt::scan_lists(blocks);
  VT_TRY(c.ensure_part_lists((size_t)lists * want));
  a.k = want;
  use_part_lists(a, c);
  VT_TRY(c.mark_begin(timed));
  VT_HIP(vt::launch_scan(a, blocks, c.stream));
  VT_TRY(c.mark_end(timed));
  VT_HIP(vt::launch_select(c.dPartKeys.p, c.dPartPay.p, lists * want, want, 0, 0, sel_status, dst, c.dSelKeys.p, c.dSelPay.p,
                           c.stream));
  return VT_OK;
}

// K6b with `a` (cosine_scan_args plus k, and lo_key or key_out) over every row: the grid, one list of a.k per block in
// the context's partial lists, ev0 / ev1 around the launch when profiling.  *blocks: the lists it leaves.
int cosine_scan_all(Ctx &c, vt::CosineScanArgs a, uint32_t *blocks) {
  *blocks = c.grid_for((a.n + 63) / 64, vt::cosine_scan_lds_bytes(a.d, a.k));
  VT_TRY(c.ensure_part_lists((size_t)*blocks * a.k));
  use_part_lists(a, c);
  VT_TRY(c.mark_begin());
  VT_HIP(vt::launch_cosine_scan(a, *blocks, c.stream));
  return c.mark_end();
}

}  // namespace
