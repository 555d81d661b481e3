// vt_device.h -- launch interface between the host index (vt_index.cpp) and the
// gfx950 kernels (vt_*.hip).  Internal; the public boundary is
// include/vettore_flat.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace vt {

// Candidate key of a row for one query:
//   key = orderable(rank_value(metric, raw)) << 32 | id_rank
// Ascending u64 order of `key` == the reference's (rank.total_cmp, id bytes)
// order (flat.rs:34-40): `id_rank` is order-isomorphic to the bytewise order of
// the row's id among the rows of this index.
struct Payload {
  uint32_t row;
  float raw;
};
struct Entry {
  uint64_t key;
  uint32_t row;
  float raw;
};
static_assert(sizeof(Entry) == 16 && sizeof(Payload) == 8, "layout");

constexpr uint64_t kEmptyKey = ~0ull;
constexpr int kTileRows = 32;     // rows per wave tile in the scan kernel
constexpr int kWavesPerBlock = 4;
constexpr int kMaxFusedK = 256;   // largest k one scan pass selects (320-slot wave buffer)
constexpr int kSmallK = 64;       // k <= kSmallK uses the 128-slot wave buffer
constexpr uint32_t kRowAlign = 64;  // slab row stride is a multiple of 64 floats (256 B)

// What the select kernel hands back (lives in pinned host memory: the kernel
// writes it through the PCIe mapping, the host reads it after the stream sync).
struct ResultBlock {
  int status;
  uint32_t count;
  uint32_t pad[2];
  Entry e[kMaxFusedK];
};

__host__ __device__ inline uint32_t padded_dim(uint32_t d) { return (d + kRowAlign - 1) / kRowAlign * kRowAlign; }

struct ScanArgs {
  const float *X;          // row-major rows, `stride` floats apart, 256-B aligned
  size_t stride;           // floats between rows (multiple of 64, >= padded_dim(d))
  const float *q;          // query padded with zeros to padded_dim(d) floats (device)
  const uint32_t *id_rank; // per row (indexed like rows of X); null => row index
  const uint32_t *gather;  // optional: scan rows X[gather[i * gather_stride]] for i < n
  uint32_t gather_stride;  // in uint32 units
  uint32_t n;              // rows to scan
  uint32_t d;              // dimensions used (prefix length)
  int metric;              // VT_* metric code
  int order;               // VT_ORDER_*
  uint32_t k;              // 1..kMaxFusedK
  uint64_t lo_key;         // keep only keys > lo_key when has_lo
  int has_lo;
  uint32_t q_nonzero;      // count of query coordinates != 0 (Jaccard)
  uint64_t *part_keys;     // [grid_blocks][k]: one merged list per block
  Payload *part_pay;       // [grid_blocks][k]
  int *status;             // device int; atomicMax'ed to VT_ERR_OVERFLOW on "metric overflow"
  // Batch mode (gathered scans only, grid.y = queries): query b = blockIdx.y uses
  // q + b * padded_dim(d), gather + b * batch_cap * gather_stride, scans
  // min(batch_counts[b], batch_cap) rows and writes list (b * grid.x + blockIdx.x).
  const uint32_t *batch_counts;
  uint32_t batch_cap;
  uint32_t batch_qstride;       // floats between the queries of a batch (0: padded_dim(d))
  uint32_t batch_gather_stride; // u32 words between the row lists of a batch (0: batch_cap * gather_stride)
  uint32_t tile_rows;      // 0 / 32 (default), 16 or 8: rows per wave tile, see scan_tile_rows()
  // Key-column mode (limits above kMaxFusedK): instead of keeping the k best, every scanned
  // position i writes key_out[i] (kEmptyKey if the row is excluded) and, if given, pay_out[i].
  uint64_t *key_out;
  Payload *pay_out;
  // Filter mode (launch_scan_filter alone; null / zero everywhere else): a row is kept iff it is valid by the rules above
  // and its rank word is <= *hi_word.  The kept rows go to surv_keys / surv_pay[0 .. surv_cap) at places claimed on
  // fsync[0]; a place past surv_cap raises fsync[1]; fsync[2] is the top ticket and fsync[kScanFilterLine * (1 + g)] the
  // ticket of block group g < kScanFilterGroups.  The caller hands fsync[0 .. kScanFilterSyncWords) over zeroed.  The block that draws the last ticket sorts the survivors and writes the k best to *out (status taken from
  // *status and cleared), then info[0] = kScanFilterDelivered; on overflow, or with no rows to scan, it leaves info alone.
  const uint32_t *hi_word;
  uint64_t *surv_keys;
  Payload *surv_pay;
  uint32_t surv_cap;
  uint32_t *fsync;
  ResultBlock *out;
  uint32_t *info;
};
constexpr uint32_t kScanFilterCap = 1024;       // the survivor list's room: select_topk_kernel's short-list bound
constexpr uint32_t kScanFilterGroups = 32;      // ticket words below the top one: a thousand blocks queue on none of them
constexpr uint32_t kScanFilterLine = 32;        // words between them: a 128-byte line each
constexpr uint32_t kScanFilterSyncWords = kScanFilterLine * (1 + kScanFilterGroups);
constexpr uint32_t kScanFilterDelivered = 3u;   // info[0] once the filtered K1 has written the result itself

// Rows per wave tile for a scan of n rows of dimension d on `resident_waves` waves:
// 32 when there is plenty of work per wave; 16 or 8 when there are few tiles per
// wave (a 32-row tile of 768 floats is ~25 us of one wave's load latency, so small
// corpora spread over more waves).  ntiles = ceil(n / result).
uint32_t scan_tile_rows(uint32_t n, uint32_t d, uint32_t resident_waves);

// LDS bytes per block the scan kernel needs for dimension d and list size k (0 = unsupported).
size_t scan_lds_bytes(uint32_t d, uint32_t k);
// LDS bytes per block of the hamming kernel for list size k.
size_t hamming_lds_bytes(uint32_t k);
// Partial lists a launch with `blocks` blocks produces (one per block).
inline uint32_t scan_lists(uint32_t blocks) { return blocks; }
hipError_t launch_scan(const ScanArgs &a, uint32_t blocks, hipStream_t s);

// K1m (vt_scan_multi.hip): the same scan for up to kMultiMaxQueries queries in ONE sweep of
// the corpus, exact arithmetic, any metric; contiguous rows only.  Block b leaves query q's
// list at part_keys/part_pay[((first_query + q) * grid_blocks + b) * k ..) -- the layout
// launch_batch_select reads.
constexpr uint32_t kMultiMaxQueries = 8;
struct MultiScanArgs {
  const float *X;
  size_t stride;
  const float *Q;           // [nq][ld] queries, zero padded (device)
  const uint32_t *id_rank;
  uint32_t n, d, ld;        // ld = padded_dim(d)
  int metric, order;
  uint32_t k;               // <= scan_multi_max_k(nq)
  uint32_t nq;              // queries of this launch, 1..kMultiMaxQueries
  uint32_t first_query;     // index of Q[0] among the lists of the whole batch
  uint32_t dbg;             // timing experiments (builds with -DVT_MULTI_TIMING_EXPERIMENTS only; VT_MQ_DBG): see the kernel
  uint32_t q_nonzero[kMultiMaxQueries];
  uint64_t *part_keys;
  Payload *part_pay;
  int *status;
};
uint32_t scan_multi_max_k(uint32_t nq);       // 64 for up to 4 queries per sweep, 32 for up to 8
uint32_t scan_multi_tile_rows(uint32_t nq);   // rows per wave tile (grid sizing)
size_t scan_multi_lds_bytes(uint32_t d, uint32_t k, int metric);
int scan_multi_blocks_per_cu(uint32_t d, uint32_t k, int metric);  // 3 for the slim build (d % 64 == 0, k <= 16, dot/L2/L1/Linf), else 2
hipError_t launch_scan_multi(const MultiScanArgs &a, uint32_t blocks, hipStream_t s);
// Batch mode: `blocks` per query x `nq` queries.
hipError_t launch_scan_batch(const ScanArgs &a, uint32_t blocks, uint32_t nq, hipStream_t s);
// K1n's last link (vt_scan_filter.hip): launch_scan_batch for ONE query in filter mode (ScanArgs::hi_word and the fields
// behind it).  No partial lists and no select behind it: the launch leaves the sorted result in *out itself whenever at
// most kScanFilterCap rows pass the filter.  dot-family metrics only (cosine, dot, negative dot).
hipError_t launch_scan_filter(const ScanArgs &a, uint32_t blocks, hipStream_t s);

// K3: selects the k smallest of keys[0..m) (kEmptyKey ignored) by radix select,
// writes them sorted ascending with their payloads to out->e, out->count;
// moves *dev_status into out->status and clears it for the next query.
// Keys <= lo_key are ignored when has_lo (multi-pass selection of k > kMaxFusedK).
// Lists of >= kSelTwoLevelMin keys are selected in two levels (kSelGroups blocks on
// slices, then one block); scratch_keys/scratch_pay hold kSelGroups * k entries.
// Exact k-th smallest of a key column by three 11-bit radix passes over the top 33 bits
// (the whole rank key and the top id-rank bit) -- or six passes over all 64 bits (RadixArgs.passes)
// --, all decisions taken on the device:
// launch_radix_pass for pass = 0, 1, 2 (.. 5) (hist zeroed beforehand), then launch_radix_collect
// appends every key below the resolved 33-bit prefix, and the keys sharing it, to a list
// (positions as payload rows); the caller selects the k best of that list.  A list overflow
// raises kStatusRetry in *status.
constexpr uint32_t kRadixBins = 2048;
struct RadixArgs {
  const uint64_t *keys;
  uint32_t n;
  uint32_t k;
  uint32_t *hist;        // [3][kRadixBins]
  uint32_t *list_count;  // cleared by pass 0
  uint64_t *list_keys;   // [cap]
  Payload *list_pay;     // [cap]: row = position in `keys`
  uint32_t cap;
  int *status;
  const Payload *pay_col;  // optional: per-position payload whose raw value travels with a collected key
  // 3 (default when 0): the threshold is the k-th key's top 33 bits (its whole rank and the top
  // id-rank bit), keys sharing them are all collected.  6: all 64 bits -- with unique keys the
  // collect pass leaves exactly the k smallest, however many rows tie in their rank
  // (hist then holds 6 * kRadixBins counters).
  int passes;
};
hipError_t launch_radix_pass(const RadixArgs &a, int pass, uint32_t blocks, hipStream_t s);
hipError_t launch_radix_collect(const RadixArgs &a, uint32_t blocks, hipStream_t s);

// A whole list of <= kSelListMax (key, payload) pairs in ascending key order into host-mapped
// memory: `out` receives the live entries, `head` their count and the scan status word.
struct BigResultHeader {
  int status;
  uint32_t count;
};
hipError_t launch_sort_list(const uint64_t *keys, const Payload *pay, uint32_t m, int *dev_status, BigResultHeader *head,
                            Entry *out, hipStream_t s);

// The k smallest of a key list as a device-resident, unsorted list (k <= kSelListMax): the
// candidate set of a following stage whose own ordering does not depend on this one.
constexpr uint32_t kSelListMax = 4096;
hipError_t launch_select_list(const uint64_t *keys, const Payload *pay, uint32_t m, const uint32_t *m_dev, uint32_t k,
                              uint64_t *out_keys, Payload *out_pay, hipStream_t s);
// One radix select per query in ONE launch (grid.y = queries): query y's list is keys/pay[y * m ..
// (y + 1) * m), its winners land, sorted, in the block at out + y * out_stride bytes
// ({i32 status = 0, u32 count, pad[2]} + k entries).
hipError_t launch_select_queries(const uint64_t *keys, const Payload *pay, uint32_t nq, uint32_t m, uint32_t k, void *out,
                                 uint32_t out_stride, hipStream_t s);
constexpr uint32_t kSelGroups = 16;
constexpr uint32_t kSelTwoLevelMin = 16384;
hipError_t launch_select(const uint64_t *keys, const Payload *pay, uint32_t m, uint32_t k, uint64_t lo_key, int has_lo,
                         int *dev_status, ResultBlock *out, uint64_t *scratch_keys, Payload *scratch_pay,
                         hipStream_t s, const uint32_t *m_dev = nullptr);

// K4's bit-matrix layout: per tile of 64 rows, word pair j of all 64 rows is
// contiguous -- [tile][pair][row % 64][2] u64 (an odd word count is padded with a
// zero word).  Index of word `w` of row `r`:
__host__ __device__ inline size_t hamming_word_index(uint32_t r, uint32_t w, uint32_t pairs) {
  return ((size_t)(r / 64) * pairs + (w >> 1)) * 128 + (size_t)(r % 64) * 2 + (w & 1);
}
// u64 words the tiled matrix of n rows occupies.
inline size_t hamming_matrix_words(uint32_t n, uint32_t words) {
  return (size_t)((n + 63) / 64) * ((words + 1) / 2) * 128;
}

struct HammingArgs {
  const uint64_t *bits;    // tiled layout above, hamming_matrix_words(n, words) words, zero-filled padding
  const uint64_t *qbits;   // [words] plain (device)
  const uint32_t *id_rank; // per row or null
  uint32_t n, words, pairs, d, k;  // pairs = (words + 1) / 2
  uint64_t lo_key;
  int has_lo;
  uint64_t *part_keys;
  Payload *part_pay;
  int jaccard;  // the bits are non-zero patterns and the score is distances.rs:327-347's (else the differing bits)
  // A PREFIX of the rows' bits (funnel stages under float hamming / jaccard, vector_top_k on the first d
  // coordinates, search.rs:38-73): words / pairs / d describe the prefix, tile_pairs the word pairs a tile of
  // the matrix really holds (0: the same as `pairs`).  Words behind the prefix are never counted.
  uint32_t tile_pairs;
};
hipError_t launch_hamming(const HammingArgs &a, uint32_t blocks, hipStream_t s);

// K4p (vt_hamming.hip): K4's pattern mode (non-zero bits; float hamming / jaccard scores) for up to
// kPatternMultiMax queries in one sweep of the column; k <= kSmallK; unsorted lists of k per
// (query, block) at part_keys / part_pay + ((first_query + q) * blocks + block) * k.
constexpr uint32_t kPatternMultiMax = 8;
struct PatternMultiArgs {
  const uint64_t *bits;     // the non-zero-bit column, K4's tiled layout
  const uint64_t *qbits;    // [nq][2 * pairs] (device): each query's words, an odd count padded with a zero word
  const uint32_t *id_rank;  // per row or null
  uint32_t n, words, pairs, d, k, nq, first_query;
  int jaccard;
  uint64_t *part_keys;
  Payload *part_pay;
};
size_t pattern_multi_lds_bytes();
bool pattern_multi_supports(uint32_t pairs);  // word-pair counts with an unrolled build (d up to 2 048 in steps)
hipError_t launch_pattern_multi(const PatternMultiArgs &a, uint32_t blocks, hipStream_t s);

// K4h (vt_hamming.hip): distance column + histogram, then threshold collect.
constexpr uint32_t kHammingHistMaxDim = 8191;  // (d + 1) u32 bins must fit comfortably in LDS
constexpr int kStatusRetry = 100;              // internal: the tie list overflowed, take the K4 path
struct HammingHistArgs {
  const uint64_t *bits;   // tiled layout, as for K4
  const uint64_t *qbits;  // [words]
  uint32_t n, words, pairs, d;
  uint16_t *dist;         // [n] out
  uint32_t *hist;         // [d + 1] this query's histogram (zero on entry)
  uint32_t *list_count;   // cleared here for the collect pass
};
struct HammingCollectArgs {
  const uint16_t *dist;
  const uint32_t *id_rank;
  uint32_t n, d, k;
  const uint32_t *hist;
  uint32_t *hist_next;    // the other histogram, cleared for the next query (null: nothing to clear)
  uint32_t *list_count;
  uint64_t *keys;         // [cap]
  Payload *pay;           // [cap]
  uint32_t cap;
  int *status;
  // launch_hamming_collect_multi (the queries of a group in one launch): `dist` is the
  // interleaved column dist[row][8] (u16), query q's histogram starts at hist + q * hist_stride,
  // its count is list_count[q], its list keys / pay + q * cap
  uint32_t dist_stride, hist_stride;
};
// K4h for up to kHammingMultiMax queries in ONE sweep of the bit matrix (concurrent / batched
// quantized searches): row r's eight distances land in dist[8 r .. 8 r + 8) (one 16-byte store),
// query q's histogram in hist + q * hist_stride (zeroed beforehand); list_count[0..8) is cleared
// for the collect pass.  qbits: [nq][2 * pairs] words, padding bits and the padding word clear.
constexpr uint32_t kHammingMultiMax = 8;
struct HammingMultiArgs {
  const uint64_t *bits;   // tiled layout, as for K4
  const uint64_t *qbits;  // [nq][words]
  uint32_t n, words, pairs, d, nq;
  uint16_t *dist;         // [n][8], 16-byte aligned
  uint32_t dist_stride;   // (unused: the column is interleaved)
  uint32_t *hist;
  uint32_t hist_stride;   // in u32, >= d + 1
  uint32_t *list_count;   // [nq]
};
size_t hamming_multi_lds_bytes(uint32_t d, uint32_t words, uint32_t nq);
hipError_t launch_hamming_dist_multi(const HammingMultiArgs &a, uint32_t blocks, hipStream_t s);
// the collect pass for the nq queries of a group in one sweep of the interleaved distance column
hipError_t launch_hamming_collect_multi(const HammingCollectArgs &a, uint32_t blocks, uint32_t nq, hipStream_t s);
// K3 for nq lists whose lengths were decided on the device: list y = keys / pay + y * m_stride,
// m_dev[y] entries; winners (sorted) to the block at out + y * out_stride bytes.
hipError_t launch_select_lists(const uint64_t *keys, const Payload *pay, uint32_t nq, uint32_t m_stride, const uint32_t *m_dev,
                               uint32_t k, void *out, uint32_t out_stride, hipStream_t s, bool spread = false);
size_t hamming_hist_lds_bytes(uint32_t d);
hipError_t launch_hamming_dist(const HammingHistArgs &a, uint32_t blocks, hipStream_t s);
hipError_t launch_hamming_collect(const HammingCollectArgs &a, uint32_t blocks, hipStream_t s);

// rows[n][stride] (first d columns) -> sign bits, bit j%64 of word j/64 set iff
// v[j] >= 0.0 (distances.rs:413-423).  tiled: K4's layout, else plain [n][words].
// nonzero: the bit says v[j] != 0.0 instead (the "truthiness" float hamming / jaccard compare,
// distances.rs:319-347).
hipError_t launch_sign_pack(const float *rows, size_t stride, uint32_t n, uint32_t d, uint64_t *bits, int tiled,
                            hipStream_t s, int nonzero = 0);

// *flag |= 1 if any of the first d columns of any row is non-finite.
hipError_t launch_check_finite(const float *rows, size_t stride, uint32_t n, uint32_t d, int *flag, hipStream_t s);

// dst[n][dst_stride] <- src[n][d], columns d..dst_stride-1 zero-filled.
hipError_t launch_pad_rows(const float *src, uint32_t n, uint32_t d, float *dst, size_t dst_stride, hipStream_t s);

// dst row map[2i + 1] <- src row map[2i] for i < count (map on the device; src rows are d floats,
// dst rows dst_stride floats, zero padded).
// A trickle of host rows lands from a pinned slot (layout in vt_ingest.hip: rows, their slab rows, id ranks): one launch.
hipError_t launch_land_rows(const float *stage_dev, uint32_t count, uint32_t ld, float *X, uint32_t *rank_col, uint32_t rank_first,
                            uint32_t nranks, hipStream_t s);
// Swap-delete on the slab: row `last` moves into row r (with its rank when rank_col is given), row `last` is zeroed.
hipError_t launch_swap_delete(float *X, uint32_t ld, uint32_t r, uint32_t last, uint32_t *rank_col, hipStream_t s);
hipError_t launch_gather_rows(const float *src, uint32_t d, const uint32_t *map, uint32_t count, float *dst,
                              size_t dst_stride, hipStream_t s);

// K5 / row norms for a device list of rows (derived data of mutated rows patched in place).
hipError_t launch_sign_pack_rows(const float *rows, size_t stride, const uint32_t *list, uint32_t count, uint32_t d,
                                 uint64_t *bits, hipStream_t s, int nonzero = 0);
hipError_t launch_row_sqnorms_rows(const float *X, size_t stride, const uint32_t *list, uint32_t count, uint32_t d,
                                   float *xnorm2, unsigned long long *out_bits, hipStream_t s);

// dst[pairs[2i]] = pairs[2i + 1] for i < n (pairs on the device).
hipError_t launch_scatter_u32(const uint32_t *pairs, uint32_t n, uint32_t *dst, hipStream_t s);

// Exact rerank for Metric::Cosine (search.rs:56-60 -> distances.rs:160-177):
// raw = clamp(f64_dot(q,x) / (sqrt(f64_dot(q,q)) * sqrt(f64_dot(x,x)))) as f32,
// one candidate per lane, sequential f64 sums.  Emits key/payload per candidate.
struct CosineRerankArgs {
  const float *X;
  size_t stride;
  const float *q;          // device, >= d floats
  const uint32_t *id_rank; // per row or null
  const uint32_t *gather;  // candidate rows (null => rows 0..n-1)
  uint32_t gather_stride;
  uint32_t n;              // candidates
  uint32_t d;
  uint64_t *out_keys;      // [n]
  Payload *out_pay;        // [n]
  int *status;
  // several queries in one launch (launch_cosine_rerank_batch, grid.y = queries): query y uses
  // q + y * q_stride, gather + y * gather_qstride and writes to out_keys / out_pay + y * n
  uint32_t q_stride, gather_qstride;
  // when set (single-query launches): only the first min(n, *n_dev) candidates exist, the other
  // slots get the empty key -- a candidate list whose length only the device knows
  const uint32_t *n_dev;
};
hipError_t launch_cosine_rerank(const CosineRerankArgs &a, hipStream_t s);
hipError_t launch_cosine_rerank_batch(const CosineRerankArgs &a, uint32_t nq, hipStream_t s);

// Cross-shard merge on the device: `blocks` is `world` ResultBlock prefixes
// (16-B header + k entries each, `block_bytes` apart) as gathered from the shards;
// writes the k smallest keys overall, sorted, to out->e / out->count, the shard of
// each winner to out_shard, and the OR of the shards' status words to out->status.
hipError_t launch_merge_blocks(const void *blocks, uint32_t world, uint32_t k, uint32_t block_bytes, ResultBlock *out,
                               uint32_t *out_shard, hipStream_t s);

// ---- K2: query batches on the FP32 matrix cores (vt_batch.hip) ----------------
struct BatchCand {
  float score;   // MFMA (approximate-order) dot product
  uint32_t row;
};
struct BatchScoreArgs {
  const float *X;         // slab
  size_t stride;
  const float *Q;         // [nq_pad][ld] queries, zero padded (device)
  uint32_t ld;            // padded_dim(d)
  uint32_t nq_pad;        // 32, 64, 128 or 256
  uint32_t n;             // rows covered by this launch (pass 0: sample rows)
  uint32_t n_total;       // rows in the index
  uint32_t sample_stride; // pass 0: tile i of the launch is row tile i * sample_stride
  float *sample;          // pass 0: [nq_pad][sample_rows] dense scores
  uint32_t sample_rows;
  const float *tau;       // pass 1: per-query candidate threshold
  BatchCand *cand;        // pass 1: [nq_pad][cand_cap]
  uint32_t *cand_count;   // pass 1: [nq_pad], may exceed cand_cap (overflow)
  uint32_t cand_cap;
  const float *xnorm2;    // null: score = q.x; else score = 2 q.x - xnorm2[row] (= |q|^2 - |q - x|^2)
  uint32_t debug;         // VT_BATCH_DEBUG timing experiments (results invalid when non-zero)
  const void *Qimage;     // K2b / K2s: the queries rounded to bf16, in fragment order (launch_batch_q_image / _q_image16)
  const void *Xshadow;    // K2s only: the rows rounded to bf16, in fragment order (shadow_index; launch_shadow_build)
  uint32_t stages;        // K2s only: depth of the LDS ring for this launch -- 4 or 5; 0: the library's default (VT_SHADOW_STAGES)
};
uint32_t batch_rows_per_block(uint32_t nq_pad);
hipError_t launch_batch_scores(const BatchScoreArgs &a, bool dense, uint32_t blocks, hipStream_t s);
// K2b (vt_batch_bf16.hip): the same two passes with both operands rounded to bf16 on the way
// into v_mfma_f32_32x32x16_bf16 -- HBM-bound instead of FP32-MFMA-bound.  Always 256 query
// columns (nq_pad = 64, 128 or 256 -- batch_bf16_pad --, the padding ones zero); a.Qimage from launch_batch_q_image.
uint32_t batch_bf16_rows_per_block();
size_t batch_bf16_image_bytes(uint32_t ld);
uint32_t batch_bf16_pad(uint32_t nq);  // columns a batch of nq <= 256 queries is padded to: 64, 128 or 256
hipError_t launch_batch_q_image(const float *Q, uint32_t ld, uint32_t nq_pad, void *image, hipStream_t s);
hipError_t launch_batch_scores_bf16(const BatchScoreArgs &a, bool dense, uint32_t blocks, hipStream_t s);
// K2s (vt_batch_shadow.hip): K2b fed from a bf16 image of the rows kept beside the slab -- half the
// HBM bytes, no conversion in the pass, both operands through LDS as whole fragments of
// v_mfma_f32_16x16x32_bf16.  Same rounding as K2b's (round to nearest even), so the same bound applies.
// Element (row, col) of the image of rows `ld` floats long (ld a multiple of 64) sits at
// [row / 16][col / 32][(col / 8) % 4][row % 16][col % 8]: 1 KiB per (16 rows, 32 columns), lane
// 16 g + r of a wave holding row r, k = 8 g .. 8 g + 7 -- one A operand.
__host__ __device__ inline size_t shadow_index(uint32_t row, uint32_t col, uint32_t ld) {
  return ((size_t)(row >> 4) * (ld >> 5) + (col >> 5)) * 512 + ((col >> 3) & 3u) * 128 + (row & 15u) * 8 + (col & 7u);
}
uint32_t batch_shadow_rows_per_block();
size_t shadow_elems(uint32_t rows, uint32_t ld);   // bf16 elements of an image of `rows` rows (padded to whole block tiles)
size_t batch_shadow_image_bytes(uint32_t ld);      // the query image of up to 256 queries
// rows [0, rows_src) of X -> image rows [0, rows_img) (rows_img a multiple of 256; rows >= rows_src zero)
hipError_t launch_shadow_build(const float *X, size_t stride, uint32_t rows_src, uint32_t rows_img, uint32_t ld, void *img,
                               hipStream_t s);
// the rows of a device list (mutated rows patched in place)
hipError_t launch_shadow_rows(const float *X, size_t stride, const uint32_t *list, uint32_t count, uint32_t ld, void *img,
                              hipStream_t s);
hipError_t launch_batch_q_image16(const float *Q, uint32_t ld, uint32_t nq_pad, void *image, hipStream_t s);
hipError_t launch_batch_scores_shadow(const BatchScoreArgs &a, bool dense, uint32_t blocks, hipStream_t s);
// the sample pass in its r05 form: per query the best score of every 64-row group of the sampled tiles --
// a.sample is [nq_pad][a.sample_rows], a.sample_rows = batch_shadow_sample_groups(tiles of the launch)
hipError_t launch_batch_sample_maxima_shadow(const BatchScoreArgs &a, uint32_t blocks, hipStream_t s);
uint32_t batch_shadow_sample_groups(uint32_t sample_tiles);
// tau[b] for the nq_real real queries; +inf for the padding columns b >= nq_real.
// (K2s since r05: the threshold from the sample's group maxima, [nq][groups] with groups <= 1 024)
hipError_t launch_sample_tau_groups(const float *maxima, uint32_t groups, uint32_t nq, uint32_t nq_real, uint32_t rank, float *tau,
                                    hipStream_t s);
hipError_t launch_sample_tau(const float *sample, uint32_t sample_rows, uint32_t nq, uint32_t nq_real, uint32_t rank,
                             float *tau, hipStream_t s);
// xnorm2[i] = (f32) sum_j x_ij^2 (f64 accumulation); *out_bits = bit pattern of
// the f64 maximum over the rows (zero it first).
hipError_t launch_row_sqnorms(const float *X, size_t stride, uint32_t n, uint32_t d, float *xnorm2,
                              unsigned long long *out_bits, hipStream_t s);
// Block b: the k smallest of keys[b][0..m) sorted ascending -> out[b][0..k), out_count[b].
// (`ex`: see batch_select_kernel -- the host-side numbers of a query batch leave with the lists)
struct BatchExport {
  const uint32_t *cand_count;  // [nq] -> cand_count_out
  uint32_t *cand_count_out;
  const float *tau;            // [nq] -> tau_out (null: not wanted)
  float *tau_out;
  int *status;                 // -> *status_out, then 0
  int *status_out;
};
hipError_t launch_batch_select(const uint64_t *keys, const Payload *pay, uint32_t nq, uint32_t m, uint32_t k, Entry *out,
                               uint32_t *out_count, hipStream_t s, const BatchExport *ex = nullptr);

// K6b: exact f64 cosine (distances.rs:160-177) of the first d coordinates of
// EVERY row against the query, fused top-k -- stage 1 of funnel_search on a
// cosine collection (collection.ex:245-260 -> search.rs:56-60).
struct CosineScanArgs {
  const float *X;
  size_t stride;
  const float *q;          // device, padded with zeros to padded_dim(d)
  double qq;               // f64_dot(q, q) over the first d coordinates (sequential, host)
  const uint32_t *id_rank;
  uint32_t n, d, k;
  uint64_t lo_key;
  int has_lo;
  uint64_t *part_keys;     // [grid_blocks][k]
  Payload *part_pay;
  int *status;
  uint64_t *key_out;       // key-column mode, as in ScanArgs
};
size_t cosine_scan_lds_bytes(uint32_t d, uint32_t k);
hipError_t launch_cosine_scan(const CosineScanArgs &a, uint32_t blocks, hipStream_t s);

// A group's sweep: stage 1 of funnel_search (collection.ex:245-260 -> search.rs:56-60) for up to kGroupSweepMax callers in
// ONE sweep of the rows' first d coordinates.  Every lane owns a row, read through a 64 x 32-float LDS panel
// (vt_panel.cuh); the queries are wave-uniform and come through the scalar cache.  Two kernels serve it:
//   K6bm (cosine collections): x.x once and q.x per query as sequential f64 chains (distances.rs:160-177) -- the values
//     are K6b's, bit for bit.  Reads Qd and qq.  No per-wave top-k buffers (eight would not fit beside the row panels).
//   K1p (the dot / L2 / L1 / Linf families): the index's own metric in K1's arithmetic -- eight separately rounded
//     products per chunk, the horizontal add in the lane order `order`, acc += chunk sum, the scalar tail
//     (distances.rs:197-262).  Reads Q, q_stride, metric and order.
// Both score "larger is better" -- raw for cosine, -rank_value for the others -- and run in two modes:
//   dense (`sample` set): the scores of every `sample_stride`-th tile of 64 rows go to sample[q * sample_rows + i]
//     (launch_sample_tau turns them into one threshold per query); with `sample_maxima` only the BEST score of every
//     sampled tile: sample[q * sample_rows + tile], sample_rows = the launch's tiles (launch_sample_tau_groups);
//   sweep: every (query, row) with score >= tau[q] is appended to the query's list as (key, {row, raw}) -- key as in the
//     single kernel -- cand_count[q] counting ALL of them; the host checks k <= count <= cap (else that query takes
//     the single path) and launch_select_lists cuts each list to its k best.
constexpr uint32_t kGroupSweepMax = 8;
struct GroupSweepArgs {
  const float *X;
  size_t stride;
  const float *Q;            // K1p: [kGroupSweepMax][q_stride] f32 queries (device; unused rows readable), q_stride % 8 == 0
  uint32_t q_stride;
  const double *Qd;          // K6bm: [kGroupSweepMax][padded_dim(d)] device: the queries' prefixes as f64 (exact), unused rows zero
  double qq[kGroupSweepMax];  // K6bm: f64_dot(q, q) over the first d coordinates (sequential, host)
  const uint32_t *id_rank;
  uint32_t n, d, nq;
  int metric, order;         // K1p runs the dot / L2 / L1 / Linf families, K6bm cosine; not the pattern metrics
  float *sample;             // dense mode when set
  uint32_t sample_stride, sample_rows;
  uint32_t sample_maxima;
  const float *tau;          // [nq] sweep mode
  uint64_t *cand_keys;       // [nq][cand_cap]
  Payload *cand_pay;
  uint32_t *cand_count;      // [nq], zeroed by the caller
  uint32_t cand_cap;
  int *status;
};
bool prefix_multi_supports(int metric);
hipError_t launch_cosine_scan_multi(const GroupSweepArgs &a, uint32_t blocks, hipStream_t s);
hipError_t launch_prefix_multi(const GroupSweepArgs &a, uint32_t blocks, hipStream_t s);
size_t group_sweep_lds_bytes();
// resident blocks per CU the launch is sized for: K1p's 2 (three or four blocks of the narrow panel fit a CU, and are
// slower: DESIGN_APPENDIX A.15); 0 -- the context's default -- where K6bm runs
inline int group_sweep_blocks_per_cu(int metric) { return prefix_multi_supports(metric) ? 2 : 0; }
// the kernel that serves a.metric
inline hipError_t launch_group_sweep(const GroupSweepArgs &a, uint32_t blocks, hipStream_t s) {
  return prefix_multi_supports(a.metric) ? launch_prefix_multi(a, blocks, s) : launch_cosine_scan_multi(a, blocks, s);
}

// Diagnostic (vt_device_read_peak): one pass of the bare LDS-DMA read stream over the whole 384-KiB tiles of
// `buf` (read_peak_bytes(bytes) of it), `blocks` blocks of 512 threads -- one per CU; launch_peak_fill puts
// random floats there first.
hipError_t launch_read_peak(const void *buf, size_t bytes, float *sink, uint32_t blocks, hipStream_t s);
size_t read_peak_bytes(size_t bytes);
hipError_t launch_peak_fill(void *buf, size_t bytes, hipStream_t s);

// K9: MaxSim / ColBERT scoring (multi_vector.rs:65-88) of a chunk of documents, for multi_vector_top_k / _score.
// The documents' vectors are one row-major matrix X (`stride` floats apart); document i owns rows
// [doc_off[i], doc_off[i + 1]).  A wave takes one document at a time, a lane one of its vectors, and walks
// the query vectors of the launch's panel -- staged in LDS -- eight at a time: every (query vector,
// document vector) pair is one lane's own chain in the reference's order (distances.rs:42-68 for eight
// metrics, :160-185 for cosine), the maximum over the document's vectors a wave reduction, the sum over the
// query vectors one sequential f32 chain in query order.  Query vectors that do not fit in one panel go in
// several launches over the same documents (panel_q0 > 0): the running sum and status live in
// total / status between them.  The launch that holds the last query vector writes one key per document:
// (~total_cmp(score) << 32) | id rank -- the smallest key is the best hit (collect_from_keys) --, and on an
// error kEmptyKey and (row << 8 | status) into *first_error (atomicMin: the earliest document wins).
constexpr int kErrScoreOverflow = 10;  // VT_ERR_SCORE_OVERFLOW
struct MaxSimArgs {
  const float *X;           // document vectors; unused when nq == 0
  size_t stride;            // floats between rows (>= d)
  const uint32_t *doc_off;  // [ndoc + 1] rows of each document (relative to X); unused when nq == 0
  uint32_t ndoc;
  const float *Q;           // [nq][q_stride] query vectors (device), zero-padded, q_stride % 8 == 0
  uint32_t q_stride;
  uint32_t nq;              // query vectors of the call (0: every document scores 0.0)
  uint32_t panel_q0, panel_qn;  // this launch's query vectors [panel_q0, panel_q0 + panel_qn)
  uint32_t d;
  int metric, order;
  const double *qnorm;      // cosine: [nq] sqrt(f64 q.q)  (launch_maxsim_norms)
  const double *tnorm;      // cosine: per row of X  sqrt(f64 t.t)
  float *total;             // [ndoc] running sum between panel launches (unused with one panel)
  int *status;              // [ndoc] 0, kErrOverflow or kErrScoreOverflow between panel launches
  const uint32_t *id_rank;  // [ndoc]
  uint32_t row0;            // the chunk's first document within the call (payload row = row0 + i)
  uint64_t *keys;           // [ndoc]
  Payload *pay;             // [ndoc] {row0 + i, score}
  unsigned long long *first_error;  // (row << 8 | status), ~0 when none
  // A resident store's slot list (vt_mv, K9r below): document i owns rows [doc_off[i], doc_off[i] + doc_cnt[i]) -- its
  // documents are not adjacent.  Null (every stateless launch): doc_off[i + 1] - doc_off[i] rows.
  const uint32_t *doc_cnt;
};
// Query vectors per panel for dimension d (0: a single query vector does not fit in LDS) and the LDS bytes of a panel.
uint32_t maxsim_panel_rows(uint32_t d, uint32_t *q_stride);
size_t maxsim_lds_bytes(uint32_t panel_qn, uint32_t q_stride);
hipError_t launch_maxsim(const MaxSimArgs &a, uint32_t blocks, hipStream_t s);
// norms[i] = sqrt(f64 sum of x[i][j]^2, j in order) for n rows `stride` floats apart (distances.rs:166-167)
hipError_t launch_maxsim_norms(const float *X, size_t stride, uint32_t n, uint32_t d, double *norms, hipStream_t s);

// K9r (vt_maxsim_resident.hip): K9's arithmetic for the documents of a resident store (host/vt_mvstore.h), which are a
// slot list over one slab: MaxSimArgs with doc_cnt set, stride = round_up(d, 4), and -- cosine -- tnorm the store's norm
// column.  A wave stages a document's rows through LDS, `1 << tile_log2` at a time, with coalesced 16-byte loads; a lane is
// (row of the tile, group of eight query vectors), 64 >> tile_log2 groups side by side.  maxsim_resident_plan chooses the
// tile by the call's query vectors and says how many of them one panel holds; false: K9r does not serve the call (no
// query vector, float Hamming / Jaccard, a dimension whose tiles do not fit in LDS) -- launch_maxsim does, over the same slab.
struct MaxSimResidentPlan {
  uint32_t tile_log2;  // 6, 5 or 4
  uint32_t ld;         // floats between the rows of an LDS tile (ld / 4 odd)
  uint32_t q_stride;   // round_up(d, 8), as K9's
  uint32_t panel;      // query vectors per launch, a multiple of a pass (8 * (64 >> tile_log2))
};
bool maxsim_resident_plan(uint32_t d, uint32_t nq, int metric, MaxSimResidentPlan *out);
size_t maxsim_resident_lds_bytes(uint32_t panel_qn, uint32_t q_stride, const MaxSimResidentPlan &p);
hipError_t launch_maxsim_resident(const MaxSimArgs &a, const MaxSimResidentPlan &p, uint32_t blocks, hipStream_t s);
// K9rb (vt_maxsim_batch.hip): K9r over many query sets in one launch.  The sets' query vectors are one matrix of slots,
// each set padded with zero rows to whole groups of eight; desc[g] describes group g (slots [8 g, 8 g + 8)): the set it
// belongs to and, in `info`, its real slots (1..8), kMaxSimBatchFirst / kMaxSimBatchLast at the set's first / last group.
// blockIdx.y picks groups[y]: a panel -- descriptors [desc0, desc0 + ndesc), whole sets, staged in LDS -- and the
// document list it is scored against, entries [list0, list0 + ndoc) of doc_first / doc_cnt / doc_rank.  Document i of
// the list leaves set s's key and payload {i, score} at keys / pay[s * key_stride + i], or kEmptyKey there and
// (i << 8 | status) in first_error[s] (atomicMin).  host/vt_mvbatch.h packs sets into panels; the tile and the slots a
// panel may hold are maxsim_resident_plan's, asked for the slots of the largest panel wanted.
constexpr uint32_t kMaxSimBatchFirst = 1u << 8, kMaxSimBatchLast = 1u << 9;
struct MaxSimBatchDesc {
  uint32_t set, info;
};
struct MaxSimBatchGroup {
  uint32_t desc0, ndesc, list0, ndoc;
};
struct MaxSimBatchArgs {
  const float *X;                  // the store's slab
  size_t stride;                   // round_up(d, 4)
  const float *Q;                  // [slots][q_stride], zero-padded rows and zero pad slots
  uint32_t q_stride, d;
  int metric, order;
  const double *qnorm;             // cosine: [slots]
  const double *tnorm;             // cosine: per row of X
  const MaxSimBatchGroup *groups;  // [ngroups]
  const MaxSimBatchDesc *desc;
  const uint32_t *doc_first, *doc_cnt, *doc_rank;
  uint32_t ngroups;                // gridDim.y (<= 65535)
  uint32_t max_ndesc;              // the longest panel of the launch: sizes the LDS request
  uint32_t key_stride;             // >= every list's ndoc
  uint64_t *keys;
  Payload *pay;
  unsigned long long *first_error;  // [sets], ~0 when none
};
hipError_t launch_maxsim_batch(const MaxSimBatchArgs &a, const MaxSimResidentPlan &p, uint32_t blocks, hipStream_t s);
// Compaction of a store: row j of outX / out_norms = row src[j] of X / norms (`stride` floats a row, a multiple of 4).
hipError_t launch_mv_compact(const float *X, const double *norms, const uint32_t *src, uint32_t rows, uint32_t stride,
                             float *outX, double *out_norms, hipStream_t s);

// K10: MUVERA fixed-dimensional encoding (muvera.rs:26-74) of a chunk of vector sets, for vt_muvera_encode.
// The chunk's vectors are one row-major matrix X, d floats apart; set i owns rows [set_off[i], set_off[i + 1]) (a set
// the host refused owns none and keeps its zero row).  launch_muvera_table writes the call's weights and signs once;
// launch_muvera_encode runs one wave per (set, group of rg repetitions) over the set's vectors in input order and
// updates the f32 slots of `full` in place (zeroed by the host); launch_muvera_sketch folds `full` into the final
// dimension.  "encoding overflow" lands in status[set].
constexpr int kErrEncodingOverflow = 28;             // VT_ERR_ENCODING_OVERFLOW
constexpr uint32_t kMuveraLdsPartitions = 4096;      // partition counts a wave keeps in LDS (document mode)
constexpr uint32_t kMuveraMaxDim = 16384;            // the staged vector: 64 KiB of LDS at most
struct MuveraArgs {
  const float *X;           // [rows][d]
  const uint32_t *set_off;  // [nsets + 1]
  uint32_t nsets;
  uint32_t d, R, k, pd;     // dimension, repetitions, SimHash projections, projection dimension
  uint32_t C;               // table columns per (repetition, coordinate): k, plus pd unless identity
  int identity;             // pd == d: the coordinates themselves (muvera.rs:141-146)
  int mode;                 // 0 query (sum), 1 document (running average)
  const float *table;       // [R][d][C]  (launch_muvera_table); unused when C == 0
  uint32_t rg, groups;      // repetitions per wave (muvera_reps_per_wave), waves per set = ceil(R / rg)
  size_t rep_size, out_size;  // 2^k * pd, R * rep_size
  float *full;              // [nsets][out_size]
  uint32_t *counts;         // document mode with more than kMuveraLdsPartitions partitions: [nsets][R][2^k], zeroed; else null
  int *status;              // [nsets], zeroed
};
uint64_t muvera_hash4(uint64_t a, uint64_t b, uint64_t c, uint64_t d);  // muvera.rs:219-225 (host: the sketch's slot lists)
uint32_t muvera_reps_per_wave(uint32_t R, uint32_t k, uint32_t C, int mode);
size_t muvera_lds_bytes(const MuveraArgs &a);
hipError_t launch_muvera_table(uint64_t seed, uint32_t R, uint32_t d, uint32_t k, uint32_t C, float *table, hipStream_t s);
hipError_t launch_muvera_encode(const MuveraArgs &a, hipStream_t s);
// K10s: K10 over the slab of a resident multi-vector store (vt_mv_encode_documents, vt_mv_fde_sync).  Set i is the
// doc_cnt[i] rows from row doc_first[i] on of a.X, `stride` floats apart (a multiple of 4 >= a.d, so every row starts on
// 16 bytes; the pad is zero and never enters a sum); a.set_off is not read.  Only the addressing and the load of a vector
// into LDS differ from K10: the arithmetic behind it is the one device function both kernels call, so the bits are K10's.
struct MuveraSlabArgs {
  MuveraArgs a;
  const uint32_t *doc_first;  // [nsets]
  const uint32_t *doc_cnt;    // [nsets]  (0: the set keeps its zero row)
  uint32_t stride;
};
size_t muvera_slab_lds_bytes(const MuveraSlabArgs &a);
hipError_t launch_muvera_encode_slab(const MuveraSlabArgs &a, hipStream_t s);
// out[set][s] = the sequential f32-rounded signed sum of full[set][i] over list[off[s] .. off[s + 1]) (low 31 bits: i,
// increasing; bit 31: sign -1)   muvera.rs:180-200
hipError_t launch_muvera_sketch(const float *full, size_t out_size, uint32_t nsets, uint32_t final_dim, const uint32_t *off,
                                const uint32_t *list, float *out, int *status, hipStream_t s);

// ---- K11 (vt_hnsw.hip): HNSW traversals, one wave each (hnsw.rs:292-434) ----------------------------------------------
// The device mirror of a graph (host/vt_hnswgraph.h): nodes are named by their slab rows.  The list of row r on layer 0
// is adj0[r * (m0 + 1)] = its length, then its rows; on layer l >= 1 (level[r] >= l) the same at
// upper[upoff[r] + (l - 1) * (m + 1)].
struct HnswDev {
  const float *X;         // the slab: `stride` floats a row (a multiple of 4), the pad zero and never read
  size_t stride;
  uint32_t d;
  const uint32_t *adj0;
  const uint32_t *level, *upoff, *upper;
  uint32_t m, m0;
};
constexpr int kHnswRetry = 100;           // internal: the traversal outgrew its scratch, run it again with more
constexpr uint32_t kHnswLdsDim = 4096;    // rows up to this long are staged through LDS, the query beside them
struct HnswTravArgs {
  HnswDev g;
  int metric, order;      // VT_L2, VT_COSINE (the f32 dot, rank 1 - raw) or VT_INNER_PRODUCT
  int mode;               // 0: search, 1: an insert's descent
  const float *Q;         // traversal t's query: Q + query(t) * q_stride, 16-byte aligned; query(t) = qmap ? qmap[t] : t
  uint32_t q_stride;
  const uint32_t *qmap;
  uint32_t entry, top;    // the graph's entry row and its level
  uint32_t node_level;    // insert: the new node's level
  uint32_t ef;            // of the search_layer calls, already cut to the node count
  uint32_t cap, hshift;   // scratch entries per slot (a power of two >= 2) and 32 - log2(2 * cap)
  uint64_t *scratch;      // [slots][3 * cap]
  // per query `out_stride` words: {status, n}, then -- search -- n results (row, raw bits), or -- insert -- n layers,
  // layer l at word 2 + l * (1 + 2 * ef): its count, then (row, rank distance bits) each
  uint32_t *out;
  uint32_t out_stride;
  uint32_t tt, ld;        // hnsw_tile_plan: rows of the LDS tile (0: nothing is staged) and floats between them
};
void hnsw_tile_plan(uint32_t d, uint32_t stride, uint32_t *tt, uint32_t *ld);
size_t hnsw_lds_bytes(uint32_t d, uint32_t tt, uint32_t ld);
hipError_t launch_hnsw_traverse(const HnswTravArgs &a, uint32_t nslots, hipStream_t s);
struct HnswPatch {
  uint64_t dst;      // index into the array `target` names: 0 adj0, 1 upper, 2 level, 3 upoff
  uint32_t val, target;
};
hipError_t launch_hnsw_patch(const HnswPatch *p, uint32_t n, uint32_t *adj0, uint32_t *upper, uint32_t *level, uint32_t *upoff,
                             hipStream_t s);
// K11c: compaction of a slab and its mirror into fresh buffers (host/vt_hnswplan.h: the plan).  New row i is old row
// src[i] (ascending): its slab row and level are copied, its upper-layer lists move to new_upoff[i], and every list
// entry -- the mirror names nodes by rows -- goes through remap[old row] = new row.  Behind a list's count its entries,
// behind them zeros up to the list's stride: the new buffers hold nothing uninitialised below rows / new_upper.
// What the old buffers hold is not trusted: nothing outside them is read, and what should not be there is reported in
// status[0 .. 4), one word per guard (0 or 1, plain stores), with kHnswNoRow or an empty list in its place.
constexpr uint32_t kHnswNoRow = 0xFFFFFFFFu;   // remap[] of a dead row
enum : uint32_t {
  kHnswCompactBeyond = 0,  // a list entry >= old_rows (checked before remap[] is read)
  kHnswCompactDead = 1,    // a list entry that names a dead row
  kHnswCompactCount = 2,   // a list's count above m0 / m (clamped)
  kHnswCompactShape = 3,   // src[], a level or an upper-layer offset of the old mirror that disagrees with the plan
  kHnswCompactGuards = 4
};
struct HnswCompactArgs {
  // the old slab and mirror: old_rows rows used, old_upper words of upper-layer lists used
  const float *X;
  const uint32_t *adj0, *level, *upoff, *upper;
  uint32_t old_rows;
  uint64_t old_upper;
  uint32_t stride, m, m0;  // floats a row (a multiple of 4), entries per upper-layer list, per layer-0 list
  // the plan: `rows` survivors, new_upper words of upper-layer lists behind them
  const uint32_t *src, *new_upoff;
  uint32_t rows;
  uint64_t new_upper;
  uint32_t *remap;         // [old_rows], filled here
  // the new buffers: at least `rows` rows, new_upper words
  float *outX;
  uint32_t *out_adj0, *out_level, *out_upoff, *out_upper;
  uint32_t *status;        // [kHnswCompactGuards], zeroed here
};
hipError_t launch_hnsw_compact(const HnswCompactArgs &a, hipStream_t s);

// ---- K15 (vt_hnsw_stage.hip): the staged searches' scores over an HNSW slab where it lies ------------------------------
// Both kernels write keys[i] / pay[i] for every scanned position i, in the key-column convention at the top of this file:
// kEmptyKey for a dead row (id_rank[row] == kHnswNoRow), for a list entry that names no row of the slab, and for a pair
// whose raw value is NaN.  id_rank: [rows], the position of the row's external id in the bytewise order of the live ids.
// Both launchers return hipSuccess without launching when there is nothing to scan.
//
// K15b: position = row, for rows [0, rows).  raw = rank = packed_hamming(compress_sign_bits(row), the query's) as f32.
// qwords: the query's sign bits in the kernel's order, hnsw_stage_qword_count(d) words from hnsw_stage_qwords(): bit
// e % 256 / 4 of word 4 * (e / 256) + e % 4 is set iff q[e] >= 0.0f, every other bit clear.
struct HnswStageBitsArgs {
  const float *X;          // the slab: `stride` floats a row (a multiple of 4, >= d), 16-byte aligned; the pad is not looked at
  size_t stride;
  uint32_t d, rows;
  const uint32_t *id_rank;
  const uint64_t *qwords;
  uint64_t *keys;          // [rows]
  Payload *pay;            // [rows]
};
inline size_t hnsw_stage_qword_count(uint32_t d) { return 4 * (((size_t)d + 255) / 256); }
void hnsw_stage_qwords(const float *q, uint32_t d, uint64_t *out);
hipError_t launch_hnsw_stage_bits(const HnswStageBitsArgs &a, hipStream_t s);
// K15p: vector_top_k's value on the first p coordinates, the query on the left; metric VT_L2, VT_COSINE (the f64 cosine,
// both norms over the prefix) or VT_INNER_PRODUCT.  Position i is row list[i], or row i when list is null (n <= rows).
struct HnswStageScoreArgs {
  const float *X;
  size_t stride;
  uint32_t d, rows;        // the slab's dimension and its used rows
  uint32_t p;              // 1 .. d
  const float *q;          // at least round_up(p, 4) floats, 16-byte aligned (device)
  double qq;               // cosine: f64_dot(q, q) over the prefix (distances.rs:179-185)
  const uint32_t *id_rank;
  const uint32_t *list;
  uint32_t n;              // positions
  int metric, order;
  uint64_t *keys;          // [n]
  Payload *pay;            // [n]
  int *status;             // raised to VT_ERR_OVERFLOW by a NaN raw value
  uint32_t tt, ld;         // (the launcher's: rows of the LDS tile, 0 when nothing is staged, and floats between them)
};
hipError_t launch_hnsw_stage_score(const HnswStageScoreArgs &a, hipStream_t s);

// ---- K12 (vt_mmr.hip): MMR reranking (vettore_distance.ex:416-519), one step kernel queued once per round ------------
// A call solves `nprob` problems over one row matrix.  Problem p owns entries [off, off + n) of the per-candidate arrays;
// candidate i of it is row rows[off + i] of X with the f64 relevance rel[off + i].  launch_mmr_step(a, t, ...) is queued
// for t = 0 .. max_p(kk_p), kk_p = min(k_p, n_p), back to back on one stream; the grid is (blocks, nprob), nothing waits
// inside a launch.  Launch t of problem p:
//   phase A (1 <= t <= kk): every block reduces the blocks' partials of launch t - 1 -- the largest score, the smallest
//     candidate on a tie (Enum.max_by keeps the first maximum), and the smallest candidate whose pair failed.  A failed
//     pair makes the problem's status kErrOverflow for good (the blocks hand the failure on through their partials);
//     otherwise block 0 appends the winner to order[off + t - 1] and sets count[p] = t;
//   phase B (t < kk, nothing failed): the winner's row is staged in LDS (rows longer than lds_dim floats are read where
//     they lie); every live candidate is scored against it by one lane -- compute(metric, candidate, winner) in the
//     reference's f32 order for `order`, f64 recovery included, then pair_similarity's f64 value --, its running
//     maximum red[off + i] updated (the first similarity replaces it), its score alpha * rel - (1 - alpha) * red formed
//     in f64 without contraction; the block's best (score, candidate) and first failed candidate go to
//     partial[t & 1][p][block].  At t = 0 there is no winner: the redundancy is 0.0, the candidates come alive and --
//     cosine -- their f64 norms are filed.
// Partials alternate by launch parity: no block of a launch reads what another block of the same launch writes.
constexpr uint32_t kMmrNone = 0xffffffffu;
constexpr uint32_t kMmrLdsDim = 4096;        // winners up to this long are staged in LDS (as K11's rows)
constexpr uint32_t kMmrBlockRows = 256;      // candidates a block takes per pass: one per thread
constexpr uint32_t kMmrMaxBlocks = 64;       // blocks per problem at most (one wave reduces their partials)
struct MmrProblem {
  uint32_t off, n, kk, pad;
  double alpha;
};
struct MmrPartial {
  double score;
  uint32_t best, failed;  // candidates, kMmrNone: none
};
static_assert(sizeof(MmrProblem) == 24 && sizeof(MmrPartial) == 16, "layout");
struct MmrArgs {
  const float *X;          // rows `stride` floats apart, 16-byte aligned (stride % 4 == 0)
  size_t stride;
  uint32_t d;
  int metric, order;
  const MmrProblem *prob;  // [nprob]
  const uint32_t *rows;    // per candidate
  const double *rel;       // per candidate
  double *red;             // per candidate: the running maximum similarity to the chosen
  double *norm;            // per candidate (cosine): sqrt(f64 x.x)
  uint32_t *live;          // per candidate: 1 until chosen
  MmrPartial *partial;     // [2][nprob][blocks]
  uint32_t *order_out;     // per candidate slot: problem p's choices at off ..
  uint32_t *count;         // [nprob] choices made
  int *status;             // [nprob] 0 or kErrOverflow
  uint32_t block_rows;     // candidates per block and pass (<= kMmrBlockRows)
  uint32_t lds_dim;        // staging limit in floats
};
size_t mmr_lds_bytes(uint32_t d, uint32_t lds_dim);
hipError_t launch_mmr_step(const MmrArgs &a, uint32_t t, uint32_t blocks, uint32_t nprob, hipStream_t s);

// normalize_l2 (distances.rs:350-361) on rows: out = (x / sqrt(f64 sum x^2)) as f32.
hipError_t launch_normalize_l2(const float *in, uint32_t n, uint32_t d, float *out, hipStream_t s);

// ---- K14 (vt_prepare.hip): prepare rows -- finite check, normalization and sign bits of a matrix in one launch ---------
// Row r of `in` (rows ld_in floats apart, the first d columns count) is checked for non-finite values, normalized as
// `mode` says (distances.rs:350-410, the reference's order of operations: serial f64 sums in index order, true f64
// divisions) and written to row r of `out` (rows ld_out floats apart; columns past d are not touched); `out` may be `in`
// when ld_out == ld_in.  words != nullptr: the sign bits of the written values (compress_sign_bits, :413-423) go to
// words[r][(d + 63) / 64].  A row holding a non-finite value is left unwritten, values and words, and *first_refused
// (set to kPrepNoRow by the caller beforehand) is lowered to its index by atomicMin; all other rows are written.
constexpr uint32_t kPrepWaveRows = 64;    // rows of a wave's tile: one lane owns one row's serial chains
constexpr uint32_t kPrepPanel = 64;       // columns a tile passes through LDS at a time
constexpr uint32_t kPrepBlockRows = 128;  // rows per block = threads per block: two waves, each with its own LDS image
constexpr int kPrepInFlight = 32;         // 256-byte runs a wave loads before it converts and stores them
constexpr uint32_t kPrepNoRow = 0xffffffffu;
enum { kPrepNone = 0, kPrepL2 = 1, kPrepZscore = 2, kPrepMinmax = 3 };  // = VT_NORM_* (include/vettore_flat.h)
struct PrepareArgs {
  const float *in;
  size_t ld_in;
  float *out;
  size_t ld_out;
  uint64_t *words;          // [n][(d + 63) / 64], or nullptr
  uint32_t *first_refused;  // one word
  uint32_t n, d;
};
hipError_t launch_prepare_rows(const PrepareArgs &a, int mode, hipStream_t s);

// ---- K1q (vt_sketch.hip): a lone dot-family or L2-family search over an int8 sketch of the rows ----------------------
// Row r is kept as X_r = round(x_r / s_r) in int8 with s_r = max_i |x_ri| / 127, beside two f32 bounds rounded up:
// rho_r >= ||x_r - s_r X_r|| (the residual, summed in f64) and nu_r >= s_r ||X_r||.  Layout, per tile of 64 rows: the
// rows' 16-byte chunk c is one 1-KiB run ((tile * (nch + 1) + c) * 1024 + (r % 64) * 16), c < nch = ld8 / 16, and the
// tile ends with one more run of {s, rho, nu, 0} per row -- a wave streams a tile, metadata included, in whole 1-KiB loads.
// The column of an L2 / squared-L2 handle keeps xx_r >= ||x_r||^2 in that fourth dword (f32, rounded up, of the f64 sum
// times 1 + 2^-30; launch_sketch_build_xx / launch_sketch_rows_xx): ||q - x||^2 = ||q||^2 + ||x||^2 - 2 q.x turns the dot's
// interval into the distance's.  Every other handle's fourth dword stays zero.
constexpr uint32_t kSketchTileRows = 64;
constexpr uint32_t kSketchMaxDim = 32768;  // (K1q's query image sits in LDS; and d * 127^2 stays far below 2^31)
__host__ __device__ inline uint32_t sketch_ld8(uint32_t d) { return (d + 127) / 128 * 128; }
__host__ __device__ inline size_t sketch_offset(uint32_t row, uint32_t chunk, uint32_t nch) {
  return ((size_t)(row / kSketchTileRows) * (nch + 1) + chunk) * 1024 + (size_t)(row % kSketchTileRows) * 16;
}
// bytes of a sketch covering `rows` rows (whole tiles)
inline size_t sketch_bytes(uint32_t rows, uint32_t d) {
  const size_t tiles = ((size_t)rows + kSketchTileRows - 1) / kSketchTileRows;
  return tiles * ((size_t)sketch_ld8(d) / 16 + 1) * 1024;
}
// Rows [0, rows_img) of the image (rows at or past n_src are zero rows); *max_norm (the bits of a non-negative f64,
// atomicMax'ed) is raised to the largest nu + rho, an upper bound of every row's norm.
hipError_t launch_sketch_build(const float *X, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d, void *img,
                               unsigned long long *max_norm, hipStream_t s);
// the same for the rows of a list
hipError_t launch_sketch_rows(const float *X, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img, uint32_t d,
                              void *img, unsigned long long *max_norm, hipStream_t s);
// the same two with xx_r in the metadata run's fourth dword (the L2 family's column)
hipError_t launch_sketch_build_xx(const float *X, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d, void *img,
                                  unsigned long long *max_norm, hipStream_t s);
hipError_t launch_sketch_rows_xx(const float *X, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img, uint32_t d,
                                 void *img, unsigned long long *max_norm, hipStream_t s);

struct SketchScanArgs {
  const void *img;
  const uint32_t *id_rank;
  const int8_t *qimg;       // [2][ld8]: the query's two int8 levels, q ~ t1 Q1 + t2 Q2
  uint32_t n, d, nch;       // nch = ld8 / 16
  int metric;               // VT_COSINE / VT_INNER_PRODUCT / VT_NEG_INNER_PRODUCT; VT_L2 / VT_L2_SQUARED (a column with xx)
  float t1, t2;
  double qn;                // >= ||q||
  double eta;               // >= ||q - t1 Q1 - t2 Q2||
  double kerr;              // K1's summation error per unit of ||q|| ||x_r||; 0 for the L2 family, whose
                            // interval of the real dot carries K1's rounding as a relative term of the distance instead
  uint32_t k;               // entries per block list (k' of DESIGN 4.10)
  uint64_t *part_keys;      // [blocks][k]: orderable(key(hi_r)) << 32 | id rank (L2 family: orderable(kmin_r))
  Payload *part_pay;        // [blocks][k]: row, key(lo_r) as a float (L2 family: kmax_r)
  double qq_lo, qq_hi;      // L2 family: ||q||^2 lies in [qq_lo, qq_hi]
};
size_t sketch_scan_lds_bytes(uint32_t d, uint32_t k);  // 0: not supported
hipError_t launch_sketch_scan(const SketchScanArgs &a, uint32_t blocks, hipStream_t s);

// One block over the lists of launch_sketch_scan: Kt = the k-th smallest key(lo) retained; every retained row whose
// key(hi) <= Kt is a candidate; certified iff they number at most `cap` and no list consists of candidates alone (a
// full list whose largest key(hi) is <= Kt).  K1q's tail.  info = {outcome, candidates, Kt bits, 0} (host-mapped), outcome
//   1: certified, and the block rescored the candidates itself with K1's arithmetic (X, q, order, metric -- the dot
//      family's products or the L2 family's squared differences and root; *status raised like K1's) and wrote the k
//      best, sorted, with the status word into *out like launch_select -- taken when they are few enough for its LDS
//      (at most 256);
//   2: certified, rows[0..*count) hold the candidates for a gathered K1;
//   0: not certified (*count = 0).
struct SketchTailArgs {
  const uint64_t *keys;     // [lists][kp], launch_sketch_scan's part_keys
  const Payload *pay;       // [lists][kp]
  uint32_t lists, kp, k, cap;
  uint32_t *rows;           // [cap]
  uint32_t *count;
  uint32_t *info;           // [4]
  const float *X;           // the f32 rows, `stride` floats apart
  size_t stride;
  const float *q;           // the query padded with zeros to padded_dim(d) floats (device)
  const uint32_t *id_rank;  // per row; null => row index
  uint32_t d;
  int metric, order;
  int *status;
  ResultBlock *out;
  uint32_t ld, ss, lds_words;  // set by the launcher
};
hipError_t launch_sketch_tail(SketchTailArgs a, hipStream_t s);

// ---- K1qm (vt_sketch_batch.hip): 2..8 such searches in one pass over the int8 sketch -----------------------------------
// Query g of the group has its own two levels, bounds and lists; the two words kept for (query g, row r) are bit for bit
// launch_sketch_scan's for that query alone.  The pass is compiled for groups of 2, 4 and 8 (sketch_scan_multi_group(ng):
// the one a group of ng runs as); qimg holds that many images, the ones past ng zero.  k <= kSmallK.
constexpr int kSketchMultiMax = 8;
struct SketchScanMultiArgs {
  const void *img;
  const uint32_t *id_rank;
  const int8_t *qimg;       // [sketch_scan_multi_group(ng)][2][ld8]
  uint32_t n, d, nch, ng;   // nch = ld8 / 16; 2 <= ng <= kSketchMultiMax
  int metric;               // as SketchScanArgs
  uint32_t k;               // entries per block list (k')
  uint64_t *part_keys;      // [ng][blocks][k], as launch_sketch_scan writes a query's
  Payload *part_pay;        // [ng][blocks][k]
  float t1[kSketchMultiMax], t2[kSketchMultiMax];  // per query, as SketchScanArgs has them
  double qn[kSketchMultiMax], eta[kSketchMultiMax], kerr[kSketchMultiMax];
  double qq_lo[kSketchMultiMax], qq_hi[kSketchMultiMax];
};
uint32_t sketch_scan_multi_group(uint32_t ng);
// (two blocks must fit a CU: 0 when `group` images and wave buffers take more than half its LDS, or k > kSmallK)
size_t sketch_scan_multi_lds_bytes(uint32_t d, uint32_t k, uint32_t group);
hipError_t launch_sketch_scan_multi(const SketchScanMultiArgs &a, uint32_t blocks, hipStream_t s);
// launch_sketch_tail for every query of a group in one launch, a block per query: `a` is query 0's; block g takes the
// slice g of keys / pay ([ng][lists][kp]) and of rows ([ng][cap]), count + g, info + 4 g, q + g * q_stride, out + g and
// status + g.  Each block's outcome is what launch_sketch_tail gives on that slice.
hipError_t launch_sketch_tail_group(SketchTailArgs a, uint32_t ng, size_t q_stride, hipStream_t s);

// The same certification behind K1s's and K1f's passes, spread over the card in two launches (vt_sketch.hip): Kt, the
// candidates, their count and the full-list check are the ones launch_sketch_tail would give; nothing is rescored (the
// caller queues the gathered K1 and its select behind).  launch_sketch_thresh: every block's k smallest key(lo) words
// to parts[], its live words to live[], and the three words of sync[] to zero.  launch_sketch_collect: Kt from parts[],
// the rows of the candidates (key(hi) <= Kt) to rows[] in no particular order, and from the block that finishes last
// *count (0 unless certified) and info = {2 if certified else 0, candidates, Kt bits, 1}.  Both take the same arguments.
struct SketchSpreadArgs {
  // launch_sketch6_scan's / launch_sketch5_scan's word arrays and payloads ([lists][kp] each)
  const uint32_t *lo_words, *hi_words;
  const Payload *pay;
  uint32_t lists, kp, k, cap;
  uint32_t *parts;          // [sketch_thresh_blocks(lists, kp)][k]
  uint32_t *live;           // [sketch_thresh_blocks(lists, kp)]
  uint32_t *sync;           // {claim, fail, ticket, -}: a 16-byte block of its own
  uint32_t *rows;           // [cap]
  uint32_t *count;
  uint32_t *info;           // [4] (host-mapped)
  uint32_t thresh_blocks, collect_blocks, collect_lists;  // set by the launchers
  // K1n's exact threshold (launch_sketch_refine below); null: both launches behave as they did without these
  uint32_t *slots = nullptr;          // [thresh_blocks][k]: launch_sketch_thresh files beside every word of parts[] the
                                      // slot of lo_words[] it came from -- distinct slots that hold that word
  const uint32_t *kt_word = nullptr;  // launch_sketch_collect takes this word for the Kt it would derive from parts[]
};
uint32_t sketch_thresh_blocks(uint32_t lists, uint32_t kp);
hipError_t launch_sketch_thresh(SketchSpreadArgs a, hipStream_t s);
hipError_t launch_sketch_collect(SketchSpreadArgs a, hipStream_t s);

// Between the two, behind K1n's pass: the threshold from exact rescoring.  One block takes the k smallest
// (word, slot) pairs of parts[] / slots[] -- Kt is the largest of those words --, reads the rows pay[slot].row and rescores
// each with K1's arithmetic in the index's reduce order (a wave per row: elem4 / chunk_sum of vt_scan.cuh, the sequential
// chain over the chunk sums, the scalar tail; the rank value formed as K1 forms it).  *kt_out = min(Kt, the largest of the
// k exact key words): the exact key of k real rows, so at least k rows have a key <= it, and it is never above Kt.  Plain
// Kt (0xffffffff with k or fewer live words) when fewer than k + 1 words are live, when any of the k values is not finite,
// or when the rows' chunk sums do not fit the block's LDS.  picked[0..k) (optional): the rows it rescored, 0xffffffff
// where it rescored none.
struct SketchRefineArgs {
  const uint32_t *parts, *slots, *live;  // launch_sketch_thresh's, [thresh_blocks][k] / [thresh_blocks]
  uint32_t thresh_blocks, k;
  const Payload *pay;       // [slots_total]
  uint32_t slots_total;     // lists * kp
  const float *X;           // the f32 rows, `stride` floats apart
  size_t stride;
  const float *q;           // the query padded with zeros to padded_dim(d) floats (device)
  uint32_t d;
  int metric, order;
  uint32_t *kt_out;
  uint32_t *picked;
  uint32_t ld, ss, np4;     // set by the launcher
};
hipError_t launch_sketch_refine(SketchRefineArgs a, hipStream_t s);

// ---- K1s (vt_sketch.hip): the same search over a 6-bit sketch in two planes -- 0.755 of K1q's bytes ------------------
// Row r is kept as X_r = round(x_r / s_r) in [-31, 31] with s_r = max_i |x_ri| / 31, split as X = 4 H + L: H = X >> 2
// (arithmetic, [-8, 7]) a signed nibble, L = X & 3 two bits; rho_r and nu_r as K1q has them.  Layout, per tile of 64 rows,
// in 1-KiB runs of 16 bytes per row (lane l: row 64 t + l): ld8 / 32 runs of H -- run c holds elements [32 c, 32 c + 32),
// nibble i of dword j is element 32 c + 8 j + i --, then ld8 / 64 runs of L -- in dword j of run c', bits [4 i, 4 i + 2)
// are element 64 c' + 8 j + i and bits [4 i + 2, 4 i + 4) element 64 c' + 32 + 8 j + i, so that w & 0x33333333 and
// (w >> 2) & 0x33333333 are nibble vectors aligned with the H-runs 2 c' and 2 c' + 1 --, then one run of {s, rho, nu, 0}.
constexpr int kSketch6Levels = 3;  // the query's signed-nibble levels (host/vt_sketch6.h writes them)
__host__ __device__ inline uint32_t sketch6_runs(uint32_t d) { return 3 * (sketch_ld8(d) / 64) + 1; }  // per tile
__host__ __device__ inline size_t sketch6_offset(uint32_t row, uint32_t run, uint32_t runs) {
  return ((size_t)(row / kSketchTileRows) * runs + run) * 1024 + (size_t)(row % kSketchTileRows) * 16;
}
inline size_t sketch6_bytes(uint32_t rows, uint32_t d) {
  const size_t tiles = ((size_t)rows + kSketchTileRows - 1) / kSketchTileRows;
  return tiles * sketch6_runs(d) * 1024;
}
// (as launch_sketch_build / launch_sketch_rows)
hipError_t launch_sketch6_build(const float *X, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d, void *img,
                                unsigned long long *max_norm, hipStream_t s);
hipError_t launch_sketch6_rows(const float *X, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img, uint32_t d,
                               void *img, unsigned long long *max_norm, hipStream_t s);

struct Sketch6ScanArgs {
  const void *img;
  const uint32_t *id_rank;
  const uint32_t *qimg;     // [kSketch6Levels][ld8 / 8]: the query's signed-nibble levels, q ~ sum_j t_j Q_j
  uint32_t n, d, ld8;
  int metric;
  float t[kSketch6Levels];
  double qn, eta, kerr;     // as SketchScanArgs
  // The last level never meets the L plane (0 <= L_i <= 3): Q3.L_r lies in [3 N3, 3 P3], P3 / N3 the sums of Q3's positive /
  // negative entries (host/vt_sketch6.h).  c3 = 1.5 t3 (P3 + N3) is added to the sum s_r multiplies, s_r w3 with
  // w3 = 1.5 t3 ||Q3||_1 to e_r; both products are exact in f64.
  double c3, w3;
  uint32_t k;               // entries per block list
  uint64_t *part_keys;      // [blocks][k], as launch_sketch_scan writes them
  Payload *part_pay;
  // [blocks][k] each, beside the lists: a slot's orderable key(lo) word and its orderable key(hi) word, 0xffffffff in both
  // for an empty slot -- what launch_sketch_thresh and launch_sketch_collect read in place of the lists themselves
  uint32_t *lo_words, *hi_words;
  // K1n's threshold from each list's best rows (launch_sketch4_scan alone; null: the pass is what it is without these).
  // The wave that stores a list rescores the list's two live slots of smallest key(lo) word (ties: the lower slot) with
  // K1's arithmetic (vt_rowscore.cuh: X, stride, q padded to padded_dim(d) floats, the index's reduce order) and leaves
  // their exact rank words in best_words[list][0..1]; 0xffffffff where the list has no such slot or the value is not
  // finite.  Any k of these words bound the corpus's k-th key word from above (launch_sketch4_rescore takes the k-th
  // smallest).  The rows' chunk sums lie in the wave buffers of the pair: padded_dim(d) / 8 + 12 <= kSketch4BestRowFloats.
  uint32_t *best_words = nullptr;  // [blocks * kSketch4BlockLists][kSketch4BestRows]
  const float *X = nullptr;
  size_t stride = 0;
  const float *q = nullptr;
  int order = 0;
};
constexpr uint32_t kSketch4BestRows = 2;         // rows a list's storing wave rescores
constexpr uint32_t kSketch4BestRowFloats = 512;  // a row's chunk sums and tail products at most: two wave buffers hold two rows
// k <= kSmallK and ld8 >= 256 (a tile of ld8 = 128 is shorter than the load ring: K1q serves those); 0: not supported
size_t sketch6_scan_lds_bytes(uint32_t d, uint32_t k);
hipError_t launch_sketch6_scan(const Sketch6ScanArgs &a, uint32_t blocks, hipStream_t s);

// ---- K1f (vt_sketch_nibble.hip): the same search over a 5-bit sketch in two planes -- 0.838 of K1s's bytes -----------------
// Row r is kept as X_r = round(x_r / s_r) in [-15, 15] with s_r = max_i |x_ri| / 15, split as X = 2 H + L: H = X >> 1
// (arithmetic, [-8, 7]) a signed nibble, L = X & 1 one bit; rho_r and nu_r as K1q has them.  Layout, per tile of 64 rows,
// in 1-KiB runs of 16 bytes per row: ld8 / 32 runs of H in K1s's H layout, then ld8 / 128 runs of L -- in dword j of run
// c', bit 4 i + b is element 128 c' + 32 b + 8 j + i, so that (w >> b) & 0x11111111 is a nibble vector aligned with dword
// j of the H-run 4 c' + b --, then one run of {s, rho, nu, 0}: 5 ld8 / 128 + 1 KiB per tile.
__host__ __device__ inline uint32_t sketch5_runs(uint32_t d) { return 5 * (sketch_ld8(d) / 128) + 1; }  // per tile
inline size_t sketch5_bytes(uint32_t rows, uint32_t d) {
  const size_t tiles = ((size_t)rows + kSketchTileRows - 1) / kSketchTileRows;
  return tiles * sketch5_runs(d) * 1024;
}
// (as launch_sketch_build / launch_sketch_rows; a run's place in the image: sketch6_offset with sketch5_runs)
hipError_t launch_sketch5_build(const float *X, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d, void *img,
                                unsigned long long *max_norm, hipStream_t s);
hipError_t launch_sketch5_rows(const float *X, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img, uint32_t d,
                               void *img, unsigned long long *max_norm, hipStream_t s);
// The pass takes Sketch6ScanArgs as K1s's does (img: the 5-bit column).  Here 0 <= L_i <= 1, so Q3.L_r lies in [N3, P3]:
// c3 = 0.5 t3 (P3 + N3) and w3 = 0.5 t3 ||Q3||_1 (host/vt_sketch5.h), and a_r = s_r (sum_{j <= 2} t_j (2 accH_j + accL_j)
// + 2 t3 accH_3 + c3).  k <= kSmallK and ld8 >= 256; 0: not supported
size_t sketch5_scan_lds_bytes(uint32_t d, uint32_t k);
hipError_t launch_sketch5_scan(const Sketch6ScanArgs &a, uint32_t blocks, hipStream_t s);

// ---- K1n (vt_sketch_nibble.hip): the same search over a 4-bit sketch in one plane -- 0.806 of K1f's bytes -------------------
// Row r is kept as X_r = round(x_r / s_r) in [-7, 7] with s_r = max_i |x_ri| / 7, one signed nibble per element; rho_r and
// nu_r as K1q has them.  Layout, per tile of 64 rows, in 1-KiB runs of 16 bytes per row: ld8 / 32 runs in K1s's H layout
// (nibble i of dword j of run c is element 32 c + 8 j + i), then one run of {s, rho, nu, 0}: ld8 / 32 + 1 KiB per tile.
constexpr uint32_t kSketch4BlockLists = 2;  // lists a block of the pass leaves: launch_sketch4_scan writes blocks * 2 of them
__host__ __device__ inline uint32_t sketch4_runs(uint32_t d) { return sketch_ld8(d) / 32 + 1; }  // per tile
inline size_t sketch4_bytes(uint32_t rows, uint32_t d) {
  const size_t tiles = ((size_t)rows + kSketchTileRows - 1) / kSketchTileRows;
  return tiles * sketch4_runs(d) * 1024;
}
// (as launch_sketch_build / launch_sketch_rows; a run's place in the image: sketch6_offset with sketch4_runs)
hipError_t launch_sketch4_build(const float *X, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d, void *img,
                                unsigned long long *max_norm, hipStream_t s);
hipError_t launch_sketch4_rows(const float *X, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img, uint32_t d,
                               void *img, unsigned long long *max_norm, hipStream_t s);
// The pass takes Sketch6ScanArgs as K1s's does (img: the 4-bit column; c3 and w3 are not read): a_r = s_r sum_j t_j acc_j.
// part_keys, part_pay, lo_words and hi_words hold [blocks * kSketch4BlockLists][k].  k <= kSmallK and ld8 >= 256; 0: not
// supported
size_t sketch4_scan_lds_bytes(uint32_t d, uint32_t k);
hipError_t launch_sketch4_scan(const Sketch6ScanArgs &a, uint32_t blocks, hipStream_t s);

// K1n's last link (vt_sketch4_rescore.hip), behind launch_sketch_refine: launch_sketch_collect and launch_scan_filter in one
// launch on the pass's grid, with no candidate array between them.  Block b takes the slots of the pass's lists
// [b * kSketch4BlockLists, + kSketch4BlockLists) whose key(hi) word is live and <= *s.hi_word -- the collect's candidates, and
// its certificate: ok = no list of candidates alone && candidates <= cap --, rescores their rows with K1's arithmetic and
// keeps the valid ones whose rank word is <= *s.hi_word as launch_scan_filter keeps them (s.surv_keys / surv_pay / surv_cap,
// s.fsync[0 .. kScanFilterSyncWords) handed over zeroed: word 1 of a group's ticket line counts the group's candidates, bit
// 1 of fsync[1] is the certificate's fail bit).  The block that draws the last ticket writes info = {outcome, candidates,
// the word, 1}: kScanFilterDelivered with the sorted result in *s.out when ok and at most surv_cap rows were kept, else 2
// when ok (the caller queues launch_sketch_collect, launch_scan_batch and launch_select over the lists) and 0 when not.
// Of `s` it reads X, stride, q, id_rank, d, metric (cosine, dot, negative dot), order, k <= kSmallK, status and the
// filter-mode fields; d is bounded by the block's LDS (sketch4_rescore_lds_bytes, 0: not supported).
struct Sketch4RescoreArgs {
  ScanArgs s;
  const uint32_t *hi_words;  // [blocks * kSketch4BlockLists][kp], launch_sketch4_scan's
  const Payload *pay;        // [blocks * kSketch4BlockLists][kp]
  uint32_t kp, cap;
  uint32_t ld, ss;           // set by the launcher
  // The threshold from the pass's best rows (Sketch6ScanArgs::best_words; null: *s.hi_word as above).  Every block finds
  // the same word before it judges a slot: Kt'' = the k-th smallest of the best_count words with multiplicity, 0xffffffff
  // when fewer than k are live (every live slot is then a candidate).  It stands wherever *s.hi_word stood, info[2]
  // included, and block 0 stores it to *kt_out.  best_count <= kSketch4BestMaxWords, k <= kSketch4BestMaxK.
  const uint32_t *best_words = nullptr;
  uint32_t best_count = 0;
  uint32_t *kt_out = nullptr;
};
constexpr uint32_t kSketch4BestMaxWords = 4096;  // sixteen words a thread
constexpr uint32_t kSketch4BestMaxK = 17;        // the words below the k-th thread minimum fit a word per thread: 16 (k - 1) <= 256
size_t sketch4_rescore_lds_bytes(uint32_t d, uint32_t kp);
hipError_t launch_sketch4_rescore(Sketch4RescoreArgs a, uint32_t blocks, hipStream_t s);

}  // namespace vt
