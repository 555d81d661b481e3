/*
 * vettore_flat.h -- C ABI of libvettore_hip.so, the MI355X (gfx950) drop-in for
 * the flat-index hot path of elchemista/vettore v0.3.2.
 *
 * Every entry point is what a NIF shim for `Vettore.Nifs` (or the plugin module
 * `Vettore.Index.FlatGpu`) binds in place of the Rust function
 * cited next to it.  Citations are paths under /root/reference.
 *
 * Conventions
 *  - plain pointers and sizes only; no exceptions cross the boundary;
 *  - every function returns a VT_* status; vt_strerror() maps the reference's
 *    error statuses to the reference's exact error strings, so the shim can
 *    build `{:error, "dimension mismatch"}` verbatim;
 *  - ids are arbitrary byte strings (Elixir binaries): pointer + length, or for
 *    batches one concatenated buffer plus `off[count + 1]` offsets;
 *  - ragged vector batches use the same layout (values + `off[count + 1]` in
 *    elements) so that a wrong-length row is reported as "dimension mismatch"
 *    exactly like native/vettore/src/flat.rs:69-85 does;
 *  - all compute runs on the GPU; there is no CPU fallback.  Without a usable
 *    HIP device the calls fail with VT_ERR_DEVICE.
 *  - thread safety: a handle is the reference's RwLock<FlatIndex> (nifs.rs:266-309):
 *    searches of one handle run concurrently with each other (each on its own HIP
 *    stream; vt_flat_search calls that meet on a busy handle are answered together
 *    in one pass over the corpus, see vt_flat_coalesce_stats), mutations are
 *    exclusive; different handles are independent.  A
 *    mutation that fails on the device after it began changing the index poisons
 *    the handle (VT_ERR_POISONED from then on), like a panic under the write lock.
 */
#ifndef VETTORE_FLAT_H
#define VETTORE_FLAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct of this header grows or an entry point changes (r04: vt_profile grew,
 * vt_flat_set_batch_shadow / vt_flat_batch_shadow / vt_flat_get_profile_sized arrived).  A binding
 * compares it with vt_abi_version() when it loads the library (vettore_amd/_lib.py, the erl_nif
 * shim's load callback): a caller built against an older header would hand vt_flat_get_profile a
 * struct that is too small. */
#define VT_ABI_VERSION 4   /* r05: vt_debug_set / vt_debug_get */

/* Metric codes == Metric::from_code, native/vettore/src/distances.rs:24-38,
 * mirrored by lib/vettore/collection.ex:1306-1315. */
enum {
  VT_L2 = 0,
  VT_L2_SQUARED = 1,
  VT_COSINE = 2,
  VT_INNER_PRODUCT = 3,
  VT_NEG_INNER_PRODUCT = 4,
  VT_MANHATTAN = 5,
  VT_CHEBYSHEV = 6,
  VT_HAMMING = 7,
  VT_JACCARD = 8
};

/* Status codes.  1..7 carry the reference's error strings. */
enum {
  VT_OK = 0,
  VT_ERR_EMPTY = 1,          /* "vector must not be empty"            flat.rs:138 */
  VT_ERR_DIMENSION = 2,      /* "dimension mismatch"                  flat.rs:141, distances.rs:44 */
  VT_ERR_NON_FINITE = 3,     /* "vector contains a non-finite value"  distances.rs:135 */
  VT_ERR_OVERFLOW = 4,       /* "metric overflow"                     distances.rs:67 */
  VT_ERR_UNKNOWN_METRIC = 5, /* "unknown metric"                      distances.rs:36 */
  VT_ERR_PREFIX = 6,         /* "invalid prefix dimensions"           search.rs:47 */
  VT_ERR_DIMS_POSITIVE = 7,  /* "dimensions must be positive"         distances.rs:463 */
  VT_ERR_POISONED = 8,       /* "flat lock poisoned"                  nifs.rs:269: an earlier mutation died half-way */
  VT_ERR_EMPTY_VECTORS = 9,  /* "vectors must not be empty"           multi_vector.rs:57, :141 */
  VT_ERR_SCORE_OVERFLOW = 10, /* "score overflow"                     multi_vector.rs:84 */
  /* statuses the reference cannot produce */
  VT_ERR_NOMEM = 16,
  VT_ERR_DEVICE = 17,        /* HIP error / no gfx950 device; see vt_last_error() */
  VT_ERR_UNSUPPORTED = 18,   /* shape outside what the device kernels cover; vt_last_error() */
  VT_ERR_ARGUMENT = 19,      /* NULL handle and the like (the shim's badarg) */
  /* MUVERA (muvera.rs:76-106, :29-42, :164-177): the reference's strings again */
  VT_ERR_EMPTY_SET = 20,          /* "empty vectors"                               muvera.rs:79 */
  VT_ERR_MUVERA_DIMENSION = 21,   /* "dimension must be positive"                  muvera.rs:82 */
  VT_ERR_MUVERA_REPETITIONS = 22, /* "num_repetitions must be positive"            muvera.rs:85 */
  VT_ERR_MUVERA_SIMHASH = 23,     /* "num_simhash_projections must be < 31"        muvera.rs:88 */
  VT_ERR_MUVERA_PROJECTION = 24,  /* "projection_dimension must be positive"       muvera.rs:91 */
  VT_ERR_MUVERA_FINAL = 25,       /* "final_projection_dimension must be positive" muvera.rs:94 */
  VT_ERR_FDE_OVERFLOW = 26,       /* "fde dimension overflow"                      muvera.rs:34, :38 */
  VT_ERR_FDE_LIMIT = 27,          /* "fde dimension exceeds safety limit"          muvera.rs:41 */
  VT_ERR_ENCODING_OVERFLOW = 28,  /* "encoding overflow"                           muvera.rs:175, :195 */
  /* HnswParams::validate, hnsw.rs:25-49, and the handle's own poisoning */
  VT_ERR_HNSW_M = 29,               /* "m must be positive" */
  VT_ERR_HNSW_M0 = 30,              /* "m0 must be positive" */
  VT_ERR_HNSW_DEGREE = 31,          /* "invalid hnsw degree" */
  VT_ERR_HNSW_EF_CONSTRUCTION = 32, /* "ef_construction must be >= m" */
  VT_ERR_HNSW_EF_LIMIT = 33,        /* "ef_construction exceeds safety limit" */
  VT_ERR_HNSW_EF_SEARCH = 34,       /* "ef_search must be positive" */
  VT_ERR_HNSW_MAX_LEVEL = 35,       /* "max_level must be positive" */
  VT_ERR_HNSW_POISONED = 36,        /* "hnsw lock poisoned"                          nifs.rs:376-426 */
  /* mmr_rerank/5, lib/vettore_distance.ex:334-405 */
  /* (37 stays unassigned: vt_strerror(37) is "unknown status") */
  VT_ERR_MMR_ARGS = 38              /* "invalid mmr args"  (:invalid_mmr_args) */
};

/* Lane order of wide::f32x8::reduce_add used for every 8-float chunk
 * (distances.rs:197-308).  The reference does not pin it (third-party crate,
 * build-flag dependent); the device kernels reproduce whichever is selected bit
 * for bit.  With l0..l7 the lanes of a chunk:
 *   VT_ORDER_PAIR ((l0+l1)+(l2+l3)) + ((l4+l5)+(l6+l7))   two f32x4 halves, SSE3 haddps / NEON vaddvq
 *   VT_ORDER_AVX  ((l0+l4)+(l2+l6)) + ((l1+l5)+(l3+l7))   one 256-bit register (target-cpu=native, Taskfile.yml:12)
 *   VT_ORDER_SEQ  (((l0+l1)+l2)+l3) + (((l4+l5)+l6)+l7)   array fallback (no SIMD target feature)
 *   VT_ORDER_SSE2 ((l0+l2)+(l1+l3)) + ((l4+l6)+(l5+l7))   two f32x4 halves, movehl + shuffle (baseline
 *                                                          x86-64: what the precompiled release NIF is built for)
 * Default VT_ORDER_SSE2 (override: VT_REDUCE_ORDER=pair|avx|seq|sse2, vt_set_default_reduce_order,
 * vt_flat_set_reduce_order).  See DESIGN.md "summation order" and INTEGRATION.md section 4 for the
 * one-line probe that tells which order a given libvettore build uses. */
enum { VT_ORDER_PAIR = 0, VT_ORDER_AVX = 1, VT_ORDER_SEQ = 2, VT_ORDER_SSE2 = 3 };

const char *vt_strerror(int status);
/* Detail text of the calling thread's last VT_ERR_DEVICE / VT_ERR_UNSUPPORTED. */
const char *vt_last_error(void);
int vt_abi_version(void);
/* Number of visible HIP devices (0 if none); never fails. */
int vt_device_count(void);
/* Diagnostic (bench.py's `measured_read_peak`): GB/s of a bare read-only stream over a scratch buffer
 * of `bytes` (random floats; allocated and freed here) on `device`, best of `reps` passes after one
 * warm-up pass, timed with HIP events.  The stream is the LDS-DMA ring the batch passes read through
 * with nothing consuming it (whole 384-KiB tiles, 1-KiB pieces, 64 KiB in flight per CU): the
 * yardstick beside the 8 TB/s spec figure -- a search kernel that reads this way and also computes
 * cannot stream faster on the same box. */
int vt_device_read_peak(int device, size_t bytes, int reps, double *gbps);

/* ------------------------------------------------------------------ settings
 * The library reads the process environment exactly ONCE, while it is being loaded (dlopen /
 * :erlang.load_nif): every VT_* variable of DESIGN_APPENDIX.md A.10 lands in a table of atomic integers
 * (csrc/vt_env.h) and no search, insert or load ever calls getenv -- inside a BEAM `System.put_env/2`
 * may run setenv on a scheduler thread at any time, and the reference NIF itself reads no process state
 * (nifs.rs:297-309).  After loading, a setting changes only through vt_debug_set: `name` is the
 * variable's name without "VT_", lower case ("batch_no_mfma", "coalesce_slots", "slab_chunk_mb" ...;
 * string-valued ones take their code: reduce_order 0..3 = VT_ORDER_*, batch_nominate VT_NOMINATE_*,
 * batch_shadow VT_SHADOW_*, slab 1 = malloc, shard_exchange 1 = host / 2 = rccl).  Four switches have
 * no environment name at all -- "force_batch_mfma", "force_sweep_groups", "force_multi_scan",
 * "force_threshold_select" (take a path on corpora the cost model would never send there) and
 * "bf16_rank" (K2b's threshold from exactly that sample rank): tests and soaks only.  A debugging and
 * testing aid, process-wide, effective for calls that start afterwards; VT_ERR_ARGUMENT for a name this
 * build does not know (the fault hooks "test_*" exist in libvettore_hip_hooks.so only, the timing experiments'
 * switches in `make experiments` only; r06 retired the A/B switches whose alternative had lost -- 24 settings are
 * left, DESIGN_APPENDIX.md A.10) and for a value the setting's own parser could not have produced
 * (reduce_order outside 0..3, batch_nominate outside 1..2 ...). */
int vt_debug_set(const char *name, long value);
int vt_debug_get(const char *name, long *value);

/* ------------------------------------------------------------------ hits
 * Vec<(String, f32)> as returned by flat_search / vector_top_k /
 * binary_top_k: ascending by (rank, id bytes). */
typedef struct vt_hits vt_hits;
size_t vt_hits_len(const vt_hits *hits);
/* id bytes of hit i (owned by `hits`, valid until vt_hits_free). */
const char *vt_hits_id(const vt_hits *hits, size_t i, size_t *len);
/* raw metric value of hit i (the f32 the NIF widens to a BEAM double). */
float vt_hits_raw(const vt_hits *hits, size_t i);
/* f32::total_cmp sort key of rank_value(metric, raw) as an order-preserving
 * u32 (distances.rs:113-119, flat.rs:34-40): what a multi-shard merge compares
 * before falling back to the id bytes. */
uint32_t vt_hits_rank_key(const vt_hits *hits, size_t i);
/* Serialises up to `cap` hits as fixed 64-byte records -- u32 rank_key, f32 raw,
 * u32 id_len, then the first 52 id bytes (zero padded) -- the wire format of the
 * cross-shard merge.  Returns the number of records written. */
#define VT_HIT_RECORD_BYTES 64
#define VT_HIT_RECORD_ID_BYTES 52
size_t vt_hits_pack(const vt_hits *hits, void *records, size_t cap);
/* The same for the `nq` hit lists of a query batch, as the process-per-GPU exchange ships them
 * (vettore_amd/sharded.py): `blocks` receives nq blocks of (limit + 1) records -- record 0 of a block
 * is its header {u32 count, u32 long_ids}: the hits that follow, and whether an id of the block is
 * longer than VT_HIT_RECORD_ID_BYTES (only its first bytes travel inline then). */
void vt_hits_pack_many(const vt_hits *const *hits, size_t nq, size_t limit, void *blocks);
/* ... and the merge on the receiving side: `blocks` holds world x nq such blocks (rank-major, as an
 * all-gather leaves them); out_blocks receives nq blocks with the `limit` best hits of each query over
 * all ranks by (rank key, id bytes) == FlatHit::cmp (flat.rs:34-40) -- one index over all rows would
 * return exactly these.  A block whose header says long_ids is merged by the inline bytes only and keeps
 * the flag: the caller must then order ties by the whole ids itself. */
int vt_hit_blocks_merge(const void *blocks, size_t world, size_t nq, size_t limit, void *out_blocks);
/* All hits in one call (bindings that would otherwise cross the ABI three times per hit):
 * vt_hits_id_bytes = total id bytes; vt_hits_export fills ids (concatenated), id_off
 * (len + 1 offsets), raw and rank_key (each len entries; null pointers are skipped). */
size_t vt_hits_id_bytes(const vt_hits *hits);
void vt_hits_export(const vt_hits *hits, char *ids, size_t *id_off, float *raw, uint32_t *rank_key);
void vt_hits_free(vt_hits *hits);
/* The same for the `n` lists a batch call returned (null entries are skipped): one call across the boundary instead of
 * `n` -- through a foreign-function interface 256 separate frees cost more than the lists took to build (r04). */
void vt_hits_free_many(vt_hits **hits, size_t n);

/* ----------------------------------------------------------- flat index
 * FlatResource(RwLock<FlatIndex>), flat.rs:13-17, :131-134. */
typedef struct vt_flat vt_flat;

/* flat_new_<metric>/0, nifs.rs:200-257.  `device` = HIP device ordinal. */
int vt_flat_new(int metric_code, int device, vt_flat **out);
/* The same resource spread over the GPUs of one node (SURVEY.md 8b "device_mask", 8e):
 * ONE handle in ONE process, like the reference's FlatResource (nifs.rs:254-257); shard i
 * lives on HIP device devices[i].  A row belongs to shard hash(id) % ndev, so every
 * operation on an id goes to one shard and the shards never talk to each other except
 * for the per-query exchange of their top-k lists.  Every entry point below accepts the
 * handle; results equal those of a one-GPU index over all rows (ids, order, raw bits).
 * ndev == 1 is vt_flat_new.  The same ordinal may be listed more than once (tests on a
 * one-GPU box); the exchange then stays on the host path. */
int vt_flat_new_sharded(int metric_code, const int *devices, size_t ndev, vt_flat **out);
size_t vt_flat_shard_count(const vt_flat *index);
int vt_flat_shard_device(const vt_flat *index, size_t shard);  /* -1: no such shard */
size_t vt_flat_shard_len(const vt_flat *index, size_t shard);
/* Where a shard's rows live: rows the slab holds without growing, its bytes, and the number of
 * physical chunks mapped into its reserved range (0: a plain allocation, the form below one
 * chunk).  A slab of one chunk or more grows by mapping further 1-GiB chunks behind the rows --
 * they never move and no second slab exists beside the first (the reference's per-row Vec
 * allocations, flat.rs:13-17, have no such step at all).  Any out pointer may be NULL. */
int vt_flat_shard_memory(const vt_flat *index, size_t shard, size_t *row_capacity, size_t *slab_bytes,
                         size_t *slab_chunks);
/* Searches that meet on one handle go together.  The reference's readers share an RwLock and
 * scale with the host's cores (nifs.rs:297-309); here every search is a pass over the corpus in
 * HBM, so a vt_flat_search that finds another one running waits for it, and everything that has
 * queued up by then (same limit, up to 256) runs as ONE batch -- one sweep of the corpus for up
 * to eight queries, the matrix-core pass beyond -- each caller getting exactly the hits its own
 * search would have produced (ids, order, raw bits).  An idle handle adds nothing: the first
 * caller runs at once, alone.  VT_COALESCE=0 in the environment switches it off.  This returns
 * how many such batches ran and how many searches they carried.  Out pointers may be NULL. */
int vt_flat_coalesce_stats(vt_flat *index, uint64_t *batches, uint64_t *batched_queries);
/* out_shard[i] = shard that owns (or would own) id i. */
int vt_flat_route_ids(const vt_flat *index, size_t count, const char *ids, const size_t *id_off,
                      uint32_t *out_shard);
/* How the shards' top-k lists meet (multi-shard handles):
 *   VT_EXCHANGE_RCCL  every shard's select kernel leaves its list in a device block; one
 *                     ncclAllGather per shard communicator (RCCL over xGMI, queued behind the
 *                     scan on the shard's stream) collects the blocks, shard 0 hands the
 *                     gathered lists to the host, which merges by (rank key, id bytes).
 *                     Default when the shards sit on distinct devices and limit <= 256.
 *   VT_EXCHANGE_HOST  every shard's select kernel writes its list straight into pinned host
 *                     memory; same merge.  Always available; used for limits above 256,
 *                     batches, and when RCCL cannot serve the device list. */
enum { VT_EXCHANGE_HOST = 0, VT_EXCHANGE_RCCL = 1 };
int vt_flat_set_exchange(vt_flat *index, int mode);
int vt_flat_exchange(const vt_flat *index);
/* Which exchange a multi-shard handle chose when it was created and, if RCCL was refused, why
 * (one line, also printed on stderr at creation when VT_LOG is set).  Empty for a plain index.
 * A search whose all-gather does not complete within VT_EXCHANGE_TIMEOUT_MS (default 20 000)
 * fails with VT_ERR_DEVICE "RCCL exchange timed out on shard s ..." and poisons the handle. */
const char *vt_flat_exchange_note(const vt_flat *index);
/* Ranks of the shard communicator (ncclCommCount), 0 while none exists. */
int vt_flat_rccl_ranks(const vt_flat *index);
/* ResourceArc drop: frees HBM, streams, pinned staging. */
void vt_flat_free(vt_flat *index);

/* flat_insert/3, nifs.rs:259-271 -> FlatIndex::insert flat.rs:59-66. */
int vt_flat_insert(vt_flat *index, const char *id, size_t id_len,
                   const float *vector, size_t n);
/* flat_insert_many/2, nifs.rs:273-284 -> FlatIndex::insert_many flat.rs:69-85:
 * validates every row first (atomic), last duplicate id wins. */
int vt_flat_insert_many(vt_flat *index, size_t count, const char *ids,
                        const size_t *id_off, const float *values,
                        const size_t *value_off);
/* flat_delete/2, nifs.rs:286-295 -> FlatIndex::delete flat.rs:88-93.
 * Unknown id is a no-op; an emptied index forgets its dimension. */
int vt_flat_delete(vt_flat *index, const char *id, size_t id_len);
/* flat_search/3, nifs.rs:297-309 -> FlatIndex::search flat.rs:96-124.
 * limit == 0 returns an empty list before the query is validated. */
int vt_flat_search(vt_flat *index, const float *query, size_t n, size_t limit,
                   vt_hits **out);

/* Extension (SURVEY.md 8b "vt_flat_search_batch"): `nq` queries of `d` floats
 * each, stored back to back, against the same index.  out[i] receives query
 * i's hits -- identical (ids, order, raw bits) to nq vt_flat_search calls; the
 * first invalid query fails the whole call like its own flat_search would.
 * Dot-family metrics take the FP32-MFMA path: Q x D^T nominates candidates,
 * the exact kernel re-scores them, an error bound proves completeness. */
int vt_flat_search_batch(vt_flat *index, const float *queries, size_t nq, size_t d,
                         size_t limit, vt_hits **out);

size_t vt_flat_len(const vt_flat *index);
/* FlatIndex.dimension: -1 = None. */
long vt_flat_dimension(const vt_flat *index);
int vt_flat_metric(const vt_flat *index);
int vt_flat_set_reduce_order(vt_flat *index, int order);
/* Which matrix-core pass nominates the candidates of vt_flat_search_batch (and of coalesced
 * vt_flat_search calls): VT_NOMINATE_BF16 (default; operands rounded to bf16, the pass is
 * HBM-bound) or VT_NOMINATE_F32 (FP32 matrix cores).  Hits are identical bit for bit under
 * both: candidates are re-scored with the exact arithmetic and completeness is certified by
 * an error bound that knows the rounding.  Override for new indexes: VT_BATCH_NOMINATE=f32. */
#define VT_NOMINATE_F32 1
#define VT_NOMINATE_BF16 2
int vt_flat_set_batch_nominate(vt_flat *index, int mode);
int vt_flat_batch_nominate(const vt_flat *index);
/* The bf16 pass reads a bf16 SHADOW of the rows when the index keeps one: an image of every row,
 * rounded once (round to nearest even, what the pass itself would do on the fly) and laid out as
 * the matrix cores take their operands, kept beside the f32 slab -- half the bytes per pass, no
 * conversion in it.  It costs dimension * 2 bytes per row (half the slab again), is built by the
 * first batch that wants it, patched per mutated row like the other derived columns, and given
 * back at once when the rows themselves need the room (a growing slab never fails because of it).
 * The hits do not depend on it: same rounding, same bound, the exact kernel decides.
 *   VT_SHADOW_AUTO (default)  keep one when, after allocating it, at least a quarter of the
 *                             card's memory is still free
 *   VT_SHADOW_OFF             never (the pass streams the f32 rows and rounds in registers)
 * Override for new indexes: VT_BATCH_SHADOW=0.  vt_flat_batch_shadow reports shard 0's state. */
enum { VT_SHADOW_OFF = 0, VT_SHADOW_AUTO = 1 };
enum { VT_SHADOW_STATE_OFF = 0, VT_SHADOW_STATE_NONE = 1, VT_SHADOW_STATE_CURRENT = 2, VT_SHADOW_STATE_STALE = 3,
       VT_SHADOW_STATE_REFUSED = 4 };
int vt_flat_set_batch_shadow(vt_flat *index, int mode);
int vt_flat_batch_shadow(const vt_flat *index);   /* VT_SHADOW_STATE_*; -1: no index */
/* Opt-in (off by default; VT_SINGLE_NOMINATE=1 for new indexes): a lone vt_flat_search on an index whose bf16 shadow is
 * current is answered like a batch of one -- the bf16 pass over the shadow (half the bytes of the exact scan) nominates
 * a few hundred rows, the exact kernel re-scores them, the bound certifies that no other row can reach the top k; a
 * query the bound cannot certify takes the exact scan as before.  Same hits bit for bit, ~0.6 of the scan's time
 * (dot-family metrics, limit <= 256, ids ranked).  The default stays the exact scan of the f32 rows: what the
 * reference does (flat.rs:96-124), and what the headline benchmark measures. */
int vt_flat_set_single_nominate(vt_flat *index, int enabled);
int vt_flat_single_nominate(const vt_flat *index);
/* Order used by indexes created afterwards and by the stateless helpers. */
int vt_set_default_reduce_order(int order);

/* Bulk extensions (SURVEY.md 8b "vt_flat_load_matrix"): same semantics as
 * insert_many of `count` rows of equal length `d`, without the ragged layout.
 * _device takes a pointer to a row-major f32 [count][d] matrix already in this
 * device's HBM; finiteness is then checked by a device kernel. */
int vt_flat_load_matrix(vt_flat *index, size_t count, size_t d, const char *ids,
                        const size_t *id_off, const float *rows);
int vt_flat_load_device_matrix(vt_flat *index, size_t count, size_t d,
                               const char *ids, const size_t *id_off,
                               const void *device_rows);

/* quantized_search, lib/vettore/collection.ex:276-295: sign-bit Hamming
 * candidate pass (search.rs:76-92 over compress_sign_bits of every stored row,
 * distances.rs:413-437) followed by exact rerank (search.rs:38-73; cosine
 * reranks with the f64 `cosine`, search.rs:56-60). */
int vt_flat_quantized_search(vt_flat *index, const float *query, size_t n,
                             size_t candidates, size_t limit, vt_hits **out);
/* `nq` quantized searches (queries of `d` floats back to back), out[i] = query i's hits --
 * identical to nq vt_flat_quantized_search calls; groups of up to eight share ONE sweep of the
 * sign-bit matrix (candidates <= 256).  Concurrent vt_flat_quantized_search callers on one handle
 * are grouped the same way (they meet in the coalescer like plain searches do). */
int vt_flat_quantized_search_batch(vt_flat *index, const float *queries, size_t nq, size_t d,
                                   size_t candidates, size_t limit, vt_hits **out);

/* funnel_search, lib/vettore/collection.ex:245-260, :674-691: for every prefix
 * length in `stages` (1..dimensions, else "invalid prefix dimensions") keep the
 * `candidates` best rows by vector_top_k on that prefix (search.rs:38-73; a
 * cosine collection scores prefixes with the f64 `cosine`), the first stage over
 * the whole corpus, then exact rerank on the full vectors, top `limit`. */
int vt_flat_funnel_search(vt_flat *index, const float *query, size_t n,
                          const size_t *stages, size_t nstages, size_t candidates,
                          size_t limit, vt_hits **out);
/* `nq` funnel searches with one set of stages (queries of `d` floats back to back), out[i] = query
 * i's hits -- identical to nq vt_flat_funnel_search calls.  Groups of up to eight share ONE sweep of the
 * rows' first stages[0] coordinates (candidates <= 256, 16 384 rows or more): the f64 cosine on a cosine
 * collection, the metric's own f32 arithmetic on dot / L2 / manhattan / chebyshev ones (r04); under float
 * hamming / jaccard every query is a pass over the prefix of the non-zero-bit column (r04).  Anything else runs
 * query by query. */
int vt_flat_funnel_search_batch(vt_flat *index, const float *queries, size_t nq, size_t d,
                                const size_t *stages, size_t nstages, size_t candidates,
                                size_t limit, vt_hits **out);

/* hybrid_search with rerank: :exact, lib/vettore/collection.ex:325-345, :515-592:
 * the union (first occurrence wins) of the candidate sets of `ngen` generators,
 * exact rerank on the full vectors, top `limit`.  Generator i is
 *   VT_GEN_FUNNEL    stages[stage_off[i] .. stage_off[i+1]) prefix passes keeping candidates[i] rows
 *   VT_GEN_QUANTIZED sign-bit Hamming top candidates[i]
 *   VT_GEN_SEARCH    the index's own search with limit = candidates[i]            */
enum { VT_GEN_FUNNEL = 0, VT_GEN_QUANTIZED = 1, VT_GEN_SEARCH = 2 };
int vt_flat_hybrid_search(vt_flat *index, const float *query, size_t n, const int *kinds,
                          const size_t *candidates, const size_t *stage_off,
                          const size_t *stages, size_t ngen, size_t limit, vt_hits **out);

/* ---- row-sharded search across GPUs, device-side exchange -----
 * A shard's candidates are u64 keys (rank key << 32 | id_rank); they compare
 * across shards iff every shard's id_rank column comes from ONE ordering of all
 * ids.  vt_rank_ids computes that ordering (bytewise, like FlatHit::cmp,
 * flat.rs:34-40) for the concatenated ids of all shards; each shard installs its
 * slice with vt_flat_set_id_ranks (valid until its next mutation).
 *
 * Per query: vt_flat_search_begin enqueues upload + scan + select on the index's
 * stream and returns WITHOUT waiting; the shard's result lands in `device_block`
 * (device memory, >= 16 + limit * 16 bytes: {i32 status, u32 count, pad[2]} then
 * `limit` entries {u64 key, u32 row, f32 raw}).  The caller gathers the blocks of
 * all shards with one collective queued on vt_flat_stream(), then
 * vt_flat_merge_gathered merges `world` blocks on the device and waits once. */
int vt_rank_ids(const char *ids, const size_t *id_off, size_t count, uint32_t *out_rank);
int vt_flat_set_id_ranks(vt_flat *index, const uint32_t *ranks, size_t count);
void *vt_flat_stream(vt_flat *index); /* hipStream_t */
int vt_flat_search_begin(vt_flat *index, const float *query, size_t n, size_t limit,
                         void *device_block);
int vt_flat_merge_gathered(vt_flat *index, const void *device_blocks, size_t world,
                           size_t limit, size_t block_bytes, uint64_t *keys,
                           uint32_t *rows, float *raw, uint32_t *shard, size_t *count);

/* ------------------------------------------------- stateless NIF helpers
 * vector_top_k/5, nifs.rs:151-162 -> search.rs:38-73. */
int vt_vector_top_k(int device, size_t count, const char *ids,
                    const size_t *id_off, const float *values,
                    const size_t *value_off, const float *query, size_t nq,
                    int metric_code, size_t dimensions, size_t limit,
                    vt_hits **out);
/* binary_top_k/4, nifs.rs:164-175 -> search.rs:76-92. */
int vt_binary_top_k(int device, size_t count, const char *ids,
                    const size_t *id_off, const uint64_t *words,
                    const size_t *word_off, const uint64_t *query, size_t nq,
                    size_t dimensions, size_t limit, vt_hits **out);
/* normalize_l2/1, nifs.rs:107-111 -> distances.rs:350-361 (rows of a
 * [count][d] matrix; count == 1 is the NIF call). */
int vt_normalize_l2(int device, size_t count, size_t d, const float *in,
                    float *out);
/* compress_sign_bits/1, nifs.rs:125-129 -> distances.rs:413-423.
 * out has count * ((d + 63) / 64) words. */
int vt_compress_sign_bits(int device, size_t count, size_t d, const float *in,
                          uint64_t *out);

/* ---- prepare rows: the collection's four normalizations (collection.ex:50), for batches
 * The arithmetic is the reference's, bit for bit (distances.rs:350-410): l2 divides by sqrt of the f64 sum of squares,
 * zscore subtracts the f64 mean and divides by the population standard deviation, minmax maps [min, max] to [0, 1]
 * (a zero norm / deviation / range gives a row of zeros); every sum is a serial f64 chain in index order, every
 * division a true f64 division.  One thing the reference leaves open: f32::min / max do not say which zero wins
 * between +0.0 and -0.0, so under minmax the sign of a zero result is unspecified for a row whose minimum is a zero
 * and that holds zeros of both signs. */
enum { VT_NORM_NONE = 0, VT_NORM_L2 = 1, VT_NORM_ZSCORE = 2, VT_NORM_MINMAX = 3 };
/* normalize_zscore/1, normalize_minmax/1, nifs.rs:113-123 -> distances.rs:363-410: the shape of vt_normalize_l2
 * (vt_prepare_rows without words). */
int vt_normalize_zscore(int device, size_t count, size_t d, const float *in, float *out);
int vt_normalize_minmax(int device, size_t count, size_t d, const float *in, float *out);
/* What Collection.prepare_embedding does per record (collection.ex:921-946), for the rows of a [count][d] matrix in one
 * call: every value finite, else VT_ERR_NON_FINITE; `mode` (VT_NORM_*, anything else: VT_ERR_ARGUMENT) applied to each
 * row into out[count][d]; words != NULL: compress_sign_bits of each NORMALIZED row into words[count][(d + 63) / 64].
 * Finiteness is checked on the host before any device is touched: on refusal nothing is written and *first_refused
 * (may be NULL) is the smallest refused row; it is `count` when every row was accepted.  Empty batches and empty rows
 * are VT_OK and write nothing.  Large inputs stream through pooled buffers in chunks (upload, kernel and download
 * overlap); after the first call of a size no device or pinned memory is allocated or freed. */
int vt_prepare_rows(int device, int mode, size_t count, size_t d, const float *in,
                    float *out, uint64_t *words, size_t *first_refused);
/* The same for rows already in this device's HBM (what feeds vt_flat_load_device_matrix): `in` is a row-major f32
 * matrix whose rows lie ld_in floats apart and whose first d columns count (ld_in >= d; columns past d are neither read
 * nor written), `out` likewise with ld_out, `words` (device, may be NULL) is [count][(d + 63) / 64] u64.  `out` may be
 * `in` itself (then ld_out == ld_in); any other overlap is not supported.  Validation happens in the kernel: a row
 * holding a non-finite value is left UNWRITTEN, values and words, every other row is written, and the call returns
 * VT_ERR_NON_FINITE with *first_refused (may be NULL) the smallest such row -- in place the matrix is then partly
 * normalized: the caller must discard it.
 * Ordering: the call waits for everything queued on the device before it starts (the producer of `in` may have used
 * any stream) and returns after its own work has finished: whatever the caller queues afterwards, on any stream, sees
 * the complete result. */
int vt_prepare_device_rows(int device, int mode, size_t count, size_t d, size_t ld_in,
                           const void *in, size_t ld_out, void *out, void *words,
                           size_t *first_refused);

/* ------------------------------------------------- MaxSim (late interaction)
 * Vectors are ragged: vector j of a list is values[value_off[j] .. value_off[j + 1]), and a
 * length that differs from the query's is the reference's "dimension mismatch".  Validation
 * follows the reference exactly: the metric code, then the query vectors on their own (first
 * non-empty, equal lengths, finite), then the documents in order -- with no query vectors every
 * document is validated on its own and scores 0.0, a document without vectors scores 0.0 -- and
 * the first error (a scoring error of an earlier document included) is the call's status.
 * Scores: per query vector the best similarity_value over the document's vectors, summed in f32
 * in query order (bit-identical to the reference for the lane order of vt_set_default_reduce_order).
 * No CPU fallback: a valid call without a device returns VT_ERR_DEVICE. */
/* multi_vector_score/3, nifs.rs:177-187 -> multi_vector.rs:40-88 */
int vt_multi_vector_score(int device, const float *query, const size_t *query_off, size_t nquery,
                          const float *doc, const size_t *doc_off, size_t ndoc, int metric_code, float *out);
/* multi_vector_top_k/4, nifs.rs:188-198 -> multi_vector.rs:90-132: the `limit` best documents by
 * descending score (f32::total_cmp), ties by ascending id bytes; vt_hits_raw is the score. */
int vt_multi_vector_top_k(int device, size_t count, const char *ids, const size_t *id_off,
                          const size_t *doc_vec_off, /* count + 1: document i owns vectors [doc_vec_off[i], doc_vec_off[i + 1]) */
                          const float *values, const size_t *value_off, const float *query, const size_t *query_off,
                          size_t nquery, int metric_code, size_t limit, vt_hits **out);

/* ------------------------------------------- resident multi-vector store
 * The documents of vt_multi_vector_top_k, put once and kept in device memory: a search uploads the query vectors and
 * nothing else.  After any sequence of puts and deletes, vt_mv_top_k returns exactly what vt_multi_vector_top_k returns
 * for the live documents handed over in the order of their last put (an upsert moves a document to the end): ids,
 * order, score bits and status -- when several documents fail on the device, the earliest in that order.
 * vt_mv_put_many is atomic: every vector is checked before anything changes (a zero-length vector is
 * VT_ERR_EMPTY_VECTORS, a length other than the store's dimension -- or, while the store has none, than the call's first
 * vector's -- VT_ERR_DIMENSION, then VT_ERR_NON_FINITE), the last of several equal ids of a call is the one stored, and
 * a failed allocation (VT_ERR_NOMEM) leaves the store as it was.  A document without vectors is legal and scores 0.0.
 * A search decodes the metric, validates the query vectors on their own, then compares their length with the store's
 * dimension (VT_ERR_DIMENSION) and only then goes to the device; without query vectors every document scores 0.0;
 * limit 0 still scores everything and returns an empty list.  Every call on a handle excludes every other call on it.
 * No CPU fallback: vt_mv_new without a device returns VT_ERR_DEVICE; a NULL handle is VT_ERR_ARGUMENT. */
typedef struct vt_mv vt_mv;
int vt_mv_new(int device, vt_mv **out);
void vt_mv_free(vt_mv *store);
/* upsert `count` documents; the layout is vt_multi_vector_top_k's (ids / id_off, doc_vec_off[count + 1], values / value_off) */
int vt_mv_put_many(vt_mv *store, size_t count, const char *ids, const size_t *id_off, const size_t *doc_vec_off,
                   const float *values, const size_t *value_off);
int vt_mv_delete(vt_mv *store, const char *id, size_t id_len); /* an unknown id: nothing happens, VT_OK */
size_t vt_mv_len(const vt_mv *store);                          /* live documents */
long vt_mv_dimension(const vt_mv *store);                      /* -1: no live document holds a vector */
int vt_mv_top_k(vt_mv *store, const float *query, const size_t *query_off, size_t nquery, int metric_code, size_t limit,
                vt_hits **out);
/* the same over the listed live documents only (unknown ids are skipped, a duplicate counts once; order and error
 * priority follow the store's order, not the list's) */
int vt_mv_top_k_ids(vt_mv *store, size_t count, const char *ids, const size_t *id_off, const float *query,
                    const size_t *query_off, size_t nquery, int metric_code, size_t limit, vt_hits **out);
/* Many query sets in one call.  Set b owns query vectors [set_vec_off[b], set_vec_off[b + 1]) of query / query_off, and,
 * for vt_mv_top_k_ids_batch, the candidate ids [set_id_off[b], set_id_off[b + 1]) of ids / id_off.  out[b] and
 * set_status[b] are exactly what vt_mv_top_k / vt_mv_top_k_ids return for set b called alone on the same store state:
 * ids, order, score bits, rank keys and status, the earliest failing document in store order deciding a set's status.
 * The whole call holds the handle's mutex once, so every set sees the same store.
 * The call's own failures return their status and leave every out[b] NULL: a NULL store, `out` or offset array is
 * VT_ERR_ARGUMENT, then an unknown metric VT_ERR_UNKNOWN_METRIC (decoded before any set is looked at).  A set's own
 * error -- an empty vector, ragged lengths, a non-finite value, a length other than the store's dimension, "metric
 * overflow" or "score overflow" on the device -- goes to set_status[b] with out[b] NULL while the call returns VT_OK
 * and the other sets are answered.  Without set_status (NULL) the first failing set in batch order gives the returned
 * status and every out[b] is NULL (vt_muvera_encode's convention).  nsets == 0 is VT_OK; limit 0 still scores, so
 * errors surface, and returns empty lists; a set without query vectors scores every document 0.0. */
int vt_mv_top_k_batch(vt_mv *store, size_t nsets, const size_t *set_vec_off /* nsets + 1 */, const float *query,
                      const size_t *query_off /* vectors + 1 */, int metric_code, size_t limit, vt_hits **out /* nsets */,
                      int *set_status /* nsets, may be NULL */);
int vt_mv_top_k_ids_batch(vt_mv *store, size_t nsets, const size_t *set_id_off /* nsets + 1 */, const char *ids,
                          const size_t *id_off, const size_t *set_vec_off, const float *query, const size_t *query_off,
                          int metric_code, size_t limit, vt_hits **out, int *set_status);
/* Totals since vt_mv_new -- scoring_launches: launches of a MaxSim scoring kernel by this handle's searches, single or
 * batched; batched_sets: query sets scored by the batched kernel (the others of a batch went through the single-set
 * path inside the same call).  Any out pointer may be NULL. */
int vt_mv_counters(const vt_mv *store, uint64_t *scoring_launches, uint64_t *batched_sets);
/* vectors: rows of live documents; row_capacity: rows the slab holds; dead_rows: rows of deleted or replaced documents
 * still in the slab; uploaded_bytes: bytes of document rows sent to the device since vt_mv_new (rows * row stride * 4:
 * searches add nothing); compactions: puts that closed the slab up first.  Any out pointer may be NULL. */
int vt_mv_memory(const vt_mv *store, size_t *vectors, size_t *row_capacity, size_t *dead_rows, uint64_t *uploaded_bytes,
                 uint64_t *compactions);

/* ------------------------------------------- HNSW index (approximate, graph-identical to the reference)
 * hnsw_new_*, hnsw_insert, hnsw_insert_many, hnsw_delete, hnsw_search, nifs.rs:311-426 -> hnsw.rs.  The reference's
 * HNSW is deterministic -- levels from an FNV-1a hash of the external id, neighbour selection a sort by (distance,
 * internal id), heaps under a total order --, so the contract is the usual one: after any inserts and deletes every
 * node's level, the entry and every adjacency list are the reference's, and a search returns its ids in its order with
 * the raw values' bits (vt_hits_raw).  The traversals run on the device, one wave each (csrc/vt_hnsw.hip); the graph's
 * book-keeping stays on the host (csrc/host/vt_hnswgraph.h).
 * vt_hnsw_new: a metric other than VT_L2, VT_COSINE (inside the graph the f32 dot with rank 1 - raw, distances.rs:50)
 * and VT_INNER_PRODUCT is VT_ERR_UNSUPPORTED (vt_last_error says so), then HnswParams::validate in its order
 * (VT_ERR_HNSW_*), and only then the device: VT_ERR_DEVICE without one, there is no CPU fallback.  The lane order is the
 * one in force (vt_set_default_reduce_order) when the handle is made.
 * vt_hnsw_insert: validate_vector against the index's dimension, then an existing node of that id goes, then the insert;
 * "metric overflow" in its traversal returns VT_ERR_OVERFLOW with the old node gone and the graph otherwise unchanged,
 * as in the reference.  vt_hnsw_insert_many validates every vector against the dimension -- or the first vector's
 * length -- before anything changes, then inserts in order: earlier inserts stay when a later one fails.  A device
 * failure half-way through a mutation poisons the handle (VT_ERR_HNSW_POISONED from then on).
 * vt_hnsw_search: limit 0 returns an empty list before the query is looked at, then validate_vector, then an empty
 * index returns an empty list; one traversal launch per call.  vt_hnsw_search_batch answers nq queries of d floats each
 * with one launch, every answer equal to the lone call's: with query_status a query's own error lands in
 * query_status[i] with out[i] NULL and the call returns VT_OK; without it the first failing query's status is returned
 * and every out[i] is NULL (vt_mv_top_k_batch's convention).
 * One mutex per handle: every call excludes every other.  A delete, and an insert of an id that exists, leaves the old
 * node's slab row and list words dead.  They come back on an insert, never on a delete: an insert that finds, behind its
 * own erasure, more dead rows than live nodes and at least 64 of them first gathers the survivors into a fresh slab and
 * renumbers every list entry on the device (compaction; the buffers may shrink), so the dead rows never exceed
 * max(live, 63) by more than the erasures since the last insert.  Graph, internal ids and hits are untouched by it.  A
 * card without room for the second set of buffers postpones it without an error; a mirror it finds apart from the graph
 * is VT_ERR_DEVICE and poisons the handle.  When the last node goes, slab and dimension go (the next insert may bring
 * another dimension; internal ids keep counting and are never reused); an internal-id counter at 2^32 returns
 * VT_ERR_NOMEM.  The slab holds at most 2^30 - 64 rows, dead ones included: a traversal on a larger slab returns
 * VT_ERR_UNSUPPORTED (vt_last_error says so). */
typedef struct vt_hnsw vt_hnsw;
int vt_hnsw_new(int metric_code, int device, size_t m, size_t m0, size_t ef_construction, size_t ef_search,
                size_t max_level, vt_hnsw **out);
void vt_hnsw_free(vt_hnsw *index);
int vt_hnsw_insert(vt_hnsw *index, const char *id, size_t id_len, const float *vector, size_t n);
int vt_hnsw_insert_many(vt_hnsw *index, size_t count, const char *ids, const size_t *id_off /* count + 1 */,
                        const float *values, const size_t *value_off /* count + 1 */);
int vt_hnsw_delete(vt_hnsw *index, const char *id, size_t id_len);
int vt_hnsw_search(vt_hnsw *index, const float *query, size_t n, size_t limit, vt_hits **out);
int vt_hnsw_search_batch(vt_hnsw *index, const float *queries, size_t nq, size_t d, size_t limit, vt_hits **out /* nq */,
                         int *query_status /* nq, may be NULL */);
/* quantized_search, funnel_search and hybrid_search (collection.ex:232-348) on the index's rows: vt_flat_quantized_search,
 * vt_flat_funnel_search and vt_flat_hybrid_search above also take an HNSW handle in the place of the flat one --
 * VT_HNSW_STAGED(index) -- and the library tells the two kinds apart (it knows every live vt_hnsw).  The set of exported
 * symbols is pinned (tests/test_fde_capi.py), so these searches have no entry points of their own.  The meanings, the
 * validation order, the statuses and the rules for an empty answer are the flat handle's, with the number of live nodes
 * for the row count -- over the same (id, vector) pairs the hits are the flat handle's, bit for bit: the slab holds the
 * vectors as given, and the stages order by (rank.total_cmp, id bytes).  VT_GEN_SEARCH is the index's own traversal with
 * limit = candidates (hnsw_candidates, collection.ex:594-600), its hits in result order.  The sign bits and prefixes are
 * read from the f32 rows where they lie (csrc/vt_hnsw_stage.hip); the first such call after the set of nodes changed
 * sorts the live ids once.  One mutex per handle, as for every other call; a poisoned handle answers
 * VT_ERR_HNSW_POISONED.  No other vt_flat_ function takes an HNSW handle. */
#define VT_HNSW_STAGED(index) ((vt_flat *)(index))
size_t vt_hnsw_len(const vt_hnsw *index);
long vt_hnsw_dimension(const vt_hnsw *index); /* -1: empty */
/* Inspection (tests compare the graph with the reference's): a live id's internal id, level and whether it is the
 * entry (VT_ERR_ARGUMENT: no such id); the internal ids of a node's list on one layer, in list order -- *count is the
 * list's length, at most cap of them are written (VT_ERR_ARGUMENT: no such node or layer). */
int vt_hnsw_node(const vt_hnsw *index, const char *id, size_t id_len, uint64_t *internal_id, uint32_t *level, int *is_entry);
int vt_hnsw_neighbors(const vt_hnsw *index, uint64_t internal_id, uint32_t layer, uint64_t *out, size_t cap, size_t *count);
/* Totals since vt_hnsw_new -- traversal_launches: launches of the traversal kernel; traversals: searches and insert
 * descents asked of it; reruns: traversals that outgrew their scratch and ran again with full-size scratch. */
int vt_hnsw_counters(const vt_hnsw *index, uint64_t *traversal_launches, uint64_t *traversals, uint64_t *reruns);
/* rows: slab rows handed out since the last compaction (live and dead; the live count right behind one); row_capacity:
 * rows the slab holds (1024 doubled until they fit; a compaction may shrink it); dead_rows: rows among `rows` whose node
 * was deleted or replaced (0 again at a compaction); edges: entries of all adjacency lists.  rows - dead_rows is
 * vt_hnsw_len.  Any out pointer may be NULL. */
int vt_hnsw_memory(const vt_hnsw *index, size_t *rows, size_t *row_capacity, size_t *dead_rows, size_t *edges);

/* ------------------------------------------- MMR reranking and diversified search
 * Vettore.Distance.mmr_rerank/5 (lib/vettore_distance.ex:334-519) and Vettore.rerank/4 (lib/vettore.ex:622-640): from an
 * initial list of (candidate, relevance score) the call chooses up to final_k candidates, each round the one with the
 * largest alpha * score - (1 - alpha) * (its largest pair_similarity to those chosen so far), the first such in list
 * order -- f32 metric values in the lane order in force, f64 combination, never fused.  The answer is `order`: indices
 * into the initial list in order of choice, min(final_k, count) of them (*order_len; `order` has room for that many);
 * the selection is the reference's for every input, and so is "metric overflow" (VT_ERR_OVERFLOW): a pair fails the call
 * in the round that scores it, a round that never runs fails nothing.  The rounds run on the device, one step launch
 * each (csrc/vt_mmr.hip), with one wait at the end; no vector comes back to the host.
 * vt_mmr_rerank: the candidates' vectors come with the call, row i of values ([count][d]) belonging to entry i.
 * Checked in this order: alpha outside [0, 1] (or NaN), final_k == 0 or a score outside the f32 range (or NaN) is
 * VT_ERR_MMR_ARGS; then the metric (VT_ERR_UNKNOWN_METRIC), d == 0 (VT_ERR_EMPTY), a non-finite value
 * (VT_ERR_NON_FINITE); only then the device (VT_ERR_DEVICE without one: no CPU fallback).  count == 0 is VT_OK with an
 * empty order.
 * vt_flat_mmr_rerank: the candidates are ids of a one-shard index, the metric and lane order the handle's, the rows read
 * where they lie in the slab.  After the checks on alpha, final_k and the scores, an id that is not in the index, or
 * occurs twice, is VT_ERR_MMR_ARGS.  A read: it shares the handle with searches.  A sharded handle returns
 * VT_ERR_UNSUPPORTED (vt_last_error says so), as do the two calls below.
 * vt_flat_mmr_search / _batch: vt_flat_search / vt_flat_search_batch with limit = candidates -- *out receives exactly
 * their hits, the candidate list --, then MMR over those hits under the same lease.  The initial scores are
 * result_values/3's (lib/vettore_distance.ex:525-546) for score_mode 0 (raw) or 1 (similarity), computed in f64 from the
 * hits' f32 raw values; any other score_mode is VT_ERR_MMR_ARGS, like a bad alpha or final_k.  `order` has room for
 * min(final_k, candidates) indices per query (query i's at order + i * that), order_len one entry per query.  All
 * queries of a batch are one chain of step launches.  A search error fails the call; a query's own MMR error follows
 * vt_hnsw_search_batch's convention: with query_status it lands in query_status[i] with out[i] NULL and the call
 * returns VT_OK, without it the first failing query's status is returned and every out[i] is NULL. */
int vt_mmr_rerank(int device, int metric_code, size_t count, size_t d, const float *values, const double *scores /* count */,
                  double alpha, size_t final_k, uint32_t *order, size_t *order_len);
int vt_flat_mmr_rerank(vt_flat *index, size_t count, const char *ids, const size_t *id_off /* count + 1 */,
                       const double *scores /* count */, double alpha, size_t final_k, uint32_t *order, size_t *order_len);
/* vt_flat_mmr_rerank for nprob problems in one chain of step launches: problem p owns entries [prob_off[p], prob_off[p + 1])
 * of ids (id_off is indexed by entry), scores and order, and has its own alpha[p] and final_k[p].  A problem's own error
 * (VT_ERR_MMR_ARGS, VT_ERR_OVERFLOW) lands in prob_status[p] with order_len[p] = 0 while the call returns VT_OK; without
 * prob_status the first failing problem's status is returned.  Every order equals the lone call's. */
int vt_flat_mmr_rerank_batch(vt_flat *index, size_t nprob, const size_t *prob_off /* nprob + 1 */, const char *ids,
                             const size_t *id_off /* entries + 1 */, const double *scores, const double *alpha /* nprob */,
                             const size_t *final_k /* nprob */, uint32_t *order, size_t *order_len /* nprob */,
                             int *prob_status /* nprob, may be NULL */);
int vt_flat_mmr_search(vt_flat *index, const float *query, size_t n, size_t candidates, size_t final_k, double alpha,
                       int score_mode, vt_hits **out, uint32_t *order, size_t *order_len);
int vt_flat_mmr_search_batch(vt_flat *index, const float *queries, size_t nq, size_t d, size_t candidates, size_t final_k,
                             double alpha, int score_mode, vt_hits **out /* nq */, uint32_t *order, size_t *order_len /* nq */,
                             int *query_status /* nq, may be NULL */);

/* ------------------------------------------- MUVERA (fixed-dimensional encoding)
 * muvera_encode_query/7, muvera_encode_document/7, nifs.rs:430-476 -> muvera.rs:26-74, for `count` sets of
 * vectors at once.  Set i owns vectors [set_vec_off[i], set_vec_off[i + 1]); vector j is
 * values[value_off[j] .. value_off[j + 1]).  mode 0 = query (per partition the sum of the projected
 * vectors), 1 = document (their running average).  final_is_some tells Some(final_projection_dimension)
 * -- Some(0) included, which is an error -- from None.  `out` is [count][vt_muvera_fde_dimension(...)],
 * bit-identical to the reference's encode().
 *
 * Validation happens on the host before any device call, in the reference's order (muvera.rs:76-106,
 * then :29-42).  With count == 1 the call is the NIF: the set's error is the returned status.  With more
 * sets an error of the configuration fails the call, and a set's own error ("empty vectors", "dimension
 * mismatch", a non-finite value, "encoding overflow") goes to set_status[i] and leaves row i of `out`
 * zero while the call returns VT_OK; without set_status the first failing set's status is returned.
 * Encoding a set inside a batch gives the bytes that encoding it alone gives.  No CPU fallback: a valid
 * call without a device returns VT_ERR_DEVICE; a dimension above 16 384 returns VT_ERR_UNSUPPORTED. */
int vt_muvera_encode(int device, int mode, size_t count, const size_t *set_vec_off /* count + 1 */,
                     const float *values, const size_t *value_off /* vectors + 1 */, size_t dimension,
                     size_t num_repetitions, size_t num_simhash_projections, uint64_t seed,
                     size_t projection_dimension, size_t final_projection_dimension, int final_is_some,
                     float *out, int *set_status /* count, may be NULL */);
/* Length of an encoding under this configuration; 0 when the configuration is not valid. */
size_t vt_muvera_fde_dimension(size_t num_repetitions, size_t num_simhash_projections, size_t projection_dimension,
                               size_t final_projection_dimension, int final_is_some);

/* ------------------------------------------- MUVERA retrieval over a resident multi-vector store
 * The reference's four steps (README, "MUVERA": encode the query, encode every document, search the encodings with
 * inner product, rerank the candidates with exact MaxSim -- muvera.rs:26-74, flat.rs:98-135, multi_vector.rs:40-122)
 * joined over documents that are already in device memory.  The configuration is vt_muvera_encode's seven trailing
 * arguments.  `index` is a flat handle that holds one row per encodable document, its document-mode encoding:
 * single-shard (else VT_ERR_UNSUPPORTED, vt_last_error says so), on the store's device (else VT_ERR_ARGUMENT), with
 * metric VT_INNER_PRODUCT (else VT_ERR_ARGUMENT), and, when it is not empty, of the encoding's dimension (else
 * VT_ERR_DIMENSION, before anything changes).  A NULL handle is VT_ERR_ARGUMENT.
 *
 * vt_mv_encode_documents: row i of `out` is what vt_muvera_encode(mode 1) returns for the vectors of document ids[i], bit
 * for bit, read from the store's rows (no upload).  The call's own checks, in order: NULL arguments, the configuration
 * (muvera.rs:81-95), the sizes (:29-42), VT_ERR_DIMENSION when the store has a dimension other than `dimension`.  A
 * listed id that is not live, or a live document without vectors, is VT_ERR_EMPTY_SET (muvera.rs:79) with a zero row;
 * "encoding overflow" on the device (muvera.rs:175, :195) likewise.  With doc_status NULL, or count 1, the first failing
 * document's status is returned (vt_muvera_encode's convention).
 *
 * vt_mv_fde_sync brings `index` in line with the store for the listed ids (count 0 with ids NULL: every live document,
 * in store order).  After VT_OK `index` holds a listed id, with exactly the row above, if the store holds it live with a
 * vector and its encoding succeeded, and does not hold it otherwise; every other id of `index` is untouched; a duplicate
 * counts once.  doc_status: VT_OK for a document stored and for an id that is not live (removed from `index`),
 * VT_ERR_EMPTY_SET for a live document without vectors (removed), VT_ERR_ENCODING_OVERFLOW (removed); with doc_status
 * NULL the first failing document's status is returned, the index synced for every listed id all the same.  The
 * encodings never visit the host.  The store's mutex is held for the whole call and the index is changed through its own
 * entry points under its own lock: a search of `index` that runs meanwhile may see the sync half applied.  A device
 * failure half-way leaves the store untouched and the index possibly partly synced; calling again repairs it.
 *
 * vt_mv_fde_top_k answers exactly vt_mv_top_k_ids(store, ids of H, query, metric, limit) -- ids, order, score bits, rank
 * keys -- where H = vt_flat_search(index, the query-mode encoding of `query`, candidates), under one hold of the store's
 * mutex.  Statuses arise in this order: NULL arguments; the index requirements; vt_mv_top_k's validation up to the device
 * (metric, the query vectors on their own, their length against the store's dimension); vt_muvera_encode(mode 0, count
 * 1)'s (no query vector: VT_ERR_EMPTY_SET); vt_flat_search's; the rerank's.  limit 0 still does all the work and returns
 * an empty list; candidates 0 or an empty index returns an empty list.
 *
 * vt_mv_fde_top_k_batch: out[b] and set_status[b] are vt_mv_fde_top_k's for set b on the same state, in one encoding
 * call, one vt_flat_search_batch and one batched rerank; NULL set_status, call-level failures and nsets == 0 follow
 * vt_mv_top_k_ids_batch. */
int vt_mv_encode_documents(vt_mv *store, size_t count, const char *ids, const size_t *id_off, size_t dimension,
                           size_t num_repetitions, size_t num_simhash_projections, uint64_t seed, size_t projection_dimension,
                           size_t final_projection_dimension, int final_is_some, float *out /* [count][fde] */,
                           int *doc_status /* count, may be NULL */);
int vt_mv_fde_sync(vt_mv *store, vt_flat *index, size_t count, const char *ids, const size_t *id_off, size_t dimension,
                   size_t num_repetitions, size_t num_simhash_projections, uint64_t seed, size_t projection_dimension,
                   size_t final_projection_dimension, int final_is_some, int *doc_status /* count, may be NULL */);
int vt_mv_fde_top_k(vt_mv *store, vt_flat *index, size_t dimension, size_t num_repetitions, size_t num_simhash_projections,
                    uint64_t seed, size_t projection_dimension, size_t final_projection_dimension, int final_is_some,
                    const float *query, const size_t *query_off, size_t nquery, size_t candidates, int metric_code,
                    size_t limit, vt_hits **out);
int vt_mv_fde_top_k_batch(vt_mv *store, vt_flat *index, size_t dimension, size_t num_repetitions,
                          size_t num_simhash_projections, uint64_t seed, size_t projection_dimension,
                          size_t final_projection_dimension, int final_is_some, size_t nsets,
                          const size_t *set_vec_off /* nsets + 1 */, const float *query, const size_t *query_off,
                          size_t candidates, int metric_code, size_t limit, vt_hits **out /* nsets */,
                          int *set_status /* nsets, may be NULL */);

/* ------------------------------------------------------------ profiling
 * Device-side timing of the dominant kernels with HIP events on the stream the
 * kernels are launched on (bench.py's roofline figure). */
typedef struct vt_profile {
  uint64_t scan_launches;   /* flat scan + fused top-k kernel launches */
  double scan_ms;           /* sum of their durations (hipEventElapsedTime) */
  uint64_t scan_rows;       /* rows scanned by those launches */
  uint64_t scan_bytes;      /* algorithmic bytes: rows * d * 4 */
  uint64_t hamming_launches; /* packed-bit passes: quantized candidates; flat searches under float hamming / jaccard */
  double hamming_ms;
  uint64_t hamming_bytes;   /* rows * ceil(d/64) * 8 per launch (one launch may serve up to 8 queries) */
  uint64_t merge_launches;
  double merge_ms;
  uint64_t batch_launches;  /* MFMA candidate passes (one per <= 256 queries) */
  double batch_ms;
  double batch_flops;       /* 2 * rows * padded queries * padded dims per pass */
  uint64_t batch_queries;
  uint64_t batch_fallbacks; /* queries the bound could not certify (re-run singly) */
  uint64_t prefix_launches; /* funnel stages over ALL rows: f64 cosine prefix scans, K1 / K1p prefix sweeps, K4 passes over the bit column's prefix */
  double prefix_ms;
  uint64_t prefix_bytes;    /* rows * prefix dimensions * 4 (rows * ceil(prefix / 64) * 8 from the bit column) */
  /* K2b: candidate passes with bf16 operands (HBM-bound; batch_* above count the FP32 passes) */
  uint64_t nominate_launches;
  double nominate_ms;
  uint64_t nominate_bytes;        /* algorithmic bytes: what a pass reads -- rows * d * 4 from the f32 rows, rows * d * 2 from the bf16 shadow */
  double nominate_flops;          /* 2 * rows * 256 * padded dims per pass */
  uint64_t nominate_queries;
  uint64_t nominate_second_passes; /* passes re-run with thresholds from a first pass's exact hits */
  uint64_t nominate_candidates;   /* rows handed to the exact rescoring, summed over queries */
  uint64_t hamming_queries;       /* queries served by grouped passes over a bit column: quantized groups, float hamming / jaccard batches (0 for single-query passes) */
  uint64_t hybrid_device_chains;  /* hybrid searches whose generators, union and rerank ran as one device chain (one host wait) */
  uint64_t prefix_queries;        /* queries served by grouped prefix scans (0 for single-query funnel searches) */
  /* r04 (VT_ABI_VERSION 3) */
  uint64_t nominate_shadow_launches; /* of nominate_launches: the passes that read the bf16 shadow (K2s) */
  uint64_t shadow_builds;            /* whole-image builds of the bf16 shadow */
  double shadow_build_ms;
  uint64_t shadow_patched_rows;      /* rows re-rounded in place after mutations */
  uint64_t sweep_queries;            /* plain searches of a batch served by K1p sweeps (their sweeps count as scan_launches) */
  /* K1q: lone searches nominated from the int8 sketch (its passes count as scan_launches / scan_ms / scan_bytes too) */
  uint64_t sketch_launches;          /* passes over the sketch */
  double sketch_ms;
  uint64_t sketch_bytes;             /* what the passes read: whole tiles of int8 rows and their metadata */
  uint64_t sketch_candidates;        /* rows handed to the exact rescoring, summed over passes */
  uint64_t sketch_fallbacks;         /* passes the bound could not certify (the search then scanned the f32 rows) */
  uint64_t sketch_builds;            /* whole builds of the sketch */
  uint64_t sketch_patched_rows;      /* rows re-quantised in place after mutations */
  uint64_t sketch_tail_rescored;     /* certified passes whose candidates the certifying block rescored itself (no gathered K1) */
  /* K1s: lone searches nominated from the 6-bit sketch (its passes count as scan_launches / scan_ms / scan_bytes too) */
  uint64_t sketch6_launches;         /* passes over the 6-bit sketch */
  double sketch6_ms;
  uint64_t sketch6_bytes;            /* what the passes read: whole tiles of both planes and their metadata */
  uint64_t sketch6_candidates;       /* rows handed to the gathered K1, summed over passes */
  uint64_t sketch6_fallbacks;        /* passes the bound could not certify (the int8 sketch or the f32 rows then served) */
  uint64_t sketch6_builds;           /* whole builds of the 6-bit sketch */
  uint64_t sketch6_patched_rows;     /* rows re-quantised in place after mutations */
  uint64_t sketch6_tail_words;       /* passes whose tail read the pass's word arrays (not the lists themselves) */
  /* K1f: lone searches nominated from the 5-bit sketch (its passes count as scan_launches / scan_ms / scan_bytes too) */
  uint64_t sketch5_launches;         /* passes over the 5-bit sketch */
  double sketch5_ms;
  uint64_t sketch5_bytes;            /* what the passes read: whole tiles of both planes and their metadata */
  uint64_t sketch5_candidates;       /* rows handed to the gathered K1, summed over passes */
  uint64_t sketch5_fallbacks;        /* passes the bound could not certify (the 6-bit sketch, the int8 sketch or the f32 rows then served) */
  uint64_t sketch5_builds;           /* whole builds of the 5-bit sketch */
  uint64_t sketch5_patched_rows;     /* rows re-quantised in place after mutations */
  /* K1n: lone searches nominated from the 4-bit sketch (its passes count as scan_launches / scan_ms / scan_bytes too) */
  uint64_t sketch4_launches;         /* passes over the 4-bit sketch */
  double sketch4_ms;
  uint64_t sketch4_bytes;            /* what the passes read: whole tiles and their metadata */
  uint64_t sketch4_candidates;       /* rows handed to the gathered K1, summed over passes */
  uint64_t sketch4_fallbacks;        /* passes the bound could not certify (the 5-bit sketch and what lies behind it then served) */
  uint64_t sketch4_builds;           /* whole builds of the 4-bit sketch */
  uint64_t sketch4_patched_rows;     /* rows re-quantised in place after mutations */
  uint64_t sketch4_best;             /* searches whose exact threshold came from each list's best rows, inside the pass (no launch between pass and rescore) */
  uint64_t sketch4_finished;        /* searches whose result the filtered K1 behind the pass wrote itself (no select, one wait) */
  /* K1qm: batches and meeting callers of 2..8 queries nominated from one pass over the int8 sketch (the lone counters
   * above are not touched by these passes) */
  uint64_t sketch_batch_launches;    /* group passes over the int8 sketch */
  uint64_t sketch_batch_queries;     /* queries that entered a group pass */
  double sketch_batch_ms;
  uint64_t sketch_batch_bytes;       /* what the group passes read: whole tiles and their metadata, once per group */
  uint64_t sketch_batch_candidates;  /* candidates the groups' tail blocks counted, summed over queries */
  uint64_t sketch_batch_fallbacks;   /* queries a group handed on unanswered (not certified, or a candidate list too long for the tail's block) */
  uint64_t sketch_batch_tail_rescored; /* queries finished by their tail block */
} vt_profile;
int vt_flat_set_profiling(vt_flat *index, int enabled);
int vt_flat_get_profile(vt_flat *index, vt_profile *out, int reset);
/* The same for a caller that says how large ITS vt_profile is: at most `out_bytes` are written
 * (a binding built against an older header keeps working). */
int vt_flat_get_profile_sized(vt_flat *index, void *out, size_t out_bytes, int reset);

#ifdef __cplusplus
}
#endif
#endif
