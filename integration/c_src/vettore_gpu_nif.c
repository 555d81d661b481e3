/*
 * vettore_gpu_nif.c -- erl_nif shim between Elixir module Vettore.Gpu.Nifs and
 * libvettore_hip.so (include/vettore_flat.h).  It is to the C ABI what
 * native/vettore/src/nifs.rs is to the Rust crate: term decoding/encoding, the
 * resource object, error tuples with the reference's strings
 * (nifs.rs:107-129, :151-175, :200-309).
 *
 * Build where OTP is installed (this repository's build image has no erl_nif.h):
 *   cc -O2 -fPIC -shared -I"$ERL_INCLUDE" -I../../include vettore_gpu_nif.c \
 *      -L../../vettore_amd/lib -lvettore_hip -o priv/vettore_gpu_nif.so
 *
 * Every NIF is a dirty job (nifs.rs marks all of them schedule = "DirtyCpu"): a
 * search blocks its scheduler thread for the duration of the scan.
 */
#include <erl_nif.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "vettore_flat.h"

static ErlNifResourceType *FLAT;
typedef struct { vt_flat *h; } flat_res;

static void flat_dtor(ErlNifEnv *env, void *obj) {
  (void)env;
  vt_flat_free(((flat_res *)obj)->h); /* ResourceArc drop: HBM, streams, pinned staging */
}

static ErlNifResourceType *HNSW;
typedef struct { vt_hnsw *h; } hnsw_res;

static void hnsw_dtor(ErlNifEnv *env, void *obj) {
  (void)env;
  vt_hnsw_free(((hnsw_res *)obj)->h);
}

/* ---------------------------------------------------------------- terms */
static ERL_NIF_TERM mk_atom(ErlNifEnv *env, const char *a) { return enif_make_atom(env, a); }

static ERL_NIF_TERM mk_binary(ErlNifEnv *env, const char *p, size_t n) {
  ERL_NIF_TERM t;
  memcpy(enif_make_new_binary(env, n, &t), p, n);
  return t;
}

/* {:error, "dimension mismatch"} etc.; device/unsupported errors carry vt_last_error() */
static ERL_NIF_TERM mk_error(ErlNifEnv *env, int st) {
  const char *msg = (st == VT_ERR_DEVICE || st == VT_ERR_UNSUPPORTED) ? vt_last_error() : vt_strerror(st);
  if (st == VT_ERR_ARGUMENT) return enif_make_badarg(env);
  return enif_make_tuple2(env, mk_atom(env, "error"), mk_binary(env, msg, strlen(msg)));
}

/* Ok(()) as rustler encodes it: {:ok, {}} (vector_algorithms_hardening_test.exs:56) */
static ERL_NIF_TERM mk_ok_unit(ErlNifEnv *env) {
  return enif_make_tuple2(env, mk_atom(env, "ok"), enif_make_tuple(env, 0));
}

/* Vec<(String, f32)> -> [{binary, float}]; frees the hits */
static ERL_NIF_TERM hits_to_list(ErlNifEnv *env, vt_hits *h) {
  ERL_NIF_TERM list = enif_make_list(env, 0);
  for (size_t i = vt_hits_len(h); i-- > 0;) {
    size_t len;
    const char *id = vt_hits_id(h, i, &len);
    ERL_NIF_TERM pair = enif_make_tuple2(env, mk_binary(env, id, len), enif_make_double(env, (double)vt_hits_raw(h, i)));
    list = enif_make_list_cell(env, pair, list);
  }
  vt_hits_free(h);
  return list;
}

static ERL_NIF_TERM ok_hits(ErlNifEnv *env, vt_hits *h) {
  return enif_make_tuple2(env, mk_atom(env, "ok"), hits_to_list(env, h));
}

/* [float] -> malloc'ed f32 array.  Anything but a float, or a double outside the f32 range,
 * is a decode failure = badarg, as with rustler's Vec<f32> (SURVEY 8b conventions; the Elixir
 * layer converts integers with `/ 1` before the call, vettore_distance.ex:659-660). */
static int get_f32_list(ErlNifEnv *env, ERL_NIF_TERM list, float **out, size_t *n) {
  unsigned len;
  if (!enif_get_list_length(env, list, &len)) return 0;
  float *v = (float *)malloc((len ? len : 1) * sizeof(float));
  if (!v) return 0;
  ERL_NIF_TERM head, tail = list;
  for (unsigned i = 0; i < len; ++i) {
    double d;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_double(env, head, &d)) { free(v); return 0; }
    if (d > 3.4028234663852886e38 || d < -3.4028234663852886e38) { free(v); return 0; }
    v[i] = (float)d;
  }
  *out = v;
  *n = len;
  return 1;
}

static int get_size(ErlNifEnv *env, ERL_NIF_TERM t, size_t *out) {
  ErlNifUInt64 v;
  if (!enif_get_uint64(env, t, &v)) return 0;
  *out = (size_t)v;
  return 1;
}

static int get_size_list(ErlNifEnv *env, ERL_NIF_TERM list, size_t **out, size_t *n) {
  unsigned len;
  if (!enif_get_list_length(env, list, &len)) return 0;
  size_t *v = (size_t *)malloc((len ? len : 1) * sizeof(size_t));
  if (!v) return 0;
  ERL_NIF_TERM head, tail = list;
  for (unsigned i = 0; i < len; ++i) {
    if (!enif_get_list_cell(env, tail, &head, &tail) || !get_size(env, head, &v[i])) { free(v); return 0; }
  }
  *out = v;
  *n = len;
  return 1;
}

static flat_res *get_flat(ErlNifEnv *env, ERL_NIF_TERM t) {
  flat_res *r;
  return enif_get_resource(env, t, FLAT, (void **)&r) ? r : NULL;
}

/* ------------------------------------------------------- index lifecycle */
/* flat_new(metric_code, [device]) -> reference | {:error, binary}
 * nifs.rs:200-257 (one NIF per metric there).  One device: a plain index; several: ONE resource
 * whose rows are spread over those GPUs (vt_flat_new_sharded) -- still one reference, one process. */
static ERL_NIF_TERM flat_new(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  int code;
  unsigned ndev;
  (void)argc;
  if (!enif_get_int(env, argv[0], &code) || !enif_get_list_length(env, argv[1], &ndev) || ndev == 0 || ndev > 64)
    return enif_make_badarg(env);
  int devs[64];
  ERL_NIF_TERM head, tail = argv[1];
  for (unsigned i = 0; i < ndev; ++i)
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_int(env, head, &devs[i]) || devs[i] < 0)
      return enif_make_badarg(env);
  vt_flat *h;
  int st = vt_flat_new_sharded(code, devs, ndev, &h);
  if (st != VT_OK) return mk_error(env, st);
  flat_res *r = (flat_res *)enif_alloc_resource(FLAT, sizeof *r);
  r->h = h;
  ERL_NIF_TERM t = enif_make_resource(env, r);
  enif_release_resource(r);
  return t;
}

/* flat_insert(ref, id, [float]) -> {:ok, {}} | {:error, binary}        nifs.rs:259-271 */
static ERL_NIF_TERM flat_insert(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  flat_res *r = get_flat(env, argv[0]);
  ErlNifBinary id;
  float *v;
  size_t n;
  (void)argc;
  if (!r || !enif_inspect_binary(env, argv[1], &id) || !get_f32_list(env, argv[2], &v, &n)) return enif_make_badarg(env);
  int st = vt_flat_insert(r->h, (const char *)id.data, id.size, v, n);
  free(v);
  return st == VT_OK ? mk_ok_unit(env) : mk_error(env, st);
}

/* flat_insert_many(ref, [{id, [float]}]) -> {:ok, {}} | {:error, binary}   nifs.rs:273-284
 * (atomic: libvettore_hip validates every row before storing any, flat.rs:69-85) */
static ERL_NIF_TERM flat_insert_many(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  flat_res *r = get_flat(env, argv[0]);
  unsigned count;
  (void)argc;
  if (!r || !enif_get_list_length(env, argv[1], &count)) return enif_make_badarg(env);
  size_t *id_off = (size_t *)calloc(count + 1, sizeof(size_t));
  size_t *val_off = (size_t *)calloc(count + 1, sizeof(size_t));
  size_t ids_cap = 64, vals_cap = 64;
  char *ids = (char *)malloc(ids_cap);
  float *vals = (float *)malloc(vals_cap * sizeof(float));
  int ok = id_off && val_off && ids && vals;
  ERL_NIF_TERM head, tail = argv[1];
  for (unsigned i = 0; ok && i < count; ++i) {
    const ERL_NIF_TERM *pair;
    int arity;
    ErlNifBinary id;
    float *v = NULL;
    size_t n = 0;
    ok = enif_get_list_cell(env, tail, &head, &tail) && enif_get_tuple(env, head, &arity, &pair) && arity == 2 &&
         enif_inspect_binary(env, pair[0], &id) && get_f32_list(env, pair[1], &v, &n);
    if (!ok) break;
    if (id_off[i] + id.size > ids_cap) {
      ids_cap = (id_off[i] + id.size) * 2 + 64;
      ids = (char *)realloc(ids, ids_cap);
    }
    if (val_off[i] + n > vals_cap) {
      vals_cap = (val_off[i] + n) * 2 + 64;
      vals = (float *)realloc(vals, vals_cap * sizeof(float));
    }
    ok = ids && vals;
    if (ok) {
      memcpy(ids + id_off[i], id.data, id.size);
      memcpy(vals + val_off[i], v, n * sizeof(float));
      id_off[i + 1] = id_off[i] + id.size;
      val_off[i + 1] = val_off[i] + n;
    }
    free(v);
  }
  ERL_NIF_TERM res;
  if (!ok) {
    res = enif_make_badarg(env);
  } else {
    int st = vt_flat_insert_many(r->h, count, ids, id_off, vals, val_off);
    res = st == VT_OK ? mk_ok_unit(env) : mk_error(env, st);
  }
  free(ids); free(vals); free(id_off); free(val_off);
  return res;
}

/* flat_load_binary(ref, [id], rows :: binary, d) -> {:ok, {}} | {:error, binary}
 * Bulk ingest without list cells: `rows` is count * d native-endian f32 (e.g. built with
 * <<x::float-32-native>> or Nx.to_binary/1).  Same semantics as insert_many.   */
static ERL_NIF_TERM flat_load_binary(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  flat_res *r = get_flat(env, argv[0]);
  unsigned count;
  ErlNifBinary rows;
  size_t d;
  (void)argc;
  if (!r || !enif_get_list_length(env, argv[1], &count) || !enif_inspect_binary(env, argv[2], &rows) ||
      !get_size(env, argv[3], &d) || rows.size != (size_t)count * d * sizeof(float))
    return enif_make_badarg(env);
  size_t *id_off = (size_t *)calloc(count + 1, sizeof(size_t));
  size_t ids_cap = 64;
  char *ids = (char *)malloc(ids_cap);
  int ok = id_off != NULL && ids != NULL;
  ERL_NIF_TERM head, tail = argv[1];
  for (unsigned i = 0; ok && i < count; ++i) {
    ErlNifBinary id;
    ok = enif_get_list_cell(env, tail, &head, &tail) && enif_inspect_binary(env, head, &id);
    if (!ok) break;
    if (id_off[i] + id.size > ids_cap) {
      ids_cap = (id_off[i] + id.size) * 2 + 64;
      ids = (char *)realloc(ids, ids_cap);
      ok = ids != NULL;
      if (!ok) break;
    }
    memcpy(ids + id_off[i], id.data, id.size);
    id_off[i + 1] = id_off[i] + id.size;
  }
  ERL_NIF_TERM res;
  if (!ok) {
    res = enif_make_badarg(env);
  } else {
    int st = vt_flat_load_matrix(r->h, count, d, ids, id_off, (const float *)rows.data);
    res = st == VT_OK ? mk_ok_unit(env) : mk_error(env, st);
  }
  free(ids); free(id_off);
  return res;
}

/* flat_delete(ref, id) -> {:ok, {}}                                      nifs.rs:286-295 */
static ERL_NIF_TERM flat_delete(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  flat_res *r = get_flat(env, argv[0]);
  ErlNifBinary id;
  (void)argc;
  if (!r || !enif_inspect_binary(env, argv[1], &id)) return enif_make_badarg(env);
  int st = vt_flat_delete(r->h, (const char *)id.data, id.size);
  return st == VT_OK ? mk_ok_unit(env) : mk_error(env, st);
}

/* ----------------------------------------------------------------- search */
/* flat_search(ref, [float], limit) -> {:ok, [{id, raw}]} | {:error, binary}   nifs.rs:297-309 */
static ERL_NIF_TERM flat_search(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  flat_res *r = get_flat(env, argv[0]);
  float *q;
  size_t n, limit;
  (void)argc;
  if (!r || !get_f32_list(env, argv[1], &q, &n) || !get_size(env, argv[2], &limit)) return enif_make_badarg(env);
  vt_hits *h;
  int st = vt_flat_search(r->h, q, n, limit, &h);
  free(q);
  return st == VT_OK ? ok_hits(env, h) : mk_error(env, st);
}

/* flat_search_batch(ref, [[float]], limit) -> {:ok, [[{id, raw}]]}: B x flat_search in one pass
 * over the corpus (FP32 matrix cores + exact rescoring); all queries must have the same length */
static ERL_NIF_TERM flat_search_batch(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  flat_res *r = get_flat(env, argv[0]);
  unsigned nq;
  size_t limit, d = 0;
  (void)argc;
  if (!r || !enif_get_list_length(env, argv[1], &nq) || !get_size(env, argv[2], &limit)) return enif_make_badarg(env);
  if (nq == 0) return enif_make_tuple2(env, mk_atom(env, "ok"), enif_make_list(env, 0));
  float *qs = NULL;
  ERL_NIF_TERM head, tail = argv[1];
  for (unsigned i = 0; i < nq; ++i) {
    float *q;
    size_t n;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !get_f32_list(env, head, &q, &n)) { free(qs); return enif_make_badarg(env); }
    if (i == 0) {
      d = n;
      qs = (float *)malloc((size_t)nq * (d ? d : 1) * sizeof(float));
    }
    if (!qs || n != d) { free(q); free(qs); return n != d ? mk_error(env, VT_ERR_DIMENSION) : enif_make_badarg(env); }
    memcpy(qs + (size_t)i * d, q, d * sizeof(float));
    free(q);
  }
  vt_hits **out = (vt_hits **)calloc(nq, sizeof(vt_hits *));
  int st = out ? vt_flat_search_batch(r->h, qs, nq, d, limit, out) : VT_ERR_NOMEM;
  free(qs);
  if (st != VT_OK) { free(out); return mk_error(env, st); }
  ERL_NIF_TERM list = enif_make_list(env, 0);
  for (unsigned i = nq; i-- > 0;) list = enif_make_list_cell(env, hits_to_list(env, out[i]), list);
  free(out);
  return enif_make_tuple2(env, mk_atom(env, "ok"), list);
}

/* [[float]] -> one malloc'ed [nq][d] f32 matrix; *st = VT_ERR_DIMENSION when the rows differ in length */
static int get_f32_matrix(ErlNifEnv *env, ERL_NIF_TERM list, unsigned nq, float **out, size_t *d, int *st) {
  float *qs = NULL;
  ERL_NIF_TERM head, tail = list;
  *st = VT_OK;
  *d = 0;
  for (unsigned i = 0; i < nq; ++i) {
    float *q;
    size_t n;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !get_f32_list(env, head, &q, &n)) { free(qs); return 0; }
    if (i == 0) {
      *d = n;
      qs = (float *)malloc((size_t)nq * (n ? n : 1) * sizeof(float));
    }
    if (!qs || n != *d) {
      free(q);
      free(qs);
      if (n != *d) { *st = VT_ERR_DIMENSION; return 1; }
      return 0;
    }
    memcpy(qs + (size_t)i * n, q, n * sizeof(float));
    free(q);
  }
  *out = qs;
  return 1;
}

/* [vt_hits *] -> [[{id, raw}]] (frees them) */
static ERL_NIF_TERM hit_lists(ErlNifEnv *env, vt_hits **out, unsigned nq) {
  ERL_NIF_TERM list = enif_make_list(env, 0);
  for (unsigned i = nq; i-- > 0;) list = enif_make_list_cell(env, hits_to_list(env, out[i]), list);
  return enif_make_tuple2(env, mk_atom(env, "ok"), list);
}

/* flat_quantized_search_batch(ref, [[float]], candidates, limit) -> {:ok, [[{id, raw}]]}: B x
 * quantized_search, groups of up to eight sharing one sweep of the sign bits */
static ERL_NIF_TERM flat_quantized_search_batch(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  flat_res *r = get_flat(env, argv[0]);
  unsigned nq;
  size_t candidates, limit, d;
  float *qs;
  int st;
  (void)argc;
  if (!r || !enif_get_list_length(env, argv[1], &nq) || !get_size(env, argv[2], &candidates) || !get_size(env, argv[3], &limit))
    return enif_make_badarg(env);
  if (nq == 0) return enif_make_tuple2(env, mk_atom(env, "ok"), enif_make_list(env, 0));
  if (!get_f32_matrix(env, argv[1], nq, &qs, &d, &st)) return enif_make_badarg(env);
  if (st != VT_OK) return mk_error(env, st);
  vt_hits **out = (vt_hits **)calloc(nq, sizeof(vt_hits *));
  st = out ? vt_flat_quantized_search_batch(r->h, qs, nq, d, candidates, limit, out) : VT_ERR_NOMEM;
  free(qs);
  if (st != VT_OK) { free(out); return mk_error(env, st); }
  ERL_NIF_TERM res = hit_lists(env, out, nq);
  free(out);
  return res;
}

/* flat_quantized_search(ref, [float], candidates, limit)   collection.ex:276-295 in one call */
static ERL_NIF_TERM flat_quantized_search(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  flat_res *r = get_flat(env, argv[0]);
  float *q;
  size_t n, candidates, limit;
  (void)argc;
  if (!r || !get_f32_list(env, argv[1], &q, &n) || !get_size(env, argv[2], &candidates) || !get_size(env, argv[3], &limit))
    return enif_make_badarg(env);
  vt_hits *h;
  int st = vt_flat_quantized_search(r->h, q, n, candidates, limit, &h);
  free(q);
  return st == VT_OK ? ok_hits(env, h) : mk_error(env, st);
}

/* flat_funnel_search(ref, [float], [stage], candidates, limit)   collection.ex:245-260, :674-691 */
static ERL_NIF_TERM flat_funnel_search(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  flat_res *r = get_flat(env, argv[0]);
  float *q;
  size_t n, nst, candidates, limit, *stages;
  (void)argc;
  if (!r || !get_f32_list(env, argv[1], &q, &n)) return enif_make_badarg(env);
  if (!get_size_list(env, argv[2], &stages, &nst) || !get_size(env, argv[3], &candidates) || !get_size(env, argv[4], &limit)) {
    free(q);
    return enif_make_badarg(env);
  }
  vt_hits *h;
  int st = vt_flat_funnel_search(r->h, q, n, stages, nst, candidates, limit, &h);
  free(q); free(stages);
  return st == VT_OK ? ok_hits(env, h) : mk_error(env, st);
}

/* flat_funnel_search_batch(ref, [[float]], [stage], candidates, limit) -> {:ok, [[{id, raw}]]}: B x
 * funnel_search with one set of stages; on a cosine collection groups of up to eight share the
 * stage-1 sweep of the prefixes */
static ERL_NIF_TERM flat_funnel_search_batch(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  flat_res *r = get_flat(env, argv[0]);
  unsigned nq;
  size_t candidates, limit, d, nst, *stages;
  float *qs;
  int st;
  (void)argc;
  if (!r || !enif_get_list_length(env, argv[1], &nq) || !get_size(env, argv[3], &candidates) || !get_size(env, argv[4], &limit))
    return enif_make_badarg(env);
  if (nq == 0) return enif_make_tuple2(env, mk_atom(env, "ok"), enif_make_list(env, 0));
  if (!get_size_list(env, argv[2], &stages, &nst)) return enif_make_badarg(env);
  if (!get_f32_matrix(env, argv[1], nq, &qs, &d, &st)) { free(stages); return enif_make_badarg(env); }
  if (st != VT_OK) { free(stages); return mk_error(env, st); }
  vt_hits **out = (vt_hits **)calloc(nq, sizeof(vt_hits *));
  st = out ? vt_flat_funnel_search_batch(r->h, qs, nq, d, stages, nst, candidates, limit, out) : VT_ERR_NOMEM;
  free(qs); free(stages);
  if (st != VT_OK) { free(out); return mk_error(env, st); }
  ERL_NIF_TERM res = hit_lists(env, out, nq);
  free(out);
  return res;
}

/* flat_hybrid_search(ref, [float], [{kind, candidates, [stage]}], limit)   collection.ex:325-345, :515-592
 * kind: 0 funnel, 1 quantized, 2 search; rerank: :exact */
static hnsw_res *get_hnsw(ErlNifEnv *env, ERL_NIF_TERM t);
/* (one body for both kinds of handle: hnsw_hybrid_search, further down, is the same call over the HNSW resource) */
static ERL_NIF_TERM hybrid_search_on(ErlNifEnv *env, const ERL_NIF_TERM argv[], int on_hnsw) {
  flat_res *r = on_hnsw ? NULL : get_flat(env, argv[0]);
  hnsw_res *g = on_hnsw ? get_hnsw(env, argv[0]) : NULL;
  float *q;
  size_t n, limit;
  unsigned ngen;
  if ((!r && !g) || !enif_get_list_length(env, argv[2], &ngen) || !get_size(env, argv[3], &limit) || !get_f32_list(env, argv[1], &q, &n))
    return enif_make_badarg(env);
  int *kinds = (int *)calloc(ngen + 1, sizeof(int));
  size_t *cands = (size_t *)calloc(ngen + 1, sizeof(size_t));
  size_t *off = (size_t *)calloc(ngen + 2, sizeof(size_t));
  size_t *stages = NULL, stages_cap = 0;
  int ok = kinds && cands && off;
  ERL_NIF_TERM head, tail = argv[2];
  for (unsigned i = 0; ok && i < ngen; ++i) {
    const ERL_NIF_TERM *t;
    int arity;
    size_t *st = NULL, nst = 0;
    ok = enif_get_list_cell(env, tail, &head, &tail) && enif_get_tuple(env, head, &arity, &t) && arity == 3 &&
         enif_get_int(env, t[0], &kinds[i]) && get_size(env, t[1], &cands[i]) && get_size_list(env, t[2], &st, &nst);
    if (!ok) break;
    if (off[i] + nst > stages_cap) {
      stages_cap = (off[i] + nst) * 2 + 8;
      stages = (size_t *)realloc(stages, stages_cap * sizeof(size_t));
    }
    if (stages) memcpy(stages + off[i], st, nst * sizeof(size_t));
    off[i + 1] = off[i] + nst;
    free(st);
    ok = stages != NULL || off[i + 1] == 0;
  }
  ERL_NIF_TERM res;
  if (!ok) {
    res = enif_make_badarg(env);
  } else {
    size_t dummy = 0;
    vt_hits *h;
    int st = vt_flat_hybrid_search(g ? VT_HNSW_STAGED(g->h) : r->h, q, n, kinds, cands, off, stages ? stages : &dummy, ngen, limit, &h);
    res = st == VT_OK ? ok_hits(env, h) : mk_error(env, st);
  }
  free(q); free(kinds); free(cands); free(off); free(stages);
  return res;
}

static ERL_NIF_TERM flat_hybrid_search(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return hybrid_search_on(env, argv, 0);
}

/* ------------------------------------------------------ stateless helpers */
/* normalize_l2([float]) -> {:ok, [float]} | {:error, binary}             nifs.rs:107-111 */
static ERL_NIF_TERM normalize_l2(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  float *v;
  size_t n;
  (void)argc;
  if (!get_f32_list(env, argv[0], &v, &n)) return enif_make_badarg(env);
  float *out = (float *)malloc((n ? n : 1) * sizeof(float));
  int st = out ? vt_normalize_l2(0, 1, n, v, out) : VT_ERR_NOMEM;
  ERL_NIF_TERM res;
  if (st != VT_OK) {
    res = mk_error(env, st);
  } else {
    ERL_NIF_TERM list = enif_make_list(env, 0);
    for (size_t i = n; i-- > 0;) list = enif_make_list_cell(env, enif_make_double(env, (double)out[i]), list);
    res = enif_make_tuple2(env, mk_atom(env, "ok"), list);
  }
  free(v); free(out);
  return res;
}

/* normalize_zscore([float]) / normalize_minmax([float]) -> {:ok, [float]} | {:error, binary}   nifs.rs:113-123 */
static ERL_NIF_TERM f32_list_term(ErlNifEnv *env, const float *v, size_t n) {
  ERL_NIF_TERM list = enif_make_list(env, 0);
  for (size_t i = n; i-- > 0;) list = enif_make_list_cell(env, enif_make_double(env, (double)v[i]), list);
  return list;
}

static ERL_NIF_TERM normalize_with(ErlNifEnv *env, ERL_NIF_TERM vector, int mode) {
  float *v;
  size_t n;
  if (!get_f32_list(env, vector, &v, &n)) return enif_make_badarg(env);
  float *out = (float *)malloc((n ? n : 1) * sizeof(float));
  int st = out ? vt_prepare_rows(0, mode, 1, n, v, out, NULL, NULL) : VT_ERR_NOMEM;
  ERL_NIF_TERM res = st != VT_OK ? mk_error(env, st) : enif_make_tuple2(env, mk_atom(env, "ok"), f32_list_term(env, out, n));
  free(v); free(out);
  return res;
}

static ERL_NIF_TERM normalize_zscore(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return normalize_with(env, argv[0], VT_NORM_ZSCORE);
}

static ERL_NIF_TERM normalize_minmax(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return normalize_with(env, argv[0], VT_NORM_MINMAX);
}

/* prepare_rows(:none | :l2 | :zscore | :minmax, [[float]]) -> {:ok, [{[float], [u64]}]} | {:error, binary}
 * Extension: what Collection.prepare_embedding does to a record's vector (collection.ex:921-946 -- validate,
 * normalize, compress_sign_bits of the result), for a batch in one call.  Vectors of one length; any other atom, a
 * ragged batch or a non-float is badarg. */
static ERL_NIF_TERM prepare_rows(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  static const char *names[] = {"none", "l2", "zscore", "minmax"};
  int mode = -1;
  unsigned count;
  (void)argc;
  for (int m = 0; m < 4; ++m)
    if (argv[0] == enif_make_atom(env, names[m])) mode = m;
  if (mode < 0 || !enif_get_list_length(env, argv[1], &count)) return enif_make_badarg(env);
  if (count == 0) return enif_make_tuple2(env, mk_atom(env, "ok"), enif_make_list(env, 0));
  float *in = NULL;
  size_t d = 0;
  ERL_NIF_TERM head, tail = argv[1];
  for (unsigned i = 0; i < count; ++i) {
    float *v;
    size_t n;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !get_f32_list(env, head, &v, &n)) { free(in); return enif_make_badarg(env); }
    if (i == 0) {
      d = n;
      in = (float *)malloc(((size_t)count * d + 1) * sizeof(float));
    }
    if (!in || n != d) { free(v); free(in); return enif_make_badarg(env); }
    memcpy(in + (size_t)i * d, v, d * sizeof(float));
    free(v);
  }
  const size_t W = (d + 63) / 64;
  float *out = (float *)malloc(((size_t)count * d + 1) * sizeof(float));
  uint64_t *words = (uint64_t *)calloc((size_t)count * W + 1, sizeof(uint64_t));
  int st = out && words ? vt_prepare_rows(0, mode, count, d, in, out, words, NULL) : VT_ERR_NOMEM;
  ERL_NIF_TERM res;
  if (st != VT_OK) {
    res = mk_error(env, st);
  } else {
    ERL_NIF_TERM list = enif_make_list(env, 0);
    for (size_t i = count; i-- > 0;) {
      ERL_NIF_TERM bits = enif_make_list(env, 0);
      for (size_t w = W; w-- > 0;) bits = enif_make_list_cell(env, enif_make_uint64(env, (ErlNifUInt64)words[i * W + w]), bits);
      list = enif_make_list_cell(env, enif_make_tuple2(env, f32_list_term(env, out + i * d, d), bits), list);
    }
    res = enif_make_tuple2(env, mk_atom(env, "ok"), list);
  }
  free(in); free(out); free(words);
  return res;
}

/* compress_sign_bits([float]) -> [u64]   (bare list, as the reference returns it) nifs.rs:113-129 */
static ERL_NIF_TERM compress_sign_bits(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  float *v;
  size_t n;
  (void)argc;
  if (!get_f32_list(env, argv[0], &v, &n)) return enif_make_badarg(env);
  size_t words = (n + 63) / 64;
  uint64_t *out = (uint64_t *)calloc(words ? words : 1, sizeof(uint64_t));
  int st = out ? vt_compress_sign_bits(0, 1, n, v, out) : VT_ERR_NOMEM;
  ERL_NIF_TERM res;
  if (st != VT_OK) {
    res = mk_error(env, st);
  } else {
    res = enif_make_list(env, 0);
    for (size_t i = words; i-- > 0;) res = enif_make_list_cell(env, enif_make_uint64(env, (ErlNifUInt64)out[i]), res);
  }
  free(v); free(out);
  return res;
}

/* [{id, [element]}] -> ids + id_off + values + value_off, as the C ABI's ragged batches expect.
 * `u64` selects [u64] rows (binary_top_k) instead of [float] rows (vector_top_k). */
typedef struct { char *ids; size_t *id_off; void *vals; size_t *val_off; unsigned count; } ragged;

static void ragged_free(ragged *g) { free(g->ids); free(g->id_off); free(g->vals); free(g->val_off); }

static int get_u64_list(ErlNifEnv *env, ERL_NIF_TERM list, uint64_t **out, size_t *n) {
  unsigned len;
  if (!enif_get_list_length(env, list, &len)) return 0;
  uint64_t *v = (uint64_t *)malloc((len ? len : 1) * sizeof(uint64_t));
  if (!v) return 0;
  ERL_NIF_TERM head, tail = list;
  for (unsigned i = 0; i < len; ++i) {
    ErlNifUInt64 w;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_uint64(env, head, &w)) { free(v); return 0; }
    v[i] = (uint64_t)w;
  }
  *out = v;
  *n = len;
  return 1;
}

static int get_ragged(ErlNifEnv *env, ERL_NIF_TERM list, int u64, ragged *g) {
  memset(g, 0, sizeof *g);
  if (!enif_get_list_length(env, list, &g->count)) return 0;
  g->id_off = (size_t *)calloc(g->count + 1, sizeof(size_t));
  g->val_off = (size_t *)calloc(g->count + 1, sizeof(size_t));
  if (!g->id_off || !g->val_off) return 0;
  const size_t esz = u64 ? sizeof(uint64_t) : sizeof(float);
  size_t ids_cap = 64, vals_cap = 64;
  g->ids = (char *)malloc(ids_cap);
  g->vals = malloc(vals_cap * esz);
  if (!g->ids || !g->vals) return 0;
  ERL_NIF_TERM head, tail = list;
  for (unsigned i = 0; i < g->count; ++i) {
    const ERL_NIF_TERM *pair;
    int arity;
    ErlNifBinary id;
    void *v = NULL;
    size_t n = 0;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_tuple(env, head, &arity, &pair) || arity != 2 ||
        !enif_inspect_binary(env, pair[0], &id))
      return 0;
    if (!(u64 ? get_u64_list(env, pair[1], (uint64_t **)&v, &n) : get_f32_list(env, pair[1], (float **)&v, &n))) return 0;
    if (g->id_off[i] + id.size > ids_cap) {
      ids_cap = (g->id_off[i] + id.size) * 2 + 64;
      g->ids = (char *)realloc(g->ids, ids_cap);
    }
    if (g->val_off[i] + n > vals_cap) {
      vals_cap = (g->val_off[i] + n) * 2 + 64;
      g->vals = realloc(g->vals, vals_cap * esz);
    }
    if (!g->ids || !g->vals) { free(v); return 0; }
    memcpy(g->ids + g->id_off[i], id.data, id.size);
    memcpy((char *)g->vals + g->val_off[i] * esz, v, n * esz);
    g->id_off[i + 1] = g->id_off[i] + id.size;
    g->val_off[i + 1] = g->val_off[i] + n;
    free(v);
  }
  return 1;
}

/* vector_top_k([{id, [float]}], [float], metric_code, dims, limit)        nifs.rs:151-162 */
static ERL_NIF_TERM vector_top_k(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  ragged g;
  float *q = NULL;
  size_t nq, dims, limit;
  int code;
  (void)argc;
  if (!get_ragged(env, argv[0], 0, &g) || !get_f32_list(env, argv[1], &q, &nq) || !enif_get_int(env, argv[2], &code) ||
      !get_size(env, argv[3], &dims) || !get_size(env, argv[4], &limit)) {
    ragged_free(&g);
    free(q);
    return enif_make_badarg(env);
  }
  vt_hits *h;
  int st = vt_vector_top_k(0, g.count, g.ids, g.id_off, (const float *)g.vals, g.val_off, q, nq, code, dims, limit, &h);
  ragged_free(&g);
  free(q);
  return st == VT_OK ? ok_hits(env, h) : mk_error(env, st);
}

/* binary_top_k([{id, [u64]}], [u64], dims, limit)                         nifs.rs:164-175 */
static ERL_NIF_TERM binary_top_k(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  ragged g;
  uint64_t *q = NULL;
  size_t nq, dims, limit;
  (void)argc;
  if (!get_ragged(env, argv[0], 1, &g) || !get_u64_list(env, argv[1], &q, &nq) || !get_size(env, argv[2], &dims) ||
      !get_size(env, argv[3], &limit)) {
    ragged_free(&g);
    free(q);
    return enif_make_badarg(env);
  }
  vt_hits *h;
  int st = vt_binary_top_k(0, g.count, g.ids, g.id_off, (const uint64_t *)g.vals, g.val_off, q, nq, dims, limit, &h);
  ragged_free(&g);
  free(q);
  return st == VT_OK ? ok_hits(env, h) : mk_error(env, st);
}

/* [[float]] -> values + value_off (ragged: every vector keeps its own length) */
static int get_vectors(ErlNifEnv *env, ERL_NIF_TERM list, float **vals, size_t **off, size_t *count) {
  unsigned len;
  *vals = NULL;
  *off = NULL;
  if (!enif_get_list_length(env, list, &len)) return 0;
  *off = (size_t *)calloc((size_t)len + 1, sizeof(size_t));
  size_t cap = 64;
  *vals = (float *)malloc(cap * sizeof(float));
  if (!*off || !*vals) return 0;
  ERL_NIF_TERM head, tail = list;
  for (unsigned i = 0; i < len; ++i) {
    float *v = NULL;
    size_t n = 0;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !get_f32_list(env, head, &v, &n)) return 0;
    if ((*off)[i] + n > cap) {
      cap = ((*off)[i] + n) * 2 + 64;
      float *grown = (float *)realloc(*vals, cap * sizeof(float));
      if (!grown) { free(v); return 0; }
      *vals = grown;
    }
    memcpy(*vals + (*off)[i], v, n * sizeof(float));
    (*off)[i + 1] = (*off)[i] + n;
    free(v);
  }
  *count = len;
  return 1;
}

/* metric_code: u8 in the reference */
static int get_metric_code(ErlNifEnv *env, ERL_NIF_TERM t, int *code) {
  return enif_get_int(env, t, code) && *code >= 0 && *code <= 255;
}

/* multi_vector_score([[float]], [[float]], metric_code)                    nifs.rs:177-187 */
static ERL_NIF_TERM multi_vector_score(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  float *q = NULL, *dv = NULL;
  size_t *qoff = NULL, *doff = NULL, nq = 0, nd = 0;
  int code;
  (void)argc;
  if (!get_vectors(env, argv[0], &q, &qoff, &nq) || !get_vectors(env, argv[1], &dv, &doff, &nd) ||
      !get_metric_code(env, argv[2], &code)) {
    free(q); free(qoff); free(dv); free(doff);
    return enif_make_badarg(env);
  }
  float score = 0.0f;
  int st = vt_multi_vector_score(0, q, qoff, nq, dv, doff, nd, code, &score);
  free(q); free(qoff); free(dv); free(doff);
  return st == VT_OK ? enif_make_tuple2(env, mk_atom(env, "ok"), enif_make_double(env, (double)score)) : mk_error(env, st);
}

/* multi_vector_top_k([{id, [[float]]}], [[float]], metric_code, limit)     nifs.rs:188-198 */
static ERL_NIF_TERM multi_vector_top_k(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  unsigned count;
  char *ids = NULL;
  size_t *id_off = NULL, *doc_vec_off = NULL, *val_off = NULL, *qoff = NULL, nq = 0, limit;
  float *vals = NULL, *q = NULL;
  int code, ok = enif_get_list_length(env, argv[0], &count);
  size_t nvec = 0, ids_cap = 64, vals_cap = 64, vecs_cap = 64;
  (void)argc;
  if (ok) {
    id_off = (size_t *)calloc((size_t)count + 1, sizeof(size_t));
    doc_vec_off = (size_t *)calloc((size_t)count + 1, sizeof(size_t));
    val_off = (size_t *)calloc(vecs_cap + 1, sizeof(size_t));
    ids = (char *)malloc(ids_cap);
    vals = (float *)malloc(vals_cap * sizeof(float));
    ok = id_off && doc_vec_off && val_off && ids && vals;
  }
  ERL_NIF_TERM head, tail = argv[0];
  for (unsigned i = 0; ok && i < count; ++i) {
    const ERL_NIF_TERM *pair;
    int arity;
    ErlNifBinary id;
    float *dv = NULL;
    size_t *doff = NULL, nd = 0;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_tuple(env, head, &arity, &pair) || arity != 2 ||
        !enif_inspect_binary(env, pair[0], &id) || !get_vectors(env, pair[1], &dv, &doff, &nd)) {
      free(dv); free(doff);
      ok = 0;
      break;
    }
    if (id_off[i] + id.size > ids_cap) {
      ids_cap = (id_off[i] + id.size) * 2 + 64;
      char *g = (char *)realloc(ids, ids_cap);
      if (g) ids = g; else ok = 0;
    }
    if (ok && val_off[nvec] + doff[nd] > vals_cap) {
      vals_cap = (val_off[nvec] + doff[nd]) * 2 + 64;
      float *g = (float *)realloc(vals, vals_cap * sizeof(float));
      if (g) vals = g; else ok = 0;
    }
    if (ok && nvec + nd > vecs_cap) {
      vecs_cap = (nvec + nd) * 2 + 64;
      size_t *g = (size_t *)realloc(val_off, (vecs_cap + 1) * sizeof(size_t));
      if (g) val_off = g; else ok = 0;
    }
    if (ok) {
      memcpy(ids + id_off[i], id.data, id.size);
      id_off[i + 1] = id_off[i] + id.size;
      memcpy(vals + val_off[nvec], dv, doff[nd] * sizeof(float));
      for (size_t j = 0; j < nd; ++j) val_off[nvec + j + 1] = val_off[nvec] + doff[j + 1];
      nvec += nd;
      doc_vec_off[i + 1] = nvec;
    }
    free(dv); free(doff);
  }
  ok = ok && get_vectors(env, argv[1], &q, &qoff, &nq) && get_metric_code(env, argv[2], &code) && get_size(env, argv[3], &limit);
  ERL_NIF_TERM res;
  if (!ok) {
    res = enif_make_badarg(env);
  } else {
    vt_hits *h;
    int st = vt_multi_vector_top_k(0, count, ids, id_off, doc_vec_off, vals, val_off, q, qoff, nq, code, limit, &h);
    res = st == VT_OK ? ok_hits(env, h) : mk_error(env, st);
  }
  free(ids); free(id_off); free(doc_vec_off); free(val_off); free(vals); free(q); free(qoff);
  return res;
}

/* Option<usize> as rustler decodes it: the atom nil is None, an integer that fits is Some(n), anything else does
 * not decode.  (An atom is an immediate term: one name, one value -- compared as OTP's own NIFs compare theirs.) */
static int get_option_size(ErlNifEnv *env, ERL_NIF_TERM t, size_t *out, int *is_some) {
  *out = 0;
  *is_some = get_size(env, t, out);
  return *is_some || t == enif_make_atom(env, "nil");
}

/* muvera_encode_query / muvera_encode_document([[float]], dimension, num_repetitions, num_simhash_projections, seed,
 * projection_dimension, final_projection_dimension | nil)                 nifs.rs:430-476 -> {:ok, [float]} */
static ERL_NIF_TERM muvera_encode(ErlNifEnv *env, const ERL_NIF_TERM argv[], int mode) {
  float *vals = NULL, *fde = NULL;
  size_t *off = NULL, count = 0, dim, reps, simhash, proj, final_dim;
  ErlNifUInt64 seed;
  int final_is_some;
  if (!get_vectors(env, argv[0], &vals, &off, &count) || !get_size(env, argv[1], &dim) || !get_size(env, argv[2], &reps) ||
      !get_size(env, argv[3], &simhash) || !enif_get_uint64(env, argv[4], &seed) || !get_size(env, argv[5], &proj) ||
      !get_option_size(env, argv[6], &final_dim, &final_is_some)) {
    free(vals); free(off);
    return enif_make_badarg(env);
  }
  const size_t set_off[2] = {0, count};
  const size_t n = vt_muvera_fde_dimension(reps, simhash, proj, final_dim, final_is_some);
  ERL_NIF_TERM res;
  fde = (float *)malloc((n ? n : 1) * sizeof(float)); /* (n == 0: the call below refuses the configuration) */
  if (!fde) {
    res = mk_error(env, VT_ERR_NOMEM);
  } else {
    int st = vt_muvera_encode(0, mode, 1, set_off, vals, off, dim, reps, simhash, seed, proj, final_dim, final_is_some, fde, NULL);
    if (st != VT_OK) {
      res = mk_error(env, st);
    } else {
      ERL_NIF_TERM list = enif_make_list(env, 0);
      for (size_t i = n; i-- > 0;) list = enif_make_list_cell(env, enif_make_double(env, (double)fde[i]), list);
      res = enif_make_tuple2(env, mk_atom(env, "ok"), list);
    }
  }
  free(vals); free(off); free(fde);
  return res;
}
static ERL_NIF_TERM muvera_encode_query(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return muvera_encode(env, argv, 0);
}
static ERL_NIF_TERM muvera_encode_document(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return muvera_encode(env, argv, 1);
}

/* ------------------------------------------------------------------ HNSW */
/* hnsw_new_l2 / _cosine / _inner_product(m, m0, ef_construction, ef_search, max_level, device)
 *   -> {:ok, reference} | {:error, binary}                                          nifs.rs:311-374
 * (the reference's five arguments and the device ordinal; HnswParams::validate's strings come back as they are) */
static hnsw_res *get_hnsw(ErlNifEnv *env, ERL_NIF_TERM t) {
  hnsw_res *r;
  return enif_get_resource(env, t, HNSW, (void **)&r) ? r : NULL;
}

static ERL_NIF_TERM hnsw_new(ErlNifEnv *env, const ERL_NIF_TERM argv[], int metric) {
  size_t p[5];
  int device;
  for (int i = 0; i < 5; ++i)
    if (!get_size(env, argv[i], &p[i])) return enif_make_badarg(env);
  if (!enif_get_int(env, argv[5], &device) || device < 0) return enif_make_badarg(env);
  vt_hnsw *h;
  int st = vt_hnsw_new(metric, device, p[0], p[1], p[2], p[3], p[4], &h);
  if (st != VT_OK) return mk_error(env, st);
  hnsw_res *r = (hnsw_res *)enif_alloc_resource(HNSW, sizeof *r);
  r->h = h;
  ERL_NIF_TERM t = enif_make_resource(env, r);
  enif_release_resource(r);
  return enif_make_tuple2(env, mk_atom(env, "ok"), t);
}
static ERL_NIF_TERM hnsw_new_l2(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return hnsw_new(env, argv, VT_L2);
}
static ERL_NIF_TERM hnsw_new_cosine(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return hnsw_new(env, argv, VT_COSINE);
}
static ERL_NIF_TERM hnsw_new_inner_product(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return hnsw_new(env, argv, VT_INNER_PRODUCT);
}

/* hnsw_insert(ref, id, [float]) -> {:ok, {}} | {:error, binary}                     nifs.rs:376-388 */
static ERL_NIF_TERM hnsw_insert(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  hnsw_res *r = get_hnsw(env, argv[0]);
  ErlNifBinary id;
  float *v;
  size_t n;
  (void)argc;
  if (!r || !enif_inspect_binary(env, argv[1], &id) || !get_f32_list(env, argv[2], &v, &n)) return enif_make_badarg(env);
  int st = vt_hnsw_insert(r->h, (const char *)id.data, id.size, v, n);
  free(v);
  return st == VT_OK ? mk_ok_unit(env) : mk_error(env, st);
}

/* hnsw_insert_many(ref, [{id, [float]}]) -> {:ok, {}} | {:error, binary}            nifs.rs:390-401
 * (every vector is validated before the first insert; earlier inserts stay when a later one fails, hnsw.rs:249-260) */
static ERL_NIF_TERM hnsw_insert_many(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  hnsw_res *r = get_hnsw(env, argv[0]);
  ragged g;
  (void)argc;
  if (!r) return enif_make_badarg(env);
  if (!get_ragged(env, argv[1], 0, &g)) {
    ragged_free(&g);
    return enif_make_badarg(env);
  }
  int st = vt_hnsw_insert_many(r->h, g.count, g.ids, g.id_off, (const float *)g.vals, g.val_off);
  ragged_free(&g);
  return st == VT_OK ? mk_ok_unit(env) : mk_error(env, st);
}

/* hnsw_delete(ref, id) -> {:ok, {}} | {:error, binary}                              nifs.rs:403-412 */
static ERL_NIF_TERM hnsw_delete(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  hnsw_res *r = get_hnsw(env, argv[0]);
  ErlNifBinary id;
  (void)argc;
  if (!r || !enif_inspect_binary(env, argv[1], &id)) return enif_make_badarg(env);
  int st = vt_hnsw_delete(r->h, (const char *)id.data, id.size);
  return st == VT_OK ? mk_ok_unit(env) : mk_error(env, st);
}

/* hnsw_search(ref, [float], limit) -> {:ok, [{id, raw}]} | {:error, binary}         nifs.rs:414-426 */
static ERL_NIF_TERM hnsw_search(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  hnsw_res *r = get_hnsw(env, argv[0]);
  float *q;
  size_t n, limit;
  (void)argc;
  if (!r || !get_f32_list(env, argv[1], &q, &n) || !get_size(env, argv[2], &limit)) return enif_make_badarg(env);
  vt_hits *h;
  int st = vt_hnsw_search(r->h, q, n, limit, &h);
  free(q);
  return st == VT_OK ? ok_hits(env, h) : mk_error(env, st);
}

/* hnsw_quantized_search(ref, [float], candidates, limit), hnsw_funnel_search(ref, [float], [stage], candidates, limit),
 * hnsw_hybrid_search(ref, [float], [{kind, candidates, [stage]}], limit) -> {:ok, [{id, raw}]} | {:error, binary}
 * (collection.ex:232-348 on the index's own rows: the flat NIFs' terms and answers; kind 2 is the index's traversal.
 * The library's three staged entry points take either kind of handle: VT_HNSW_STAGED, include/vettore_flat.h) */
static ERL_NIF_TERM hnsw_quantized_search(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  hnsw_res *r = get_hnsw(env, argv[0]);
  float *q;
  size_t n, candidates, limit;
  (void)argc;
  if (!r || !get_f32_list(env, argv[1], &q, &n) || !get_size(env, argv[2], &candidates) || !get_size(env, argv[3], &limit))
    return enif_make_badarg(env);
  vt_hits *h;
  int st = vt_flat_quantized_search(VT_HNSW_STAGED(r->h), q, n, candidates, limit, &h);
  free(q);
  return st == VT_OK ? ok_hits(env, h) : mk_error(env, st);
}

static ERL_NIF_TERM hnsw_funnel_search(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  hnsw_res *r = get_hnsw(env, argv[0]);
  float *q;
  size_t n, nst, candidates, limit, *stages;
  (void)argc;
  if (!r || !get_f32_list(env, argv[1], &q, &n)) return enif_make_badarg(env);
  if (!get_size_list(env, argv[2], &stages, &nst) || !get_size(env, argv[3], &candidates) || !get_size(env, argv[4], &limit)) {
    free(q);
    return enif_make_badarg(env);
  }
  vt_hits *h;
  int st = vt_flat_funnel_search(VT_HNSW_STAGED(r->h), q, n, stages, nst, candidates, limit, &h);
  free(q); free(stages);
  return st == VT_OK ? ok_hits(env, h) : mk_error(env, st);
}

static ERL_NIF_TERM hnsw_hybrid_search(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return hybrid_search_on(env, argv, 1);
}

/* hnsw_memory(ref) -> {:ok, {rows, row_capacity, dead_rows, edges}} | {:error, binary}
 * (no counterpart in the reference: vt_hnsw_memory's four numbers.  rows counts the slab rows handed out since the last
 * compaction, dead_rows returns to 0 at one: include/vettore_flat.h) */
static ERL_NIF_TERM hnsw_memory(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  hnsw_res *r = get_hnsw(env, argv[0]);
  size_t rows, cap, dead, edges;
  (void)argc;
  if (!r) return enif_make_badarg(env);
  int st = vt_hnsw_memory(r->h, &rows, &cap, &dead, &edges);
  if (st != VT_OK) return mk_error(env, st);
  return enif_make_tuple2(env, mk_atom(env, "ok"),
                          enif_make_tuple(env, 4, enif_make_uint64(env, (ErlNifUInt64)rows), enif_make_uint64(env, (ErlNifUInt64)cap),
                                          enif_make_uint64(env, (ErlNifUInt64)dead), enif_make_uint64(env, (ErlNifUInt64)edges)));
}

/* ------------------------------------------------------- MMR reranking
 * Vettore.Distance.mmr_rerank/5 and Vettore.rerank/4 on the device.  The Elixir layer validates in the reference's
 * order and converts numbers with `/ 1` (flat_gpu.ex); what crosses here is floats, and what comes back is the chosen
 * entries' indices into the initial list, in order of choice. */
static int get_f64_list(ErlNifEnv *env, ERL_NIF_TERM list, double **out, size_t *n) {
  unsigned len;
  if (!enif_get_list_length(env, list, &len)) return 0;
  double *v = (double *)malloc((len ? len : 1) * sizeof(double));
  if (!v) return 0;
  ERL_NIF_TERM head, tail = list;
  for (unsigned i = 0; i < len; ++i) {
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_double(env, head, &v[i])) { free(v); return 0; }
  }
  *out = v;
  *n = len;
  return 1;
}

static ERL_NIF_TERM index_list(ErlNifEnv *env, const uint32_t *order, size_t n) {
  ERL_NIF_TERM list = enif_make_list(env, 0);
  for (size_t i = n; i-- > 0;) list = enif_make_list_cell(env, enif_make_uint64(env, order[i]), list);
  return list;
}

/* mmr_rerank(metric_code, [[float]], [float], alpha, final_k) -> {:ok, [index]} | {:error, binary}
 * row i of the matrix is the vector of initial entry i, scores[i] its relevance */
static ERL_NIF_TERM mmr_rerank(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  int code, st;
  unsigned count;
  float *rows = NULL;
  double *scores = NULL, alpha;
  size_t d = 0, ns, final_k, got = 0;
  (void)argc;
  if (!enif_get_int(env, argv[0], &code) || !enif_get_list_length(env, argv[1], &count) ||
      !get_f64_list(env, argv[2], &scores, &ns) || !enif_get_double(env, argv[3], &alpha) || !get_size(env, argv[4], &final_k)) {
    free(scores);
    return enif_make_badarg(env);
  }
  if (ns != count || !get_f32_matrix(env, argv[1], count, &rows, &d, &st)) { free(scores); return enif_make_badarg(env); }
  if (st != VT_OK) { free(scores); return mk_error(env, st); }
  uint32_t *order = (uint32_t *)malloc((count ? count : 1) * sizeof(uint32_t));
  st = order ? vt_mmr_rerank(0, code, count, count ? d : 1, rows, scores, alpha, final_k, order, &got) : VT_ERR_NOMEM;
  free(rows);
  free(scores);
  ERL_NIF_TERM res = st == VT_OK ? enif_make_tuple2(env, mk_atom(env, "ok"), index_list(env, order, got)) : mk_error(env, st);
  free(order);
  return res;
}

/* flat_mmr_rerank(ref, [{id, score}], alpha, final_k) -> {:ok, [index]} | {:error, binary}: the rows are the index's own */
static ERL_NIF_TERM flat_mmr_rerank(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  flat_res *r = get_flat(env, argv[0]);
  unsigned count;
  double alpha;
  size_t final_k, got = 0;
  (void)argc;
  if (!r || !enif_get_list_length(env, argv[1], &count) || !enif_get_double(env, argv[2], &alpha) ||
      !get_size(env, argv[3], &final_k))
    return enif_make_badarg(env);
  size_t *off = (size_t *)calloc((size_t)count + 1, sizeof(size_t));
  double *scores = (double *)malloc((count ? count : 1) * sizeof(double));
  uint32_t *order = (uint32_t *)malloc((count ? count : 1) * sizeof(uint32_t));
  char *ids = NULL;
  size_t cap = 0;
  int ok = off && scores && order;
  ERL_NIF_TERM head, tail = argv[1];
  for (unsigned i = 0; ok && i < count; ++i) {
    const ERL_NIF_TERM *pair;
    int arity;
    ErlNifBinary id;
    ok = enif_get_list_cell(env, tail, &head, &tail) && enif_get_tuple(env, head, &arity, &pair) && arity == 2 &&
         enif_inspect_binary(env, pair[0], &id) && enif_get_double(env, pair[1], &scores[i]);
    if (!ok) break;
    if (off[i] + id.size > cap) {
      cap = (off[i] + id.size) * 2 + 64;
      char *grown = (char *)realloc(ids, cap);
      if (!grown) { ok = 0; break; }
      ids = grown;
    }
    memcpy(ids + off[i], id.data, id.size);
    off[i + 1] = off[i] + id.size;
  }
  ERL_NIF_TERM res;
  if (!ok) {
    res = enif_make_badarg(env);
  } else {
    int st = vt_flat_mmr_rerank(r->h, count, ids ? ids : "", off, scores, alpha, final_k, order, &got);
    res = st == VT_OK ? enif_make_tuple2(env, mk_atom(env, "ok"), index_list(env, order, got)) : mk_error(env, st);
  }
  free(ids);
  free(off);
  free(scores);
  free(order);
  return res;
}

/* flat_mmr_search(ref, [float], candidates, limit, alpha, score_mode) -> {:ok, {[{id, raw}], [index]}} | {:error, binary}
 * flat_search(limit = candidates), its hits unchanged, then MMR over them; score_mode 0 :raw, 1 :similarity */
static ERL_NIF_TERM flat_mmr_search(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  flat_res *r = get_flat(env, argv[0]);
  float *q;
  size_t n, candidates, limit, got = 0;
  double alpha;
  int mode;
  (void)argc;
  if (!r || !get_size(env, argv[2], &candidates) || !get_size(env, argv[3], &limit) || !enif_get_double(env, argv[4], &alpha) ||
      !enif_get_int(env, argv[5], &mode) || !get_f32_list(env, argv[1], &q, &n))
    return enif_make_badarg(env);
  const size_t cap = limit < candidates ? limit : candidates;
  uint32_t *order = (uint32_t *)malloc((cap ? cap : 1) * sizeof(uint32_t));
  vt_hits *h = NULL;
  int st = order ? vt_flat_mmr_search(r->h, q, n, candidates, limit, alpha, mode, &h, order, &got) : VT_ERR_NOMEM;
  free(q);
  ERL_NIF_TERM res = st == VT_OK ? enif_make_tuple2(env, mk_atom(env, "ok"),
                                                    enif_make_tuple2(env, hits_to_list(env, h), index_list(env, order, got)))
                                 : mk_error(env, st);
  free(order);
  return res;
}

/* flat_mmr_search_batch(ref, [[float]], candidates, limit, alpha, score_mode)
 *   -> {:ok, [{:ok, {[{id, raw}], [index]}} | {:error, binary}]} | {:error, binary}: all queries one chain of launches */
static ERL_NIF_TERM flat_mmr_search_batch(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  flat_res *r = get_flat(env, argv[0]);
  unsigned nq;
  size_t candidates, limit, d;
  double alpha;
  int mode, st;
  float *qs = NULL;
  (void)argc;
  if (!r || !enif_get_list_length(env, argv[1], &nq) || !get_size(env, argv[2], &candidates) || !get_size(env, argv[3], &limit) ||
      !enif_get_double(env, argv[4], &alpha) || !enif_get_int(env, argv[5], &mode))
    return enif_make_badarg(env);
  if (nq == 0) return enif_make_tuple2(env, mk_atom(env, "ok"), enif_make_list(env, 0));
  if (!get_f32_matrix(env, argv[1], nq, &qs, &d, &st)) return enif_make_badarg(env);
  if (st != VT_OK) return mk_error(env, st);
  const size_t cap = limit < candidates ? limit : candidates;
  vt_hits **out = (vt_hits **)calloc(nq, sizeof(vt_hits *));
  const size_t slots = (size_t)nq * cap;
  uint32_t *order = (uint32_t *)malloc((slots > 0 ? slots : 1) * sizeof(uint32_t));
  size_t *lens = (size_t *)calloc(nq, sizeof(size_t));
  int *status = (int *)calloc(nq, sizeof(int));
  st = out && order && lens && status
           ? vt_flat_mmr_search_batch(r->h, qs, nq, d, candidates, limit, alpha, mode, out, order, lens, status)
           : VT_ERR_NOMEM;
  free(qs);
  ERL_NIF_TERM res;
  if (st != VT_OK) {
    res = mk_error(env, st);
  } else {
    ERL_NIF_TERM list = enif_make_list(env, 0);
    for (unsigned i = nq; i-- > 0;) {
      ERL_NIF_TERM one = status[i] == VT_OK
                             ? enif_make_tuple2(env, mk_atom(env, "ok"),
                                                enif_make_tuple2(env, hits_to_list(env, out[i]), index_list(env, order + (size_t)i * cap, lens[i])))
                             : mk_error(env, status[i]);
      list = enif_make_list_cell(env, one, list);
    }
    res = enif_make_tuple2(env, mk_atom(env, "ok"), list);
  }
  free(out);
  free(order);
  free(lens);
  free(status);
  return res;
}

static int load(ErlNifEnv *env, void **priv, ERL_NIF_TERM info) {
  (void)priv; (void)info;
  /* a libvettore_hip.so built from another header would be handed structs of the wrong size */
  if (vt_abi_version() != VT_ABI_VERSION) return 1;
  FLAT = enif_open_resource_type(env, NULL, "vettore_gpu_flat", flat_dtor, ERL_NIF_RT_CREATE, NULL);
  HNSW = enif_open_resource_type(env, NULL, "vettore_gpu_hnsw", hnsw_dtor, ERL_NIF_RT_CREATE, NULL);
  return FLAT && HNSW ? 0 : 1;
}

static ErlNifFunc funcs[] = {
  {"flat_new", 2, flat_new, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"flat_insert", 3, flat_insert, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"flat_insert_many", 2, flat_insert_many, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"flat_load_binary", 4, flat_load_binary, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"flat_delete", 2, flat_delete, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"flat_search", 3, flat_search, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"flat_search_batch", 3, flat_search_batch, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"flat_quantized_search", 4, flat_quantized_search, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"flat_quantized_search_batch", 4, flat_quantized_search_batch, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"flat_funnel_search_batch", 5, flat_funnel_search_batch, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"flat_funnel_search", 5, flat_funnel_search, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"flat_hybrid_search", 4, flat_hybrid_search, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"normalize_l2", 1, normalize_l2, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"compress_sign_bits", 1, compress_sign_bits, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"normalize_zscore", 1, normalize_zscore, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"normalize_minmax", 1, normalize_minmax, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"prepare_rows", 2, prepare_rows, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"vector_top_k", 5, vector_top_k, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"binary_top_k", 4, binary_top_k, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"multi_vector_score", 3, multi_vector_score, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"multi_vector_top_k", 4, multi_vector_top_k, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"muvera_encode_query", 7, muvera_encode_query, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"muvera_encode_document", 7, muvera_encode_document, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"hnsw_new_l2", 6, hnsw_new_l2, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"hnsw_new_cosine", 6, hnsw_new_cosine, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"hnsw_new_inner_product", 6, hnsw_new_inner_product, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"hnsw_insert", 3, hnsw_insert, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"hnsw_insert_many", 2, hnsw_insert_many, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"hnsw_delete", 2, hnsw_delete, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"hnsw_search", 3, hnsw_search, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"hnsw_quantized_search", 4, hnsw_quantized_search, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"hnsw_funnel_search", 5, hnsw_funnel_search, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"hnsw_hybrid_search", 4, hnsw_hybrid_search, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"hnsw_memory", 1, hnsw_memory, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"mmr_rerank", 5, mmr_rerank, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"flat_mmr_rerank", 4, flat_mmr_rerank, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"flat_mmr_search", 6, flat_mmr_search, ERL_NIF_DIRTY_JOB_IO_BOUND},
  {"flat_mmr_search_batch", 6, flat_mmr_search_batch, ERL_NIF_DIRTY_JOB_IO_BOUND},
};

ERL_NIF_INIT(Elixir.Vettore.Gpu.Nifs, funcs, load, NULL, NULL, NULL)
