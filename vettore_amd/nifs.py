"""Python mirror of `Vettore.Nifs` for the flat-index hot path
(/root/reference/lib/vettore_nifs.ex:58-174, native/vettore/src/nifs.rs).

Same function names, argument meaning and return shapes as the Elixir stubs,
with Elixir terms spelled as Python values:

    {:ok, value}        -> ("ok", value)
    {:ok, {}}           -> ("ok", ())          (Rustler's encoding of Ok(()))
    {:error, "string"}  -> ("error", "string") (the reference's exact strings)
    bare reference      -> FlatRef

Every call goes through the C ABI of libvettore_hip.so into HIP kernels; badly
typed arguments raise (the NIF's ArgumentError / badarg).
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

DEVICE = 0  # HIP device ordinal used by flat_new_* and the stateless helpers
USIZE_MAX = (1 << 64) - 1
_F32_MAX = float(np.finfo(np.float32).max)

METRICS = [
    "l2", "l2_squared", "cosine", "inner_product", "negative_inner_product",
    "manhattan", "chebyshev", "hamming", "jaccard",
]
METRIC_CODE = {name: i for i, name in enumerate(METRICS)}


def set_device(device: int):
    global DEVICE
    DEVICE = int(device)


class FlatRef:
    """The `reference()` returned by flat_new_*: owns a vt_flat handle; the
    finalizer plays the role of the ResourceArc destructor."""

    def __init__(self, handle, metric: int):
        self._h = handle
        self.metric = metric

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:   # (module globals are None while the interpreter shuts down)
            _lib.load().vt_flat_free(h)

    @property
    def handle(self):
        if not self._h:
            raise ValueError("flat index already freed")
        return self._h

    def __len__(self):
        return _lib.load().vt_flat_len(self.handle)

    @property
    def dimension(self):
        d = _lib.load().vt_flat_dimension(self.handle)
        return None if d < 0 else d


def _bytes(x) -> bytes:
    if isinstance(x, str):
        return x.encode()
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    raise TypeError("badarg: id must be a binary")


def _f32_list(v) -> np.ndarray:
    """Rustler decodes [float] into Vec<f32>: non-floats and doubles outside
    the f32 range are badarg; NaN/inf doubles narrow to f32 NaN/inf."""
    a = np.asarray(v, dtype=np.float64).reshape(-1) if not isinstance(v, np.ndarray) else v.reshape(-1)
    if a.dtype != np.float32:
        a64 = np.asarray(a, dtype=np.float64)
        finite = np.isfinite(a64)
        if np.any(np.abs(a64[finite]) > _F32_MAX):
            raise TypeError("badarg: float out of f32 range")
        with np.errstate(over="ignore"):
            a = a64.astype(np.float32)
    return np.ascontiguousarray(a)


def _u64_list(v) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(v, dtype=np.uint64).reshape(-1))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _szp(a):
    return a.ctypes.data_as(C.POINTER(C.c_size_t))


def _pack_ids(ids: Iterable) -> Tuple[bytes, np.ndarray]:
    bs = [_bytes(i) for i in ids]
    off = np.zeros(len(bs) + 1, dtype=np.uintp)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs])
    return b"".join(bs), off


def _pack_ragged(rows: Sequence[np.ndarray], dtype) -> Tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(rows) + 1, dtype=np.uintp)
    if rows:
        off[1:] = np.cumsum([r.size for r in rows])
    vals = np.ascontiguousarray(np.concatenate(rows)) if rows and off[-1] else np.zeros(0, dtype)
    return vals.astype(dtype, copy=False), off


def _err(status: int):
    return ("error", _lib.error_text(status))


def _export_hits(h, with_keys: bool):
    """One bulk copy across the ABI, then Python slicing."""
    L = _lib.load()
    try:
        n = L.vt_hits_len(h)
        if n == 0:
            return []
        blob = C.create_string_buffer(max(1, L.vt_hits_id_bytes(h)))
        off = (C.c_size_t * (n + 1))()
        raw = (C.c_float * n)()
        keys = (C.c_uint32 * n)() if with_keys else None
        L.vt_hits_export(h, blob, off, raw, keys)
        data = blob.raw
        if with_keys:
            return [(data[off[i]:off[i + 1]], float(raw[i]), int(keys[i])) for i in range(n)]
        return [(data[off[i]:off[i + 1]], float(raw[i])) for i in range(n)]
    finally:
        L.vt_hits_free(h)


def _take_hits(h) -> List[Tuple[bytes, float]]:
    return _export_hits(h, False)


def _take_hits_with_keys(h):
    return _export_hits(h, True)


# ----------------------------------------------------------------- flat_new_*
def _flat_new(metric: int) -> FlatRef:
    h = C.c_void_p()
    st = _lib.load().vt_flat_new(metric, DEVICE, C.byref(h))
    if st != 0:
        raise RuntimeError("flat_new: " + _lib.error_text(st))
    return FlatRef(h, metric)


def flat_new_sharded(metric: int, devices: Sequence[int]) -> FlatRef:
    """One resource over several GPUs of the node (vt_flat_new_sharded): same handle, same
    calls, rows dealt to the shards by a hash of their id."""
    devs = (C.c_int * len(devices))(*[int(d) for d in devices])
    h = C.c_void_p()
    st = _lib.load().vt_flat_new_sharded(metric, devs, len(devices), C.byref(h))
    if st != 0:
        raise RuntimeError("flat_new_sharded: " + _lib.error_text(st))
    return FlatRef(h, metric)


def flat_shard_count(index: FlatRef) -> int:
    return int(_lib.load().vt_flat_shard_count(index.handle))


def flat_shard_lens(index: FlatRef) -> List[int]:
    L = _lib.load()
    return [int(L.vt_flat_shard_len(index.handle, s)) for s in range(flat_shard_count(index))]


def flat_coalesce_stats(index: FlatRef):
    """(batches, searches they carried) of the searches that met on this handle (vt_flat_coalesce_stats)."""
    a, b = C.c_uint64(), C.c_uint64()
    st = _lib.load().vt_flat_coalesce_stats(index.handle, C.byref(a), C.byref(b))
    if st != 0:
        raise RuntimeError("flat_coalesce_stats: " + _lib.error_text(st))
    return int(a.value), int(b.value)


def flat_shard_memory(index: FlatRef, shard: int = 0):
    """(row capacity, slab bytes, mapped chunks) of a shard (vt_flat_shard_memory)."""
    cap, nbytes, chunks = C.c_size_t(), C.c_size_t(), C.c_size_t()
    st = _lib.load().vt_flat_shard_memory(index.handle, shard, C.byref(cap), C.byref(nbytes), C.byref(chunks))
    if st != 0:
        raise RuntimeError("flat_shard_memory: " + _lib.error_text(st))
    return int(cap.value), int(nbytes.value), int(chunks.value)


def flat_route_ids(index: FlatRef, ids_packed: Tuple[bytes, np.ndarray]) -> np.ndarray:
    """Shard of every id of a packed id batch."""
    blob, off = ids_packed
    off = np.ascontiguousarray(off, dtype=np.uintp)
    out = np.zeros(len(off) - 1, dtype=np.uint32)
    st = _lib.load().vt_flat_route_ids(index.handle, len(off) - 1, blob, _szp(off), out.ctypes.data_as(C.POINTER(C.c_uint32)))
    if st != 0:
        raise RuntimeError(_lib.error_text(st))
    return out


def flat_set_exchange(index: FlatRef, mode: int):
    st = _lib.load().vt_flat_set_exchange(index.handle, mode)
    return "ok" if st == 0 else _err(st)


def flat_exchange(index: FlatRef) -> int:
    return int(_lib.load().vt_flat_exchange(index.handle))


def flat_exchange_note(index: FlatRef) -> str:
    """Which exchange a multi-shard handle chose at creation, and why RCCL was refused if it was."""
    return (_lib.load().vt_flat_exchange_note(index.handle) or b"").decode()


def flat_rccl_ranks(index: FlatRef) -> int:
    return int(_lib.load().vt_flat_rccl_ranks(index.handle))


def flat_new_l2(): return _flat_new(0)                       # nifs.rs:200-204
def flat_new_l2_squared(): return _flat_new(1)               # nifs.rs:206-210
def flat_new_cosine(): return _flat_new(2)                   # nifs.rs:212-216
def flat_new_inner_product(): return _flat_new(3)            # nifs.rs:218-222
def flat_new_negative_inner_product(): return _flat_new(4)   # nifs.rs:224-228
def flat_new_manhattan(): return _flat_new(5)                # nifs.rs:230-234
def flat_new_chebyshev(): return _flat_new(6)                # nifs.rs:236-240
def flat_new_hamming(): return _flat_new(7)                  # nifs.rs:242-246
def flat_new_jaccard(): return _flat_new(8)                  # nifs.rs:248-252


def flat_insert(index: FlatRef, id_, vector):
    """nifs.rs:259-271."""
    b, v = _bytes(id_), _f32_list(vector)
    st = _lib.load().vt_flat_insert(index.handle, b, len(b), _fp(v), v.size)
    return ("ok", ()) if st == 0 else _err(st)


def flat_insert_many(index: FlatRef, vectors: Sequence[Tuple[object, Sequence[float]]]):
    """nifs.rs:273-284."""
    ids, ioff = _pack_ids(i for i, _ in vectors)
    vals, voff = _pack_ragged([_f32_list(v) for _, v in vectors], np.float32)
    st = _lib.load().vt_flat_insert_many(index.handle, len(vectors), ids, _szp(ioff), _fp(vals), _szp(voff))
    return ("ok", ()) if st == 0 else _err(st)


def flat_delete(index: FlatRef, id_):
    """nifs.rs:286-295."""
    b = _bytes(id_)
    st = _lib.load().vt_flat_delete(index.handle, b, len(b))
    return ("ok", ()) if st == 0 else _err(st)


def flat_search(index: FlatRef, query, limit: int):
    """nifs.rs:297-309 -> [(id, raw)] ascending by (rank, id)."""
    if not isinstance(limit, int) or limit < 0 or limit > USIZE_MAX:
        raise TypeError("badarg: limit must fit usize")
    q = _f32_list(query)
    h = C.c_void_p()
    st = _lib.load().vt_flat_search(index.handle, _fp(q), q.size, limit, C.byref(h))
    return ("ok", _take_hits(h)) if st == 0 else _err(st)


def flat_search_batch(index: FlatRef, queries, limit: int):
    """Extension: `queries` is an [nq][d] matrix; returns ("ok", [hits per query]),
    each list identical to flat_search of that query."""
    q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
    if q.ndim != 2:
        raise TypeError("badarg: queries must be a matrix")
    nq, d = q.shape
    outs = (C.c_void_p * max(nq, 1))()
    st = _lib.load().vt_flat_search_batch(index.handle, _fp(q.reshape(-1)), nq, d, limit, outs)
    if st != 0:
        return _err(st)
    return ("ok", [_take_hits(C.c_void_p(outs[i])) for i in range(nq)])


def flat_search_packed(index: FlatRef, query, limit: int, records: np.ndarray):
    """flat_search whose hits land as 64-byte wire records (vt_hits_pack) in the
    caller's uint8 array [>= limit][64]; returns ("ok", (count, any_long_id)) with
    one C call for the search and one for the serialisation."""
    q = _f32_list(query)
    L = _lib.load()
    h = C.c_void_p()
    st = L.vt_flat_search(index.handle, _fp(q), q.size, limit, C.byref(h))
    if st != 0:
        return _err(st)
    try:
        cap = records.shape[0]
        n = L.vt_hits_pack(h, records.ctypes.data_as(C.c_void_p), cap)
        lens = records[:n, 8:12].view(np.uint32).reshape(-1)
        long_ids = None
        if n and int(lens.max()) > 52:  # ids that do not fit a record travel separately
            ln = C.c_size_t()
            long_ids = [C.string_at(L.vt_hits_id(h, i, C.byref(ln)), ln.value) for i in range(n)]
    finally:
        L.vt_hits_free(h)
    return ("ok", (int(n), long_ids))


def flat_search_batch_blocks(index: FlatRef, queries, limit: int, blocks: np.ndarray):
    """flat_search_batch whose hit lists land as wire blocks (vt_hits_pack_many) in the caller's
    uint8 array [nq][limit + 1][64]: record 0 of a block is its header {u32 count, u32 long_ids}.
    Returns ("ok", long_ids) where long_ids is None or, when some id does not fit a record, the
    ids of every hit as [[bytes] per query]."""
    q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
    if q.ndim != 2:
        raise TypeError("badarg: queries must be a matrix")
    nq, d = q.shape
    assert blocks.dtype == np.uint8 and blocks.shape == (nq, limit + 1, 64) and blocks.flags.c_contiguous
    L = _lib.load()
    outs = (C.c_void_p * max(nq, 1))()
    st = L.vt_flat_search_batch(index.handle, _fp(q.reshape(-1)), nq, d, limit, outs)
    if st != 0:
        return _err(st)
    try:
        L.vt_hits_pack_many(outs, nq, limit, blocks.ctypes.data_as(C.c_void_p))
        long_ids = None
        if nq and int(blocks[:, 0, 4:8].view(np.uint32).max()) != 0:
            ln = C.c_size_t()
            long_ids = [[C.string_at(L.vt_hits_id(C.c_void_p(outs[i]), j, C.byref(ln)), ln.value)
                         for j in range(L.vt_hits_len(C.c_void_p(outs[i])))] for i in range(nq)]
    finally:
        for i in range(nq):
            L.vt_hits_free(C.c_void_p(outs[i]))
    return ("ok", long_ids)


def hit_blocks_merge(blocks: np.ndarray, world: int, nq: int, limit: int) -> np.ndarray:
    """[world][nq][limit + 1][64] gathered wire blocks -> [nq][limit + 1][64]: per query the `limit` best
    over all ranks by (rank key, id bytes) (vt_hit_blocks_merge; FlatHit::cmp, flat.rs:34-40)."""
    b = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(world, nq, limit + 1, 64)
    out = np.zeros((nq, limit + 1, 64), dtype=np.uint8)
    st = _lib.load().vt_hit_blocks_merge(b.ctypes.data_as(C.c_void_p), world, nq, limit, out.ctypes.data_as(C.c_void_p))
    if st != 0:
        raise RuntimeError(_lib.error_text(st))
    return out


def unpack_block(block: np.ndarray):
    """[(id, raw)] of one wire block ([limit + 1][64]); ids longer than 52 bytes come back as None."""
    head = block[0, :8].view(np.uint32)
    return [(h[0], h[1]) for h in unpack_records(block[1:], int(head[0]))]


def unpack_records(records: np.ndarray, count: int):
    """[(id, raw, rank_key)] from `count` wire records (ids longer than 52 bytes come back as None)."""
    out = []
    for i in range(count):
        rec = records[i]
        w = rec[:12].view(np.uint32)
        n = int(w[2])
        out.append((bytes(rec[12:12 + n]) if n <= 52 else None, float(rec[4:8].view(np.float32)[0]), int(w[0])))
    return out


def flat_search_with_keys(index: FlatRef, query, limit: int):
    """flat_search plus each hit's rank sort key (for cross-shard merges)."""
    q = _f32_list(query)
    h = C.c_void_p()
    st = _lib.load().vt_flat_search(index.handle, _fp(q), q.size, limit, C.byref(h))
    return ("ok", _take_hits_with_keys(h)) if st == 0 else _err(st)


# -------------------------------------------------------- stateless helpers
def vector_top_k(vectors, query, metric_code: int, dimensions: int, limit: int):
    """nifs.rs:151-162."""
    if not isinstance(metric_code, int) or not 0 <= metric_code <= 255:
        raise TypeError("badarg: metric_code is a u8")
    ids, ioff = _pack_ids(i for i, _ in vectors)
    vals, voff = _pack_ragged([_f32_list(v) for _, v in vectors], np.float32)
    q = _f32_list(query)
    h = C.c_void_p()
    st = _lib.load().vt_vector_top_k(DEVICE, len(vectors), ids, _szp(ioff), _fp(vals), _szp(voff), _fp(q), q.size,
                                     metric_code, dimensions, limit, C.byref(h))
    return ("ok", _take_hits(h)) if st == 0 else _err(st)


def _vector_list(vectors) -> Tuple[np.ndarray, np.ndarray]:
    """Vec<Vec<f32>>: ragged, every vector carries its own length."""
    return _pack_ragged([_f32_list(v) for v in vectors], np.float32)


def multi_vector_score(query_vectors, document_vectors, metric_code: int):
    """nifs.rs:177-187: ("ok", score) or ("error", reason)."""
    if not isinstance(metric_code, int) or not 0 <= metric_code <= 255:
        raise TypeError("badarg: metric_code is a u8")
    qv, qoff = _vector_list(query_vectors)
    dv, doff = _vector_list(document_vectors)
    out = C.c_float()
    st = _lib.load().vt_multi_vector_score(DEVICE, _fp(qv), _szp(qoff), qoff.size - 1, _fp(dv), _szp(doff),
                                           doff.size - 1, metric_code, C.byref(out))
    return ("ok", float(out.value)) if st == 0 else _err(st)


def multi_vector_top_k(documents, query_vectors, metric_code: int, limit: int):
    """nifs.rs:188-198: documents are [(id, [[float]])]; ("ok", [(id, score)]) best first."""
    if not isinstance(metric_code, int) or not 0 <= metric_code <= 255:
        raise TypeError("badarg: metric_code is a u8")
    if not isinstance(limit, int) or not 0 <= limit <= USIZE_MAX:
        raise TypeError("badarg: limit is a usize")
    ids, ioff = _pack_ids(i for i, _ in documents)
    per_doc = [[_f32_list(v) for v in vecs] for _, vecs in documents]
    doc_vec_off = np.zeros(len(per_doc) + 1, dtype=np.uintp)
    if per_doc:
        doc_vec_off[1:] = np.cumsum([len(v) for v in per_doc])
    vals, voff = _pack_ragged([v for vecs in per_doc for v in vecs], np.float32)
    qv, qoff = _vector_list(query_vectors)
    h = C.c_void_p()
    st = _lib.load().vt_multi_vector_top_k(DEVICE, len(documents), ids, _szp(ioff), _szp(doc_vec_off), _fp(vals),
                                           _szp(voff), _fp(qv), _szp(qoff), qoff.size - 1, metric_code, limit,
                                           C.byref(h))
    return ("ok", _take_hits(h)) if st == 0 else _err(st)


# ---------------------------------------------- resident multi-vector store (vt_mv_*; no NIF of the reference's)
class MvRef:
    """A vt_mv handle, freed with the object."""

    def __init__(self, handle):
        self.handle = handle

    def __del__(self):
        try:
            if self.handle:
                _lib.load().vt_mv_free(self.handle)
                self.handle = None
        except Exception:
            pass


def mv_new(device: Optional[int] = None) -> MvRef:
    h = C.c_void_p()
    st = _lib.load().vt_mv_new(DEVICE if device is None else device, C.byref(h))
    if st != 0:
        raise RuntimeError("mv_new: " + _lib.error_text(st))
    return MvRef(h)


def _pack_documents(documents):
    ids, ioff = _pack_ids(i for i, _ in documents)
    per_doc = [[_f32_list(v) for v in vecs] for _, vecs in documents]
    doc_vec_off = np.zeros(len(per_doc) + 1, dtype=np.uintp)
    if per_doc:
        doc_vec_off[1:] = np.cumsum([len(v) for v in per_doc])
    vals, voff = _pack_ragged([v for vecs in per_doc for v in vecs], np.float32)
    return ids, ioff, doc_vec_off, vals, voff


def mv_put_many(store: MvRef, documents):
    """Upsert [(id, [[float]])]: "ok" or ("error", reason); nothing changes on an error."""
    ids, ioff, doc_vec_off, vals, voff = _pack_documents(documents)
    st = _lib.load().vt_mv_put_many(store.handle, len(documents), ids, _szp(ioff), _szp(doc_vec_off), _fp(vals), _szp(voff))
    return "ok" if st == 0 else _err(st)


def mv_delete(store: MvRef, id_):
    b = _bytes(id_)
    st = _lib.load().vt_mv_delete(store.handle, b, len(b))
    return "ok" if st == 0 else _err(st)


def mv_len(store: MvRef) -> int:
    return _lib.load().vt_mv_len(store.handle)


def mv_dimension(store: MvRef):
    d = _lib.load().vt_mv_dimension(store.handle)
    return None if d < 0 else d


def _mv_search_args(metric_code, limit):
    if not isinstance(metric_code, int) or not 0 <= metric_code <= 255:
        raise TypeError("badarg: metric_code is a u8")
    if not isinstance(limit, int) or not 0 <= limit <= USIZE_MAX:
        raise TypeError("badarg: limit is a usize")


def mv_top_k(store: MvRef, query_vectors, metric_code: int, limit: int, with_keys: bool = False):
    """multi_vector_top_k over the store's live documents in the order of their last put (`with_keys`: each hit's rank
    sort key as well)."""
    _mv_search_args(metric_code, limit)
    qv, qoff = _vector_list(query_vectors)
    h = C.c_void_p()
    st = _lib.load().vt_mv_top_k(store.handle, _fp(qv), _szp(qoff), qoff.size - 1, metric_code, limit, C.byref(h))
    return ("ok", _export_hits(h, with_keys)) if st == 0 else _err(st)


def mv_top_k_ids(store: MvRef, ids, query_vectors, metric_code: int, limit: int, with_keys: bool = False):
    """The same over the listed live documents only."""
    _mv_search_args(metric_code, limit)
    idb, ioff = _pack_ids(ids)
    qv, qoff = _vector_list(query_vectors)
    h = C.c_void_p()
    st = _lib.load().vt_mv_top_k_ids(store.handle, ioff.size - 1, idb, _szp(ioff), _fp(qv), _szp(qoff), qoff.size - 1,
                                     metric_code, limit, C.byref(h))
    return ("ok", _export_hits(h, with_keys)) if st == 0 else _err(st)


def _pack_sets(sets):
    """[[vector]] per set -> (values, vector offsets, per-set vector offsets)."""
    per_set = [[_f32_list(v) for v in vecs] for vecs in sets]
    set_off = np.zeros(len(per_set) + 1, dtype=np.uintp)
    if per_set:
        set_off[1:] = np.cumsum([len(v) for v in per_set])
    vals, voff = _pack_ragged([v for vecs in per_set for v in vecs], np.float32)
    return vals, voff, set_off


def _mv_batch_results(st, outs, status, nsets, with_keys):
    """Takes (and frees) every hit list a batch call left; one ("ok", hits) | ("error", reason) per set."""
    take = _take_hits_with_keys if with_keys else _take_hits
    lists = [take(C.c_void_p(outs[b])) if outs[b] else None for b in range(nsets)]
    if st != 0:
        return _err(st)
    return [("ok", lists[b]) if status[b] == 0 else _err(status[b]) for b in range(nsets)]


def mv_top_k_batch(store: MvRef, sets, metric_code: int, limit: int, with_keys: bool = False):
    """mv_top_k for every query set of `sets` in one call: [("ok", hits) | ("error", reason)] per set, each exactly what
    mv_top_k returns for that set alone; ("error", reason) when the call itself fails (an unknown metric)."""
    _mv_search_args(metric_code, limit)
    qv, qoff, set_off = _pack_sets(sets)
    n = len(set_off) - 1
    outs, status = (C.c_void_p * max(n, 1))(), (C.c_int * max(n, 1))()
    st = _lib.load().vt_mv_top_k_batch(store.handle, n, _szp(set_off), _fp(qv), _szp(qoff), metric_code, limit, outs, status)
    return _mv_batch_results(st, outs, status, n, with_keys)


def mv_top_k_ids_batch(store: MvRef, id_lists, sets, metric_code: int, limit: int, with_keys: bool = False):
    """mv_top_k_ids for every (id list, query set) pair in one call."""
    _mv_search_args(metric_code, limit)
    if len(id_lists) != len(sets):
        raise ValueError("badarg: one id list per query set")
    id_lists = [list(ids) for ids in id_lists]
    idb, ioff = _pack_ids(i for ids in id_lists for i in ids)
    set_id_off = np.zeros(len(id_lists) + 1, dtype=np.uintp)
    if id_lists:
        set_id_off[1:] = np.cumsum([len(ids) for ids in id_lists])
    qv, qoff, set_off = _pack_sets(sets)
    n = len(set_off) - 1
    outs, status = (C.c_void_p * max(n, 1))(), (C.c_int * max(n, 1))()
    st = _lib.load().vt_mv_top_k_ids_batch(store.handle, n, _szp(set_id_off), idb, _szp(ioff), _szp(set_off), _fp(qv),
                                           _szp(qoff), metric_code, limit, outs, status)
    return _mv_batch_results(st, outs, status, n, with_keys)


def mv_counters(store: MvRef) -> dict:
    launches, sets = C.c_uint64(), C.c_uint64()
    st = _lib.load().vt_mv_counters(store.handle, C.byref(launches), C.byref(sets))
    if st != 0:
        raise RuntimeError("mv_counters: " + _lib.error_text(st))
    return {"scoring_launches": launches.value, "batched_sets": sets.value}


def mv_memory(store: MvRef) -> dict:
    vectors, cap, dead = C.c_size_t(), C.c_size_t(), C.c_size_t()
    up, comp = C.c_uint64(), C.c_uint64()
    st = _lib.load().vt_mv_memory(store.handle, C.byref(vectors), C.byref(cap), C.byref(dead), C.byref(up), C.byref(comp))
    if st != 0:
        raise RuntimeError("mv_memory: " + _lib.error_text(st))
    return {"vectors": vectors.value, "row_capacity": cap.value, "dead_rows": dead.value, "uploaded_bytes": up.value,
            "compactions": comp.value}


# ------------------------------------------------------------------ MUVERA
MUVERA_QUERY, MUVERA_DOCUMENT = 0, 1
U64_MAX = (1 << 64) - 1
# ---------------------------------------------- HNSW index (hnsw_* NIFs, nifs.rs:311-426; vt_hnsw_*)
class HnswRef:
    """The `reference()` returned by hnsw_new_*: owns a vt_hnsw handle, freed with the object."""

    def __init__(self, handle, metric: int):
        self.handle = handle
        self.metric = metric

    def __del__(self):
        try:
            if self.handle:
                _lib.load().vt_hnsw_free(self.handle)
                self.handle = None
        except Exception:
            pass

    def __len__(self):
        return _lib.load().vt_hnsw_len(self.handle)

    @property
    def dimension(self):
        d = _lib.load().vt_hnsw_dimension(self.handle)
        return None if d < 0 else d


def _hnsw_new(metric: int, m, m0, ef_construction, ef_search, max_level, device=None):
    """nifs.rs:311-374: ("ok", ref) | ("error", HnswParams::validate's string); no device: RuntimeError."""
    for v in (m, m0, ef_construction, ef_search, max_level):
        if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= USIZE_MAX:
            raise TypeError("badarg: hnsw parameters are usize")
    h = C.c_void_p()
    st = _lib.load().vt_hnsw_new(metric, DEVICE if device is None else device, m, m0, ef_construction, ef_search, max_level,
                                 C.byref(h))
    if 29 <= st <= 35:
        return _err(st)
    if st != 0:
        raise RuntimeError("hnsw_new: " + _lib.error_text(st))
    return ("ok", HnswRef(h, metric))


def hnsw_new_l2(m, m0, ef_construction, ef_search, max_level, device=None):
    return _hnsw_new(0, m, m0, ef_construction, ef_search, max_level, device)


def hnsw_new_cosine(m, m0, ef_construction, ef_search, max_level, device=None):
    return _hnsw_new(2, m, m0, ef_construction, ef_search, max_level, device)


def hnsw_new_inner_product(m, m0, ef_construction, ef_search, max_level, device=None):
    return _hnsw_new(3, m, m0, ef_construction, ef_search, max_level, device)


def hnsw_insert(index: HnswRef, id_, vector):
    """nifs.rs:376-388."""
    b, v = _bytes(id_), _f32_list(vector)
    st = _lib.load().vt_hnsw_insert(index.handle, b, len(b), _fp(v), v.size)
    return ("ok", ()) if st == 0 else _err(st)


def hnsw_insert_many(index: HnswRef, vectors: Sequence[Tuple[object, Sequence[float]]]):
    """nifs.rs:390-401."""
    vectors = list(vectors)
    ids, ioff = _pack_ids(i for i, _ in vectors)
    vals, voff = _pack_ragged([_f32_list(v) for _, v in vectors], np.float32)
    st = _lib.load().vt_hnsw_insert_many(index.handle, len(vectors), ids, _szp(ioff), _fp(vals), _szp(voff))
    return ("ok", ()) if st == 0 else _err(st)


def hnsw_delete(index: HnswRef, id_):
    """nifs.rs:403-412."""
    b = _bytes(id_)
    st = _lib.load().vt_hnsw_delete(index.handle, b, len(b))
    return ("ok", ()) if st == 0 else _err(st)


def hnsw_search(index: HnswRef, query, limit: int, with_keys: bool = False):
    """nifs.rs:414-426 -> [(id, raw)] ascending by (rank, id)."""
    if not isinstance(limit, int) or limit < 0 or limit > USIZE_MAX:
        raise TypeError("badarg: limit must fit usize")
    q = _f32_list(query)
    h = C.c_void_p()
    st = _lib.load().vt_hnsw_search(index.handle, _fp(q), q.size, limit, C.byref(h))
    return ("ok", _export_hits(h, with_keys)) if st == 0 else _err(st)


def hnsw_search_batch(index: HnswRef, queries, limit: int, with_keys: bool = False):
    """Extension: `queries` is an [nq][d] matrix, one traversal launch for all of them: [("ok", hits) | ("error",
    reason)] per query, each exactly what hnsw_search returns for that query alone."""
    if not isinstance(limit, int) or limit < 0 or limit > USIZE_MAX:
        raise TypeError("badarg: limit must fit usize")
    q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
    if q.ndim != 2:
        raise TypeError("badarg: queries must be a matrix")
    nq, d = q.shape
    outs, status = (C.c_void_p * max(nq, 1))(), (C.c_int * max(nq, 1))()
    st = _lib.load().vt_hnsw_search_batch(index.handle, _fp(q.reshape(-1)), nq, d, limit, outs, status)
    return _mv_batch_results(st, outs, status, nq, with_keys)


def hnsw_node(index: HnswRef, id_):
    """(internal id, level, is_entry) of a live id, None when there is none (inspection: tests compare graphs)."""
    b = _bytes(id_)
    iid, level, entry = C.c_uint64(), C.c_uint32(), C.c_int()
    st = _lib.load().vt_hnsw_node(index.handle, b, len(b), C.byref(iid), C.byref(level), C.byref(entry))
    return (iid.value, level.value, bool(entry.value)) if st == 0 else None


def hnsw_neighbors(index: HnswRef, internal_id: int, layer: int):
    """The internal ids of a node's list on one layer, in list order; None: no such node or layer."""
    L = _lib.load()
    n = C.c_size_t()
    if L.vt_hnsw_neighbors(index.handle, internal_id, layer, None, 0, C.byref(n)) != 0:
        return None
    out = (C.c_uint64 * max(n.value, 1))()
    L.vt_hnsw_neighbors(index.handle, internal_id, layer, out, n.value, C.byref(n))
    return [int(out[i]) for i in range(n.value)]


def hnsw_counters(index: HnswRef) -> dict:
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    st = _lib.load().vt_hnsw_counters(index.handle, C.byref(a), C.byref(b), C.byref(c))
    if st != 0:
        raise RuntimeError("hnsw_counters: " + _lib.error_text(st))
    return {"traversal_launches": a.value, "traversals": b.value, "reruns": c.value}


def hnsw_memory(index: HnswRef) -> dict:
    a, b, c, d = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    st = _lib.load().vt_hnsw_memory(index.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    if st != 0:
        raise RuntimeError("hnsw_memory: " + _lib.error_text(st))
    return {"rows": a.value, "row_capacity": b.value, "dead_rows": c.value, "edges": d.value}


_MUVERA_SET_ERRORS = (2, 3, 20, 28)  # dimension mismatch, non-finite, "empty vectors", "encoding overflow"
_FDE_DOC_ERRORS = (20, 28)           # what a resident document can answer: "empty vectors", "encoding overflow"


def _usize(v, what):
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= USIZE_MAX:
        raise TypeError("badarg: %s is a usize" % what)
    return v


def muvera_fde_dimension(num_repetitions: int, num_simhash_projections: int, projection_dimension: int,
                         final_projection_dimension) -> int:
    """Length of an encoding under this configuration (0: the configuration is not valid)."""
    some = final_projection_dimension is not None
    return int(_lib.load().vt_muvera_fde_dimension(num_repetitions, num_simhash_projections, projection_dimension,
                                                   final_projection_dimension if some else 0, 1 if some else 0))


def _muvera_call(sets, mode, dimension, num_repetitions, num_simhash_projections, seed, projection_dimension,
                 final_projection_dimension, want_status):
    for name, v in (("dimension", dimension), ("num_repetitions", num_repetitions),
                    ("num_simhash_projections", num_simhash_projections), ("projection_dimension", projection_dimension)):
        _usize(v, name)
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed <= U64_MAX:
        raise TypeError("badarg: seed is a u64")
    some = final_projection_dimension is not None
    if some:
        _usize(final_projection_dimension, "final_projection_dimension")
    per_set = [[_f32_list(v) for v in vectors] for vectors in sets]
    set_off = np.zeros(len(per_set) + 1, dtype=np.uintp)
    if per_set:
        set_off[1:] = np.cumsum([len(v) for v in per_set])
    vals, voff = _pack_ragged([v for vectors in per_set for v in vectors], np.float32)
    fde = muvera_fde_dimension(num_repetitions, num_simhash_projections, projection_dimension, final_projection_dimension)
    out = np.zeros((len(per_set), fde), dtype=np.float32)
    status = np.zeros(max(len(per_set), 1), dtype=np.intc)
    st = _lib.load().vt_muvera_encode(DEVICE, mode, len(per_set), _szp(set_off), _fp(vals), _szp(voff), dimension,
                                      num_repetitions, num_simhash_projections, seed, projection_dimension,
                                      final_projection_dimension if some else 0, 1 if some else 0,
                                      _fp(out.reshape(-1)) if out.size else None,
                                      status.ctypes.data_as(C.POINTER(C.c_int)) if want_status else None)
    return st, out, status[:len(per_set)]


def _muvera_one(vectors, mode, *config):
    st, out, _ = _muvera_call([vectors], mode, *config, want_status=False)
    return ("ok", [float(x) for x in out[0]]) if st == 0 else _err(st)


def muvera_encode_query(vectors, dimension: int, num_repetitions: int, num_simhash_projections: int, seed: int,
                        projection_dimension: int, final_projection_dimension):
    """nifs.rs:430-451: ("ok", [float]) or ("error", reason); final_projection_dimension is None or an integer."""
    return _muvera_one(vectors, MUVERA_QUERY, dimension, num_repetitions, num_simhash_projections, seed,
                       projection_dimension, final_projection_dimension)


def muvera_encode_document(vectors, dimension: int, num_repetitions: int, num_simhash_projections: int, seed: int,
                           projection_dimension: int, final_projection_dimension):
    """nifs.rs:455-476."""
    return _muvera_one(vectors, MUVERA_DOCUMENT, dimension, num_repetitions, num_simhash_projections, seed,
                       projection_dimension, final_projection_dimension)


def muvera_encode_batch(sets, mode: int, dimension: int, num_repetitions: int, num_simhash_projections: int, seed: int,
                        projection_dimension: int, final_projection_dimension):
    """Extension: every set of `sets` in one call.  ("ok", (matrix [count][fde] float32, [reason or None per set])) --
    a set with a reason keeps a zero row --, or ("error", reason) when the configuration itself is refused."""
    st, out, status = _muvera_call(sets, mode, dimension, num_repetitions, num_simhash_projections, seed,
                                   projection_dimension, final_projection_dimension, want_status=True)
    if st != 0 and len(status) == 1 and st in _MUVERA_SET_ERRORS:
        status = [st]   # (one set is the NIF call: its own error is the call's status)
    elif st != 0:
        return _err(st)
    return ("ok", (out, [None if s == 0 else _lib.error_text(int(s)) for s in status]))


# ---------------------------------------------- MUVERA retrieval over a resident store (vt_mv_encode_documents, vt_mv_fde_*)
def _muvera_cfg(config):
    """(dimension, num_repetitions, num_simhash_projections, seed, projection_dimension, final_projection_dimension | None)
    -> vt_muvera_encode's seven trailing arguments."""
    dimension, num_repetitions, num_simhash_projections, seed, projection_dimension, final_projection_dimension = config
    for name, v in (("dimension", dimension), ("num_repetitions", num_repetitions),
                    ("num_simhash_projections", num_simhash_projections), ("projection_dimension", projection_dimension)):
        _usize(v, name)
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed <= U64_MAX:
        raise TypeError("badarg: seed is a u64")
    some = final_projection_dimension is not None
    if some:
        _usize(final_projection_dimension, "final_projection_dimension")
    return (dimension, num_repetitions, num_simhash_projections, seed, projection_dimension,
            final_projection_dimension if some else 0, 1 if some else 0)


def mv_encode_documents(store: MvRef, ids, config):
    """The document-mode encoding of every listed resident document, read from the store's rows:
    ("ok", (matrix [count][fde] float32, [reason or None per document])) -- a document with a reason keeps a zero row --,
    or ("error", reason) when the call itself is refused."""
    cfg = _muvera_cfg(config)
    idb, ioff = _pack_ids(ids)
    n = ioff.size - 1
    fde = muvera_fde_dimension(config[1], config[2], config[4], config[5])
    out = np.zeros((n, fde), dtype=np.float32)
    status = np.zeros(max(n, 1), dtype=np.intc)
    st = _lib.load().vt_mv_encode_documents(store.handle, n, idb, _szp(ioff), *cfg, _fp(out.reshape(-1)) if out.size else None,
                                            status.ctypes.data_as(C.POINTER(C.c_int)))
    if st != 0 and n == 1 and st in _FDE_DOC_ERRORS:
        status = [st]   # (one document: its own error is the call's status)
    elif st != 0:
        return _err(st)
    return ("ok", (out, [None if s == 0 else _lib.error_text(int(s)) for s in status[:n]]))


def mv_fde_sync(store: MvRef, index: FlatRef, ids, config):
    """Brings `index` in line with the store for the listed ids (None: every live document).  ("ok", [reason or None per
    listed id]) -- a reason means the id is absent from `index` --, or ("error", reason)."""
    cfg = _muvera_cfg(config)
    if ids is None:
        st = _lib.load().vt_mv_fde_sync(store.handle, index.handle, 0, None, None, *cfg, None)
        return ("ok", []) if st == 0 or st in _FDE_DOC_ERRORS else _err(st)
    idb, ioff = _pack_ids(ids)
    n = ioff.size - 1
    status = np.zeros(max(n, 1), dtype=np.intc)
    st = _lib.load().vt_mv_fde_sync(store.handle, index.handle, n, idb, _szp(ioff), *cfg, status.ctypes.data_as(C.POINTER(C.c_int)))
    if st != 0 and n == 1 and st in _FDE_DOC_ERRORS:
        status = [st]
    elif st != 0:
        return _err(st)
    return ("ok", [None if s == 0 else _lib.error_text(int(s)) for s in status[:n]])


def mv_fde_top_k(store: MvRef, index: FlatRef, config, query_vectors, candidates: int, metric_code: int, limit: int,
                 with_keys: bool = False):
    """mv_top_k_ids over the `candidates` documents whose encodings in `index` have the largest inner product with the
    query's encoding."""
    _mv_search_args(metric_code, limit)
    _usize(candidates, "candidates")
    cfg = _muvera_cfg(config)
    qv, qoff = _vector_list(query_vectors)
    h = C.c_void_p()
    st = _lib.load().vt_mv_fde_top_k(store.handle, index.handle, *cfg, _fp(qv), _szp(qoff), qoff.size - 1, candidates, metric_code,
                                     limit, C.byref(h))
    return ("ok", _export_hits(h, with_keys)) if st == 0 else _err(st)


def mv_fde_top_k_batch(store: MvRef, index: FlatRef, config, sets, candidates: int, metric_code: int, limit: int,
                       with_keys: bool = False):
    """mv_fde_top_k for every query set in one call: [("ok", hits) | ("error", reason)] per set; ("error", reason) when
    the call itself fails."""
    _mv_search_args(metric_code, limit)
    _usize(candidates, "candidates")
    cfg = _muvera_cfg(config)
    qv, qoff, set_off = _pack_sets(sets)
    n = len(set_off) - 1
    outs, status = (C.c_void_p * max(n, 1))(), (C.c_int * max(n, 1))()
    st = _lib.load().vt_mv_fde_top_k_batch(store.handle, index.handle, *cfg, n, _szp(set_off), _fp(qv), _szp(qoff), candidates,
                                           metric_code, limit, outs, status)
    return _mv_batch_results(st, outs, status, n, with_keys)


def binary_top_k(vectors, query, dimensions: int, limit: int):
    """nifs.rs:164-175."""
    ids, ioff = _pack_ids(i for i, _ in vectors)
    vals, voff = _pack_ragged([_u64_list(v) for _, v in vectors], np.uint64)
    q = _u64_list(query)
    h = C.c_void_p()
    st = _lib.load().vt_binary_top_k(DEVICE, len(vectors), ids, _szp(ioff), _up(vals), _szp(voff), _up(q), q.size,
                                     dimensions, limit, C.byref(h))
    return ("ok", _take_hits(h)) if st == 0 else _err(st)


def normalize_l2(vector):
    """nifs.rs:107-111."""
    v = _f32_list(vector)
    out = np.empty_like(v)
    st = _lib.load().vt_normalize_l2(DEVICE, 1, v.size, _fp(v), _fp(out))
    return ("ok", out) if st == 0 else _err(st)


def compress_sign_bits(vector):
    """nifs.rs:125-129: bare list of u64 words."""
    v = _f32_list(vector)
    words = np.zeros((v.size + 63) // 64, dtype=np.uint64)
    st = _lib.load().vt_compress_sign_bits(DEVICE, 1, v.size, _fp(v), _up(words))
    if st != 0:
        raise RuntimeError("compress_sign_bits: " + _lib.error_text(st))
    return [int(w) for w in words]


def normalize_zscore(vector):
    """nifs.rs:113-117."""
    v = _f32_list(vector)
    out = np.empty_like(v)
    st = _lib.load().vt_normalize_zscore(DEVICE, 1, v.size, _fp(v), _fp(out))
    return ("ok", out) if st == 0 else _err(st)


def normalize_minmax(vector):
    """nifs.rs:119-123."""
    v = _f32_list(vector)
    out = np.empty_like(v)
    st = _lib.load().vt_normalize_minmax(DEVICE, 1, v.size, _fp(v), _fp(out))
    return ("ok", out) if st == 0 else _err(st)


NORM_MODES = {"none": 0, "l2": 1, "zscore": 2, "minmax": 3}   # VT_NORM_*


def _norm_mode(mode) -> int:
    if isinstance(mode, str):
        if mode not in NORM_MODES:
            raise TypeError("badarg: unknown normalization")
        return NORM_MODES[mode]
    return int(mode)


def prepare_rows(matrix, mode):
    """Extension: Collection.prepare_embedding's vector work (collection.ex:921-946) for every row of a [count][d]
    matrix in one call -- finite check, normalization `mode` ("none" | "l2" | "zscore" | "minmax", or VT_NORM_*), sign
    bits of the normalized rows.  ("ok", (normalized float32 [count][d], words uint64 [count][(d + 63) // 64])), or
    ("error", reason, first_refused) with the smallest refused row (None when the call was refused as a whole)."""
    m = np.ascontiguousarray(matrix, dtype=np.float32)
    if m.ndim != 2:
        raise TypeError("badarg: matrix must be two-dimensional")
    count, d = m.shape
    out = np.empty_like(m)
    words = np.zeros((count, (d + 63) // 64), dtype=np.uint64)
    first = C.c_size_t(count)
    st = _lib.load().vt_prepare_rows(DEVICE, _norm_mode(mode), count, d, _fp(m.reshape(-1)), _fp(out.reshape(-1)),
                                     _up(words.reshape(-1)), C.byref(first))
    if st != 0:
        return ("error", _lib.error_text(st), int(first.value) if first.value < count else None)
    return ("ok", (out, words))


def prepare_device_rows(mode, count: int, d: int, in_ptr: int, ld_in: int, out_ptr: int, ld_out: int, words_ptr: int = 0):
    """Extension: prepare_rows on rows already resident in this device's HBM (raw device pointers, like
    flat_load_device_matrix): row-major f32 at `in_ptr` with rows `ld_in` floats apart, normalized into `out_ptr`
    (`ld_out`; may be `in_ptr` itself), sign words into `words_ptr` (0: none).  ("ok", ()) or
    ("error", reason, first_refused): refused rows are unwritten, every other row is written."""
    first = C.c_size_t(count)
    st = _lib.load().vt_prepare_device_rows(DEVICE, _norm_mode(mode), count, d, ld_in, C.c_void_p(in_ptr), ld_out,
                                            C.c_void_p(out_ptr), C.c_void_p(words_ptr) if words_ptr else None,
                                            C.byref(first))
    if st != 0:
        return ("error", _lib.error_text(st), int(first.value) if first.value < count else None)
    return ("ok", ())


# -------------------------------------------- bulk / device-side extensions
def flat_load_matrix(index: FlatRef, ids: Sequence, matrix: np.ndarray):
    """insert_many of equal-length rows from one dense host matrix."""
    m = np.ascontiguousarray(matrix, dtype=np.float32)
    idb, ioff = _pack_ids(ids)
    st = _lib.load().vt_flat_load_matrix(index.handle, m.shape[0], m.shape[1], idb, _szp(ioff), _fp(m.reshape(-1)))
    return ("ok", ()) if st == 0 else _err(st)


def flat_load_device_matrix(index: FlatRef, ids_packed: Tuple[bytes, np.ndarray], device_ptr: int, count: int, d: int):
    """insert_many of `count` rows already resident in this device's HBM
    (row-major f32 [count][d] at `device_ptr`)."""
    idb, ioff = ids_packed
    st = _lib.load().vt_flat_load_device_matrix(index.handle, count, d, idb, _szp(ioff), C.c_void_p(device_ptr))
    return ("ok", ()) if st == 0 else _err(st)


def flat_quantized_search(index: FlatRef, query, candidates: int, limit: int):
    """collection.ex:276-295 as one native call on the resident corpus."""
    q = _f32_list(query)
    h = C.c_void_p()
    st = _lib.load().vt_flat_quantized_search(index.handle, _fp(q), q.size, candidates, limit, C.byref(h))
    return ("ok", _take_hits(h)) if st == 0 else _err(st)


def flat_quantized_search_batch(index: FlatRef, queries, candidates: int, limit: int):
    """Extension: nq quantized searches in one call ([nq][d] matrix); each hit list identical to
    flat_quantized_search of that query -- groups of up to eight share a sweep of the sign bits."""
    q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
    if q.ndim != 2:
        raise TypeError("badarg: queries must be a matrix")
    nq, d = q.shape
    outs = (C.c_void_p * max(nq, 1))()
    st = _lib.load().vt_flat_quantized_search_batch(index.handle, _fp(q.reshape(-1)), nq, d, candidates, limit, outs)
    if st != 0:
        return _err(st)
    return ("ok", [_take_hits(C.c_void_p(outs[i])) for i in range(nq)])


def flat_funnel_search(index: FlatRef, query, stages: Sequence[int], candidates: int, limit: int):
    """collection.ex:245-260 as one native call on the resident corpus."""
    q = _f32_list(query)
    st = np.ascontiguousarray(np.asarray(list(stages), dtype=np.uintp))
    h = C.c_void_p()
    rc = _lib.load().vt_flat_funnel_search(index.handle, _fp(q), q.size, _szp(st), st.size, candidates, limit, C.byref(h))
    return ("ok", _take_hits(h)) if rc == 0 else _err(rc)


def flat_funnel_search_batch(index: FlatRef, queries, stages: Sequence[int], candidates: int, limit: int):
    """Extension: nq funnel searches with one set of stages in one call ([nq][d] matrix); each hit list
    identical to flat_funnel_search of that query -- on a cosine collection groups of up to eight
    share the stage-1 sweep of the prefixes."""
    q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
    if q.ndim != 2:
        raise TypeError("badarg: queries must be a matrix")
    nq, d = q.shape
    st = np.ascontiguousarray(np.asarray(list(stages), dtype=np.uintp))
    outs = (C.c_void_p * max(nq, 1))()
    rc = _lib.load().vt_flat_funnel_search_batch(index.handle, _fp(q.reshape(-1)), nq, d, _szp(st), st.size, candidates, limit, outs)
    if rc != 0:
        return _err(rc)
    return ("ok", [_take_hits(C.c_void_p(outs[i])) for i in range(nq)])


GEN_FUNNEL, GEN_QUANTIZED, GEN_SEARCH = 0, 1, 2


def flat_hybrid_search(index: FlatRef, query, generators, limit: int):
    """hybrid_search(rerank: :exact) on the resident corpus.  `generators` is a list of
    (kind, candidates, stages) with kind in GEN_*; stages only for GEN_FUNNEL."""
    q = _f32_list(query)
    kinds = (C.c_int * len(generators))(*[g[0] for g in generators])
    cands = np.ascontiguousarray([g[1] for g in generators], dtype=np.uintp)
    flat_stages, off = [], [0]
    for g in generators:
        flat_stages.extend(g[2] if g[0] == GEN_FUNNEL else [])
        off.append(len(flat_stages))
    st = np.ascontiguousarray(flat_stages if flat_stages else [0], dtype=np.uintp)
    so = np.ascontiguousarray(off, dtype=np.uintp)
    h = C.c_void_p()
    rc = _lib.load().vt_flat_hybrid_search(index.handle, _fp(q), q.size, kinds, _szp(cands), _szp(so), _szp(st),
                                           len(generators), limit, C.byref(h))
    return ("ok", _take_hits(h)) if rc == 0 else _err(rc)


def hnsw_quantized_search(index: HnswRef, query, candidates: int, limit: int, with_keys: bool = False):
    """collection.ex:276-295 on the HNSW index's rows: flat_quantized_search's answer over the same (id, vector) pairs.
    (The library's three staged entry points take either kind of handle: include/vettore_flat.h, VT_HNSW_STAGED.)"""
    q = _f32_list(query)
    h = C.c_void_p()
    st = _lib.load().vt_flat_quantized_search(index.handle, _fp(q), q.size, candidates, limit, C.byref(h))
    return ("ok", _export_hits(h, with_keys)) if st == 0 else _err(st)


def hnsw_funnel_search(index: HnswRef, query, stages: Sequence[int], candidates: int, limit: int, with_keys: bool = False):
    """collection.ex:245-260 on the HNSW index's rows: flat_funnel_search's answer over the same (id, vector) pairs."""
    q = _f32_list(query)
    st = np.ascontiguousarray(np.asarray(list(stages), dtype=np.uintp))
    h = C.c_void_p()
    rc = _lib.load().vt_flat_funnel_search(index.handle, _fp(q), q.size, _szp(st), st.size, candidates, limit, C.byref(h))
    return ("ok", _export_hits(h, with_keys)) if rc == 0 else _err(rc)


def hnsw_hybrid_search(index: HnswRef, query, generators, limit: int, with_keys: bool = False):
    """hybrid_search(rerank: :exact) on the HNSW index's rows.  `generators` as flat_hybrid_search takes them; GEN_SEARCH is
    the index's own traversal with limit = candidates (hnsw_candidates, collection.ex:594-600)."""
    q = _f32_list(query)
    kinds = (C.c_int * len(generators))(*[g[0] for g in generators])
    cands = np.ascontiguousarray([g[1] for g in generators], dtype=np.uintp)
    flat_stages, off = [], [0]
    for g in generators:
        flat_stages.extend(g[2] if g[0] == GEN_FUNNEL else [])
        off.append(len(flat_stages))
    st = np.ascontiguousarray(flat_stages if flat_stages else [0], dtype=np.uintp)
    so = np.ascontiguousarray(off, dtype=np.uintp)
    h = C.c_void_p()
    rc = _lib.load().vt_flat_hybrid_search(index.handle, _fp(q), q.size, kinds, _szp(cands), _szp(so), _szp(st),
                                           len(generators), limit, C.byref(h))
    return ("ok", _export_hits(h, with_keys)) if rc == 0 else _err(rc)


def rank_ids(ids_packed: Tuple[bytes, np.ndarray]) -> np.ndarray:
    """Position of every id in the bytewise order of all of them (vt_rank_ids)."""
    blob, off = ids_packed
    n = len(off) - 1
    out = np.empty(n, dtype=np.uint32)
    st = _lib.load().vt_rank_ids(blob, _szp(off), n, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    if st != 0:
        raise RuntimeError("rank_ids: " + _lib.error_text(st))
    return out


def flat_set_id_ranks(index: FlatRef, ranks: np.ndarray):
    r = np.ascontiguousarray(ranks, dtype=np.uint32)
    st = _lib.load().vt_flat_set_id_ranks(index.handle, r.ctypes.data_as(C.POINTER(C.c_uint32)), r.size)
    return "ok" if st == 0 else _err(st)


def flat_stream(index: FlatRef) -> int:
    """The hipStream_t (as an integer) the index enqueues its kernels on."""
    return int(_lib.load().vt_flat_stream(index.handle) or 0)


def flat_search_begin(index: FlatRef, query, limit: int, device_block_ptr: int):
    """Enqueue one shard's search; the result block lands at `device_block_ptr`."""
    q = _f32_list(query)
    st = _lib.load().vt_flat_search_begin(index.handle, _fp(q), q.size, limit, C.c_void_p(device_block_ptr))
    return "ok" if st == 0 else _err(st)


class MergeBuffers:
    """Reusable output arrays of flat_merge_gathered."""

    def __init__(self, cap: int = 256):
        self.keys = np.zeros(cap, dtype=np.uint64)
        self.rows = np.zeros(cap, dtype=np.uint32)
        self.raw = np.zeros(cap, dtype=np.float32)
        self.shard = np.zeros(cap, dtype=np.uint32)
        self.count = C.c_size_t()
        self.ptrs = (self.keys.ctypes.data_as(C.POINTER(C.c_uint64)), self.rows.ctypes.data_as(C.POINTER(C.c_uint32)),
                     self.raw.ctypes.data_as(C.POINTER(C.c_float)), self.shard.ctypes.data_as(C.POINTER(C.c_uint32)))


def flat_merge_gathered(index: FlatRef, device_blocks_ptr: int, world: int, limit: int, block_bytes: int,
                        bufs: MergeBuffers):
    """Merge `world` gathered shard blocks on the device, wait, return the number of winners
    (their keys / rows / raw / shard are in `bufs`)."""
    st = _lib.load().vt_flat_merge_gathered(index.handle, C.c_void_p(device_blocks_ptr), world, limit, block_bytes,
                                            *bufs.ptrs, C.byref(bufs.count))
    return ("ok", int(bufs.count.value)) if st == 0 else _err(st)


def flat_set_reduce_order(index: FlatRef, order: int):
    st = _lib.load().vt_flat_set_reduce_order(index.handle, order)
    return "ok" if st == 0 else _err(st)


def flat_set_batch_nominate(index: FlatRef, mode: int):
    """Which matrix-core pass nominates batch candidates: _lib.NOMINATE_BF16 (default) or NOMINATE_F32."""
    st = _lib.load().vt_flat_set_batch_nominate(index.handle, mode)
    return "ok" if st == 0 else _err(st)


def flat_batch_nominate(index: FlatRef) -> int:
    return int(_lib.load().vt_flat_batch_nominate(index.handle))


def flat_set_batch_shadow(index: FlatRef, mode: int):
    """Whether the bf16 nomination pass may keep a bf16 shadow of the rows: _lib.SHADOW_AUTO (default) or SHADOW_OFF."""
    st = _lib.load().vt_flat_set_batch_shadow(index.handle, mode)
    return ("ok", ()) if st == _lib.VT_OK else ("error", _lib.error_text(st))


def flat_set_single_nominate(index: FlatRef, enabled: bool):
    """Opt-in: lone flat_search calls go through the bf16 shadow like a batch of one (same hits, ~0.6 of the scan's time)."""
    st = _lib.load().vt_flat_set_single_nominate(index.handle, 1 if enabled else 0)
    return ("ok", ()) if st == _lib.VT_OK else ("error", _lib.error_text(st))


def flat_batch_shadow(index: FlatRef) -> str:
    """State of shard 0's shadow: "off", "none" (not built yet), "current", "stale" or "refused" (no room)."""
    return _lib.SHADOW_STATE.get(int(_lib.load().vt_flat_batch_shadow(index.handle)), "?")


# ----------------------------------------------------------------- MMR reranking
_MMR_INVALID = ("error", "invalid_mmr_args")
_MMR_ARGS = 38  # VT_ERR_MMR_ARGS
_SCORE_MODE = {"raw": 0, "similarity": 1}


def _is_number(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _finite_number(v) -> bool:
    """finite_number?/1 (lib/vettore_distance.ex:407-414): an integer or a float within the f32 range."""
    return _is_number(v) and -_F32_MAX <= v <= _F32_MAX


def _is_binary(v) -> bool:
    return isinstance(v, (bytes, bytearray, str))


def _mmr_guards(alpha, final_k) -> bool:
    return (_is_number(alpha) and 0 <= alpha <= 1 and isinstance(final_k, int) and not isinstance(final_k, bool)
            and final_k > 0)


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _f64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def mmr_rerank(initial, embeddings, metric, alpha, final_k):
    """`Vettore.Distance.mmr_rerank/5` (lib/vettore_distance.ex:334-519) with the reference's validation order and atoms:
    ("ok", [(id, score)]) -- the chosen entries of `initial`, the caller's own objects, in order of choice --,
    ("error", "invalid_mmr_args"), ("error", ("unknown_metric", metric)) or ("error", "metric_overflow").  The rounds run
    on the device (vt_mmr_rerank): the vectors of the initial entries go up once, nothing but the order comes back."""
    if not (isinstance(initial, list) and isinstance(embeddings, list) and _mmr_guards(alpha, final_k)):
        return _MMR_INVALID
    if not (isinstance(metric, str) and metric in METRIC_CODE):
        return ("error", ("unknown_metric", metric))
    vectors, expected = {}, None
    for embedding in embeddings:  # validate_mmr_embeddings (:347-387)
        if not (isinstance(embedding, tuple) and len(embedding) == 2):
            return _MMR_INVALID
        id_, vector = embedding
        if not (_is_binary(id_) and len(id_) > 0 and isinstance(vector, list) and vector != []):
            return _MMR_INVALID
        if id_ in vectors or expected not in (None, len(vector)) or not all(_finite_number(v) for v in vector):
            return _MMR_INVALID
        vectors[id_] = vector
        expected = expected or len(vector)
    seen = set()
    for entry in initial:  # validate_mmr_initial (:389-405)
        if not (isinstance(entry, tuple) and len(entry) == 2 and _is_binary(entry[0]) and len(entry[0]) > 0):
            return _MMR_INVALID
        id_, score = entry
        if not (_finite_number(score) and id_ in vectors and id_ not in seen):
            return _MMR_INVALID
        seen.add(id_)
    n = len(initial)
    if n == 0:
        return ("ok", [])
    rows = np.ascontiguousarray(np.array([[float(v) for v in vectors[id_]] for id_, _ in initial], dtype=np.float64)
                                .astype(np.float32))
    scores = np.ascontiguousarray(np.array([float(s) for _, s in initial], dtype=np.float64))
    order = np.zeros(n, dtype=np.uint32)
    count = C.c_size_t()
    st = _lib.load().vt_mmr_rerank(DEVICE, METRIC_CODE[metric], n, rows.shape[1], _fp(rows.reshape(-1)), _f64p(scores),
                                   float(alpha), min(final_k, n), _u32p(order), C.byref(count))
    if st == 4:
        return ("error", "metric_overflow")
    if st != 0:
        return _err(st)
    return ("ok", [initial[int(i)] for i in order[:count.value]])


def flat_mmr_rerank(index: FlatRef, initial, alpha, final_k):
    """mmr_rerank over the rows resident in `index` (one shard), under its metric: `initial` is [(id, score)];
    ("ok", [(id, score)]) -- the caller's entries in order of choice --, or ("error", reason) with the library's strings
    ("invalid mmr args": a bad alpha, final_k or score, an id that is not in the index or occurs twice; "metric
    overflow")."""
    if not (isinstance(initial, list) and _mmr_guards(alpha, final_k)
            and all(isinstance(e, tuple) and len(e) == 2 and _is_binary(e[0]) and _finite_number(e[1]) for e in initial)):
        return _err(_MMR_ARGS)
    n = len(initial)
    ids, off = _pack_ids(e[0] for e in initial)
    scores = np.ascontiguousarray(np.array([float(e[1]) for e in initial], dtype=np.float64))
    order = np.zeros(max(n, 1), dtype=np.uint32)
    count = C.c_size_t()
    st = _lib.load().vt_flat_mmr_rerank(index.handle, n, ids, _szp(off), _f64p(scores), float(alpha), min(final_k, max(n, 1)),
                                        _u32p(order), C.byref(count))
    if st != 0:
        return _err(st)
    return ("ok", [initial[int(i)] for i in order[:count.value]])


def flat_mmr_rerank_batch(index: FlatRef, problems):
    """Extension: flat_mmr_rerank for every (initial, alpha, final_k) of `problems` in one call, all of them one chain
    of step launches: [("ok", [(id, score)]) | ("error", reason)] per problem, each what flat_mmr_rerank returns for it
    alone; ("error", reason) when the call itself fails."""
    results = [None] * len(problems)
    live = []
    for p, (initial, alpha, final_k) in enumerate(problems):
        if not (isinstance(initial, list) and _mmr_guards(alpha, final_k)
                and all(isinstance(e, tuple) and len(e) == 2 and _is_binary(e[0]) and _finite_number(e[1]) for e in initial)):
            results[p] = _err(_MMR_ARGS)
        else:
            live.append(p)
    entries = [e for p in live for e in problems[p][0]]
    prob_off = np.zeros(len(live) + 1, dtype=np.uintp)
    if live:
        prob_off[1:] = np.cumsum([len(problems[p][0]) for p in live])
    ids, off = _pack_ids(e[0] for e in entries)
    scores = np.ascontiguousarray(np.array([float(e[1]) for e in entries] or [0.0], dtype=np.float64))
    alphas = np.ascontiguousarray(np.array([float(problems[p][1]) for p in live] or [0.0], dtype=np.float64))
    ks = np.array([min(problems[p][2], max(len(problems[p][0]), 1)) for p in live] or [1], dtype=np.uintp)
    order = np.zeros(max(len(entries), 1), dtype=np.uint32)
    counts = np.zeros(max(len(live), 1), dtype=np.uintp)
    status = (C.c_int * max(len(live), 1))()
    st = _lib.load().vt_flat_mmr_rerank_batch(index.handle, len(live), _szp(prob_off), ids, _szp(off), _f64p(scores),
                                              _f64p(alphas), _szp(ks), _u32p(order), _szp(counts), status)
    if st != 0:
        return _err(st)
    for j, p in enumerate(live):
        base = int(prob_off[j])
        results[p] = (("ok", [problems[p][0][int(i)] for i in order[base:base + int(counts[j])]]) if status[j] == 0
                      else _err(status[j]))
    return results


def _mmr_search_args(candidates, limit, alpha, score_mode):
    if not isinstance(candidates, int) or candidates < 0 or candidates > USIZE_MAX:
        raise TypeError("badarg: candidates must fit usize")
    if score_mode not in _SCORE_MODE:
        raise TypeError("badarg: score_mode must be \"raw\" or \"similarity\"")
    return _mmr_guards(alpha, limit)


def flat_mmr_search(index: FlatRef, query, candidates: int, limit: int, alpha, score_mode: str = "raw"):
    """Extension: flat_search(query, candidates), then MMR over its hits -- scored by result_values/3 for `score_mode` --
    down to `limit`, in one call under one lease: ("ok", (hits, order)) with `hits` exactly flat_search's and `order`
    the chosen hits' indices in order of choice; or ("error", reason)."""
    if not _mmr_search_args(candidates, limit, alpha, score_mode):
        return _err(_MMR_ARGS)
    q = _f32_list(query)
    cap = max(1, min(limit, candidates))
    order = np.zeros(cap, dtype=np.uint32)
    count = C.c_size_t()
    h = C.c_void_p()
    st = _lib.load().vt_flat_mmr_search(index.handle, _fp(q), q.size, candidates, min(limit, USIZE_MAX), float(alpha),
                                        _SCORE_MODE[score_mode], C.byref(h), _u32p(order), C.byref(count))
    if st != 0:
        return _err(st)
    return ("ok", (_take_hits(h), [int(i) for i in order[:count.value]]))


def flat_mmr_search_batch(index: FlatRef, queries, candidates: int, limit: int, alpha, score_mode: str = "raw"):
    """flat_mmr_search for every row of the [nq][d] matrix `queries` in one call, all queries one chain of step
    launches: ("ok", [("ok", (hits, order)) | ("error", reason) per query]), or ("error", reason) when the call itself
    fails (a search error, bad arguments)."""
    if not _mmr_search_args(candidates, limit, alpha, score_mode):
        return _err(_MMR_ARGS)
    q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
    if q.ndim != 2:
        raise TypeError("badarg: queries must be a matrix")
    nq, d = q.shape
    cap = max(1, min(limit, candidates))
    outs, status = (C.c_void_p * max(nq, 1))(), (C.c_int * max(nq, 1))()
    order = np.zeros(max(nq, 1) * cap, dtype=np.uint32)
    counts = np.zeros(max(nq, 1), dtype=np.uintp)
    st = _lib.load().vt_flat_mmr_search_batch(index.handle, _fp(q.reshape(-1)), nq, d, candidates, min(limit, USIZE_MAX),
                                              float(alpha), _SCORE_MODE[score_mode], outs, _u32p(order), _szp(counts), status)
    lists = [_take_hits(C.c_void_p(outs[b])) if outs[b] else None for b in range(nq)]
    if st != 0:
        return _err(st)
    cap = min(limit, candidates)
    return ("ok", [("ok", (lists[b], [int(i) for i in order[b * cap:b * cap + int(counts[b])]])) if status[b] == 0
                   else _err(status[b]) for b in range(nq)])


def set_default_reduce_order(order: int):
    st = _lib.load().vt_set_default_reduce_order(order)
    return "ok" if st == 0 else _err(st)


def debug_set(name: str, value: int):
    """A library setting by name (vt_debug_set, include/vettore_flat.h): the VT_* variables are read once,
    when the library is loaded; afterwards -- and for the switches that have no variable ("force_batch_mfma"
    ...) -- this is the way in.  Process-wide; tests and probes only."""
    st = _lib.load().vt_debug_set(name.encode(), int(value))
    if st != 0:
        raise KeyError("libvettore_hip has no setting %r" % name)


def debug_get(name: str) -> int:
    v = C.c_long()
    if _lib.load().vt_debug_get(name.encode(), C.byref(v)) != 0:
        raise KeyError("libvettore_hip has no setting %r" % name)
    return int(v.value)


class debug_setting:
    """`with nifs.debug_setting("batch_no_mfma", 1): ...` -- the old value comes back afterwards."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = debug_get(self.name)
        debug_set(self.name, self.value)
        return self

    def __exit__(self, *exc):
        debug_set(self.name, self.old)
        return False


def device_read_peak(device: int = 0, nbytes: int = 8 << 30, reps: int = 5):
    """GB/s of the plainest read-only streaming kernel on this box (diagnostic, bench.py)."""
    g = C.c_double()
    st = _lib.load().vt_device_read_peak(device, nbytes, reps, C.byref(g))
    return ("ok", float(g.value)) if st == 0 else _err(st)


def flat_set_profiling(index: FlatRef, enabled: bool):
    _lib.load().vt_flat_set_profiling(index.handle, 1 if enabled else 0)


def flat_get_profile(index: FlatRef, reset: bool = False) -> dict:
    p = _lib.Profile()
    _lib.load().vt_flat_get_profile(index.handle, C.byref(p), 1 if reset else 0)
    return {name: getattr(p, name) for name, _ in _lib.Profile._fields_}


pack_ids = _pack_ids
