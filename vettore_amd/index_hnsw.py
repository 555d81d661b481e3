"""Python mirror of `Vettore.Index.HNSW` (the reference's lib/vettore/index/hnsw.ex) over the GPU library: the module a
maintainer would name `Vettore.Index.HnswGpu` and select with `index: Vettore.Index.HnswGpu`.  The
graph is the reference's, node for node, and so are the hits (include/vettore_flat.h, "HNSW index").

Return conventions as in index_flat.py: "ok" | ("ok", value) | ("error", reason), atoms as plain strings.
"""
from __future__ import annotations

from typing import List

from . import nifs
from .index_flat import MAX_NIF_USIZE, FlatGpu, Result, Stages, _normalize_ok, _to_result

DEFAULT_OPTIONS = {"m": 16, "m0": 32, "ef_construction": 100, "ef_search": 64, "max_level": 12}  # hnsw.ex:13-19
MAX_M, MAX_M0, MAX_EF, MAX_LEVEL = 1_024, 2_048, 1_000_000, 64                                    # hnsw.ex:22-25

_NEW = {
    "l2": nifs.hnsw_new_l2,
    "cosine": nifs.hnsw_new_cosine,
    "inner_product": nifs.hnsw_new_inner_product,
}


def _positive(v):
    return isinstance(v, int) and not isinstance(v, bool) and v > 0


def _valid_options(o):
    """hnsw.ex:142-167."""
    m, m0, efc, efs, lvl = o["m"], o["m0"], o["ef_construction"], o["ef_search"], o["max_level"]
    return (_positive(m) and m <= MAX_M and _positive(m0) and m0 >= m and m0 <= MAX_M0 and
            _positive(efc) and efc >= m and efc <= MAX_EF and _positive(efs) and efs <= MAX_EF and
            _positive(lvl) and lvl <= MAX_LEVEL)


class HnswGpu:
    """`@behaviour Vettore.Index` with callbacks new/2, put/2, put_many/2, delete/2, search/3 (hnsw.ex:28-68)."""

    @staticmethod
    def defaults():
        return dict(DEFAULT_OPTIONS)

    @staticmethod
    def new(metric: str, opts=None):
        """hnsw.ex:31-35, :122-137.  A keyword list arrives as a list of pairs (duplicate keys are an error, as
        there) or as a dict; `device: n` is this module's one extra option, as for FlatGpu."""
        if opts is None:
            opts = []
        if isinstance(opts, dict):
            pairs = list(opts.items())
        elif isinstance(opts, (list, tuple)) and all(isinstance(p, tuple) and len(p) == 2 for p in opts):
            pairs = list(opts)
        else:
            return ("error", "invalid_hnsw_options")
        keys = [k for k, _ in pairs]
        if any(k not in DEFAULT_OPTIONS and k != "device" for k in keys) or len(set(keys)) != len(keys):
            return ("error", "invalid_hnsw_options")
        given = dict(pairs)
        device = given.pop("device", None)
        if device is not None and not (isinstance(device, int) and not isinstance(device, bool) and device >= 0):
            return ("error", "invalid_hnsw_options")
        options = dict(DEFAULT_OPTIONS, **given)
        if not _valid_options(options):
            return ("error", "invalid_hnsw_options")
        make = _NEW.get(metric)
        if make is None:
            return ("error", ("unsupported_hnsw_metric", metric))   # hnsw.ex:109
        try:
            return make(options["m"], options["m0"], options["ef_construction"], options["ef_search"],
                        options["max_level"], device)
        except RuntimeError as e:  # no such device, out of memory: the NIF's {:error, msg}
            return ("error", str(e))

    @staticmethod
    def put(collection, embedding):
        return _normalize_ok(nifs.hnsw_insert(collection.index_state, embedding.id, embedding.vector))

    @staticmethod
    def put_many(collection, embeddings):
        vectors = [(e.id, e.vector) for e in embeddings]          # hnsw.ex:48-51
        return _normalize_ok(nifs.hnsw_insert_many(collection.index_state, vectors))

    @staticmethod
    def delete(collection, id_):
        return _normalize_ok(nifs.hnsw_delete(collection.index_state, id_))

    @staticmethod
    def memory(collection):
        """What the index holds on the device: {"rows", "row_capacity", "dead_rows", "edges"} (vt_hnsw_memory).  `rows`
        are the slab rows handed out since the last compaction; an insert that finds more dead rows than live ones, and
        at least 64 of them, compacts first, and `dead_rows` is 0 again.  A delete never compacts."""
        return nifs.hnsw_memory(collection.index_state)

    @staticmethod
    def search(collection, query, opts=None):
        opts = {} if opts is None else opts
        if not isinstance(opts, dict) or any(k != "limit" for k in opts):
            return ("error", "invalid_search_options")            # hnsw.ex:175-182
        limit = opts.get("limit", 10)
        if not (isinstance(limit, int) and not isinstance(limit, bool) and 0 < limit <= MAX_NIF_USIZE):
            return ("error", "invalid_limit")                      # hnsw.ex:92-97
        prepared = collection.prepare_query(query)
        if prepared[0] != "ok":
            return prepared
        res = nifs.hnsw_search(collection.index_state, prepared[1], limit)
        if res[0] != "ok":
            return res
        out: List[Result] = []
        for id_, raw in res[1]:
            out.extend(_to_result(collection, id_, raw))          # hnsw.ex:70-90
        return ("ok", out)


HNSW_STAGES = Stages(nifs.hnsw_quantized_search, nifs.hnsw_funnel_search, nifs.hnsw_hybrid_search, nifs.hnsw_search,
                     ("hnsw", "quantized"), True)   # collection.ex:513: default_hybrid_generators of an :hnsw collection


class HnswStagedGpu(HnswGpu):
    """HnswGpu with the collection's staged searches (collection.ex:232-348) answered from the index's own rows
    (nifs.hnsw_quantized_search, hnsw_funnel_search, hnsw_hybrid_search): option handling and error atoms are
    FlatGpu's -- the same code --, the generators "hnsw" and "search" are both the index's own traversal, and
    hybrid_search defaults to ["hnsw", "quantized"].  Selected with index_options={"staged_searches": True}
    (collection.py); Vettore.Index.HnswGpu itself exports the three functions unconditionally."""

    @staticmethod
    def quantized_search(collection, query, opts=None):
        return FlatGpu.quantized_search(collection, query, opts, HNSW_STAGES)

    @staticmethod
    def funnel_search(collection, query, opts=None):
        return FlatGpu.funnel_search(collection, query, opts, HNSW_STAGES)

    @staticmethod
    def hybrid_search(collection, query, opts=None):
        return FlatGpu.hybrid_search(collection, query, opts, HNSW_STAGES)
