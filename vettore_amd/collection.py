"""Caller side of the flat hot path: the parts of `Vettore.Collection`
(/root/reference/lib/vettore/collection.ex) that sit directly above the index
plugin -- option defaults, prepare_query, two-phase put with rollback, search
dispatch and quantized_search.  The canonical record store (ETS in the
reference, lib/vettore/store/ets.ex) is a plain dict here: it is out of scope
 and only holds ids, values and metadata.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import numpy as np

from . import nifs
from .index_flat import FlatGpu, Result, result_values, MAX_NIF_USIZE
from .index_hnsw import HnswGpu, HnswStagedGpu
from .mv_store import ResidentMultiVector
from . import muvera as muvera_mod

F32_MAX = 3.4028234663852886e38  # collection.ex:61
METRIC_ALIASES = {"euclidean": "l2", "dot": "inner_product", "dot_product": "inner_product"}  # :1300-1304
METRICS = nifs.METRICS


@dataclass
class Embedding:
    """Vettore.Embedding (lib/vettore_embedding.ex)."""
    id: Any = None
    value: Any = None
    vector: Any = None
    binary_vector: Optional[List[int]] = None
    metadata: Any = None
    vectors: Optional[List[List[float]]] = None   # multi-vector (late-interaction) form; `vector` is then their mean


def _finite_f32(v) -> bool:  # collection.ex:1264-1270
    if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
        return False
    v = float(v)
    return not math.isnan(v) and -F32_MAX <= v <= F32_MAX


def _validate_vector(vector, dimensions):  # collection.ex:1087-1093
    if not isinstance(vector, (list, tuple, np.ndarray)):
        return ("error", "invalid_vector")
    if len(vector) != dimensions:
        return ("error", "dimension_mismatch")
    if all(_finite_f32(x) for x in vector):
        return "ok"
    return ("error", "invalid_vector")


class Collection:
    """%Vettore.Collection{} for `store: dict`, `index: FlatGpu` (or any object
    with the five Vettore.Index callbacks -- the reference's plugin point,
    collection.ex:72, :1283-1298)."""

    def __init__(self):
        raise TypeError("use Collection.new(...)")

    @classmethod
    def new(cls, dimensions=None, metric="cosine", normalize=None, index="flat", index_options=None,
            score="raw", name=None):
        metric = METRIC_ALIASES.get(metric, metric)
        if not (isinstance(dimensions, int) and dimensions > 0):
            return ("error", "invalid_dimensions")
        if metric not in METRICS:
            return ("error", "invalid_metric")
        if normalize is None:
            normalize = "l2" if metric == "cosine" else "none"     # collection.ex:1317-1319
        if normalize not in ("none", "l2", "zscore", "minmax"):      # collection.ex:50
            return ("error", "invalid_normalization")
        if score not in ("raw", "similarity"):
            return ("error", "invalid_score_mode")
        index_mod = FlatGpu if index in ("flat", "flat_gpu") else HnswGpu if index in ("hnsw", "hnsw_gpu") else index
        for cb in ("new", "put", "put_many", "delete", "search"):
            if not hasattr(index_mod, cb):
                return ("error", "invalid_index")
        # `staged_searches: true` is the collection's own option too, for the HNSW index alone: the index module becomes
        # HnswStagedGpu, which answers quantized_search / funnel_search / hybrid_search from the index's rows.  Without it
        # an `index: "hnsw"` collection keeps answering {:error, :not_supported_by_index} (INTEGRATION.md 3.4 says why).
        if isinstance(index_options, dict) and "staged_searches" in index_options:
            index_options = dict(index_options)
            staged = index_options.pop("staged_searches")
            if not isinstance(staged, bool) or index_mod is not HnswGpu:
                return ("error", "invalid_index_options")
            if staged:
                index_mod = HnswStagedGpu
        # `resident_multi_vector: true` is the collection's own option (not the index module's): every stored
        # embedding's vectors are mirrored into a device-resident store (mv_store.py) that the multi-vector searches read
        resident = False
        if isinstance(index_options, dict) and "resident_multi_vector" in index_options:
            index_options = dict(index_options)
            resident = index_options.pop("resident_multi_vector")
            if not isinstance(resident, bool):
                return ("error", "invalid_index_options")
        # `muvera: {...}` (the collection's own as well, only beside resident_multi_vector: true): the resident documents'
        # fixed-dimensional encodings are kept in a second, inner-product flat handle that muvera_search draws candidates from
        muvera_cfg = None
        if isinstance(index_options, dict) and "muvera" in index_options:
            index_options = dict(index_options)
            given = muvera_mod._keyword(index_options.pop("muvera"))
            if given is None or not resident:
                return ("error", "invalid_index_options")
            normalized = muvera_mod._normalize_config(given, dimensions)   # (defaults: muvera.ex:83-94)
            if isinstance(normalized, str):
                return ("error", "invalid_index_options")
            muvera_cfg = muvera_mod._args(normalized)
        made = index_mod.new(metric, index_options or [])
        if made[0] != "ok":
            return made
        mv_store = None
        if resident:
            device = (index_options or {}).get("device", ((index_options or {}).get("devices") or [nifs.DEVICE])[0])
            try:
                mv_store = ResidentMultiVector(device)
            except RuntimeError as e:
                return ("error", str(e))
        fde_index = None
        if muvera_cfg is not None:
            try:
                fde_index = nifs.flat_new_sharded(nifs.METRIC_CODE["inner_product"], [device])
            except RuntimeError as e:
                return ("error", str(e))
        self = object.__new__(cls)
        self.mv_store = mv_store
        self.muvera_config, self.fde_index = muvera_cfg, fde_index
        self.name, self.dimensions, self.metric = name, dimensions, metric
        self.normalize, self.score = normalize, score
        self.index_mod, self.index_state = index_mod, made[1]
        self.store: Dict[bytes, Embedding] = {}
        self.open = True
        return ("ok", self)

    # -- store (ETS stand-in) ------------------------------------------------
    def get(self, id_):
        emb = self.store.get(nifs._bytes(id_))
        return ("ok", emb) if emb is not None else ("error", "not_found")

    def all(self):
        return ("ok", list(self.store.values()))

    def close(self):
        self.open = False
        return "ok"

    # -- collection.ex:352-357 ----------------------------------------------
    def prepare_query(self, query):
        if not self.open:
            return ("error", "closed")
        ok = _validate_vector(query, self.dimensions)
        if ok != "ok":
            return ok
        return self._normalize(query)

    def _normalize(self, vector):
        if self.normalize == "none":
            return ("ok", [float(x) / 1 for x in vector])
        fn = {"l2": nifs.normalize_l2, "zscore": nifs.normalize_zscore, "minmax": nifs.normalize_minmax}[self.normalize]
        res = fn([float(x) for x in vector])                    # vettore_distance.ex:62-66
        if res[0] != "ok":
            return ("error", "invalid_vector")
        return ("ok", res[1])

    # -- collection.ex:963-991: every vector validated and normalized; anything but a non-empty list is refused
    def _prepare_vectors(self, vectors):
        if not isinstance(vectors, (list, tuple)) or len(vectors) == 0:
            return ("error", "invalid_multi_vector")
        out = []
        for v in vectors:
            ok = _validate_vector(v, self.dimensions)
            if ok != "ok":
                return ok
            n = self._normalize(v)
            if n[0] != "ok":
                return n
            out.append(n[1])
        return ("ok", out)

    # -- collection.ex:921-937, :993-1017 -------------------------------------
    @staticmethod
    def _check_embedding(emb):
        """The checks that come before any vector is looked at: ("ok", Embedding) or the error."""
        if isinstance(emb, dict):
            emb = Embedding(id=emb.get("id"), value=emb.get("value"), vector=emb.get("vector"),
                            metadata=emb.get("metadata"), vectors=emb.get("vectors"))
        if not isinstance(emb, Embedding):
            return ("error", "invalid_embedding")
        if not isinstance(emb.id, (str, bytes)) or len(emb.id) == 0:
            return ("error", "missing_id")
        return ("ok", emb)

    def _prepare_embedding(self, emb):
        checked = self._check_embedding(emb)
        if checked[0] != "ok":
            return checked
        emb = checked[1]
        vectors = None
        if emb.vectors is not None:
            pv = self._prepare_vectors(emb.vectors)
            if pv[0] != "ok":
                return pv
            vectors = pv[1]
        if emb.vector is None and vectors is not None:
            # mean_vector: an f64 sum in order, divided by the count, then the collection's normalization
            acc = [0.0] * self.dimensions
            for v in vectors:
                acc = [a + float(x) for a, x in zip(acc, v)]
            vec = self._normalize([a / len(vectors) for a in acc])
        else:
            ok = _validate_vector(emb.vector, self.dimensions)
            if ok != "ok":
                return ok
            vec = self._normalize(emb.vector)
        if vec[0] != "ok":
            return vec
        bits = nifs.compress_sign_bits(vec[1])                  # collection.ex:926, :941-946
        idb = nifs._bytes(emb.id)
        return ("ok", Embedding(id=idb, value=emb.value if emb.value is not None else idb, vector=vec[1],
                                binary_vector=bits, metadata=emb.metadata, vectors=vectors))

    # -- collection.ex:168-189, :459-479 -------------------------------------
    def put(self, emb):
        p = self._prepare_embedding(emb)
        if p[0] != "ok":
            return p
        e = p[1]
        if e.id in self.store:
            return ("error", "duplicate_id")
        self.store[e.id] = e
        res = self.index_mod.put(self, e)
        if res == "ok":
            res = self._mirror_put([e])
        if res != "ok":
            self._rollback([e])
            return res
        return "ok"

    def put_many(self, embs):
        if not isinstance(embs, list):
            return ("error", "invalid_embeddings")
        # Every embedding is checked in order and the first error is the answer, as in a loop of _prepare_embedding; the
        # ones that carry `vectors` are prepared right there, the plain `vector`s of the batch wait for ONE prepare_rows
        # call (normalization and sign bits of all of them: a checked vector cannot be refused any more).
        prepared, plain = [], []
        for emb in embs:
            checked = self._check_embedding(emb)
            if checked[0] != "ok":
                return checked
            emb = checked[1]
            if emb.vectors is not None:
                p = self._prepare_embedding(emb)
                if p[0] != "ok":
                    return p
                prepared.append(p[1])
                continue
            ok = _validate_vector(emb.vector, self.dimensions)
            if ok != "ok":
                return ok
            plain.append((len(prepared), emb))
            prepared.append(None)
        if plain:
            rows = [[float(x) for x in emb.vector] for _, emb in plain]
            with np.errstate(over="ignore"):
                matrix = np.asarray(rows, dtype=np.float64).astype(np.float32)
            res = nifs.prepare_rows(matrix, self.normalize)
            if res[0] != "ok":
                return ("error", "invalid_vector")
            normalized, words = res[1]
            for k, (at, emb) in enumerate(plain):
                # (normalize: none keeps the caller's numbers as they came, like _normalize)
                vec = [x / 1 for x in rows[k]] if self.normalize == "none" else np.array(normalized[k])
                idb = nifs._bytes(emb.id)
                prepared[at] = Embedding(id=idb, value=emb.value if emb.value is not None else idb, vector=vec,
                                         binary_vector=[int(w) for w in words[k]], metadata=emb.metadata, vectors=None)
        ids = [e.id for e in prepared]
        if len(set(ids)) != len(ids) or any(i in self.store for i in ids):
            return ("error", "duplicate_id")
        for e in prepared:
            self.store[e.id] = e
        res = self.index_mod.put_many(self, prepared)
        if res == "ok":
            res = self._mirror_put(prepared)
        if res != "ok":
            self._rollback(prepared)
            return res
        return "ok"

    def _rollback(self, embs):
        for e in embs:
            self.index_mod.delete(self, e.id)
            if self.mv_store is not None:
                self.mv_store.delete(e.id)
            self.store.pop(e.id, None)
        self._fde_follow([e.id for e in embs])

    def _fde_follow(self, ids):
        """The FDE index follows the resident store for the ids a call touched.  A document whose encoding overflows is
        simply absent from it (the put stands); only a failure of the call itself is an error."""
        if self.fde_index is None or not ids:
            return "ok"
        res = self.mv_store.fde_sync(self.fde_index, ids, self.muvera_config)
        return "ok" if res[0] == "ok" else res

    _MV_ERRORS = {"score overflow": "score_overflow", "dimension mismatch": "dimension_mismatch",
                  "vector contains a non-finite value": "invalid_multi_vector"}

    def _mirror_put(self, embs):
        """The resident store follows the index: the embedding's prepared `vectors`, or its one `vector` (what
        _multi_vector_results hands over per call).  All or nothing, like the index's put_many."""
        if self.mv_store is None:
            return "ok"
        res = self.mv_store.put_many([(e.id, e.vectors if e.vectors else [e.vector]) for e in embs])
        if res != "ok":
            return ("error", self._MV_ERRORS.get(res[1], res[1]))
        return self._fde_follow([e.id for e in embs])

    def delete(self, id_):
        if not isinstance(id_, (str, bytes)):
            return ("error", "invalid_id")
        idb = nifs._bytes(id_)
        res = self.index_mod.delete(self, idb)
        if res == "ok":
            if self.mv_store is not None:
                self.mv_store.delete(idb)
                self._fde_follow([idb])
            self.store.pop(idb, None)
        return res

    # -- collection.ex:224-228 -----------------------------------------------
    def search(self, query, opts=None):
        opts = {} if opts is None else opts
        if not isinstance(opts, dict):
            return ("error", "invalid_options")
        bad = [k for k in opts if k != "limit"]
        if bad:
            return ("error", ("unsupported_option", bad[0]))
        return self.index_mod.search(self, query, opts)

    # -- collection.ex:234-345: funnel_search / quantized_search / hybrid_search --------------------
    # The reference checks the option keys (validate_options, collection.ex:237, :267, :330) and then runs its own
    # ETS + CPU-NIF composition whatever the index module is.  With the dispatch INTEGRATION.md section 3 adds to
    # collection.ex -- `if function_exported?(collection.index_mod, :quantized_search, 3), do: ...` -- an index module
    # that keeps the corpus resident answers instead.  This mirror has no ETS composition of its own (the store is out
    # of scope): an index module without the function is {:error, :not_supported_by_index} here.
    def _staged(self, name, allowed, query, opts):
        opts = {} if opts is None else opts
        if not isinstance(opts, dict):
            return ("error", "invalid_options")                         # collection.ex:1133
        bad = [k for k in opts if k not in allowed]
        if bad:
            return ("error", ("unsupported_option", bad[0]))            # collection.ex:1125-1126
        fn = getattr(self.index_mod, name, None)
        if fn is None:
            return ("error", "not_supported_by_index")
        return fn(self, query, opts)

    def funnel_search(self, query, opts=None):
        return self._staged("funnel_search", ("limit", "candidates", "stages", "dimensions"), query, opts)   # :56

    def quantized_search(self, query, opts=None):
        return self._staged("quantized_search", ("limit", "candidates"), query, opts)                        # :57

    def hybrid_search(self, query, opts=None):
        return self._staged("hybrid_search", ("limit", "generators", "rerank"), query, opts)                 # :59

    # -- collection.ex:298-323 ------------------------------------------------
    def multi_vector_search(self, query_vectors, opts=None):
        """MaxSim over every stored embedding (its `vectors`, or its one `vector`): Results carry the score."""
        parsed = self._multi_vector_options(opts)
        if parsed[0] != "ok":
            return parsed
        _, metric, limit = parsed
        qv = self._prepare_vectors(query_vectors)
        if qv[0] != "ok":
            return qv
        if self.mv_store is not None:
            return self._resident_results(qv[1], None, metric, limit)
        return self._multi_vector_results(qv[1], list(self.store.values()), metric, limit)

    def _multi_vector_options(self, opts):
        """("ok", metric, limit) of multi_vector_search's options, or the error every search with them returns."""
        opts = {} if opts is None else opts
        if not isinstance(opts, dict):
            return ("error", "invalid_options")
        bad = [k for k in opts if k not in ("limit", "metric")]
        if bad:
            return ("error", ("unsupported_option", bad[0]))
        limit = opts.get("limit", 10)
        if not (isinstance(limit, int) and not isinstance(limit, bool) and 0 < limit <= MAX_NIF_USIZE):
            return ("error", "invalid_limit")
        metric = METRIC_ALIASES.get(opts.get("metric", self.metric), opts.get("metric", self.metric))
        if metric not in METRICS:
            return ("error", "invalid_metric")
        return ("ok", metric, limit)

    def multi_vector_search_batch(self, query_vector_lists, opts=None):
        """multi_vector_search for every entry of a list of query-vector lists (an extension of the adapter): a list,
        element-wise equal to calling multi_vector_search per entry.  With a resident store the valid entries are one
        batched call on it; without one, a loop."""
        if not isinstance(query_vector_lists, (list, tuple)):
            return ("error", "invalid_multi_vector")
        parsed = self._multi_vector_options(opts)
        if self.mv_store is None or parsed[0] != "ok":
            return [self.multi_vector_search(q, opts) for q in query_vector_lists]
        _, metric, limit = parsed
        out = [self._prepare_vectors(q) for q in query_vector_lists]
        valid = [i for i, qv in enumerate(out) if qv[0] == "ok"]
        res = self.mv_store.top_k_batch([out[i][1] for i in valid], nifs.METRIC_CODE[metric], limit)
        if not isinstance(res, list):   # the call itself failed: every entry's answer
            res = [res] * len(valid)
        for i, r in zip(valid, res):
            out[i] = self._resident_answer(r, metric)
        return out

    # -- the reference's MUVERA flow (README: encode, search the encodings by inner product, rerank with MaxSim) over
    # the resident store and its FDE index
    def _muvera_options(self, opts):
        """("ok", metric, limit, candidates), or the error every search with these options returns."""
        opts = {} if opts is None else opts
        if not isinstance(opts, dict):
            return ("error", "invalid_options")
        bad = [k for k in opts if k not in ("limit", "candidates", "metric")]
        if bad:
            return ("error", ("unsupported_option", bad[0]))
        parsed = self._multi_vector_options({k: v for k, v in opts.items() if k != "candidates"})
        if parsed[0] != "ok":
            return parsed
        _, metric, limit = parsed
        candidates = opts.get("candidates", max(limit * 10, limit))      # candidate_count, collection.ex:510
        if not (isinstance(candidates, int) and not isinstance(candidates, bool) and limit <= candidates <= MAX_NIF_USIZE):
            return ("error", "invalid_candidates")                          # collection.ex:889-895
        return ("ok", metric, limit, candidates)

    def muvera_search(self, query_vectors, opts=None):
        """multi_vector_search over the `candidates` stored embeddings whose encodings score highest against the
        query's: Results carry the exact MaxSim score."""
        if self.fde_index is None:
            return ("error", "muvera_not_configured")
        parsed = self._muvera_options(opts)
        if parsed[0] != "ok":
            return parsed
        _, metric, limit, candidates = parsed
        qv = self._prepare_vectors(query_vectors)
        if qv[0] != "ok":
            return qv
        res = self.mv_store.fde_top_k(self.fde_index, self.muvera_config, qv[1], candidates, nifs.METRIC_CODE[metric], limit)
        return self._resident_answer(res, metric)

    def muvera_search_batch(self, query_vector_lists, opts=None):
        """muvera_search for every entry of a list of query-vector lists: element-wise what muvera_search returns, the
        valid entries in one batched call."""
        if self.fde_index is None:
            return ("error", "muvera_not_configured")
        if not isinstance(query_vector_lists, (list, tuple)):
            return ("error", "invalid_multi_vector")
        parsed = self._muvera_options(opts)
        if parsed[0] != "ok":
            return [parsed for _ in query_vector_lists]
        _, metric, limit, candidates = parsed
        out = [self._prepare_vectors(q) for q in query_vector_lists]
        valid = [i for i, qv in enumerate(out) if qv[0] == "ok"]
        res = self.mv_store.fde_top_k_batch(self.fde_index, self.muvera_config, [out[i][1] for i in valid], candidates,
                                            nifs.METRIC_CODE[metric], limit)
        if not isinstance(res, list):   # the call itself failed: every entry's answer
            res = [res] * len(valid)
        for i, r in zip(valid, res):
            out[i] = self._resident_answer(r, metric)
        return out

    # -- collection.ex:742-806: the documents, one native call, errors as atoms, Results with score only
    def _multi_vector_results(self, query_vectors, embeddings, metric, limit):
        documents = []
        for e in embeddings:
            vectors = e.vectors if e.vectors else [e.vector]
            for v in vectors:
                ok = _validate_vector(v, self.dimensions)
                if ok != "ok":
                    return ok
            documents.append((e.id, vectors))
        res = nifs.multi_vector_top_k(documents, query_vectors, nifs.METRIC_CODE[metric], limit)
        if res[0] != "ok":
            return ("error", self._MV_ERRORS.get(res[1], res[1]))
        by_id = {e.id: e for e in embeddings}
        return ("ok", [Result(id=i, value=by_id[i].value, score=float(score), distance=None, metric=metric,
                              metadata=by_id[i].metadata) for i, score in res[1] if i in by_id])

    def _resident_results(self, query_vectors, ids, metric, limit):
        """_multi_vector_results from the resident store: over every stored embedding (ids None) or the listed ones."""
        code = nifs.METRIC_CODE[metric]
        if ids is None:
            res = self.mv_store.top_k(query_vectors, code, limit)
        else:
            res = self.mv_store.top_k_ids(ids, query_vectors, code, limit)
        return self._resident_answer(res, metric)

    def _resident_answer(self, res, metric):
        if res[0] != "ok":
            return ("error", self._MV_ERRORS.get(res[1], res[1]))
        return ("ok", [Result(id=i, value=self.store[i].value, score=float(score), distance=None, metric=metric,
                              metadata=self.store[i].metadata) for i, score in res[1] if i in self.store])

    # -- lib/vettore.ex:622-640: rerank/4 -> Vettore.Distance.mmr_rerank/5 --------------------------
    def rerank(self, initial, opts=None):
        """MMR over `initial` = [(id, score)] under the collection's metric: ("ok", the chosen entries in order of
        choice).  Options: limit (10), alpha (0.5).  A FlatGpu index reads the rows where they are resident; any other
        index module goes through the stateless call with the vectors of the initial entries from the store (the
        reference hands mmr_rerank/5 the whole table; the stored vectors it would validate are valid by construction)."""
        opts = {} if opts is None else opts
        if not isinstance(initial, list) or not isinstance(opts, dict):
            return ("error", "invalid_arguments")                          # vettore.ex:642
        if any(k not in ("limit", "alpha") for k in opts):
            return ("error", "invalid_options")                            # vettore.ex:628, :638
        limit, alpha = opts.get("limit", 10), opts.get("alpha", 0.5)
        fn = getattr(self.index_mod, "rerank", None)
        if fn is not None:
            res = fn(self, initial, alpha, limit)
            if res is not None:
                return res
        conv, pairs, seen = [], [], set()
        for entry in initial:
            if isinstance(entry, tuple) and len(entry) == 2 and isinstance(entry[0], (str, bytes)):
                idb = nifs._bytes(entry[0])
                conv.append((idb, entry[1]))
                if idb in self.store and idb not in seen:
                    seen.add(idb)
                    pairs.append((idb, [float(x) for x in self.store[idb].vector]))
            else:
                conv.append(entry)
        res = nifs.mmr_rerank(conv, pairs, self.metric, alpha, limit)
        if res[0] != "ok":
            return res
        place = {id(e): i for i, e in enumerate(conv)}
        return ("ok", [initial[place[id(e)]] for e in res[1]])

    def _mmr_composed(self, query, opts):
        """mmr_search as its definition: search(limit: candidates), then rerank over the results' (id, score)."""
        lc = FlatGpu._mmr_options(opts)
        if lc[0] != "ok":
            return lc
        found = self.search(query, {"limit": lc[2]})
        if found[0] != "ok":
            return found
        res = self.rerank([(r.id, r.score) for r in found[1]], {"limit": lc[1], "alpha": lc[3]})
        if res[0] != "ok":
            return res
        by_id = {r.id: r for r in found[1]}
        return ("ok", [by_id[i] for i, _ in res[1]])

    def mmr_search(self, query, opts=None):
        """Diversified search (an extension of the adapter): Results in MMR order, equal to search(limit: candidates)
        followed by rerank(limit: limit, alpha: alpha).  Options: limit (10), candidates (max(limit * 10, limit)), alpha (0.5)."""
        opts = {} if opts is None else opts
        if not isinstance(opts, dict):
            return ("error", "invalid_options")
        bad = [k for k in opts if k not in ("limit", "candidates", "alpha")]
        if bad:
            return ("error", ("unsupported_option", bad[0]))
        fn = getattr(self.index_mod, "mmr_search", None)
        if fn is not None:
            res = fn(self, query, opts)
            if res is not None:
                return res
        return self._mmr_composed(query, opts)

    def mmr_search_batch(self, queries, opts=None):
        """mmr_search for a list of queries: ("ok", [("ok", [Result]) | ("error", reason) per query]); with a FlatGpu
        index all of them are one call and one chain of step launches."""
        opts = {} if opts is None else opts
        if not isinstance(opts, dict):
            return ("error", "invalid_options")
        bad = [k for k in opts if k not in ("limit", "candidates", "alpha")]
        if bad:
            return ("error", ("unsupported_option", bad[0]))
        fn = getattr(self.index_mod, "mmr_search_batch", None)
        if fn is not None:
            res = fn(self, queries, opts)
            if res is not None:
                return res
        lc = FlatGpu._mmr_options(opts)
        if lc[0] != "ok":
            return lc
        return ("ok", [self._mmr_composed(q, opts) for q in queries])

    # (extensions of the adapter: lists of queries, one call)
    def search_batch(self, queries, opts=None):
        return self._staged("search_batch", ("limit",), queries, opts)

    def quantized_search_batch(self, queries, opts=None):
        return self._staged("quantized_search_batch", ("limit", "candidates"), queries, opts)

    def funnel_search_batch(self, queries, opts=None):
        return self._staged("funnel_search_batch", ("limit", "candidates", "stages", "dimensions"), queries, opts)
