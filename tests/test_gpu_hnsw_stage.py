"""quantized_search, funnel_search and hybrid_search on the HNSW index (vt_flat_quantized_search, vt_flat_funnel_search and
vt_flat_hybrid_search handed an HNSW handle; K15: vt_hnsw_stage.hip) -- `-m gpu`.  Every corpus goes into an HNSW handle and, the same
(id, vector) pairs, into a flat handle: hits and statuses are the flat handle's, ids, order and the f32 bits of every raw
value (that path is held to the oracle by tests/test_gpu_parity.py).  The hybrid search's SEARCH generator is composed
from the oracle's pieces with tests/hnsw_ref.py's traversal.  No tolerance anywhere."""
import numpy as np
import pytest

from hnsw_ref import COSINE, INNER_PRODUCT, L2, HnswIndex
from test_gpu_hnsw import assert_same_graph, new_gpu, params, ref_order  # noqa: F401  (ref_order: a fixture)
from test_gpu_parity import nifs  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

METRICS = [L2, COSINE, INNER_PRODUCT]
NAMES = ["600x16", "300x65", "200x100", "150x768", "300x3"]


def bits(hits):
    return [(h[0], np.float32(h[1]).tobytes()) for h in hits]


def same(res):
    return ("ok", bits(res[1])) if res[0] == "ok" else res


def corpus(name):
    rng = np.random.default_rng(sum(name.encode()) + 1)
    ids = lambda n: [b"k%d" % ((i * 7919) % 100003) for i in range(n)]  # byte order differs from insertion order
    if name == "600x16":  # blocks of 25 identical rows under different ids
        v = rng.standard_normal((600, 16)).astype(np.float32)
        for b in (100, 300, 575):
            v[b:b + 25] = v[b]
        return ids(600), v, params(4, 8, 40)
    if name == "300x65":  # two sign patterns: hundreds of rows tie at the k-th Hamming distance
        pat = np.where(rng.random((2, 65)) < 0.5, -1.0, 1.0).astype(np.float32)
        v = pat[rng.integers(0, 2, 300)] * rng.uniform(0.5, 2.0, (300, 65)).astype(np.float32)
        return ids(300), v, params(4, 8, 30)
    if name == "200x100":
        return ids(200), rng.standard_normal((200, 100)).astype(np.float32), params(4, 8, 30)
    if name == "150x768":
        return ids(150), rng.standard_normal((150, 768)).astype(np.float32), params(4, 8, 30)
    if name == "300x3":  # the reference's sin / cos corpus
        v = np.array([[np.sin(np.float32(i)), np.cos(np.float32(i)), np.float32(i) / np.float32(300.0)] for i in range(300)], np.float32)
        return [b"node-%03d" % i for i in range(300)], v, params(4, 8, 40)
    raise KeyError(name)


class Pair:
    """The same (id, vector) pairs in an HNSW handle, a flat handle and -- for the traversal -- the restatement."""

    def __init__(self, nifs, metric, p, order):
        self.nifs, self.metric = nifs, metric
        self.hnsw = new_gpu(nifs, metric, p)
        self.flat = nifs._flat_new(metric)
        nifs.flat_set_reduce_order(self.flat, order)
        self.ref = HnswIndex(metric, **p)
        self.rows = {}

    def insert_many(self, items):
        assert self.nifs.hnsw_insert_many(self.hnsw, items) == ("ok", ())
        assert self.nifs.flat_insert_many(self.flat, items) in ("ok", ("ok", ()))
        self.ref.insert_many(items)
        for i, v in items:
            self.rows.pop(i, None)  # (an upsert moves the id to the end, as a dict rebuilt in insertion order would)
            self.rows[i] = np.asarray(v, np.float32)

    def delete(self, id_):
        assert self.nifs.hnsw_delete(self.hnsw, id_) == ("ok", ())
        assert self.nifs.flat_delete(self.flat, id_) in ("ok", ("ok", ()))
        self.ref.delete(id_)
        self.rows.pop(id_, None)


def queries_for(vecs, rng, count=2):
    d = vecs.shape[1]
    out = [rng.standard_normal(d).astype(np.float32) for _ in range(count - 1)]
    return out + [vecs[len(vecs) // 2].copy()]


def stage_sets(d):
    return [s for s in ([d], [max(d // 4, 1), max(d // 2, 1)], [3, 5, d]) if all(1 <= x <= d for x in s)]


def assert_staged_equal(nifs, pair, d, rng, vecs, full=True):
    """quantized, funnel and hybrid (funnel / quantized generators): the flat handle's hits and statuses"""
    n = len(pair.rows)
    for q in queries_for(vecs, rng):
        for limit in ((1, 10, 256) if full else (10,)):
            for cand in ((10, 256, 257, 300, n + 50) if full else (10, 300)):
                got = nifs.hnsw_quantized_search(pair.hnsw, q, cand, limit)
                assert same(got) == same(nifs.flat_quantized_search(pair.flat, q, cand, limit)), ("quantized", cand, limit)
                for st in stage_sets(d):
                    got = nifs.hnsw_funnel_search(pair.hnsw, q, st, cand, limit)
                    assert same(got) == same(nifs.flat_funnel_search(pair.flat, q, st, cand, limit)), ("funnel", st, cand, limit)
            gens = [(nifs.GEN_FUNNEL, 60, stage_sets(d)[-1]), (nifs.GEN_QUANTIZED, 80, []), (nifs.GEN_QUANTIZED, 80, []),
                    (nifs.GEN_FUNNEL, 300, [d])]
            got = nifs.hnsw_hybrid_search(pair.hnsw, q, gens, limit)
            assert same(got) == same(nifs.flat_hybrid_search(pair.flat, q, gens, limit)), ("hybrid", limit)


def assert_hybrid_with_search(nifs, oracle_mod, pair, d, rng, vecs):
    """hybrid_search with the SEARCH generator: the composition of test_hybrid_generator_mixes_match_oracle_composition,
    hnsw_ref's traversal with limit = candidates as that generator's ids"""
    rows = list(pair.rows.items())
    by_id = pair.rows
    obits = [(i, oracle_mod.compress_sign_bits(v)) for i, v in rows]
    metric = pair.metric
    mixes = [
        [(nifs.GEN_SEARCH, 30, [])],
        [(nifs.GEN_FUNNEL, 60, [max(d // 2, 1)]), (nifs.GEN_QUANTIZED, 80, []), (nifs.GEN_SEARCH, 30, [])],
        [(nifs.GEN_SEARCH, 40, []), (nifs.GEN_SEARCH, 40, [])],
        [(nifs.GEN_SEARCH, 300, []), (nifs.GEN_QUANTIZED, 300, [])],
    ]
    for q in queries_for(vecs, rng):
        for gens in mixes:
            for limit in (1, 10, 256):
                union = []
                for kind, cand, stages in gens:
                    if kind == nifs.GEN_FUNNEL:
                        cur = rows
                        for st in stages:
                            cur = [(i, by_id[i]) for i, _ in oracle_mod.vector_top_k(cur, q, metric, st, cand)]
                        union += [i for i, _ in cur]
                    elif kind == nifs.GEN_QUANTIZED:
                        union += [i for i, _ in oracle_mod.binary_top_k(obits, oracle_mod.compress_sign_bits(q), d, cand)]
                    else:
                        union += [i for i, _ in pair.ref.search(q, cand)]
                uniq = list(dict.fromkeys(union))
                want = oracle_mod.vector_top_k([(i, by_id[i]) for i in uniq], q, metric, d, limit)
                got = nifs.hnsw_hybrid_search(pair.hnsw, q, gens, limit)
                assert got[0] == "ok" and bits(got[1]) == bits(want), (gens, limit)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", NAMES)
def test_staged_searches_are_the_flat_handles(nifs, oracle_mod, ref_order, name, metric):
    ids, vecs, p = corpus(name)
    d = vecs.shape[1]
    pair = Pair(nifs, metric, p, ref_order)
    pair.insert_many(list(zip(ids, vecs)))
    rng = np.random.default_rng(5)
    assert_staged_equal(nifs, pair, d, rng, vecs, full=name in ("600x16", "300x65"))
    assert_hybrid_with_search(nifs, oracle_mod, pair, d, rng, vecs)


@pytest.mark.parametrize("metric", METRICS)
def test_validation_and_empty_answers_are_the_flat_handles(nifs, ref_order, metric):
    ids, vecs, p = corpus("200x100")
    d = 100
    pair = Pair(nifs, metric, p, ref_order)
    q = vecs[3]
    # an empty handle
    assert nifs.hnsw_quantized_search(pair.hnsw, q, 10, 5) == nifs.flat_quantized_search(pair.flat, q, 10, 5) == ("ok", [])
    assert nifs.hnsw_funnel_search(pair.hnsw, q, [8], 10, 5) == nifs.flat_funnel_search(pair.flat, q, [8], 10, 5) == ("ok", [])
    gens = [(nifs.GEN_SEARCH, 10, []), (nifs.GEN_QUANTIZED, 10, [])]
    assert nifs.hnsw_hybrid_search(pair.hnsw, q, gens, 5) == nifs.flat_hybrid_search(pair.flat, q, gens, 5) == ("ok", [])
    pair.insert_many(list(zip(ids, vecs)))
    nan_q = q.copy()
    nan_q[5] = np.nan
    for query in (q[:50], nan_q, q):
        for cand, limit in ((10, 5), (10, 0), (0, 5)):
            assert same(nifs.hnsw_quantized_search(pair.hnsw, query, cand, limit)) == same(nifs.flat_quantized_search(pair.flat, query, cand, limit))
            for st in ([8], [0], [d + 1], [8, d + 1], []):
                assert (same(nifs.hnsw_funnel_search(pair.hnsw, query, st, cand, limit)) ==
                        same(nifs.flat_funnel_search(pair.flat, query, st, cand, limit))), (len(query), st, cand, limit)
        for gens in ([(nifs.GEN_FUNNEL, 10, [0])], [(nifs.GEN_FUNNEL, 10, [d + 1])], [(nifs.GEN_FUNNEL, 10, [])],
                     [(nifs.GEN_QUANTIZED, 0, [])], [], [(nifs.GEN_QUANTIZED, 10, [])]):
            for limit in (5, 0):
                assert (same(nifs.hnsw_hybrid_search(pair.hnsw, query, gens, limit)) ==
                        same(nifs.flat_hybrid_search(pair.flat, query, gens, limit))), (len(query), gens, limit)
    assert nifs.hnsw_funnel_search(pair.hnsw, q, [d + 1], 10, 5) == ("error", "invalid prefix dimensions")
    assert nifs.hnsw_quantized_search(pair.hnsw, q[:50], 10, 5) == ("error", "dimension mismatch")


@pytest.mark.parametrize("metric", METRICS)
def test_dead_rows_upserts_and_a_compaction(nifs, oracle_mod, ref_order, metric):
    ids, vecs, p = corpus("600x16")
    ids, vecs = ids[:300], vecs[:300]
    pair = Pair(nifs, metric, p, ref_order)
    pair.insert_many(list(zip(ids, vecs)))
    rng = np.random.default_rng(8)
    assert_staged_equal(nifs, pair, 16, rng, vecs, full=False)   # (the rank column is built here ...)
    gone = [ids[0], ids[299]] + [ids[i] for i in range(5, 269, 3)]
    assert len(gone) == 90
    for i in gone:
        pair.delete(i)
    fresh = rng.standard_normal((60, 16)).astype(np.float32)
    pair.insert_many([(ids[3 * (i + 1)], fresh[i]) for i in range(60)])   # upserts: the old rows die, new ones are appended
    assert nifs.hnsw_memory(pair.hnsw)["dead_rows"] == 150
    assert_staged_equal(nifs, pair, 16, rng, vecs, full=False)   # (... and again here, behind the changes)
    assert_hybrid_with_search(nifs, oracle_mod, pair, 16, rng, vecs)
    # delete until the dead rows outnumber the live ones, then one insert compacts
    live = list(pair.rows)
    while nifs.hnsw_memory(pair.hnsw)["dead_rows"] <= len(pair.rows):
        pair.delete(live.pop())
    mem = nifs.hnsw_memory(pair.hnsw)
    assert mem["dead_rows"] > len(pair.rows) and mem["dead_rows"] >= 64
    pair.insert_many([(b"after", vecs[7])])
    assert nifs.hnsw_memory(pair.hnsw)["dead_rows"] == 0
    assert_staged_equal(nifs, pair, 16, rng, vecs, full=False)
    assert_hybrid_with_search(nifs, oracle_mod, pair, 16, rng, vecs)
    assert_same_graph(nifs, pair.hnsw, pair.ref)


def test_overflow_in_any_stage_is_reported(nifs, ref_order):
    """as test_funnel_overflow_in_any_stage_is_reported does for the flat handle"""
    n, d = 300, 16
    rng = np.random.default_rng(77)
    x = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    ids = [b"r%03d" % i for i in range(n)]
    q = np.full(d, 2.0, np.float32)
    early, late = x.copy(), x.copy()
    early[7, :] = 2e19                 # (0 - 2e19)^2 overflows f32 already on the 8-wide prefix; in f64 the distance is finite
    late[9, 8:] = 2e19                 # ... only in the full-width rerank
    for m in (early, late):
        pair = Pair(nifs, L2, params(4, 8, 30), ref_order)
        pair.insert_many(list(zip(ids, m)))
        for cand in (50, 300):
            # the f32 chain overflows, the f64 recovery is finite: the flat handle's hits, the far rows last
            for limit in (5, 300):
                got = nifs.hnsw_funnel_search(pair.hnsw, q, [8], cand, limit)
                assert got[0] == "ok" and same(got) == same(nifs.flat_funnel_search(pair.flat, q, [8], cand, limit))
                got = nifs.hnsw_quantized_search(pair.hnsw, q, cand, limit)
                assert got[0] == "ok" and same(got) == same(nifs.flat_quantized_search(pair.flat, q, cand, limit))
    # a recovery that is not finite: an inner-product handle whose rows, each finite, overflow against the query
    big = x.copy()
    big[9, :8] = 100.0
    big[9, 8:] = 1e30
    pair = Pair(nifs, INNER_PRODUCT, params(4, 8, 30), ref_order)
    pair.insert_many(list(zip(ids, big)))
    huge = np.full(d, 3e38, np.float32)
    for cand in (50, 300):
        assert nifs.flat_funnel_search(pair.flat, huge, [8], cand, 5) == ("error", "metric overflow")
        assert nifs.hnsw_funnel_search(pair.hnsw, huge, [8], cand, 5) == ("error", "metric overflow")
        assert nifs.hnsw_quantized_search(pair.hnsw, huge, cand, 5) == nifs.flat_quantized_search(pair.flat, huge, cand, 5)
        gens = [(nifs.GEN_QUANTIZED, cand, [])]
        assert nifs.hnsw_hybrid_search(pair.hnsw, huge, gens, 5) == nifs.flat_hybrid_search(pair.flat, huge, gens, 5)
    # the flag does not leak into the next call
    assert nifs.hnsw_funnel_search(pair.hnsw, np.zeros(d, np.float32), [8], 50, 5)[0] == "ok"


@pytest.mark.parametrize("metric", ["l2", "cosine", "inner_product"])
def test_collection_with_staged_searches(nifs, ref_order, metric):
    from vettore_amd.collection import Collection, Embedding
    from vettore_amd.index_hnsw import HnswStagedGpu
    rng = np.random.default_rng(41)
    vecs = rng.standard_normal((150, 12)).astype(np.float32)
    embs = [Embedding(id=b"c%03d" % ((i * 37) % 150), vector=[float(x) for x in vecs[i]], value=i) for i in range(150)]
    q = [float(x) for x in vecs[11]]
    for score in ("raw", "similarity"):
        made = Collection.new(dimensions=12, metric=metric, index="hnsw", score=score,
                              index_options={"staged_searches": True, "m": 4, "m0": 8, "ef_construction": 30})
        assert made[0] == "ok", made
        col = made[1]
        assert col.index_mod is HnswStagedGpu
        flat = Collection.new(dimensions=12, metric=metric, index="flat", score=score)[1]
        nifs.flat_set_reduce_order(flat.index_state, ref_order)
        for c in (col, flat):
            assert c.put_many(embs) == "ok"
            assert c.delete(embs[10].id) == "ok"
        for opts in ({}, {"limit": 7}, {"limit": 7, "candidates": 20}, {"limit": 0}, {"limit": 7, "candidates": 3}, {"k": 3}):
            assert col.quantized_search(q, opts) == flat.quantized_search(q, opts), opts
        for opts in ({}, {"limit": 7, "stages": [3, 6]}, {"dimensions": 4}, {"stages": [13]}, {"stages": []}, {"limit": 7, "candidates": 2}):
            assert col.funnel_search(q, opts) == flat.funnel_search(q, opts), opts
        for opts in ({"generators": ["funnel", "quantized"]}, {"limit": 5, "generators": [("funnel", {"stages": [4, 8], "candidates": 30}), "quantized"]},
                     {"generators": []}, {"generators": ["nope"]}, {"generators": [("quantized", {"stages": [3]})]}, {"limit": 0},
                     {"generators": ["quantized"], "rerank": "nope"}):
            assert col.hybrid_search(q, opts) == flat.hybrid_search(q, opts), opts
        assert col.quantized_search(q[:5], {}) == flat.quantized_search(q[:5], {})
        # the default generators are ["hnsw", "quantized"]; "hnsw" and "search" are both the index's own traversal
        default = col.hybrid_search(q, {"limit": 6})
        assert default[0] == "ok" and len(default[1]) == 6
        assert default == col.hybrid_search(q, {"limit": 6, "generators": ["hnsw", "quantized"]})
        assert default == col.hybrid_search(q, {"limit": 6, "generators": ["search", "quantized"]})
        assert col.hybrid_search(q, {"generators": [("hnsw", {"candidates": 20})]})[0] == "ok"
        assert flat.hybrid_search(q, {"generators": ["hnsw"]}) == ("error", "hnsw_index_required")
        # the plain search is untouched
        assert col.search(q, {"limit": 4})[0] == "ok"


def test_the_collections_option(nifs):
    from vettore_amd.collection import Collection
    from vettore_amd.index_hnsw import HnswGpu
    plain = Collection.new(dimensions=8, metric="l2", index="hnsw", index_options={"m": 4, "m0": 8, "ef_construction": 30})[1]
    assert plain.index_mod is HnswGpu
    assert plain.quantized_search([1.0] * 8, {"limit": 3}) == ("error", "not_supported_by_index")
    off = Collection.new(dimensions=8, metric="l2", index="hnsw_gpu", index_options={"staged_searches": False})[1]
    assert off.index_mod is HnswGpu and off.hybrid_search([1.0] * 8, {}) == ("error", "not_supported_by_index")
    assert Collection.new(dimensions=8, metric="l2", index="flat", index_options={"staged_searches": True}) == ("error", "invalid_index_options")
    for bad in (1, "yes", None):
        assert Collection.new(dimensions=8, metric="l2", index="hnsw", index_options={"staged_searches": bad}) == ("error", "invalid_index_options")
