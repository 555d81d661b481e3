"""The resident multi-vector store on the device (vt_mv_*, K9r: vt_maxsim_resident.hip) -- `-m gpu`.  After any puts and
deletes a search returns what the reference's top_k (tests/maxsim_ref.py, built from the CPU oracle's distances) returns
for the live documents in the order of their last put, and what the stateless multi_vector_top_k returns for them:
the same ids in the same order with the same float32 bits -- tolerance zero everywhere."""
import numpy as np
import pytest

import maxsim_ref
from test_gpu_parity import nifs  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

TOKENS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 130)   # around K9r's tiles of 16, 32 and 64 rows, and several tiles
DIMS = (1, 7, 8, 13, 64, 100, 128)                # pad, tail only, whole chunks, both
QUERY_COUNTS = (0, 1, 7, 8, 9, 33)                # one lane group, its edge, two groups, four groups and a second pass


def f32bits(x):
    return np.float32(x).tobytes()


@pytest.fixture
def ref_order(nifs, oracle_mod):
    """The oracle folds a chunk in the lane order the library uses."""
    order = nifs.debug_get("reduce_order")
    oracle_mod.set_reduce_order(order)
    yield order
    oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


def vectors(rng, n, d, metric):
    v = rng.uniform(-1, 1, size=(n, d)).astype(np.float32)
    if metric in (7, 8):  # float hamming / jaccard count non-zeros: zeros must occur
        v[rng.uniform(size=v.shape) < 0.35] = 0.0
    if metric == 2 and n > 2:
        v[1] = 0.0  # a zero norm scores 0.0
    return [list(map(float, r)) for r in v]


def documents(rng, d, metric, tokens=TOKENS):
    return [("doc-%d" % i, vectors(rng, t, d, metric)) for i, t in enumerate(tokens)]


def store_of(docs):
    from vettore_amd.mv_store import ResidentMultiVector
    store = ResidentMultiVector()
    assert store.put_many(docs) == "ok"
    return store


def check(nifs, got, docs, query, metric, limit, ctx):
    """`got` against the reference and against the stateless call over `docs` (the live documents in store order)."""
    want = maxsim_ref.top_k(docs, query, metric, limit)
    assert got[0] == "ok", (ctx, got)
    assert [h[0] for h in got[1]] == [h[0] for h in want], ctx
    assert [f32bits(h[1]) for h in got[1]] == [f32bits(h[1]) for h in want], ctx
    assert nifs.multi_vector_top_k(docs, query, metric, limit) == got, ctx


@pytest.mark.parametrize("metric", range(9))
def test_every_metric_over_every_token_count(nifs, ref_order, metric):
    rng = np.random.default_rng(900 + metric)
    docs = documents(rng, 13, metric)
    store = store_of(docs)
    assert len(store) == len(docs) and store.dimension == 13
    query = vectors(rng, 9, 13, metric)
    query[0] = docs[4][1][0]  # an exact match somewhere
    for limit in (len(docs) + 3, 4):
        check(nifs, store.top_k(query, metric, limit), docs, query, metric, limit, (metric, limit))


@pytest.mark.parametrize("metric", [3, 0, 2])
def test_dimensions(nifs, ref_order, metric):
    rng = np.random.default_rng(910 + metric)
    for d in DIMS:
        docs = documents(rng, d, metric)
        store = store_of(docs)
        query = vectors(rng, 9, d, metric)
        check(nifs, store.top_k(query, metric, len(docs)), docs, query, metric, len(docs), (metric, d))
    # a dimension whose tiles do not fit in LDS: K9 over the same slab
    docs = documents(rng, 772, metric, (0, 1, 33))
    store = store_of(docs)
    query = vectors(rng, 3, 772, metric)
    check(nifs, store.top_k(query, metric, 3), docs, query, metric, 3, (metric, 772))


@pytest.mark.parametrize("metric", [3, 0, 2])
def test_query_counts(nifs, ref_order, metric):
    rng = np.random.default_rng(920 + metric)
    docs = documents(rng, 13, metric)
    store = store_of(docs)
    for nq in QUERY_COUNTS:
        query = vectors(rng, nq, 13, metric)
        check(nifs, store.top_k(query, metric, len(docs)), docs, query, metric, len(docs), (metric, nq))
    # d = 256 leaves LDS for 32 query vectors beside the tiles: 33 go in two panels, the sums waiting in between
    docs = documents(rng, 256, metric, (0, 1, 17, 33))
    store = store_of(docs)
    query = vectors(rng, 33, 256, metric)
    check(nifs, store.top_k(query, metric, 4), docs, query, metric, 4, (metric, "two panels"))


def test_the_four_lane_orders(nifs, oracle_mod, vt_debug):
    rng = np.random.default_rng(930)
    docs = documents(rng, 13, 3)
    store = store_of(docs)
    query = vectors(rng, 9, 13, 3)
    try:
        for order in (0, 1, 2, 3):
            vt_debug.set("reduce_order", order)
            oracle_mod.set_reduce_order(order)
            for metric in (3, 5):
                check(nifs, store.top_k(query, metric, len(docs)), docs, query, metric, len(docs), (order, metric))
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


def test_ties_come_back_in_id_byte_order(nifs, ref_order):
    rng = np.random.default_rng(940)
    same = vectors(rng, 5, 8, 3)
    docs = [(i, same) for i in ("b", "a", "ab", "", "a\x00", "B")] + [("other", vectors(rng, 3, 8, 3))]
    store = store_of(docs)
    query = vectors(rng, 4, 8, 3)
    got = store.top_k(query, 3, len(docs) + 10)
    check(nifs, got, docs, query, 3, len(docs) + 10, "ties")
    tied = [h[0] for h in got[1] if h[0] != b"other"]
    assert tied == sorted(tied) and len(tied) == 6
    assert store.top_k(query, 3, 0) == ("ok", [])


def test_mutations_growth_and_compaction(nifs, ref_order):
    rng = np.random.default_rng(950)
    metric, d = 3, 8
    query = vectors(rng, 2, d, metric)
    live = {}                                  # id -> vectors, in the order of the last put

    def put(store, docs):
        assert store.put_many(docs) == "ok"
        for i, v in docs:
            live.pop(i, None)
            live[i] = v

    def same(store, ctx):
        docs = list(live.items())
        assert len(store) == len(docs)
        check(nifs, store.top_k(query, metric, len(docs) + 1), docs, query, metric, len(docs) + 1, ctx)

    from vettore_amd.mv_store import ResidentMultiVector
    store = ResidentMultiVector()
    assert store.dimension is None and store.top_k(query, metric, 3) == ("ok", [])
    put(store, [("s%d" % i, vectors(rng, t, d, metric)) for i, t in enumerate((3, 0, 5, 1, 2, 4))])
    same(store, "first put")
    put(store, [("s2", vectors(rng, 9, d, metric))])   # an upsert with another token count moves to the end
    assert list(live)[-1] == "s2" and store.memory()["dead_rows"] == 5
    same(store, "upsert")
    assert store.delete("s0") == "ok" and store.delete("nobody") == "ok"
    del live["s0"]
    same(store, "delete")
    # a duplicate id in one call: the last one is stored
    put(store, [("s3", vectors(rng, 2, d, metric)), ("s9", vectors(rng, 1, d, metric)), ("s3", vectors(rng, 4, d, metric))])
    same(store, "duplicate in a call")
    # a refused put -- a bad row in the middle -- changes nothing
    before = (len(store), store.memory(), store.top_k(query, metric, 100))
    bad = vectors(rng, 3, d, metric)
    bad[1][4] = float("inf")
    assert store.put_many([("n1", vectors(rng, 2, d, metric)), ("s1", bad), ("n2", vectors(rng, 2, d, metric))]) == \
        ("error", "vector contains a non-finite value")
    assert store.put_many([("n1", vectors(rng, 2, d, metric)), ("n2", [[1.0] * (d + 1)])]) == ("error", "dimension mismatch")
    assert store.put_many([("n1", vectors(rng, 2, d, metric)), ("n2", [[]])]) == ("error", "vectors must not be empty")
    assert (len(store), store.memory(), store.top_k(query, metric, 100)) == before
    # more than 4 096 rows: the slab doubles, the rows survive the move
    assert store.memory()["row_capacity"] == 4096
    put(store, [("g%02d" % i, vectors(rng, 64, d, metric)) for i in range(66)])
    m = store.memory()
    assert m["row_capacity"] == 8192 and m["vectors"] == sum(len(v) for v in live.values()) > 4096
    same(store, "growth")
    # more dead rows than live ones: the next put compacts first
    for i in range(40):
        assert store.delete("g%02d" % i) == "ok"
        del live["g%02d" % i]
    m0 = store.memory()
    assert m0["dead_rows"] > m0["vectors"] and m0["compactions"] == 0
    same(store, "before the compaction")
    put(store, [("after", vectors(rng, 7, d, metric))])
    m1 = store.memory()
    assert m1["compactions"] == 1 and m1["dead_rows"] == 0 and m1["vectors"] == m0["vectors"] + 7
    same(store, "compaction")
    # deleting everything forgets the dimension
    for i in list(live):
        assert store.delete(i) == "ok"
    live.clear()
    assert len(store) == 0 and store.dimension is None and store.memory()["row_capacity"] == 0
    query = vectors(rng, 2, 5, metric)
    put(store, [("x", vectors(rng, 3, 5, metric)), ("y", [])])
    assert store.dimension == 5
    same(store, "another dimension")


def test_subset_search(nifs, ref_order):
    rng = np.random.default_rng(960)
    docs = documents(rng, 13, 0)
    store = store_of(docs)
    assert store.delete("doc-5") == "ok"
    query = vectors(rng, 9, 13, 0)
    listed = ["doc-8", "doc-2", "nobody", "doc-5", "doc-2", "doc-0", "doc-9", "doc-3"]
    live = [(i, v) for i, v in docs if i in listed and i != "doc-5"]   # store order, the duplicate once
    for metric in (0, 2, 7):
        for limit in (10, 2, 0):
            check(nifs, store.top_k_ids(listed, query, metric, limit), live, query, metric, limit, (metric, limit))
    assert store.top_k_ids(["nobody"], query, 0, 3) == ("ok", [])
    assert store.top_k_ids([], query, 0, 3) == ("ok", [])


def test_errors_and_their_precedence(nifs):
    ip = 3
    store = store_of([("a", [[1.0, 0.5]]), ("b", [[0.0, 0.25]])])
    assert store.top_k([[1.0]], ip, 3) == ("error", "dimension mismatch")
    assert store.top_k([[1.0, float("nan")]], ip, 3) == ("error", "vector contains a non-finite value")
    assert store.top_k([[1.0, 2.0]], 9, 3) == ("error", "unknown metric")
    assert store.top_k([[1.0, float("nan")]], 9, 3) == ("error", "unknown metric")   # the metric is decoded first
    assert store.top_k([[]], ip, 3) == ("error", "vectors must not be empty")
    assert store.top_k_ids(["a"], [[1.0]], ip, 3) == ("error", "dimension mismatch")
    # the inputs of test_gpu_multi_vector.py: q.t = 2e40 in f32 and in f64 is "metric overflow"
    assert store.put_many([("c", [[1e20, 1e20]])]) == "ok"
    assert store.top_k([[1e20, 1e20]], ip, 3) == ("error", "metric overflow")
    assert store.top_k([[1e20, 1e20]], ip, 0) == ("error", "metric overflow")
    assert store.top_k_ids(["a", "b"], [[1e20, 1e20]], ip, 3)[0] == "ok"
    # ... and finite maxima whose f32 sum is not finite are "score overflow"
    query = [[1.0e19]] * 4
    docs = [("ok1", [[1.0]]), ("sum", [[1.0e19]]), ("ok2", [[2.0]]), ("pair", [[1.0e20]])]
    store = store_of(docs)
    assert nifs.multi_vector_top_k(docs, query, ip, 5) == ("error", "score overflow")
    assert store.top_k(query, ip, 5) == ("error", "score overflow")       # the earlier-put document's status
    assert store.top_k_ids(["pair", "sum", "ok1"], query, ip, 5) == ("error", "score overflow")   # store order, not list order
    assert store.top_k_ids(["pair", "ok1"], query, ip, 5) == ("error", "metric overflow")
    assert store.put_many([("sum", [[1.0e19]])]) == "ok"                  # upserted: now behind "pair"
    docs = [docs[0], docs[2], docs[3], docs[1]]
    assert nifs.multi_vector_top_k(docs, query, ip, 5) == ("error", "metric overflow")
    assert store.top_k(query, ip, 5) == ("error", "metric overflow")
    assert store.delete("pair") == "ok" and store.top_k(query, ip, 5) == ("error", "score overflow")
    assert store.delete("sum") == "ok" and store.top_k(query, ip, 5)[0] == "ok"


def test_a_search_uploads_no_document(nifs):
    rng = np.random.default_rng(970)
    docs = documents(rng, 8, 3, (3, 0, 40, 7))
    store = store_of(docs)
    up = store.memory()["uploaded_bytes"]
    assert up == 50 * 8 * 4
    query = vectors(rng, 3, 8, 3)
    for k in range(10):
        assert (store.top_k(query, 3, 4) if k % 2 else store.top_k_ids(["doc-2", "doc-0"], query, 3, 4))[0] == "ok"
    assert store.memory()["uploaded_bytes"] == up
    assert store.put_many([("more", vectors(rng, 6, 8, 3))]) == "ok"
    assert store.memory()["uploaded_bytes"] == up + 6 * 8 * 4


def test_collection_with_a_resident_store(nifs):
    from vettore_amd.collection import Collection, Embedding
    rng = np.random.default_rng(980)
    d = 16
    plain = Collection.new(dimensions=d, metric="l2", normalize="none")[1]
    resident = Collection.new(dimensions=d, metric="l2", normalize="none", index_options={"resident_multi_vector": True})[1]
    assert plain.mv_store is None and resident.mv_store is not None

    def embedding(i):
        vecs = [list(map(float, v)) for v in rng.uniform(-1, 1, size=(int(rng.integers(1, 9)), d)).astype(np.float32)]
        if i % 3 == 0:
            return Embedding(id="v%02d" % i, vector=vecs[0])
        if i % 3 == 1:
            return Embedding(id="m%02d" % i, vectors=vecs)
        return Embedding(id="b%02d" % i, vector=vecs[0], vectors=vecs[1:] or vecs)

    def both(fn):
        a, b = fn(plain), fn(resident)
        assert a == b, (a, b)
        return a

    embs = [embedding(i) for i in range(60)]
    assert both(lambda c: c.put_many(embs[:50])) == "ok"
    for e in embs[50:]:
        assert both(lambda c: c.put(e)) == "ok"
    assert both(lambda c: c.delete("v03")) == "ok"
    again = embedding(4)
    assert both(lambda c: c.delete("m04")) == "ok" and both(lambda c: c.put(again)) == "ok"   # an upsert
    assert both(lambda c: c.put(Embedding(id="bad", vectors=[[1.0] * (d - 1)]))) == ("error", "dimension_mismatch")
    assert len(resident.mv_store) == len(resident.store) == 59
    query = list(map(float, rng.uniform(-1, 1, size=d).astype(np.float32)))
    qv = [list(map(float, v)) for v in rng.uniform(-1, 1, size=(5, d)).astype(np.float32)]
    up = resident.mv_store.memory()["uploaded_bytes"]
    for metric in ("l2", "inner_product", "cosine", "hamming"):
        got = both(lambda c: c.multi_vector_search(qv, {"limit": 7, "metric": metric}))
        assert got[0] == "ok" and len(got[1]) == 7
    assert both(lambda c: c.multi_vector_search(qv, {"limit": 0})) == ("error", "invalid_limit")
    assert both(lambda c: c.multi_vector_search([[1.0] * (d - 1)], {})) == ("error", "dimension_mismatch")
    for rerank in (("multi_vector", qv), ("multi_vector", qv, {"metric": "inner_product"})):
        for gens in ([("search", {"candidates": 20})], [("search", {"candidates": 10}), "quantized"]):
            got = both(lambda c: c.hybrid_search(query, {"limit": 5, "generators": gens, "rerank": rerank}))
            assert got[0] == "ok" and len(got[1]) == 5
    assert resident.mv_store.memory()["uploaded_bytes"] == up
