"""Batched search of the resident multi-vector store on the device (vt_mv_top_k_batch / vt_mv_top_k_ids_batch, K9rb:
vt_maxsim_batch.hip) -- `-m gpu`.  Every set of a batch comes back as the single-set call returns it on the same store
state: ids, order, float32 bits, rank keys and status -- tolerance zero everywhere.  Which path a set took is asserted
with vt_mv_counters, never timed."""
import ctypes as C

import numpy as np
import pytest

import maxsim_ref
from test_gpu_mv_store import TOKENS, check, documents, f32bits, store_of, vectors
from test_gpu_parity import nifs  # noqa: F401  (a fixture)
from test_gpu_mv_store import ref_order  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 7, 8, 9, 33, 8, 1)   # no vector, one lane group and its edges, a second pass at four groups of eight


def canon(res):
    """A result with its scores as float32 bits (-0.0 and 0.0 differ, a NaN equals itself)."""
    if res[0] != "ok":
        return res
    return ("ok", [(h[0], f32bits(h[1])) + tuple(h[2:]) for h in res[1]])


def plain(res):
    """A result without its rank keys: what store.top_k returns."""
    return res if res[0] != "ok" else ("ok", [h[:2] for h in res[1]])


def same_as_singles(nifs, store, sets, metric, limit, id_lists=None, ctx=None):
    """The batch call against a loop of single calls, rank keys included; returns the batch's answers."""
    if id_lists is None:
        singles = [nifs.mv_top_k(store.ref, s, metric, limit, True) for s in sets]
        got = nifs.mv_top_k_batch(store.ref, sets, metric, limit, True)
    else:
        singles = [nifs.mv_top_k_ids(store.ref, i, s, metric, limit, True) for i, s in zip(id_lists, sets)]
        got = nifs.mv_top_k_ids_batch(store.ref, id_lists, sets, metric, limit, True)
    assert isinstance(got, list) and len(got) == len(sets), (ctx, got)
    for b, (g, w) in enumerate(zip(got, singles)):
        assert canon(g) == canon(w), (ctx, b, g, w)
    return got


def grown(store, fn):
    """(scoring_launches, batched_sets) added by fn()."""
    before = store.counters()
    fn()
    after = store.counters()
    return after["scoring_launches"] - before["scoring_launches"], after["batched_sets"] - before["batched_sets"]


@pytest.mark.parametrize("metric", range(9))
def test_whole_store_mixed_sets(nifs, ref_order, metric):
    rng = np.random.default_rng(1100 + metric)
    docs = documents(rng, 13, metric)
    store = store_of(docs)
    sets = [vectors(rng, n, 13, metric) for n in COUNTS]
    sets[4][0] = docs[4][1][0]  # an exact match somewhere
    for limit in (len(docs) + 3, 4, 0):
        got = same_as_singles(nifs, store, sets, metric, limit, ctx=(metric, limit))
        if metric in (3, 0, 2):
            for b, query in enumerate(sets):
                want = maxsim_ref.top_k(docs, query, metric, limit)
                assert got[b][0] == "ok" and [(h[0], f32bits(h[1])) for h in got[b][1]] == [(h[0], f32bits(h[1])) for h in want], \
                    (metric, limit, b)
    if metric < 7:   # the sets with a vector went through K9rb, the one without through the single path
        assert grown(store, lambda: store.top_k_batch(sets, metric, 4)) == (2, 7)
    else:            # float Hamming / Jaccard: every set through the single path
        assert grown(store, lambda: store.top_k_batch(sets, metric, 4))[1] == 0


@pytest.mark.parametrize("metric", [3, 0, 2])
def test_panels_and_the_lone_big_set(nifs, ref_order, metric):
    rng = np.random.default_rng(1110 + metric)
    docs = documents(rng, 256, metric, (0, 1, 17, 33, 65))
    store = store_of(docs)
    sets = [vectors(rng, n, 256, metric) for n in (9, 9, 9, 33, 9, 16, 1)]
    launches, batched = grown(store, lambda: same_as_singles(nifs, store, sets, metric, 4, ctx=metric))
    singles = grown(store, lambda: [store.top_k(s, metric, 4) for s in sets])[0]
    # d = 256 leaves LDS for 32 slots beside the tiles: two padded sets of 16 a panel, the set of 33 (40 slots) alone
    assert launches - singles > 1 and batched == 6 < len(sets)


@pytest.mark.parametrize("metric", [3, 7, 8])
def test_fallbacks(nifs, ref_order, metric):
    rng = np.random.default_rng(1120 + metric)
    if metric == 3:   # a dimension whose tiles do not fit in LDS
        docs = documents(rng, 772, metric, (0, 1, 33))
        sets = [vectors(rng, n, 772, metric) for n in (3, 1, 9)]
    else:             # float Hamming / Jaccard
        docs = documents(rng, 13, metric)
        sets = [vectors(rng, n, 13, metric) for n in (9, 1, 33, 0)]
    store = store_of(docs)
    assert grown(store, lambda: same_as_singles(nifs, store, sets, metric, 5, ctx=metric))[1] == 0
    ids = [[d[0] for d in docs[:2]]] * len(sets)
    assert grown(store, lambda: same_as_singles(nifs, store, sets, metric, 5, ids, ctx=metric))[1] == 0


def test_ids_mode_and_the_counters(nifs, ref_order):
    rng = np.random.default_rng(1130)
    docs = documents(rng, 13, 0)
    store = store_of(docs)
    assert store.delete("doc-5") == "ok"
    everyone = [d[0] for d in docs]
    id_lists = [["doc-8", "doc-2", "nobody", "doc-2", "doc-0"],        # an unknown id, a duplicate
                ["doc-9", "doc-5", "doc-3", "doc-1"],                  # a deleted id, scrambled
                [], ["doc-7"], everyone, ["nobody"], list(reversed(everyone)), ["doc-0", "doc-0"]]
    sets = [vectors(rng, n, 13, 0) for n in (9, 1, 7, 8, 9, 2, 5, 3)]
    up = store.memory()["uploaded_bytes"]
    for metric in (0, 2, 3):
        for limit in (10, 2, 0):
            got = same_as_singles(nifs, store, sets, metric, limit, id_lists, ctx=(metric, limit))
            live = [d for d in docs if d[0] in id_lists[0]]
            check(nifs, plain(got[0]), live, sets[0], metric, limit, (metric, limit))
            assert got[2] == got[5] == ("ok", [])
    assert grown(store, lambda: store.top_k_ids_batch(id_lists, sets, 0, 10)) == (1, 8)
    assert grown(store, lambda: store.top_k_batch(sets, 0, 10)) == (1, 8)
    assert grown(store, lambda: [store.top_k(s, 0, 10) for s in sets]) == (8, 0)
    assert grown(store, lambda: [store.top_k_ids(everyone, s, 0, 10) for s in sets]) == (8, 0)
    assert store.memory()["uploaded_bytes"] == up
    # limits above one select pass: the lists are cut set by set
    same_as_singles(nifs, store, sets, 0, 300, id_lists, ctx="limit 300")
    same_as_singles(nifs, store, sets, 0, 300, ctx="limit 300")
    assert nifs.mv_top_k_batch(store.ref, [], 0, 3) == [] and nifs.mv_top_k_ids_batch(store.ref, [], [], 0, 3) == []
    assert nifs.mv_top_k_batch(store.ref, sets[:1], 0, 3) == [store.top_k(sets[0], 0, 3)]   # a batch of one


def raw_batch(nifs, store, sets, metric, limit, id_lists=None):
    """The C call without set_status: (status, [out[b] is NULL])."""
    import vettore_amd._lib as L
    qv, qoff, set_off = nifs._pack_sets(sets)
    outs = (C.c_void_p * len(sets))()
    if id_lists is None:
        st = L.load().vt_mv_top_k_batch(store.ref.handle, len(sets), nifs._szp(set_off), nifs._fp(qv), nifs._szp(qoff), metric,
                                        limit, outs, None)
    else:
        idb, ioff = nifs._pack_ids(i for ids in id_lists for i in ids)
        set_id_off = np.zeros(len(id_lists) + 1, dtype=np.uintp)
        set_id_off[1:] = np.cumsum([len(ids) for ids in id_lists])
        st = L.load().vt_mv_top_k_ids_batch(store.ref.handle, len(sets), nifs._szp(set_id_off), idb, nifs._szp(ioff),
                                            nifs._szp(set_off), nifs._fp(qv), nifs._szp(qoff), metric, limit, outs, None)
    null = [not outs[b] for b in range(len(sets))]
    for b in range(len(sets)):
        if outs[b]:
            L.load().vt_hits_free(C.c_void_p(outs[b]))
    return st, null


def test_errors_stay_with_their_set(nifs):
    ip = 3
    # "metric overflow": q.t = 2e40 in f32 and in f64 (test_errors_and_their_precedence's documents and query)
    store = store_of([("a", [[1.0, 0.5]]), ("b", [[0.0, 0.25]]), ("c", [[1e20, 1e20]])])
    sets = [[[1.0, 2.0]], [[1e20, 1e20]], [[0.5, -0.5]], [[1.0]], [[1.0, float("nan")]], [[]], [[2.0, 1.0]]]
    for limit in (3, 0):
        got = same_as_singles(nifs, store, sets, ip, limit, ctx="metric overflow")
        assert [g[0] for g in got] == ["ok", "error", "ok", "error", "error", "error", "ok"]
        assert [g[1] for g in got if g[0] == "error"] == ["metric overflow", "dimension mismatch",
                                                          "vector contains a non-finite value", "vectors must not be empty"]
    assert grown(store, lambda: store.top_k_batch(sets, ip, 3)) == (1, 4)   # the four valid sets: one panel, one pass
    got = same_as_singles(nifs, store, sets, ip, 3, [["c", "a"], ["a", "b"], ["c"], ["a"], ["a"], ["a"], ["b", "c", "a"]], "ids")
    assert [g[0] for g in got] == ["ok", "ok", "ok", "error", "error", "error", "ok"]
    # without set_status the first failing set in batch order is the call's status, and nothing else comes back
    st, null = raw_batch(nifs, store, sets, ip, 3)
    assert nifs._lib.error_text(st) == "metric overflow" and null == [True] * 7
    st, null = raw_batch(nifs, store, sets[2:], ip, 3)
    assert nifs._lib.error_text(st) == "dimension mismatch" and null == [True] * 5
    st, null = raw_batch(nifs, store, [sets[0], sets[2], sets[6]], ip, 3)
    assert st == 0 and null == [False] * 3
    st, null = raw_batch(nifs, store, sets, ip, 3, [["a"]] * 7)
    assert nifs._lib.error_text(st) == "dimension mismatch" and null == [True] * 7
    # an unknown metric fails the call, even when a set holds a NaN
    assert nifs.mv_top_k_batch(store.ref, sets, 9, 3) == ("error", "unknown metric")
    assert nifs.mv_top_k_ids_batch(store.ref, [["a"]] * 7, sets, 9, 3) == ("error", "unknown metric")
    assert nifs._lib.error_text(raw_batch(nifs, store, sets, 9, 3)[0]) == "unknown metric"
    # NULL `out` or offsets with a store in hand
    import vettore_amd._lib as L
    off = (C.c_size_t * 2)(0, 0)
    outs = (C.c_void_p * 1)()
    assert L.load().vt_mv_top_k_batch(store.ref.handle, 1, off, None, None, ip, 1, None, None) == 19
    assert L.load().vt_mv_top_k_batch(store.ref.handle, 1, None, None, None, ip, 1, outs, None) == 19
    assert L.load().vt_mv_top_k_ids_batch(store.ref.handle, 1, None, b"", off, off, None, None, ip, 1, outs, None) == 19
    assert L.load().vt_mv_top_k_batch(store.ref.handle, 0, off, None, None, ip, 1, outs, None) == 0

    # "score overflow": finite maxima whose f32 sum is not finite -- the total must not reach the next set of the pass
    query = [[1.0e19]] * 4
    docs = [("ok1", [[1.0]]), ("sum", [[1.0e19]]), ("ok2", [[2.0]]), ("pair", [[1.0e20]])]
    store = store_of(docs)
    sets = [[[1.0]], query, [[3.0]], [[1.0e19]] * 3, [[-2.0]] * 5, query, [[0.5]]]
    got = same_as_singles(nifs, store, sets, ip, 5, ctx="score overflow")
    assert got[1] == got[5] == ("error", "score overflow") and got[3] == ("error", "metric overflow")
    assert [g[0] for g in got] == ["ok", "error", "ok", "error", "ok", "error", "ok"]
    assert grown(store, lambda: store.top_k_batch(sets, ip, 5)) == (1, 7)
    # ids mode: a set's status is decided by store order, not list order
    id_lists = [["pair", "sum", "ok1"], ["pair", "ok1"], ["ok2", "ok1"], ["sum"], ["pair", "sum", "ok1"]]
    got = same_as_singles(nifs, store, [query] * 4 + [[[1.0]]], ip, 5, id_lists, "store order")
    assert [g[1] for g in got[:2]] == ["score overflow", "metric overflow"] and got[2][0] == "ok" and got[4][0] == "ok"
    assert got[3] == ("error", "score overflow")
    assert store.put_many([("sum", [[1.0e19]])]) == "ok"                  # upserted: now behind "pair"
    got = same_as_singles(nifs, store, [query] * 4 + [[[1.0]]], ip, 5, id_lists, "after the upsert")
    assert got[0] == ("error", "metric overflow")


def test_the_four_lane_orders(nifs, oracle_mod, vt_debug):
    rng = np.random.default_rng(1140)
    docs = documents(rng, 13, 3)
    store = store_of(docs)
    sets = [vectors(rng, n, 13, 3) for n in (9, 1, 33, 8)]
    try:
        for order in (0, 1, 2, 3):
            vt_debug.set("reduce_order", order)
            oracle_mod.set_reduce_order(order)
            for metric in (3, 5):
                got = same_as_singles(nifs, store, sets, metric, len(docs), ctx=(order, metric))
                for b, query in enumerate(sets):
                    check(nifs, plain(got[b]), docs, query, metric, len(docs), (order, metric, b))
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


def test_after_mutations(nifs, ref_order):
    rng = np.random.default_rng(1150)
    metric, d = 3, 8
    sets = [vectors(rng, n, d, metric) for n in (2, 9, 1)]
    live = {}

    def put(store, docs):
        assert store.put_many(docs) == "ok"
        for i, v in docs:
            live.pop(i, None)
            live[i] = v

    def same(store, ctx):
        docs = list(live.items())
        got = same_as_singles(nifs, store, sets, metric, len(docs) + 1, ctx=ctx)
        want = maxsim_ref.top_k(docs, sets[1], metric, len(docs) + 1)
        assert [(h[0], f32bits(h[1])) for h in got[1][1]] == [(h[0], f32bits(h[1])) for h in want], ctx
        some = list(live)[::3] + ["nobody"]
        same_as_singles(nifs, store, sets, metric, 5, [some, list(live)[:1], list(reversed(list(live)))], ctx)

    from vettore_amd.mv_store import ResidentMultiVector
    store = ResidentMultiVector()
    assert store.top_k_batch(sets, metric, 3) == [("ok", [])] * 3
    put(store, [("s%d" % i, vectors(rng, t, d, metric)) for i, t in enumerate((3, 0, 5, 1, 2, 4))])
    same(store, "first put")
    put(store, [("s2", vectors(rng, 9, d, metric))])   # an upsert moves to the end
    same(store, "upsert")
    assert store.delete("s0") == "ok"
    del live["s0"]
    same(store, "delete")
    put(store, [("g%02d" % i, vectors(rng, 64, d, metric)) for i in range(66)])   # past 4 096 rows: the slab doubles
    assert store.memory()["row_capacity"] == 8192
    same(store, "growth")
    for i in range(40):
        assert store.delete("g%02d" % i) == "ok"
        del live["g%02d" % i]
    same(store, "before the compaction")
    put(store, [("after", vectors(rng, 7, d, metric))])
    assert store.memory()["compactions"] == 1
    same(store, "compaction")


def test_width(nifs, ref_order):
    rng = np.random.default_rng(1160)
    docs = documents(rng, 13, 0)
    store = store_of(docs)
    sets = [vectors(rng, 1, 13, 0) for _ in range(300)]
    assert grown(store, lambda: same_as_singles(nifs, store, sets, 0, 3, ctx="300 sets"))[1] == 300
    # id lists of 0, 1 and 130 ids in one call
    docs = [("w%03d" % i, vectors(rng, 1 + i % 3, 8, 3)) for i in range(130)]
    store = store_of(docs)
    order = [docs[i][0] for i in rng.permutation(130)]
    sets = [vectors(rng, n, 8, 3) for n in (3, 9, 4)]
    got = same_as_singles(nifs, store, sets, 3, 140, [[], order[:1], order], ctx="0, 1 and 130 ids")
    assert [len(g[1]) for g in got] == [0, 1, 130]
    check(nifs, plain(got[2]), docs, sets[2], 3, 140, "130 ids")


def test_collection_search_batch(nifs):
    from vettore_amd.collection import Collection, Embedding
    rng = np.random.default_rng(1170)
    d = 16
    plain = Collection.new(dimensions=d, metric="l2", normalize="none")[1]
    resident = Collection.new(dimensions=d, metric="l2", normalize="none", index_options={"resident_multi_vector": True})[1]
    embs = []
    for i in range(30):
        vecs = [list(map(float, v)) for v in rng.uniform(-1, 1, size=(int(rng.integers(1, 9)), d)).astype(np.float32)]
        embs.append(Embedding(id="e%02d" % i, vector=vecs[0]) if i % 3 == 0 else Embedding(id="e%02d" % i, vectors=vecs))
    assert plain.put_many(embs) == "ok" and resident.put_many(embs) == "ok"
    queries = [[list(map(float, v)) for v in rng.uniform(-1, 1, size=(n, d)).astype(np.float32)] for n in (5, 1, 9, 33)]
    queries += [[[1.0] * (d - 1)], [], "nonsense", [[float("nan")] * d]]
    for opts in ({"limit": 7}, {"limit": 3, "metric": "inner_product"}, {"metric": "cosine"}, {"metric": "hamming"}, None,
                 {"limit": 0}, {"metric": "nope"}, {"candidates": 3}, "nonsense"):
        a, b = plain.multi_vector_search_batch(queries, opts), resident.multi_vector_search_batch(queries, opts)
        assert a == b, (opts, a, b)
        assert a == [plain.multi_vector_search(q, opts) for q in queries], opts
        assert b == [resident.multi_vector_search(q, opts) for q in queries], opts
    before = resident.mv_store.counters()["batched_sets"]
    got = resident.multi_vector_search_batch(queries, {"limit": 7})
    assert [g[0] for g in got[:4]] == ["ok"] * 4 and all(len(g[1]) == 7 for g in got[:4])
    assert resident.mv_store.counters()["batched_sets"] == before + 4
    assert plain.multi_vector_search_batch("nonsense") == resident.multi_vector_search_batch("nonsense") == ("error", "invalid_multi_vector")
    assert resident.multi_vector_search_batch([], {"limit": 7}) == []
