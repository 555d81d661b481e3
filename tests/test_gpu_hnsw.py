"""The HNSW index on the device (vt_hnsw_*, K11: vt_hnsw.hip) -- `-m gpu`.  The reference's HNSW is deterministic, so
everything here is equality with its restatement (tests/hnsw_ref.py, distances from the CPU oracle): after any inserts
and deletes every node's internal id, level and adjacency lists and the entry are the restatement's, and a search
returns its ids in its order with the same float32 bits.  No tolerance anywhere."""
import math

import numpy as np
import pytest

import hnsw_ref
import support
from hnsw_ref import COSINE, INNER_PRODUCT, L2, HnswError, HnswIndex
from test_gpu_parity import nifs  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

METRICS = {L2: "l2", COSINE: "cosine", INNER_PRODUCT: "inner_product"}


def f32bits(x):
    return np.float32(x).tobytes()


@pytest.fixture
def ref_order(nifs, oracle_mod):
    """The oracle folds a chunk in the lane order the library uses."""
    order = nifs.debug_get("reduce_order")
    oracle_mod.set_reduce_order(order)
    yield order
    oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


def new_gpu(nifs, metric, p):
    make = {L2: nifs.hnsw_new_l2, COSINE: nifs.hnsw_new_cosine, INNER_PRODUCT: nifs.hnsw_new_inner_product}[metric]
    res = make(p["m"], p["m0"], p["ef_construction"], p["ef_search"], p["max_level"])
    assert res[0] == "ok", res
    return res[1]


def params(m, m0, efc, efs=16, max_level=12):
    return {"m": m, "m0": m0, "ef_construction": efc, "ef_search": efs, "max_level": max_level}


def assert_same_graph(nifs, idx, ref):
    assert len(idx) == len(ref.nodes)
    assert idx.dimension == ref.dimension
    for nid, node in ref.nodes.items():
        got = nifs.hnsw_node(idx, node.external_id)
        assert got == (nid, node.layer, nid == ref.entry), node.external_id
        for layer, conn in enumerate(node.connections):
            assert nifs.hnsw_neighbors(idx, nid, layer) == conn, (node.external_id, layer)
        assert nifs.hnsw_neighbors(idx, nid, node.layer + 1) is None


def search_both(nifs, idx, ref, query, limit):
    """("ok", [(id, raw bits)]) or ("error", text) from each side."""
    try:
        want = ("ok", [(i, f32bits(r)) for i, r in ref.search(query, limit)])
    except HnswError as e:
        want = ("error", str(e))
    got = nifs.hnsw_search(idx, query, limit)
    if got[0] == "ok":
        got = ("ok", [(i, f32bits(r)) for i, r in got[1]])
    return got, want


def assert_same_search(nifs, idx, ref, query, limit):
    got, want = search_both(nifs, idx, ref, query, limit)
    assert got == want


_BUILT = {}


def corpus(name):
    """(ids, vectors, parameters, limit) of a named corpus: made once, never changed."""
    if name in _BUILT:
        return _BUILT[name]
    rng = np.random.default_rng(sum(name.encode()))
    ids = lambda n: [b"k%d" % ((i * 7919) % 100003) for i in range(n)]  # byte order differs from insertion order
    if name == "600x16":
        c = (ids(600), rng.standard_normal((600, 16)).astype(np.float32), params(4, 8, 40), 10)
    elif name == "400x16":
        c = (ids(400), rng.standard_normal((400, 16)).astype(np.float32), params(8, 16, 100), 10)
    elif name == "300x3":  # the reference's sin / cos corpus, a limit above n
        v = np.array([[np.sin(np.float32(i)), np.cos(np.float32(i)), np.float32(i) / np.float32(300.0)] for i in range(300)], np.float32)
        c = ([b"node-%03d" % i for i in range(300)], v, params(8, 16, 200, 200), 1000)
    elif name == "200x100":  # a scalar tail: 12 chunks plus 4
        c = (ids(200), rng.standard_normal((200, 100)).astype(np.float32), params(4, 8, 30), 10)
    elif name == "150x768":  # the LDS tile at production width
        c = (ids(150), rng.standard_normal((150, 768)).astype(np.float32), params(8, 32, 40), 10)
    elif name == "300x8-long":  # lists longer than a wave
        c = (ids(300), rng.standard_normal((300, 8)).astype(np.float32), params(40, 70, 80), 10)
    elif name == "40x4100":  # rows too long for LDS: walked in global memory
        c = (ids(40), rng.standard_normal((40, 4100)).astype(np.float32), params(4, 8, 20), 5)
    else:
        raise KeyError(name)
    _BUILT[name] = c
    return c


@pytest.mark.parametrize("metric", [L2, COSINE, INNER_PRODUCT])
@pytest.mark.parametrize("name", ["600x16", "400x16", "300x3", "200x100", "150x768", "300x8-long", "40x4100"])
def test_graph_and_hits_are_the_restatements(nifs, ref_order, name, metric):
    ids, vecs, p, limit = corpus(name)
    ref = HnswIndex(metric, **p)
    ref.insert_many(list(zip(ids, vecs)))
    idx = new_gpu(nifs, metric, p)
    assert nifs.hnsw_insert_many(idx, list(zip(ids, vecs))) == ("ok", ())
    assert_same_graph(nifs, idx, ref)
    c = nifs.hnsw_counters(idx)
    assert c["traversals"] == len(ids) - 1 and c["traversal_launches"] == len(ids) - 1 + c["reruns"]
    rng = np.random.default_rng(5)
    d = vecs.shape[1]
    for q in [vecs[0], vecs[len(ids) // 2], np.zeros(d, np.float32)] + list(rng.standard_normal((3, d)).astype(np.float32)):
        assert_same_search(nifs, idx, ref, q, limit)
    if name == "300x3":
        assert len(nifs.hnsw_search(idx, [0.0, 1.0, 0.5], 1000)[1]) == 300


_ORDER_CORPORA = {}


def order_corpus(oracle_mod, name):
    """(ids, vectors, queries, parameters, limit) for the lane-order test: "120x13" is staged in LDS and has one full
    chunk and a scalar tail of five, "24x4100" lies past kHnswLdsDim and is walked in global memory.  The data must tell
    the lane orders apart, or an index that ignored its order would pass: with these seeds the oracle's distances under
    any two of the four orders differ in their bits for some (row, query) pair of either shape under L2 and under inner
    product (worked out on the CPU when the test was written; orders 0 and 3: 120x13 -- 37 of 360 pairs under L2, 95 under
    inner product; 24x4100 -- 5 and 56 of 72), and the assertion below keeps it so."""
    if name not in _ORDER_CORPORA:
        n, d, p, limit = {"120x13": (120, 13, params(4, 8, 30), 10), "24x4100": (24, 4100, params(4, 8, 20), 5)}[name]
        rng = np.random.default_rng(sum(name.encode()))
        vecs = rng.standard_normal((n, d)).astype(np.float32)
        queries = rng.standard_normal((3, d)).astype(np.float32)
        for metric in (L2, INNER_PRODUCT):
            bits = []
            for order in (0, 1, 2, 3):
                oracle_mod.set_reduce_order(order)
                bits.append(tuple(f32bits(oracle_mod.compute(metric, v, q)) for v in vecs for q in queries))
            assert len(set(bits)) == 4, (name, metric)
        _ORDER_CORPORA[name] = ([b"k%d" % ((i * 7919) % 100003) for i in range(n)], vecs, queries, p, limit)
    return _ORDER_CORPORA[name]


@pytest.mark.parametrize("metric", [L2, INNER_PRODUCT])
@pytest.mark.parametrize("name,order", [("120x13", 0), ("120x13", 1), ("120x13", 2), ("120x13", 3), ("24x4100", 1)])
def test_the_four_lane_orders(nifs, oracle_mod, vt_debug, name, order, metric):
    """K11's chains in every lane order (an index takes the library's order when it is made): graph and hits are the
    restatement's under the same order."""
    try:
        ids, vecs, queries, p, limit = order_corpus(oracle_mod, name)
        vt_debug.set("reduce_order", order)
        oracle_mod.set_reduce_order(order)
        ref = HnswIndex(metric, **p)
        ref.insert_many(list(zip(ids, vecs)))
        idx = new_gpu(nifs, metric, p)
        assert nifs.hnsw_insert_many(idx, list(zip(ids, vecs))) == ("ok", ())
        assert_same_graph(nifs, idx, ref)
        for q in [vecs[0]] + list(queries):
            assert_same_search(nifs, idx, ref, q, limit)
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


@pytest.mark.parametrize("metric", [L2, INNER_PRODUCT])
def test_ties_duplicates_and_signed_zeros(nifs, ref_order, metric):
    """An integer grid with many duplicate vectors: equal distances everywhere, so every (distance, id) tie-break and
    every IEEE `<` beside the total order decides something.  Under inner product a row orthogonal to the query has
    raw +0.0 and rank -0.0; the zero query gives every row that rank."""
    rng = np.random.default_rng(11)
    vecs = rng.integers(-1, 2, (240, 8)).astype(np.float32)
    vecs[::5] = vecs[0]
    vecs[3::7, :4] = 0.0
    ids = [b"t%d" % ((i * 7919) % 1009) for i in range(240)]
    p = params(4, 8, 20, 8)
    ref = HnswIndex(metric, **p)
    ref.insert_many(list(zip(ids, vecs)))
    idx = new_gpu(nifs, metric, p)
    assert nifs.hnsw_insert_many(idx, list(zip(ids, vecs))) == ("ok", ())
    assert_same_graph(nifs, idx, ref)
    queries = [np.zeros(8, np.float32), -np.zeros(8, np.float32), vecs[0], np.float32([0, 0, 0, 0, 1, -1, 0, 0]),
               np.float32([1, 0, 0, 0, 0, 0, 0, 0]), np.float32([-1, 1, -1, 1, 0, 0, 0, 0])]
    for q in queries:
        for limit in (1, 7, 240):
            assert_same_search(nifs, idx, ref, q, limit)
    got = nifs.hnsw_search(idx, np.zeros(8, np.float32), 3, with_keys=True)[1]
    if metric == INNER_PRODUCT:
        assert all(f32bits(r) == f32bits(0.0) and k == hnsw_ref.total_key(-0.0) for _, r, k in got)


def test_edge_cases_of_limit_and_ef(nifs, ref_order):
    rng = np.random.default_rng(3)
    vecs = rng.standard_normal((50, 5)).astype(np.float32)
    ids = [b"e%02d" % i for i in range(50)]
    p = params(4, 8, 100, 1)  # ef_search 1, ef_construction above n
    idx = new_gpu(nifs, L2, p)
    ref = HnswIndex(L2, **p)
    # limit 0 answers before validation, on an empty index and later; an empty index answers a valid query with nothing
    assert nifs.hnsw_search(idx, [], 0) == ("ok", [])
    assert nifs.hnsw_search(idx, [math.nan], 0) == ("ok", [])
    assert nifs.hnsw_search(idx, [1.0, 2.0], 5) == ("ok", [])
    assert nifs.hnsw_search(idx, [], 5) == ("error", "vector must not be empty")
    assert nifs.hnsw_search(idx, [math.inf], 5) == ("error", "vector contains a non-finite value")
    ref.insert_many(list(zip(ids, vecs)))
    assert nifs.hnsw_insert_many(idx, list(zip(ids, vecs))) == ("ok", ())
    assert_same_graph(nifs, idx, ref)
    assert nifs.hnsw_search(idx, [1.0], 0) == ("ok", [])
    for limit in (1, 2, 10, 49, 50, 51, 4_294_967_295):  # limit above ef_search, above n
        for q in (vecs[7], vecs[49] + np.float32(0.25)):
            assert_same_search(nifs, idx, ref, q, limit)


def test_errors_come_in_the_references_order(nifs, ref_order):
    p = params(4, 8, 20)
    idx = new_gpu(nifs, L2, p)
    ref = HnswIndex(L2, **p)
    for i in range(12):
        v = [float(i), float(-i)]
        ref.insert(b"v%d" % i, v)
        assert nifs.hnsw_insert(idx, b"v%d" % i, v) == ("ok", ())
    assert nifs.hnsw_insert(idx, b"x", []) == ("error", "vector must not be empty")
    assert nifs.hnsw_insert(idx, b"x", [1.0]) == ("error", "dimension mismatch")
    assert nifs.hnsw_insert(idx, b"x", [math.nan]) == ("error", "dimension mismatch")   # dimension before finiteness
    assert nifs.hnsw_insert(idx, b"x", [math.nan, 1.0]) == ("error", "vector contains a non-finite value")
    assert nifs.hnsw_search(idx, [1.0], 1) == ("error", "dimension mismatch")
    assert nifs.hnsw_search(idx, [math.inf, 0.0], 1) == ("error", "vector contains a non-finite value")
    assert_same_graph(nifs, idx, ref)
    # "metric overflow" on a search: the f64 recovery cannot represent the distance either
    big = [3e38, -3e38]
    got, want = search_both(nifs, idx, ref, big, 3)
    assert got == want == ("error", "metric overflow")
    # ... and on an insert whose id existed: the old node is gone, the graph otherwise the restatement's
    with pytest.raises(HnswError) as e:
        ref.insert(b"v5", big)
    assert str(e.value) == "metric overflow"
    assert nifs.hnsw_insert(idx, b"v5", big) == ("error", "metric overflow")
    assert nifs.hnsw_node(idx, b"v5") is None and len(idx) == 11
    assert_same_graph(nifs, idx, ref)
    ref.insert(b"after", [0.5, 0.5])
    assert nifs.hnsw_insert(idx, b"after", [0.5, 0.5]) == ("ok", ())
    assert_same_graph(nifs, idx, ref)   # the internal id the failed insert took is not handed out again
    # insert_many: one bad vector and the index stays as it was
    for bad in ([1.0], [math.inf, 0.0], []):
        assert nifs.hnsw_insert_many(idx, [(b"n1", [1.0, 1.0]), (b"n2", bad)])[0] == "error"
    assert_same_graph(nifs, idx, ref)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_one_overflowing_pair_in_any_tile_round_fails_the_traversal(nifs, ref_order, sign):
    """d = 768: the LDS tile holds 16 rows, so a hop's 32 neighbours take two rounds.  One stored row has 2e38 in a
    coordinate; a query with 3 there overflows against that row alone (6e38 is no f32, in f64 either).  Under inner
    product that row is the FIRST of every list when the others hold +0.5 there (the first round) and the LAST when
    they hold -0.5 (the last round): either way the search and the insert must end in "metric overflow"."""
    rng = np.random.default_rng(61)
    d, n = 768, 33
    vecs = (rng.standard_normal((n, d)) * 0.01).astype(np.float32)
    vecs[:, 0] = sign * 0.5
    vecs[n - 1, 0] = 2e38
    ids = [b"o%02d" % i for i in range(n)]
    p = params(16, 32, 40, 8)
    probe = HnswIndex(INNER_PRODUCT, **p)
    assert probe.level_for(ids[n - 1]) == 0   # (never the entry: the entry's own distance is computed alone)
    ref = HnswIndex(INNER_PRODUCT, **p)
    ref.insert_many(list(zip(ids, vecs)))
    idx = new_gpu(nifs, INNER_PRODUCT, p)
    assert nifs.hnsw_insert_many(idx, list(zip(ids, vecs))) == ("ok", ())
    assert_same_graph(nifs, idx, ref)
    big = n - 1
    entry_list = ref.nodes[ref.entry].connections[0]
    assert len(entry_list) == 32 and entry_list.index(big) == (0 if sign > 0 else 31)
    q = (rng.standard_normal(d) * 0.01).astype(np.float32)
    q[0] = 3.0
    got, want = search_both(nifs, idx, ref, q, 5)
    assert got == want == ("error", "metric overflow")
    with pytest.raises(HnswError) as e:
        ref.insert(b"new", q)
    assert str(e.value) == "metric overflow"
    assert nifs.hnsw_insert(idx, b"new", q) == ("error", "metric overflow")
    assert_same_graph(nifs, idx, ref)
    batch = nifs.hnsw_search_batch(idx, np.stack([q, vecs[3]]), 5)
    assert batch[0] == ("error", "metric overflow") and batch[1][0] == "ok"
    assert_same_search(nifs, idx, ref, vecs[3], 5)


def test_mutations_follow_the_restatement(nifs, ref_order):
    rng = np.random.default_rng(17)
    p = params(4, 8, 24, 12)
    idx = new_gpu(nifs, COSINE, p)
    ref = HnswIndex(COSINE, **p)
    live = []
    d = 6

    def both_insert(ext, v):
        ref.insert(ext, v)
        assert nifs.hnsw_insert(idx, ext, v) == ("ok", ())
        if ext not in live:
            live.append(ext)

    def both_delete(ext):
        ref.delete(ext)
        assert nifs.hnsw_delete(idx, ext) == ("ok", ())
        if ext in live:
            live.remove(ext)

    for i in range(40):
        both_insert(b"m%d" % ((i * 7919) % 101), rng.standard_normal(d).astype(np.float32))
    both_insert(live[3], rng.standard_normal(d).astype(np.float32))          # an upsert
    both_delete(ref.nodes[ref.entry].external_id)                             # the entry goes
    both_delete(b"missing")
    assert_same_graph(nifs, idx, ref)
    for step in range(300):                                                   # a random interleaving
        r = rng.random()
        if r < 0.45 or len(live) < 5:
            both_insert(b"m%d" % int(rng.integers(0, 400)), rng.standard_normal(d).astype(np.float32))
        elif r < 0.6:
            both_insert(live[int(rng.integers(0, len(live)))], rng.standard_normal(d).astype(np.float32))
        elif r < 0.8:
            both_delete(live[int(rng.integers(0, len(live)))] if rng.random() < 0.8 else ref.nodes[ref.entry].external_id)
        else:
            assert_same_search(nifs, idx, ref, rng.standard_normal(d).astype(np.float32), int(rng.integers(1, 20)))
        if step % 50 == 49:
            assert_same_graph(nifs, idx, ref)
    assert_same_graph(nifs, idx, ref)
    mem = nifs.hnsw_memory(idx)
    assert mem["rows"] - mem["dead_rows"] == len(live) and mem["edges"] == sum(len(l) for n in ref.nodes.values() for l in n.connections)
    # everything goes, then another dimension comes: internal ids keep counting
    for ext in list(live):
        both_delete(ext)
    assert len(idx) == 0 and idx.dimension is None and nifs.hnsw_memory(idx)["rows"] == 0
    assert nifs.hnsw_search(idx, [1.0, 2.0, 3.0], 4) == ("ok", [])
    for i in range(20):
        both_insert(b"z%d" % i, rng.standard_normal(3).astype(np.float32))
    assert_same_graph(nifs, idx, ref)
    assert_same_search(nifs, idx, ref, [0.1, 0.2, 0.3], 20)


def test_search_batch_equals_the_lone_searches(nifs, ref_order):
    ids, vecs, p, _ = corpus("400x16")
    idx = new_gpu(nifs, L2, p)
    assert nifs.hnsw_insert_many(idx, list(zip(ids, vecs))) == ("ok", ())
    rng = np.random.default_rng(23)
    queries = rng.standard_normal((64, 16)).astype(np.float32)
    queries[5, 3] = np.nan
    queries[17, 0] = np.inf
    queries[40] = 3e38      # "metric overflow"
    queries[41, ::2] = -3e38
    before = nifs.hnsw_counters(idx)
    batch = nifs.hnsw_search_batch(idx, queries, 12, with_keys=True)
    mid = nifs.hnsw_counters(idx)
    assert mid["traversal_launches"] - before["traversal_launches"] == 1 and mid["reruns"] == before["reruns"]
    assert mid["traversals"] - before["traversals"] == 62   # the two invalid queries never reach the device
    lone = [nifs.hnsw_search(idx, q, 12, with_keys=True) for q in queries]
    after = nifs.hnsw_counters(idx)
    assert after["traversal_launches"] - mid["traversal_launches"] == 62
    assert len(batch) == 64
    for b, l in zip(batch, lone):
        if b[0] == "ok":
            b, l = [(i, f32bits(r), k) for i, r, k in b[1]], [(i, f32bits(r), k) for i, r, k in l[1]]
        assert b == l
    assert batch[5] == batch[17] == ("error", "vector contains a non-finite value")
    assert batch[40] == ("error", "metric overflow")
    assert sum(1 for b in batch if b[0] == "ok") >= 60
    # without per-query statuses the first failing query fails the call
    import ctypes as C
    import vettore_amd._lib as L
    outs = (C.c_void_p * 64)()
    q = np.ascontiguousarray(queries)
    st = L.load().vt_hnsw_search_batch(idx.handle, q.ctypes.data_as(C.POINTER(C.c_float)), 64, 16, 12, outs, None)
    assert st == 3 and not any(outs)
    assert nifs.hnsw_search_batch(idx, queries[:0], 12) == []
    assert all(r == ("ok", []) for r in nifs.hnsw_search_batch(idx, queries, 0))   # limit 0 before validation


def test_forced_scratch_overflow_reruns_with_the_same_answers(request, nifs, ref_order, vt_debug):
    """(test_hnsw_scratch_cap, libvettore_hip_hooks.so only: the test re-runs itself there.)"""
    if support.rerun_with_hooks_library(request):
        return
    ids, vecs, p, limit = corpus("600x16")
    ids, vecs = ids[:200], vecs[:200]
    ref = HnswIndex(INNER_PRODUCT, **p)
    ref.insert_many(list(zip(ids, vecs)))
    vt_debug.set("test_hnsw_scratch_cap", 8)
    idx = new_gpu(nifs, INNER_PRODUCT, p)
    assert nifs.hnsw_insert_many(idx, list(zip(ids, vecs))) == ("ok", ())
    assert_same_graph(nifs, idx, ref)
    built = nifs.hnsw_counters(idx)
    assert built["reruns"] > 0
    queries = np.random.default_rng(2).standard_normal((9, 16)).astype(np.float32)
    for q in queries:
        assert_same_search(nifs, idx, ref, q, limit)
    batch = nifs.hnsw_search_batch(idx, queries, limit)
    assert [("ok", [(i, f32bits(r)) for i, r in b[1]]) for b in batch] == [search_both(nifs, idx, ref, q, limit)[1] for q in queries]
    after = nifs.hnsw_counters(idx)
    assert after["reruns"] >= built["reruns"] + 18
    vt_debug.reset("test_hnsw_scratch_cap")
    assert_same_search(nifs, idx, ref, queries[0], limit)
    assert nifs.hnsw_counters(idx)["reruns"] == after["reruns"]


@pytest.mark.parametrize("metric", ["l2", "cosine", "inner_product"])
def test_collection_with_an_hnsw_index(nifs, ref_order, metric):
    from vettore_amd.collection import Collection, Embedding
    from vettore_amd.index_flat import result_values
    code = {"l2": L2, "cosine": COSINE, "inner_product": INNER_PRODUCT}[metric]
    made = Collection.new(dimensions=8, metric=metric, normalize="none", index="hnsw", index_options={"m": 4, "m0": 8, "ef_construction": 30})
    assert made[0] == "ok", made
    col = made[1]
    ref = HnswIndex(code, m=4, m0=8, ef_construction=30)
    rng = np.random.default_rng(31)
    vecs = rng.standard_normal((120, 8)).astype(np.float32)
    embs = [Embedding(id=b"c%03d" % ((i * 37) % 120), vector=[float(x) for x in vecs[i]], value=i) for i in range(120)]
    assert col.put(embs[0]) == "ok"
    ref.insert(embs[0].id, vecs[0])
    assert col.put_many(embs[1:]) == "ok"
    ref.insert_many([(e.id, vecs[i + 1]) for i, e in enumerate(embs[1:])])
    assert col.delete(embs[10].id) == "ok"
    ref.delete(embs[10].id)
    assert_same_graph(nifs, col.index_state, ref)
    for q in (vecs[3], vecs[77]):
        got = col.search([float(x) for x in q], {"limit": 9})
        assert got[0] == "ok"
        want = ref.search(q, 9)
        assert [r.id for r in got[1]] == [i for i, _ in want]
        for r, (_, raw) in zip(got[1], want):
            assert (r.score, r.distance) == result_values(metric, float(raw), "raw")
    assert col.search([1.0] * 8, {"limit": 0}) == ("error", "invalid_limit")
    assert col.index_mod.search(col, [1.0] * 8, {"k": 3}) == ("error", "invalid_search_options")
    assert col.index_mod.search(col, [1.0] * 8, [("limit", 3)]) == ("error", "invalid_search_options")
    # the staged searches stay the flat index's
    assert col.quantized_search([1.0] * 8, {"limit": 3}) == ("error", "not_supported_by_index")
