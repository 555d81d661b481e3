"""Collection.rerank / mmr_search / mmr_search_batch (vettore_amd/collection.py) -- `-m gpu`: Vettore.rerank/4 and the
diversified search over it, on a flat collection (the resident rows), on a sharded flat and an HNSW collection (the
stateless route with vectors from the store).  Every answer equals the restatement's (tests/mmr_ref.py) over the
collection's stored vectors."""
import numpy as np
import pytest

import mmr_ref
from test_gpu_parity import nifs  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture
def ref_order(nifs, oracle_mod):
    oracle_mod.set_reduce_order(nifs.debug_get("reduce_order"))
    yield
    oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


def make(nifs, metric, index="flat", index_options=None, score="raw", n=80, d=8, seed=3):
    from vettore_amd.collection import Collection, Embedding
    made = Collection.new(dimensions=d, metric=metric, index=index, index_options=index_options, score=score)
    assert made[0] == "ok", made
    col = made[1]
    rng = np.random.default_rng(seed)
    embs = [Embedding(id="doc%03d" % i, vector=[float(v) for v in rng.normal(size=d)], metadata={"i": i}) for i in range(n)]
    assert col.put_many(embs) == "ok"
    return col


def restated(col, initial, alpha, limit):
    pairs = [(i, [float(v) for v in e.vector]) for i, e in col.store.items()]
    conv = [(nifs_bytes(i), s) for i, s in initial]
    res = mmr_ref.mmr_rerank(conv, pairs, col.metric, alpha, limit)
    if res[0] != "ok":
        return res
    place = {e[0]: i for i, e in enumerate(conv)}
    return ("ok", [initial[place[i]] for i, _ in res[1]])


def nifs_bytes(x):
    return x.encode() if isinstance(x, str) else x


@pytest.mark.parametrize("metric,index,options", [("cosine", "flat", None), ("l2", "flat", None), ("l2", "flat", {"devices": [0, 0]}),
                                                  ("cosine", "hnsw", {"m": 4, "m0": 8, "ef_construction": 30}),
                                                  ("inner_product", "hnsw", {"m": 4, "m0": 8, "ef_construction": 30})])
def test_rerank_equals_the_reference_over_the_stored_vectors(nifs, ref_order, metric, index, options):
    col = make(nifs, metric, index, options)
    rng = np.random.default_rng(9)
    pick = ["doc%03d" % i for i in rng.permutation(80)[:30]]
    initial = [(i, float(s)) for i, s in zip(pick, rng.uniform(0, 1, size=30))]
    for opts in (None, {"limit": 30}, {"limit": 4, "alpha": 0.2}, {"alpha": 1}, {"limit": 99, "alpha": 0}):
        o = opts or {}
        got = col.rerank(initial, opts)
        assert got == restated(col, initial, o.get("alpha", 0.5), o.get("limit", 10)), opts
        assert all(any(g is e for e in initial) for g in got[1])
    assert col.rerank([], None) == ("ok", [])
    assert col.delete("doc%03d" % int(pick[0][3:])) == "ok"
    assert col.rerank(initial, None) == ("error", "invalid_mmr_args")      # an id the collection no longer holds
    assert col.rerank(initial[1:], None) == restated(col, initial[1:], 0.5, 10)


def test_rerank_option_and_argument_errors(nifs):
    col = make(nifs, "l2", n=5)
    ok = [("doc001", 0.5), ("doc002", 0.4)]
    assert col.rerank(ok, {"unknown": True}) == ("error", "invalid_options")
    assert col.rerank(ok, ["limit"]) == ("error", "invalid_arguments")
    assert col.rerank("doc001", None) == ("error", "invalid_arguments")
    inv = ("error", "invalid_mmr_args")
    assert col.rerank(ok, {"alpha": 1.5}) == inv
    assert col.rerank(ok, {"limit": 0}) == inv
    assert col.rerank(ok, {"limit": 2.0}) == inv
    assert col.rerank(ok + [ok[0]], None) == inv
    assert col.rerank([("nope", 0.5)], None) == inv
    assert col.rerank([("doc001", float("nan"))], None) == inv
    assert col.rerank(["doc001"], None) == inv
    hn = make(nifs, "l2", "hnsw", {"m": 4, "m0": 8, "ef_construction": 30}, n=5)
    for bad in ({"alpha": 1.5}, {"limit": 0}):
        assert hn.rerank(ok, bad) == inv
    assert hn.rerank(ok + [ok[0]], None) == inv and hn.rerank([("nope", 0.5)], None) == inv
    assert hn.rerank(ok, {"unknown": True}) == ("error", "invalid_options")


@pytest.mark.parametrize("metric,score", [("cosine", "raw"), ("cosine", "similarity"), ("l2", "similarity"), ("manhattan", "raw")])
def test_mmr_search_is_search_then_rerank(nifs, ref_order, metric, score):
    col = make(nifs, metric, score=score, n=120)
    rng = np.random.default_rng(2)
    queries = [[float(v) for v in rng.normal(size=8)] for _ in range(4)]
    for opts in ({}, {"limit": 5}, {"limit": 7, "candidates": 40, "alpha": 0.3}, {"limit": 20, "candidates": 20, "alpha": 1}):
        limit = opts.get("limit", 10)
        candidates = opts.get("candidates", max(limit * 10, limit))
        lone = []
        for q in queries:
            found = col.search(q, {"limit": candidates})
            assert found[0] == "ok"
            want = restated(col, [(r.id, r.score) for r in found[1]], opts.get("alpha", 0.5), limit)
            got = col.mmr_search(q, opts)
            assert got[0] == "ok" and [(r.id, r.score) for r in got[1]] == want[1], opts
            by_id = {r.id: r for r in found[1]}
            assert got[1] == [by_id[r.id] for r in got[1]]   # whole Results, as search hands them out
            lone.append(got)
        assert col.mmr_search_batch(queries, opts) == ("ok", lone)
    assert col.mmr_search_batch([], {}) == ("ok", [])


def test_mmr_search_option_errors_and_other_indexes(nifs, ref_order):
    col = make(nifs, "l2", n=30)
    q = [0.5] * 8
    assert col.mmr_search(q, {"stages": [4]}) == ("error", ("unsupported_option", "stages"))
    assert col.mmr_search(q, ["limit"]) == ("error", "invalid_options")
    assert col.mmr_search(q, {"limit": 0}) == ("error", "invalid_limit")
    assert col.mmr_search(q, {"limit": 5, "candidates": 3}) == ("error", "invalid_candidates")
    assert col.mmr_search(q, {"alpha": -1}) == ("error", "invalid_mmr_args")
    assert col.mmr_search(q[:3], {}) == ("error", "dimension_mismatch")
    assert col.mmr_search_batch([q], {"alpha": 2}) == ("error", "invalid_mmr_args")
    assert col.mmr_search_batch([q], {"nope": 1}) == ("error", ("unsupported_option", "nope"))
    # a sharded flat and an HNSW collection compose the same call from search and rerank
    for index, options in (("flat", {"devices": [0, 0]}), ("hnsw", {"m": 4, "m0": 8, "ef_construction": 30})):
        other = make(nifs, "l2", index, options, n=30)
        found = other.search(q, {"limit": 12})
        want = restated(other, [(r.id, r.score) for r in found[1]], 0.4, 6)
        got = other.mmr_search(q, {"limit": 6, "candidates": 12, "alpha": 0.4})
        assert got[0] == "ok" and [(r.id, r.score) for r in got[1]] == want[1]
        assert other.mmr_search_batch([q, q], {"limit": 6, "candidates": 12, "alpha": 0.4}) == ("ok", [got, got])
        assert other.mmr_search(q, {"alpha": 7}) == ("error", "invalid_mmr_args")
