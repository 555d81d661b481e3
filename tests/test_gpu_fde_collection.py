"""A Collection with `resident_multi_vector` and `muvera` (vettore_amd/collection.py) -- `-m gpu`: after every put,
put_many, delete and rolled-back put_many, muvera_search and muvera_search_batch return the composition of the three
reference models (tests/muvera_ref.py, the oracle's FlatIndex, tests/maxsim_ref.py) over col.all()."""
import numpy as np
import pytest

import maxsim_ref
import muvera_ref
from test_gpu_parity import nifs  # noqa: F401  (a fixture)
from test_gpu_mv_store import ref_order  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

D = 6
MUVERA = {"num_repetitions": 3, "num_simhash_projections": 3, "seed": 11, "projection_dimension": 4}
CFG = (D, 3, 3, 11, 4, None)
FMAX = float(np.finfo(np.float32).max)


def vecs(rng, n):
    return [list(map(float, r)) for r in rng.uniform(-1, 1, size=(n, D)).astype(np.float32)]


def make(**extra):
    from vettore_amd.collection import Collection
    options = {"resident_multi_vector": True, "muvera": dict(MUVERA)}
    options.update(extra)
    return Collection.new(dimensions=D, metric="inner_product", normalize="none", index_options=options)


def composition(oracle_mod, col, query, metric, limit, candidates):
    docs = [(e.id, e.vectors if e.vectors else [e.vector]) for e in col.all()[1]]
    rows = {i: muvera_ref.encode_document(v, *CFG) for i, v in docs}
    good = [(i, r[1]) for i, r in rows.items() if r[0] == "ok"]
    if not good:
        return []
    ix = oracle_mod.FlatIndex(3)
    ix.insert_matrix([i for i, _ in good], np.stack([r for _, r in good]))
    q = muvera_ref.encode_query(query, *CFG)
    assert q[0] == "ok"
    found = {i for i, _ in ix.search(q[1], candidates)}
    return maxsim_ref.top_k([(i, v) for i, v in docs if i in found], query, nifs_metric(metric), limit)


def nifs_metric(name):
    from vettore_amd import nifs as n
    return n.METRIC_CODE[name]


def check(oracle_mod, col, rng, ctx):
    queries = [vecs(rng, n) for n in (3, 1, 5)]
    for opts, metric, limit, candidates in (({"limit": 4, "candidates": 9}, "inner_product", 4, 9),
                                            ({"limit": 3, "metric": "cosine"}, "cosine", 3, 30),
                                            (None, "inner_product", 10, 100)):
        want = [composition(oracle_mod, col, q, metric, limit, candidates) for q in queries]
        lone = [col.muvera_search(q, opts) for q in queries]
        for res, w in zip(lone, want):
            assert res[0] == "ok", (ctx, res)
            assert [r.id for r in res[1]] == [h[0] for h in w], (ctx, opts)
            assert [np.float32(r.score).tobytes() for r in res[1]] == [np.float32(h[1]).tobytes() for h in w], (ctx, opts)
            assert all(r.metric == metric and r.distance is None and r.value == col.store[r.id].value for r in res[1])
        mixed = queries + [[], [[1.0] * (D - 1)], "nonsense"]
        batch = col.muvera_search_batch(mixed, opts)
        assert batch == lone + [col.muvera_search(q, opts) for q in mixed[3:]], (ctx, opts)
        assert [b[0] for b in batch[3:]] == ["error"] * 3


def test_collection_follows_its_store(nifs, oracle_mod, ref_order):
    from vettore_amd.collection import Embedding
    rng = np.random.default_rng(606)
    status, col = make()
    assert status == "ok" and col.fde_index is not None and col.muvera_config == CFG
    assert col.muvera_search(vecs(rng, 2)) == ("ok", [])

    def embedding(i):
        v = vecs(rng, int(rng.integers(1, 9)))
        return Embedding(id="e%03d" % i, vector=v[0]) if i % 4 == 0 else Embedding(id="e%03d" % i, vectors=v)

    assert col.put(embedding(0)) == "ok" and col.put(embedding(1)) == "ok"
    assert len(col.fde_index) == 2
    check(oracle_mod, col, rng, "put")
    assert col.put_many([embedding(i) for i in range(2, 60)]) == "ok"
    assert len(col.fde_index) == 60
    check(oracle_mod, col, rng, "put_many")
    # a duplicate id inside the batch, and one that is stored already: nothing changes
    assert col.put_many([embedding(60), embedding(61), embedding(60)]) == ("error", "duplicate_id")
    assert col.put_many([embedding(62), embedding(5)]) == ("error", "duplicate_id")
    assert len(col.fde_index) == 60 and len(col.mv_store) == 60
    # an embedding whose encoding overflows is stored, and absent from the FDE index
    assert col.put(Embedding(id="ovf", vectors=[[FMAX] * D] * 3)) == "ok"
    assert muvera_ref.encode_document([[FMAX] * D] * 3, *CFG) == ("error", "encoding overflow")
    assert len(col.fde_index) == 60 and len(col.mv_store) == 61
    assert col.delete("ovf") == "ok"
    for i in (0, 7, 33):
        assert col.delete("e%03d" % i) == "ok"
    assert col.delete("never-there") == "ok" or col.delete("never-there")[0] == "error"
    assert len(col.fde_index) == 57 and len(col.mv_store) == 57
    check(oracle_mod, col, rng, "delete")
    # a put_many that fails behind the store's put (the sync reports a failure once its rows are in): rolled back everywhere
    real, calls = col.mv_store.fde_sync, []

    def failing(index, ids, cfg):
        calls.append(list(ids))
        res = real(index, ids, cfg)
        return ("error", "device error") if len(calls) == 1 else res
    col.mv_store.fde_sync = failing
    try:
        assert col.put_many([embedding(i) for i in range(70, 75)]) == ("error", "device error")
    finally:
        del col.mv_store.fde_sync
    assert len(calls) == 2 and calls[0] == calls[1] == [b"e%03d" % i for i in range(70, 75)]
    assert len(col.fde_index) == 57 and len(col.mv_store) == 57 and len(col.all()[1]) == 57
    check(oracle_mod, col, rng, "rollback")
    assert col.put_many([embedding(i) for i in range(70, 75)]) == "ok" and len(col.fde_index) == 62
    check(oracle_mod, col, rng, "after the rollback")


def test_options(nifs):
    from vettore_amd.collection import Collection
    rng = np.random.default_rng(607)
    q = vecs(rng, 2)
    # only beside resident_multi_vector: true, and only a well-formed configuration of the collection's dimension
    for options in ({"muvera": dict(MUVERA)}, {"resident_multi_vector": False, "muvera": dict(MUVERA)},
                    {"resident_multi_vector": True, "muvera": {"num_repetitions": 0}},
                    {"resident_multi_vector": True, "muvera": {"dimension": D + 1}},
                    {"resident_multi_vector": True, "muvera": {"repetitions": 3}},
                    {"resident_multi_vector": True, "muvera": 5}):
        assert Collection.new(dimensions=D, metric="inner_product", index_options=options) == ("error", "invalid_index_options"), options
    # the reference's defaults (muvera.ex:83-94): one repetition, no SimHash, seed 1, the identity projection
    status, col = Collection.new(dimensions=D, metric="inner_product", normalize="none",
                                 index_options={"resident_multi_vector": True, "muvera": {}})
    assert status == "ok" and col.muvera_config == (D, 1, 0, 1, D, None)
    # without the option: as before, and the new searches say so
    for options in (None, {"resident_multi_vector": True}):
        status, plain = Collection.new(dimensions=D, metric="inner_product", normalize="none", index_options=options)
        assert status == "ok" and plain.fde_index is None
        assert plain.muvera_search(q) == ("error", "muvera_not_configured")
        assert plain.muvera_search_batch([q]) == ("error", "muvera_not_configured")
    status, col = make()
    assert status == "ok"
    assert col.muvera_search(q, "nonsense") == ("error", "invalid_options")
    assert col.muvera_search(q, {"stages": [1]}) == ("error", ("unsupported_option", "stages"))
    assert col.muvera_search(q, {"limit": 0}) == ("error", "invalid_limit")
    assert col.muvera_search(q, {"metric": "nope"}) == ("error", "invalid_metric")
    assert col.muvera_search(q, {"limit": 5, "candidates": 4}) == ("error", "invalid_candidates")
    assert col.muvera_search(q, {"candidates": True}) == ("error", "invalid_candidates")
    assert col.muvera_search([], None) == ("error", "invalid_multi_vector")
    assert col.muvera_search_batch("nonsense") == ("error", "invalid_multi_vector")
    assert col.muvera_search_batch([q, q], {"limit": 0}) == [("error", "invalid_limit")] * 2
