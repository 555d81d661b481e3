"""The four MMR NIFs of the erl_nif shim (integration/c_src/vettore_gpu_nif.c: mmr_rerank/5, flat_mmr_rerank/4,
flat_mmr_search/6, flat_mmr_search_batch/6) EXECUTED against the real library on the GPU through the fake runtime
(tests/nif_runtime.py), in the manner of tests/test_gpu_hnsw_nif.py: what comes back -- index lists, hit lists, the
library's error strings, ArgumentError -- is compared with the restatement of mmr_rerank/5 (tests/mmr_ref.py)."""
import numpy as np
import pytest

import mmr_ref
import nif_runtime
from nif_runtime import ArgumentError, ERROR, OK

pytestmark = pytest.mark.gpu

UNIT = (OK, ())
CODES = {"l2": 0, "l2_squared": 1, "cosine": 2, "inner_product": 3, "negative_inner_product": 4, "manhattan": 5,
         "chebyshev": 6, "hamming": 7, "jaccard": 8}


@pytest.fixture(scope="module")
def rt():
    import vettore_amd._lib as L
    assert L.load().vt_device_count() >= 1, "no HIP device: GPU tests need the real hardware"
    return nif_runtime.Runtime()


@pytest.fixture
def ref_order(oracle_mod):
    from vettore_amd import nifs
    oracle_mod.set_reduce_order(nifs.debug_get("reduce_order"))
    yield
    oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


def floats(v):
    return [float(x) for x in v]


def bits(hits):
    return [(h[0], np.float32(h[1]).tobytes()) for h in hits]


def case(n, d, seed):
    rng = np.random.default_rng(seed)
    rows = rng.normal(size=(n, d)).astype(np.float32)
    return rows, floats(rng.uniform(-1, 1, size=n))


def test_the_table_holds_the_four_nifs(rt):
    funcs = rt.functions()
    for name, arity in (("mmr_rerank", 5), ("flat_mmr_rerank", 4), ("flat_mmr_search", 6), ("flat_mmr_search_batch", 6)):
        assert (name, arity) in funcs, name
        assert funcs[(name, arity)] != 0   # a dirty scheduler: every call waits for the device


@pytest.mark.parametrize("metric", ["l2", "cosine", "inner_product", "jaccard"])
def test_stateless_rerank_through_the_shim(rt, ref_order, metric):
    rows, scores = case(33, 9, 5)
    for alpha, k in ((0.5, 33), (0.3, 4), (1.0, 40), (0.0, 1)):
        want = mmr_ref.order_of_rows(rows.tolist(), scores, metric, alpha, k)
        assert rt.call("mmr_rerank", CODES[metric], [floats(r) for r in rows], scores, alpha, k) == (OK, want[1]), (alpha, k)


def test_stateless_rerank_errors_and_bad_terms(rt, ref_order):
    rows, scores = case(4, 3, 6)
    mat = [floats(r) for r in rows]
    assert rt.call("mmr_rerank", 0, [], [], 0.5, 3) == (OK, [])
    assert rt.call("mmr_rerank", 0, mat, scores, 1.5, 3) == (ERROR, b"invalid mmr args")
    assert rt.call("mmr_rerank", 0, mat, scores, 0.5, 0) == (ERROR, b"invalid mmr args")
    assert rt.call("mmr_rerank", 0, mat, [1.0, 2.0, 3.0, float("inf")], 0.5, 2) == (ERROR, b"invalid mmr args")
    assert rt.call("mmr_rerank", 77, mat, scores, 0.5, 2) == (ERROR, b"unknown metric")
    assert rt.call("mmr_rerank", 0, [[1.0], [1.0, 2.0]], [1.0, 2.0], 0.5, 2) == (ERROR, b"dimension mismatch")
    assert rt.call("mmr_rerank", 1, [[1.5e19], [-1.5e19]], [1.0, 0.5], 0.5, 2) == (ERROR, b"metric overflow")
    assert rt.call("mmr_rerank", 1, [[1.5e19], [-1.5e19]], [1.0, 0.5], 0.5, 1) == (OK, [0])
    for bad in ((0, mat, scores[:3], 0.5, 2), (0, mat, scores, 1, 2), (0, mat, [1, 2, 3, 4], 0.5, 2), (0, mat, scores, 0.5, -1),
                (0, nif_runtime.Atom("rows"), scores, 0.5, 2), (0.5, mat, scores, 0.5, 2)):
        with pytest.raises(ArgumentError):
            rt.call("mmr_rerank", *bad)


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_resident_rerank_and_search_through_the_shim(rt, ref_order, metric):
    from vettore_amd.index_flat import result_values
    rows, _ = case(120, 8, 9)
    ids = [b"row%03d" % i for i in range(120)]
    ref = rt.call("flat_new", CODES[metric], [0])
    assert isinstance(ref, nif_runtime.Resource)
    assert rt.call("flat_insert_many", ref, [(i, floats(r)) for i, r in zip(ids, rows)]) == UNIT
    assert rt.call("flat_delete", ref, ids[0]) == UNIT          # the last row moves into row 0
    vectors = {ids[i]: rows[i] for i in range(1, 120)}
    embeddings = [(i, floats(v)) for i, v in vectors.items()]
    rng = np.random.default_rng(4)
    pick = [ids[i] for i in 1 + rng.permutation(119)[:25]]
    initial = [(i, float(s)) for i, s in zip(pick, rng.uniform(0, 1, size=25))]
    for alpha, k in ((0.5, 25), (0.2, 6), (1.0, 30)):
        want = mmr_ref.order_of(initial, embeddings, metric, alpha, k)
        assert rt.call("flat_mmr_rerank", ref, initial, alpha, k) == (OK, want[1]), (alpha, k)
    assert rt.call("flat_mmr_rerank", ref, [], 0.5, 3) == (OK, [])
    assert rt.call("flat_mmr_rerank", ref, initial + [(ids[0], 0.5)], 0.5, 3) == (ERROR, b"invalid mmr args")
    assert rt.call("flat_mmr_rerank", ref, initial + [initial[0]], 0.5, 3) == (ERROR, b"invalid mmr args")
    assert rt.call("flat_mmr_rerank", ref, initial, 2.0, 3) == (ERROR, b"invalid mmr args")
    for bad in ((ref, [(b"row001", 1)], 0.5, 3), (ref, [b"row001"], 0.5, 3), (ref, initial, 1, 3), (b"ref", initial, 0.5, 3)):
        with pytest.raises(ArgumentError):
            rt.call("flat_mmr_rerank", *bad)
    queries = [floats(q) for q in rng.normal(size=(3, 8))]
    for mode, mode_name in ((0, "raw"), (1, "similarity")):
        lone = []
        for q in queries:
            found = rt.call("flat_search", ref, q, 30)
            got = rt.call("flat_mmr_search", ref, q, 30, 7, 0.4, mode)
            assert got[0] == OK and bits(got[1][0]) == bits(found[1])
            init = [(i, result_values(metric, raw, mode_name)[0]) for i, raw in found[1]]
            want = mmr_ref.order_of(init, [(i, floats(vectors[i])) for i, _ in found[1]], metric, 0.4, 7)
            assert got[1][1] == want[1]
            lone.append((bits(got[1][0]), got[1][1]))
        batch = rt.call("flat_mmr_search_batch", ref, queries, 30, 7, 0.4, mode)
        assert batch[0] == OK and [(b[0], bits(b[1][0]), b[1][1]) for b in batch[1]] == [(OK, h, o) for h, o in lone]
    assert rt.call("flat_mmr_search_batch", ref, [], 30, 7, 0.4, 0) == (OK, [])
    assert rt.call("flat_mmr_search", ref, queries[0], 30, 0, 0.4, 0) == (ERROR, b"invalid mmr args")
    assert rt.call("flat_mmr_search", ref, queries[0], 30, 7, 0.4, 5) == (ERROR, b"invalid mmr args")
    assert rt.call("flat_mmr_search", ref, queries[0][:3], 30, 7, 0.4, 0) == (ERROR, b"dimension mismatch")
    assert rt.call("flat_mmr_search_batch", ref, [queries[0], queries[1][:3]], 30, 7, 0.4, 0) == (ERROR, b"dimension mismatch")
    with pytest.raises(ArgumentError):
        rt.call("flat_mmr_search", ref, queries[0], 30, 7, 1, 0)
    sharded = rt.call("flat_new", CODES[metric], [0, 0])
    assert rt.call("flat_insert_many", sharded, [(i, floats(r)) for i, r in zip(ids[:5], rows[:5])]) == UNIT
    res = rt.call("flat_mmr_rerank", sharded, [(ids[1], 0.5)], 0.5, 1)
    assert res[0] == ERROR and b"sharded" in res[1]
