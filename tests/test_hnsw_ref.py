"""tests/hnsw_ref.py pinned to the reference's own tests (native/vettore/src/hnsw.rs:523-795): what the GPU index is
held to is the restatement, so the restatement is held to what the reference asserts of itself.  CPU only."""
import math

import numpy as np
import pytest

import oracle
from hnsw_ref import COSINE, INNER_PRODUCT, L2, HnswError, HnswIndex, hash64, total_key
from support import load

GOLD = load("hnsw_rs.json")
PARAMS = GOLD["params"]


def make(metric, **over):
    return HnswIndex(metric, **dict(PARAMS, **over))


def test_validates_parameters():
    make(L2)
    assert len(GOLD["invalid"]) == 11
    for over, message in GOLD["invalid"]:
        with pytest.raises(HnswError) as e:
            make(L2, **over)
        assert str(e.value) == message, over


def test_every_inserted_node_remains_reachable():
    index = make(L2)
    index.insert_many([("%03d" % v, [float(v)]) for v in range(100)])
    hits = index.search([99.0], 100)
    assert len(hits) == 100 and len({i for i, _ in hits}) == 100
    for v in range(100):
        assert index.search([float(v)], 1)[0][0] == b"%03d" % v


def test_batch_validation_is_atomic_and_replace_delete_work():
    index = make(INNER_PRODUCT)
    index.insert("a", [1.0, 0.0])
    with pytest.raises(HnswError) as e:
        index.insert_many([("b", [0.0, 1.0]), ("bad", [1.0])])
    assert str(e.value) == "dimension mismatch"
    assert len(index.nodes) == 1
    index.insert("a", [0.0, 1.0])
    assert index.search([0.0, 1.0], 1)[0][0] == b"a"
    index.delete("a")
    assert index.search([0.0, 1.0], 1) == []
    assert index.dimension is None
    assert index.next == 2  # internal ids are never reused


def test_rejects_non_finite_and_mismatched_vectors():
    index = make(COSINE)
    for call, message in [
        (lambda: index.insert("empty", []), "vector must not be empty"),
        (lambda: index.insert("a", [1.0, 0.0]), None),
        (lambda: index.insert("short", [1.0]), "dimension mismatch"),
        (lambda: index.insert("nan", [math.nan, 0.0]), "vector contains a non-finite value"),
        (lambda: index.search([1.0], 1), "dimension mismatch"),
        (lambda: index.search([math.inf, 0.0], 1), "vector contains a non-finite value"),
    ]:
        if message is None:
            call()
            continue
        with pytest.raises(HnswError) as e:
            call()
        assert str(e.value) == message


def test_empty_index_paths():
    empty = make(L2)
    assert empty.search([1.0], 10) == []
    with pytest.raises(HnswError):
        empty.search([], 10)
    assert empty.search([], 0) == []  # limit 0 before validation
    assert empty.search_layer(999, np.float32([1.0]), 0, 10) == []
    index = make(L2)
    index.insert("a", [1.0])
    index.prune(999, 0)
    index.prune(index.entry, 999)


def test_heap_orders_use_distance_then_id():
    assert (total_key(2.0), 1) < (total_key(2.0), 2)
    assert total_key(-0.0) < total_key(0.0) and not (-0.0 < 0.0)
    assert total_key(-1.0) < total_key(-0.0) < total_key(1e-30) < total_key(float("inf"))


def test_high_ef_search_matches_exact_l2_on_a_grid():
    index = make(L2)
    vectors = [("%02d-%02d" % (x, y), [float(x), float(y)]) for x in range(15) for y in range(15)]
    index.insert_many(vectors)
    for query in GOLD["grid_queries"]:
        expected = [(i.encode(), oracle.compute(L2, query, v)) for i, v in vectors]
        expected.sort(key=lambda h: (total_key(h[1]), h[0]))
        got = index.search(query, 20)
        assert [(i, np.float32(r).tobytes()) for i, r in got] == [(i, np.float32(r).tobytes()) for i, r in expected[:20]]


def test_self_queries_recall_every_unit_vector():
    vectors = []
    for k in range(64):
        angle = np.float32(np.float32(2.0 * math.pi) * np.float32(k) / np.float32(64.0))
        vectors.append(("unit-%02d" % k, [np.cos(angle, dtype=np.float32), np.sin(angle, dtype=np.float32)]))
    for metric in (COSINE, INNER_PRODUCT):
        index = make(metric)
        index.insert_many(vectors)
        for i, v in vectors:
            assert index.search(v, 1)[0][0] == i.encode()


def test_graph_degrees_and_references_remain_well_formed():
    index = make(L2)
    index.insert_many([("node-%03d" % v, [np.sin(np.float32(v)), np.cos(np.float32(v)), np.float32(v) / np.float32(300.0)])
                       for v in range(300)])
    for node_id, node in index.nodes.items():
        for layer, connections in enumerate(node.connections):
            assert len(connections) <= (index.m0 if layer == 0 else index.m)
            assert len(set(connections)) == len(connections)
            assert node_id not in connections
            assert all(i in index.nodes for i in connections)
    hits = index.search([0.0, 1.0, 0.5], 1000)
    assert len(hits) == len(index.nodes) == len({i for i, _ in hits})


def test_deleting_an_entry_selects_a_deterministic_replacement():
    index = make(L2)
    index.insert_many([("id-%02d" % v, [float(v)]) for v in range(80)])
    old_entry = index.entry
    old_id = index.nodes[old_entry].external_id
    index.delete("missing")
    assert index.entry == old_entry
    index.delete(old_id)
    top = max(n.layer for n in index.nodes.values())
    expected = min(n.external_id for n in index.nodes.values() if n.layer == top)
    assert index.nodes[index.entry].external_id == expected
    assert index.search([0.0], 0) == []


def test_level_assignment_is_bounded_and_seedless():
    first, second = make(L2), make(L2)
    for i in GOLD["level_ids"]:
        b = i.encode()
        assert first.level_for(b) == second.level_for(b) <= first.max_level
    assert hash64(b"") == 0xCBF29CE484222325
    assert hash64(b"a") == 0xAF63DC4C8601EC8C  # FNV-1a's published test vector
    one = HnswIndex(L2, max_level=1)
    assert max(one.level_for(b"%d" % k) for k in range(200)) == 1
