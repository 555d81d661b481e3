"""The HNSW index gives the rows of deleted nodes back (host/vt_hnswplan.h: the rule; K11c in vt_hnsw.hip: the move) --
`-m gpu`.  An insert that finds more dead rows than live ones, and at least 64 of them, first gathers the survivors into
a fresh slab and mirror with every list entry renumbered; a delete never does.  As in tests/test_gpu_hnsw.py everything is
equality with the restatement (tests/hnsw_ref.py): the graph and the hits do not know that rows moved.  What shows is
vt_hnsw_memory: `rows` falls to the live count, `dead_rows` to 0, `row_capacity` may shrink."""
import numpy as np
import pytest

import hnsw_ref
import support  # noqa: F401  (the suite's helpers: imported as test_gpu_hnsw.py does)
from hnsw_ref import COSINE, INNER_PRODUCT, L2, HnswIndex
from test_gpu_hnsw import assert_same_graph, assert_same_search, f32bits, new_gpu, params, ref_order, search_both  # noqa: F401
from test_gpu_parity import nifs  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

D = 6
P = params(4, 8, 24, 12)


def edges_of(ref):
    return sum(len(l) for n in ref.nodes.values() for l in n.connections)


def churned(nifs, metric):
    """200 inserts, then 130 deletes that take the entry and a node above layer 0 and leave a node on layer 2 or above:
    (index, restatement, live ids, rng) with 130 dead rows and no compaction yet."""
    rng = np.random.default_rng(101)
    ids = [b"c%d" % ((i * 7919) % 100003) for i in range(200)]
    vecs = rng.standard_normal((200, D)).astype(np.float32)
    ref = HnswIndex(metric, **P)
    idx = new_gpu(nifs, metric, P)
    ref.insert_many(list(zip(ids, vecs)))
    assert nifs.hnsw_insert_many(idx, list(zip(ids, vecs))) == ("ok", ())
    level = {i: ref.level_for(i) for i in ids}
    entry = ref.nodes[ref.entry].external_id
    keep = next(i for i in ids if level[i] >= 2 and i != entry)
    others = [i for i in ids if i not in (entry, keep)]
    doomed = [entry] + [others[k] for k in rng.permutation(len(others))[:129]]
    survivors = [i for i in ids if i not in set(doomed)]
    assert len(doomed) == 130 and len(survivors) == 70
    assert entry in doomed and any(level[i] >= 1 for i in doomed) and any(level[i] >= 2 for i in survivors)
    for ext in doomed:
        ref.delete(ext)
        assert nifs.hnsw_delete(idx, ext) == ("ok", ())
    return idx, ref, survivors, rng


@pytest.mark.parametrize("metric", [L2, COSINE, INNER_PRODUCT])
def test_an_insert_compacts_when_the_dead_outnumber_the_live(nifs, ref_order, metric):
    idx, ref, live, rng = churned(nifs, metric)
    mem = nifs.hnsw_memory(idx)
    assert (mem["rows"], mem["dead_rows"], mem["row_capacity"]) == (200, 130, 1024)   # deletes do not compact
    assert_same_graph(nifs, idx, ref)
    v = rng.standard_normal(D).astype(np.float32)
    ref.insert(b"one-more", v)
    assert nifs.hnsw_insert(idx, b"one-more", v) == ("ok", ())
    mem = nifs.hnsw_memory(idx)
    assert (mem["rows"], mem["dead_rows"], mem["row_capacity"]) == (71, 0, 1024)
    assert mem["edges"] == edges_of(ref)
    assert_same_graph(nifs, idx, ref)
    for q in rng.standard_normal((10, D)).astype(np.float32):
        for limit in (1, 5, 70):
            assert_same_search(nifs, idx, ref, q, limit)


def test_life_goes_on_across_several_compactions(nifs, ref_order):
    idx, ref, live, rng = churned(nifs, COSINE)
    rows_seen = [nifs.hnsw_memory(idx)["rows"]]

    def after_step():
        mem = nifs.hnsw_memory(idx)
        rows_seen.append(mem["rows"])
        assert mem["rows"] - mem["dead_rows"] == len(live) == len(ref.nodes)
        assert mem["dead_rows"] <= max(len(live), 63) + 1, (mem, len(live))

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

    # the insert that closes the first test's sequence: 200 rows become 71, the first fall
    both_insert(b"one-more", rng.standard_normal(D).astype(np.float32))
    after_step()
    assert rows_seen == [200, 71]
    # then test_gpu_hnsw.py's random interleaving, with new ids from a pool of 100 so that upserts keep the dead rows coming:
    # about 0.4 erasures a step against some 100 live nodes make the next compaction due after some 250 steps
    for step in range(300):
        r = rng.random()
        if r < 0.45 or len(live) < 5:
            both_insert(b"m%d" % int(rng.integers(0, 100)), rng.standard_normal(D).astype(np.float32))
        elif r < 0.6:
            both_insert(live[int(rng.integers(0, len(live)))], rng.standard_normal(D).astype(np.float32))
        elif r < 0.8:
            both_delete(live[int(rng.integers(0, len(live)))] if rng.random() < 0.8 else ref.nodes[ref.entry].external_id)
        else:
            assert_same_search(nifs, idx, ref, rng.standard_normal(D).astype(np.float32), int(rng.integers(1, 20)))
        after_step()
        if step % 50 == 49:
            assert_same_graph(nifs, idx, ref)
    assert_same_graph(nifs, idx, ref)
    falls = sum(1 for a, b in zip(rows_seen, rows_seen[1:]) if b < a)
    assert falls >= 2, rows_seen
    assert nifs.hnsw_memory(idx)["edges"] == edges_of(ref)


def test_the_slab_shrinks(nifs, ref_order):
    p = params(2, 4, 4)
    rng = np.random.default_rng(202)
    ids = [b"s%d" % ((i * 7919) % 100003) for i in range(1100)]
    vecs = rng.standard_normal((1100, 4)).astype(np.float32)
    ref = HnswIndex(L2, **p)
    idx = new_gpu(nifs, L2, p)
    ref.insert_many(list(zip(ids, vecs)))
    assert nifs.hnsw_insert_many(idx, list(zip(ids, vecs))) == ("ok", ())
    assert nifs.hnsw_memory(idx)["row_capacity"] == 2048
    for ext in ids[:900]:
        ref.delete(ext)
        assert nifs.hnsw_delete(idx, ext) == ("ok", ())
    mem = nifs.hnsw_memory(idx)
    assert (mem["rows"], mem["dead_rows"], mem["row_capacity"]) == (1100, 900, 2048)
    v = rng.standard_normal(4).astype(np.float32)
    ref.insert(b"after", v)
    assert nifs.hnsw_insert(idx, b"after", v) == ("ok", ())
    mem = nifs.hnsw_memory(idx)
    assert (mem["rows"], mem["dead_rows"], mem["row_capacity"]) == (201, 0, 1024)
    assert mem["edges"] == edges_of(ref)
    assert_same_graph(nifs, idx, ref)
    queries = rng.standard_normal((10, 4)).astype(np.float32)
    lone = []
    for q in queries:
        got, want = search_both(nifs, idx, ref, q, 10)
        assert got == want
        lone.append(got)
    batch = nifs.hnsw_search_batch(idx, queries, 10)
    assert [("ok", [(i, f32bits(r)) for i, r in b[1]]) for b in batch] == lone


def test_a_compaction_between_two_inserts_of_one_call(nifs, ref_order):
    rng = np.random.default_rng(303)
    ids = [b"u%d" % ((i * 7919) % 100003) for i in range(230)]
    vecs = rng.standard_normal((230, D)).astype(np.float32)
    ref = HnswIndex(INNER_PRODUCT, **P)
    idx = new_gpu(nifs, INNER_PRODUCT, P)
    ref.insert_many(list(zip(ids, vecs)))
    assert nifs.hnsw_insert_many(idx, list(zip(ids, vecs))) == ("ok", ())
    for ext in ids[150:]:
        ref.delete(ext)
        assert nifs.hnsw_delete(idx, ext) == ("ok", ())
    mem = nifs.hnsw_memory(idx)
    assert (mem["rows"], mem["dead_rows"]) == (230, 80)
    # 150 upserts in one call: the 70th erasure makes 150 dead rows beside 149 live ones, and its insert compacts first
    again = rng.standard_normal((150, D)).astype(np.float32)
    ref.insert_many(list(zip(ids[:150], again)))
    assert nifs.hnsw_insert_many(idx, list(zip(ids[:150], again))) == ("ok", ())
    mem = nifs.hnsw_memory(idx)
    assert (mem["rows"], mem["dead_rows"], mem["row_capacity"]) == (230, 80, 1024) and mem["dead_rows"] < 150
    assert mem["edges"] == edges_of(ref)
    assert_same_graph(nifs, idx, ref)
    for q in rng.standard_normal((5, D)).astype(np.float32):
        for limit in (1, 10, 150):
            assert_same_search(nifs, idx, ref, q, limit)


def test_a_collection_reports_its_memory(nifs, ref_order):
    from vettore_amd.collection import Collection, Embedding
    from vettore_amd.index_hnsw import DEFAULT_OPTIONS, HnswGpu
    made = Collection.new(dimensions=D, metric="cosine", index="hnsw")
    assert made[0] == "ok", made
    col = made[1]
    ref = HnswIndex(COSINE, **DEFAULT_OPTIONS)
    rng = np.random.default_rng(404)
    vecs = rng.standard_normal((151, D)).astype(np.float32)
    embs = [Embedding(id=b"c%03d" % ((i * 37) % 151), vector=[float(x) for x in vecs[i]], value=i) for i in range(151)]

    def stored(e):   # what the collection handed the index: the vector as the collection normalized it
        got = col.get(e.id)
        assert got[0] == "ok"
        return np.asarray(got[1].vector, np.float32)

    assert col.put_many(embs[:150]) == "ok"
    ref.insert_many([(e.id, stored(e)) for e in embs[:150]])
    for e in embs[:100]:
        assert col.delete(e.id) == "ok"
        ref.delete(e.id)
    assert HnswGpu.memory(col) == nifs.hnsw_memory(col.index_state)
    assert HnswGpu.memory(col)["dead_rows"] == 100
    assert col.put(embs[150]) == "ok"
    ref.insert(embs[150].id, stored(embs[150]))
    mem = HnswGpu.memory(col)
    assert (mem["rows"], mem["dead_rows"], mem["row_capacity"], mem["edges"]) == (51, 0, 1024, edges_of(ref))
    assert_same_graph(nifs, col.index_state, ref)
    for q in (vecs[120], vecs[3]):
        got = col.search([float(x) for x in q], {"limit": 9})
        assert got[0] == "ok"
        prepared = col.prepare_query([float(x) for x in q])
        assert prepared[0] == "ok"
        want = ref.search(np.asarray(prepared[1], np.float32), 9)
        assert [r.id for r in got[1]] == [i for i, _ in want] and len(want) == 9


def test_the_nif_reports_the_memory(nifs, ref_order):
    import nif_runtime
    from nif_runtime import OK
    rt = nif_runtime.Runtime()
    funcs = rt.functions()
    assert ("hnsw_memory", 1) in funcs and funcs[("hnsw_memory", 1)] != 0   # a dirty scheduler: the call takes the handle's lock
    made = rt.call("hnsw_new_cosine", 4, 8, 24, 12, 12, 0)
    assert made[0] == OK
    h = made[1]
    assert rt.call("hnsw_memory", h) == (OK, (0, 0, 0, 0))
    rng = np.random.default_rng(505)
    ids = [b"n%d" % ((i * 7919) % 100003) for i in range(200)]
    vecs = rng.standard_normal((200, D)).astype(np.float32)
    ref = HnswIndex(COSINE, **P)
    ref.insert_many(list(zip(ids, vecs)))
    assert rt.call("hnsw_insert_many", h, [(i, [float(x) for x in v]) for i, v in zip(ids, vecs)]) == (OK, ())
    for ext in ids[:130]:
        ref.delete(ext)
        assert rt.call("hnsw_delete", h, ext) == (OK, ())
    assert rt.call("hnsw_memory", h) == (OK, (200, 1024, 130, edges_of(ref)))
    v = rng.standard_normal(D).astype(np.float32)
    ref.insert(b"one-more", v)
    assert rt.call("hnsw_insert", h, b"one-more", [float(x) for x in v]) == (OK, ())
    got = rt.call("hnsw_memory", h)
    assert got == (OK, (71, 1024, 0, edges_of(ref))) and all(isinstance(x, int) for x in got[1])
    with pytest.raises(nif_runtime.ArgumentError):
        rt.call("hnsw_memory", b"not a reference")
    q = [float(x) for x in vecs[150]]
    hits = rt.call("hnsw_search", h, q, 5)
    assert hits[0] == OK and [(i, f32bits(r)) for i, r in hits[1]] == [(i, f32bits(r)) for i, r in ref.search(vecs[150], 5)]
    h.release()
