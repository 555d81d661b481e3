"""MaxSim on the device (K9, vt_maxsim.hip) -- `-m gpu`: multi_vector_top_k / multi_vector_score against the
reference's composition of the oracle's distances (tests/maxsim_ref.py), bit for bit: every score and the exact
ordered id list, all nine metrics, two lane orders, ragged shapes, error precedence, the chunked upload and one
large call."""
import ctypes as C

import numpy as np
import pytest

import maxsim_ref
from test_gpu_parity import nifs  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 8, 9, 17, 128, 768)
QUERY_COUNTS = (0, 1, 7, 32)


def f32bits(x):
    return np.float32(x).tobytes()


def assert_same_hits(got, want, ctx):
    assert got[0] == "ok", (ctx, got)
    assert [h[0] for h in got[1]] == [h[0] for h in want], ctx
    assert [f32bits(h[1]) for h in got[1]] == [f32bits(h[1]) for h in want], ctx


def vectors(rng, n, d, metric):
    v = rng.uniform(-1, 1, size=(n, d)).astype(np.float32)
    if metric in (7, 8):  # float hamming / jaccard count non-zeros: zeros must occur
        v[rng.uniform(size=v.shape) < 0.35] = 0.0
    if metric == 2 and n > 2:
        v[1] = 0.0  # a zero norm scores 0.0
    return [list(map(float, r)) for r in v]


def documents(rng, d, metric):
    """Empty documents, one-vector ones, a wave and a vector more, duplicates (score ties) and ids that share
    prefixes."""
    sizes = (0, 1, 3, 64, 65, 2, 0, 300 if d <= 17 else 130)
    docs = [("doc-%d" % i, vectors(rng, t, d, metric)) for i, t in enumerate(sizes)]
    docs.append(("doc", docs[3][1]))        # the same vectors as doc-3 under a prefix of its id
    docs.append(("doc-10", docs[2][1]))     # ... and doc-2's under an id that doc-1 prefixes
    docs.append(("a", docs[4][1]))
    return docs


@pytest.mark.parametrize("order", [3, 0])
@pytest.mark.parametrize("metric", range(9))
def test_top_k_bitwise_against_the_reference(nifs, oracle_mod, vt_debug, metric, order):
    vt_debug.set("reduce_order", order)
    oracle_mod.set_reduce_order(order)
    try:
        rng = np.random.default_rng(100 * metric + order)
        for d in DIMS:
            docs = documents(rng, d, metric)
            for nq in QUERY_COUNTS:
                if d == 768 and order != 3 and nq == 7:
                    continue  # (the biggest shape once per order is enough: 32 query vectors take two LDS panels)
                query = vectors(rng, nq, d, metric)
                if nq:
                    query[0] = docs[4][1][0]  # an exact match somewhere
                want = maxsim_ref.top_k(docs, query, metric, len(docs) + 5)
                for limit in (0, 1, 7, len(docs), len(docs) + 5):
                    got = nifs.multi_vector_top_k(docs, query, metric, limit)
                    assert_same_hits(got, want[:limit], (metric, order, d, nq, limit))
                # the single-document form scores what the batch does
                for i in (2, 4, 7):
                    got = nifs.multi_vector_score(query, docs[i][1], metric)
                    exp = maxsim_ref.score(query, docs[i][1], metric)
                    assert got[0] == "ok" and f32bits(got[1]) == f32bits(exp), (metric, order, d, nq, i)
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


@pytest.mark.parametrize("order", [1, 2])
def test_the_other_two_lane_orders(nifs, oracle_mod, vt_debug, order):
    """Orders 1 and 2 through the stateless kernel: a lane with one chunk and a scalar tail (d = 9) or two chunks and one
    (d = 17), documents of one vector, of a wave and of a wave and a vector more (a second lane round), one query vector
    and nine (a second group of eight whose last seven slots are clamped).  The seed is one under which the data tells
    either order from the default one: under inner product and under L2 some score's bits differ between the two
    (found on the CPU, and asserted below)."""
    try:
        rng = np.random.default_rng(4460 + order)
        for metric in (3, 0, 6):
            told_apart = False
            for d in (9, 17):
                docs = [("one", vectors(rng, 1, d, metric)), ("wave", vectors(rng, 64, d, metric)),
                        ("wave+1", vectors(rng, 65, d, metric))]
                for nq in (1, 9):
                    query = vectors(rng, nq, d, metric)
                    oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)
                    default = maxsim_ref.top_k(docs, query, metric, len(docs))
                    oracle_mod.set_reduce_order(order)
                    want = maxsim_ref.top_k(docs, query, metric, len(docs))
                    told_apart |= sorted((h[0], f32bits(h[1])) for h in want) != sorted((h[0], f32bits(h[1])) for h in default)
                    vt_debug.set("reduce_order", order)
                    got = nifs.multi_vector_top_k(docs, query, metric, len(docs))
                    assert_same_hits(got, want, (metric, order, d, nq))
            assert told_apart or metric == 6, (metric, order)  # (a maximum is the same in any order)
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


def test_error_precedence_follows_the_document_order(nifs):
    ip = 3
    ok = [[1.0, 0.5]]
    overflow = [[1e20, 1e20]]          # q.t = 2e40 in f32 and in f64: "metric overflow"
    query = [[1e20, 1e20]]
    docs = [("d%d" % i, [[0.0, 0.25]]) for i in range(7)]
    docs[3] = ("d3", overflow)
    docs[5] = ("d5", [[1.0]])          # dimension mismatch
    assert nifs.multi_vector_top_k(docs, query, ip, 3) == ("error", "metric overflow")
    assert nifs.multi_vector_top_k(docs, query, ip, 0) == ("error", "metric overflow")
    docs[3], docs[5] = ("d3", [[1.0]]), ("d5", overflow)
    assert nifs.multi_vector_top_k(docs, query, ip, 3) == ("error", "dimension mismatch")
    # a document after the first error is never looked at
    docs[3], docs[5] = ("d3", [[1.0, float("nan")]]), ("d5", [[1.0]])
    assert nifs.multi_vector_top_k(docs, query, ip, 3) == ("error", "vector contains a non-finite value")
    assert nifs.multi_vector_top_k([("x", ok)], query, ip, 1)[0] == "ok"


def test_score_overflow_literal(nifs):
    # multi_vector.rs:250-258: finite pair scores whose running total overflows
    query = [[1.0e19]] * 4
    document = [[1.0e19]]
    assert nifs.multi_vector_score(query, document, 3) == ("error", "score overflow")
    docs = [("a", [[1.0]]), ("b", document), ("c", [[1.0, 2.0]])]
    assert nifs.multi_vector_top_k(docs, query, 3, 5) == ("error", "score overflow")
    # a metric overflow at an earlier query vector than the running total's wins
    query = [[1.0e20], [1.0e19], [1.0e19], [1.0e19]]
    assert nifs.multi_vector_score(query, [[1.0e20]], 3) == ("error", "metric overflow")


@pytest.mark.parametrize("metric", [2, 3, 5])
def test_many_chunks_forced(nifs, oracle_mod, vt_debug, metric):
    rng = np.random.default_rng(7 + metric)
    d = 9
    docs = [("m%03d" % i, vectors(rng, int(rng.integers(0, 12)), d, metric)) for i in range(120)]
    docs.append(("big", vectors(rng, 40, d, metric)))  # larger than a chunk on its own
    query = vectors(rng, 5, d, metric)
    want = maxsim_ref.top_k(docs, query, metric, len(docs))
    for chunk in (36, 200, 1000):
        vt_debug.set("maxsim_chunk_bytes", chunk)
        got = nifs.multi_vector_top_k(docs, query, metric, len(docs))
        assert_same_hits(got, want, (metric, chunk))
        got = nifs.multi_vector_top_k(docs, query, metric, 7)
        assert_same_hits(got, want[:7], (metric, chunk, 7))


def _packed_top_k(lib, ids, doc_vec_off, values, d, query, metric, limit):
    """vt_multi_vector_top_k on packed arrays (a large call without Python lists)."""
    from vettore_amd import nifs as N
    idb, ioff = N._pack_ids(ids)
    nvec = int(doc_vec_off[-1])
    voff = (np.arange(nvec + 1, dtype=np.uintp) * d).astype(np.uintp)
    q = np.ascontiguousarray(query, dtype=np.float32).reshape(-1)
    qoff = (np.arange(len(query) + 1, dtype=np.uintp) * d).astype(np.uintp)
    h = C.c_void_p()
    st = lib.vt_multi_vector_top_k(N.DEVICE, len(ids), idb, N._szp(ioff), N._szp(doc_vec_off), N._fp(values),
                                   N._szp(voff), N._fp(q), N._szp(qoff), len(query), metric, limit, C.byref(h))
    assert st == 0, lib.vt_strerror(st)
    return N._take_hits(h)


@pytest.mark.parametrize("metric", [3, 2])
def test_one_large_call_sampled(nifs, oracle_mod, metric):
    from vettore_amd import _lib
    rng = np.random.default_rng(2026 + metric)
    n, d, nq, limit = 20000, 128, 32, 100
    counts = rng.integers(0, 257, size=n)
    doc_vec_off = np.zeros(n + 1, dtype=np.uintp)
    doc_vec_off[1:] = np.cumsum(counts)
    values = rng.standard_normal(size=(int(doc_vec_off[-1]), d), dtype=np.float32)
    query = rng.standard_normal(size=(nq, d), dtype=np.float32)
    ids = ["doc%06d" % i for i in range(n)]
    got = _packed_top_k(_lib.load(), ids, doc_vec_off, values, d, query, metric, limit)
    assert len(got) == limit
    qv = [list(map(float, r)) for r in query]
    kth = (-float(got[-1][1]), got[-1][0])
    returned = {h[0]: h[1] for h in got}
    for i in list(rng.choice(n, size=24, replace=False)) + [int(np.argmax(counts))]:
        vecs = [list(map(float, r)) for r in values[doc_vec_off[i]:doc_vec_off[i + 1]]]
        exp = maxsim_ref.score(qv, vecs, metric)
        one = nifs.multi_vector_score(qv, vecs, metric)
        assert one[0] == "ok" and f32bits(one[1]) == f32bits(exp), i
        idb = ids[i].encode()
        if idb in returned:
            assert f32bits(returned[idb]) == f32bits(exp), i
        else:
            assert (-float(exp), idb) > kth, i  # no unreturned sampled document beats the k-th
    # the returned list is sorted best first
    assert got == sorted(got, key=lambda h: (-h[1], h[0]))


# ---- collection level: Collection.multi_vector_search and hybrid_search's multi-vector rerank -------------------------
def _collection(nifs, metric, rng, n=60, d=16):
    from vettore_amd.collection import Collection, Embedding
    col = Collection.new(dimensions=d, metric=metric, normalize="none")[1]
    embs = []
    for i in range(n):
        vecs = [list(map(float, v)) for v in rng.uniform(-1, 1, size=(int(rng.integers(1, 9)), d)).astype(np.float32)]
        if i % 3 == 0:
            embs.append(Embedding(id="v%02d" % i, vector=vecs[0]))            # one vector: its own document
        elif i % 3 == 1:
            embs.append(Embedding(id="m%02d" % i, vectors=vecs))             # primary vector = their mean
        else:
            embs.append(Embedding(id="b%02d" % i, vector=vecs[0], vectors=vecs[1:] or vecs))
    assert col.put_many(embs) == "ok"
    return col


def _stored_documents(col, ids=None):
    return [(e.id, e.vectors or [e.vector]) for e in col.store.values() if ids is None or e.id in ids]


def test_collection_multi_vector_search(nifs, oracle_mod):
    rng = np.random.default_rng(77)
    col = _collection(nifs, "inner_product", rng)
    # the primary vector of a multi-vector embedding is the f64 mean of its vectors
    e = col.get("m01")[1]
    mean = [sum(float(v[j]) for v in e.vectors) / len(e.vectors) for j in range(16)]
    assert e.vector == mean
    qv = [list(map(float, v)) for v in rng.uniform(-1, 1, size=(5, 16)).astype(np.float32)]
    for metric, code in (("inner_product", 3), ("l2", 0), ("euclidean", 0), ("cosine", 2)):
        got = col.multi_vector_search(qv, {"limit": 7, "metric": metric})
        want = maxsim_ref.top_k(_stored_documents(col), qv, code, 7)
        assert got[0] == "ok"
        assert [r.id for r in got[1]] == [h[0] for h in want], metric
        assert [f32bits(r.score) for r in got[1]] == [f32bits(h[1]) for h in want], metric
        assert all(r.distance is None for r in got[1])
    assert col.multi_vector_search(qv, {"limit": 0}) == ("error", "invalid_limit")
    assert col.multi_vector_search(qv, {"metric": "nope"}) == ("error", "invalid_metric")
    assert col.multi_vector_search(qv, {"k": 1}) == ("error", ("unsupported_option", "k"))
    assert col.multi_vector_search([], {}) == ("error", "invalid_multi_vector")
    assert col.multi_vector_search([[1.0] * 15], {}) == ("error", "dimension_mismatch")


def test_hybrid_search_multi_vector_rerank(nifs, oracle_mod):
    from vettore_amd.index_flat import FlatGpu
    rng = np.random.default_rng(78)
    col = _collection(nifs, "l2", rng, n=120)
    embs = list(col.store.values())
    x = np.array([e.vector for e in embs], dtype=np.float32)
    packed = oracle_mod.pack_ids([e.id for e in embs])
    query = list(map(float, rng.uniform(-1, 1, size=16).astype(np.float32)))
    qv = [list(map(float, v)) for v in rng.uniform(-1, 1, size=(3, 16)).astype(np.float32)]
    for rerank, code in ((("multi_vector", qv), 0), (("multi_vector", qv, {"metric": "inner_product"}), 3)):
        got = FlatGpu.hybrid_search(col, query, {"limit": 5, "generators": [("search", {"candidates": 20})],
                                                 "rerank": rerank})
        cand = {h[0] for h in oracle_mod.matrix_search(0, x, packed, query, 20)}
        want = maxsim_ref.top_k(_stored_documents(col, cand), qv, code, 5)
        assert got[0] == "ok", got
        assert [r.id for r in got[1]] == [h[0] for h in want]
        assert [f32bits(r.score) for r in got[1]] == [f32bits(h[1]) for h in want]
    # the union of two generators: each one's candidate set is its own call with limit = candidates
    got = FlatGpu.hybrid_search(col, query, {"limit": 6, "generators": [("search", {"candidates": 10}), "quantized"],
                                             "rerank": ("multi_vector", qv)})
    cand = {h[0] for h in nifs.flat_search(col.index_state, query, 10)[1]}
    cand |= {h[0] for h in nifs.flat_quantized_search(col.index_state, query, 60, 60)[1]}
    want = maxsim_ref.top_k(_stored_documents(col, cand), qv, 0, 6)
    assert [r.id for r in got[1]] == [h[0] for h in want]
    # exact rerank and the refusals stay as they were
    assert FlatGpu.hybrid_search(col, query, {"limit": 5, "rerank": "exact"})[0] == "ok"
    assert FlatGpu.hybrid_search(col, query, {"limit": 5, "rerank": "other"}) == ("error", ("invalid_rerank", "other"))
    assert FlatGpu.hybrid_search(col, query, {"limit": 5, "rerank": ("multi_vector", qv, {"x": 1})}) == \
        ("error", ("unsupported_option", "x"))
