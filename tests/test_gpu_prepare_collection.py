"""The four normalizations at the collection (collection.ex:50): Collection.new accepts them, put_many prepares the plain
vectors of a batch in one prepare_rows call, and what lands in the store and the index is byte for byte what put, one
embedding at a time, produces."""
import numpy as np
import pytest

import prepare_ref

pytestmark = pytest.mark.gpu

D, N = 24, 300
WITH_VECTORS = (3, 150, 299)   # these embeddings carry `vectors` (and no `vector`: it is their normalized mean)


def _embeddings():
    from vettore_amd.collection import Embedding
    rng = np.random.default_rng(300)
    embs = []
    for i in range(N):
        if i in WITH_VECTORS:
            vectors = [[float(v) for v in rng.normal(size=D)] for _ in range(3)]
            embs.append(Embedding(id="doc%03d" % i, vectors=vectors, metadata={"i": i}))
        elif i == 10:
            embs.append({"id": "doc010", "vector": [4.0] * D})                      # a constant row, as a map
        elif i == 11:
            embs.append(Embedding(id=b"doc011", vector=[0.1 * (j + 1) for j in range(D)], value="eleven"))   # doubles that round
        else:
            embs.append(Embedding(id="doc%03d" % i, vector=[float(v) for v in rng.normal(size=D) * 10.0 ** rng.integers(-3, 3)],
                                  metadata={"i": i}))
    return embs


def _bytes_of(vector):
    # (normalize: none keeps Python floats, the others hand back float32 arrays: compare what is there)
    if isinstance(vector, np.ndarray):
        return (str(vector.dtype), vector.tobytes())
    return ("list", np.asarray(vector, dtype=np.float64).tobytes())


def _collection(normalize):
    from vettore_amd.collection import Collection
    made = Collection.new(dimensions=D, metric="cosine", normalize=normalize)
    assert made[0] == "ok", made
    return made[1]


@pytest.mark.parametrize("normalize", prepare_ref.MODES)
def test_put_many_stores_what_put_one_by_one_stores(normalize):
    embs = _embeddings()
    many, single = _collection(normalize), _collection(normalize)
    assert many.put_many(embs) == "ok"
    for e in embs:
        assert single.put(e) == "ok"
    assert list(many.store) == list(single.store) and len(many.store) == N
    for key, a in many.store.items():
        b = single.store[key]
        assert (a.id, a.value, a.metadata) == (b.id, b.value, b.metadata), key
        assert _bytes_of(a.vector) == _bytes_of(b.vector), key
        assert a.binary_vector == b.binary_vector and all(type(w) is int for w in a.binary_vector), key
        assert (a.vectors is None) == (b.vectors is None), key
        if a.vectors is not None:
            assert [_bytes_of(v) for v in a.vectors] == [_bytes_of(v) for v in b.vectors], key
    # the plain rows are the model's, bit for bit
    plain = [e for e in embs if not isinstance(e, dict) and e.vectors is None][:40]
    x = np.array([e.vector for e in plain], dtype=np.float64).astype(np.float32)
    want, want_words = prepare_ref.prepare_rows(x, normalize)
    for k, e in enumerate(plain):
        key = e.id if isinstance(e.id, bytes) else e.id.encode()
        stored = many.store[key]
        assert np.asarray(stored.vector, dtype=np.float32).tobytes() == want[k].tobytes(), key
        assert stored.binary_vector == [int(w) for w in want_words[k]], key
    rng = np.random.default_rng(9)
    for _ in range(3):
        q = [float(v) for v in rng.normal(size=D)]
        pq = many.prepare_query(q)
        assert pq[0] == "ok"
        want_q = prepare_ref.normalize(np.array(q, dtype=np.float64).astype(np.float32), normalize)
        if normalize == "none":
            assert pq[1] == q
        else:
            assert np.asarray(pq[1]).dtype == np.float32 and np.asarray(pq[1]).tobytes() == want_q.tobytes()
        for name, opts in (("search", {"limit": 10}), ("quantized_search", {"limit": 10, "candidates": 50}),
                           ("multi_vector_search", {"limit": 10})):
            arg = [q, [float(v) for v in rng.normal(size=D)]] if name == "multi_vector_search" else q
            got, want_hits = getattr(many, name)(arg, opts), getattr(single, name)(arg, opts)
            assert got[0] == "ok" and len(got[1]) == 10, (name, got)
            assert repr(got) == repr(want_hits), name


@pytest.mark.parametrize("normalize", prepare_ref.MODES)
def test_a_bad_embedding_fails_the_batch_like_the_loop_of_puts(normalize):
    from vettore_amd.collection import Embedding
    good = _embeddings()[:12]
    bads = [Embedding(id="bad", vector=[1.0] * (D - 1)), Embedding(id="bad", vector=[1.0] * (D - 1) + [float("nan")]),
            Embedding(id="bad", vector=[1.0] * (D - 1) + [float("inf")]), Embedding(id="", vector=[1.0] * D),
            Embedding(id="bad", vector=None), Embedding(id="bad", vectors=[]), Embedding(id="bad", vectors=[[1.0] * D, [2.0]]),
            "not an embedding", Embedding(id="doc005", vector=[1.0] * D)]
    for bad in bads:
        batch = good[:7] + [bad] + good[7:]
        many, single = _collection(normalize), _collection(normalize)
        loop = "ok"
        for e in batch:
            loop = single.put(e)
            if loop != "ok":
                break
        assert loop != "ok", bad
        assert many.put_many(batch) == loop, bad
        assert many.store == {} and many.search([1.0] * D, {"limit": 5}) == ("ok", []), bad
    # an earlier embedding's error wins over a later one's, whichever path prepares them
    many = _collection(normalize)
    assert many.put_many(good[:3] + [bads[1]] + [bads[3]]) == ("error", "invalid_vector")
    assert many.put_many(good[:4] + [bads[3]] + [bads[1]]) == ("error", "missing_id")
    assert many.store == {}
