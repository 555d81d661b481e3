"""MUVERA encoding on the device (K10, vt_muvera.hip) -- `-m gpu`: muvera_encode_query / _document / _batch against
the restatement of muvera.rs in tests/muvera_ref.py, byte for byte.

The tolerance is zero, and not from a measurement: the hash is integer arithmetic, the weight a fixed chain of
IEEE conversions, every dot product one sequential f64 sum of exact products, the accumulation and the count
sketch sequential with one f32 rounding per step.  A differing byte is a defect of the kernel."""
import json
import os

import numpy as np
import pytest

import muvera_ref
from test_gpu_parity import nifs  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "muvera_rs.json")
U64_MAX = (1 << 64) - 1
MODES = {"query": muvera_ref.QUERY, "document": muvera_ref.DOCUMENT}


def golden():
    return json.load(open(GOLDEN))


def cfg_args(c):
    return (c["dimension"], c["num_repetitions"], c["num_simhash_projections"], c["seed"], c["projection_dimension"],
            c["final_projection_dimension"])


def as_vectors(rows):
    return [[float("nan") if x == "NaN" else x for x in v] for v in rows]


def encode(nifs, vectors, mode, *args):
    return (nifs.muvera_encode_query if mode == muvera_ref.QUERY else nifs.muvera_encode_document)(vectors, *args)


def f32bytes(values):
    return np.asarray(values, dtype=np.float32).tobytes()


def assert_same(got, want, ctx):
    """("ok", list) against ("ok", float32 array), or the same error string."""
    assert got[0] == want[0], (ctx, got[:1], want)
    if want[0] == "error":
        assert got[1] == want[1], ctx
        return
    g, w = np.asarray(got[1], dtype=np.float32), np.asarray(want[1], dtype=np.float32)
    assert g.shape == w.shape, (ctx, g.shape, w.shape)
    if g.tobytes() != w.tobytes():
        bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
        raise AssertionError((ctx, "differs at", bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist(), len(bad)))


def test_golden_entries(nifs):
    for c in golden()["cases"]:
        got = encode(nifs, as_vectors(c["vectors"]), MODES[c["mode"]], *cfg_args(c["config"]))
        e = c["expect"]
        if "ok" in e:
            assert got[0] == "ok" and f32bytes(got[1]) == f32bytes(e["ok"]), (c["name"], got)
        elif "len" in e:
            assert got[0] == "ok" and len(got[1]) == e["len"], (c["name"], got[0])
        else:
            assert got == ("error", e["error"] if e["error"] is not None else e["string"]), (c["name"], got)


def random_set(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[rng.uniform(size=x.shape) < 0.05] = 0.0           # a zero dot product is `>= 0.0`
    x[rng.uniform(size=x.shape) < 0.02] = -0.0
    if n > 1:
        x[n // 2] = x[0]                                # a repeated vector: the same partition twice
    return [list(map(float, r)) for r in x]


GRID = dict(d=(1, 2, 7, 64, 128), R=(1, 3), k=(0, 1, 4, 8), pd=("d", 1, 5, 16), final=(None, 1, 5, 257),
            seed=(0, 1, 42, U64_MAX), n=(1, 2, 33, 200), mode=(muvera_ref.QUERY, muvera_ref.DOCUMENT))


def grid_cases(extra=150):
    """A fixed subsample of the cross product: first every value of every axis in turn (so each appears), then
    `extra` random points."""
    keys = list(GRID)
    width = max(len(v) for v in GRID.values())
    cases = [tuple(GRID[k][(i + s) % len(GRID[k])] for s, k in enumerate(keys)) for i in range(2 * width)]
    rng = np.random.default_rng(20260907)
    for _ in range(extra):
        cases.append(tuple(GRID[k][int(rng.integers(len(GRID[k])))] for k in keys))
    seen = {k: set() for k in keys}
    for c in cases:
        for k, v in zip(keys, c):
            seen[k].add(v)
    assert all(seen[k] == set(GRID[k]) for k in keys)
    return [dict(zip(keys, c)) for c in cases]


def test_bytes_equal_the_reference_over_the_grid(nifs):
    rng = np.random.default_rng(7)
    for i, c in enumerate(grid_cases()):
        d = c["d"]
        pd = d if c["pd"] == "d" else c["pd"]
        args = (d, c["R"], c["k"], c["seed"], pd, c["final"])
        vectors = random_set(rng, c["n"], d)
        want = muvera_ref.encode(vectors, *args, c["mode"])
        assert want[0] == "ok", (i, c, want)
        assert_same(encode(nifs, vectors, c["mode"], *args), want, (i, c))


def test_shapes_beside_the_grid(nifs):
    """What the grid does not reach: more table columns than a wave has lanes, partition counts in device memory
    (document mode, more than 4 096 partitions), repetition groups with a short tail, the largest staged vector."""
    rng = np.random.default_rng(11)
    shapes = [  # d, R, k, seed, pd, final, n
        (7, 2, 4, 5, 100, None, 9), (7, 2, 4, 5, 100, 33, 9), (5, 1, 0, 9, 70, None, 3),
        (7, 3, 13, 3, 2, 5, 40), (3, 2, 13, 3, 3, None, 20),
        (64, 70, 0, 1, 64, None, 5), (6, 23, 2, 8, 6, 11, 12), (9, 11, 3, 4, 4, None, 65),
        (16384, 1, 2, 6, 3, None, 2),
    ]
    for d, R, k, seed, pd, final, n in shapes:
        vectors = random_set(rng, n, d)
        for mode in (muvera_ref.QUERY, muvera_ref.DOCUMENT):
            want = muvera_ref.encode(vectors, d, R, k, seed, pd, final, mode)
            assert_same(encode(nifs, vectors, mode, d, R, k, seed, pd, final), want, (d, R, k, seed, pd, final, n, mode))
    got = nifs.muvera_encode_query([[0.0] * 16385], 16385, 1, 0, 1, 16385, None)
    assert got[0] == "error" and got[1].startswith("unsupported on device"), got


def test_order_and_seed(nifs):
    """muvera.rs:359-378: the query encoding does not depend on the order of the vectors, the document encoding
    only within 1e-6, and another seed gives another encoding."""
    p = golden()["permutation"]
    vectors, args = p["vectors"], cfg_args(p["config"])
    query = nifs.muvera_encode_query(vectors, *args)
    assert query[0] == "ok" and nifs.muvera_encode_query(vectors[::-1], *args) == query
    doc, rdoc = nifs.muvera_encode_document(vectors, *args), nifs.muvera_encode_document(vectors[::-1], *args)
    assert doc[0] == rdoc[0] == "ok" and doc != query
    assert all(abs(a - b) <= p["document_tolerance"] for a, b in zip(doc[1], rdoc[1]))
    other = list(args)
    other[3] += 1
    assert nifs.muvera_encode_query(vectors, *other)[1] != query[1]


def ragged_batch(rng, d):
    sets = [random_set(rng, int(rng.integers(1, 41)), d) for _ in range(300)]
    fmax = float(np.finfo(np.float32).max)
    sets[5] = []                                           # "empty vectors"
    sets[17] = [sets[17][0], sets[17][0][:-1]]            # "dimension mismatch"
    sets[40][-1][3] = float("nan")                         # non-finite
    sets[41] = [[1.0] * (d + 1), [float("inf")] * d]       # both: the length comes first
    sets[77] = [[fmax] * d, [fmax] * d, [fmax] * d]        # "encoding overflow"
    return sets


@pytest.mark.parametrize("final", [None, 37])
@pytest.mark.parametrize("mode", [muvera_ref.QUERY, muvera_ref.DOCUMENT])
def test_batch_equals_solo_encodings(nifs, vt_debug, mode, final):
    d = 16
    args = (d, 3, 3, 42, 4, final)
    sets = ragged_batch(np.random.default_rng(300 + mode), d)
    status, (matrix, reasons) = nifs.muvera_encode_batch(sets, mode, *args)
    assert status == "ok" and matrix.shape == (300, muvera_ref.fde_dimension(3, 3, 4, final)) and matrix.dtype == np.float32
    assert reasons[5] == "empty vectors" and reasons[17] == "dimension mismatch" and reasons[41] == "dimension mismatch"
    assert reasons[40] == "vector contains a non-finite value" and reasons[77] == "encoding overflow"
    for i, vectors in enumerate(sets):
        want = muvera_ref.encode(vectors, *args, mode)
        solo = encode(nifs, vectors, mode, *args)
        assert_same(solo, want, ("solo", i))
        if want[0] == "error":
            assert reasons[i] == want[1] and not matrix[i].any(), (i, reasons[i], want)
        else:
            assert reasons[i] is None and matrix[i].tobytes() == f32bytes(solo[1]), i
    # without a place for statuses the first failing set's status is the call's
    import ctypes as C
    import vettore_amd._lib as L
    per_set = [[np.asarray(v, dtype=np.float32) for v in s] for s in sets[:8]]
    set_off = np.cumsum([0] + [len(s) for s in per_set]).astype(np.uintp)
    flat = [v for s in per_set for v in s]
    val_off = np.cumsum([0] + [v.size for v in flat]).astype(np.uintp)
    values = np.concatenate(flat)
    out = np.ones((8, matrix.shape[1]), dtype=np.float32)
    sz, fp = C.POINTER(C.c_size_t), C.POINTER(C.c_float)
    st = L.load().vt_muvera_encode(0, mode, 8, set_off.ctypes.data_as(sz), values.ctypes.data_as(fp), val_off.ctypes.data_as(sz),
                                   d, 3, 3, 42, 4, final or 0, 0 if final is None else 1, out.ctypes.data_as(fp), None)
    assert st == 20 and out[:5].tobytes() == matrix[:5].tobytes() and not out[5:].any()
    # a budget of a few KiB: many chunks, the same bytes and the same statuses
    vt_debug.set("muvera_chunk_bytes", 6000)
    status, (chunked, chunked_reasons) = nifs.muvera_encode_batch(sets, mode, *args)
    assert status == "ok" and chunked.tobytes() == matrix.tobytes() and chunked_reasons == reasons
    vt_debug.set("muvera_chunk_bytes", 1)
    status, (chunked, chunked_reasons) = nifs.muvera_encode_batch(sets[:50], mode, *args)
    assert status == "ok" and chunked.tobytes() == matrix[:50].tobytes() and chunked_reasons == reasons[:50]


def test_batch_configuration_errors_fail_the_call(nifs):
    sets = [[[1.0, 0.0]], [[0.0, 1.0]]]
    assert nifs.muvera_encode_batch(sets, 0, 2, 0, 0, 1, 2, None) == ("error", "num_repetitions must be positive")
    assert nifs.muvera_encode_batch(sets, 0, 2, 1, 0, 1, 2, 0) == ("error", "final_projection_dimension must be positive")
    assert nifs.muvera_encode_batch([], 0, 2, 1, 0, 1, 2, None)[0] == "ok"


def test_four_document_fixture_end_to_end(nifs):
    """test/vector_integration_test.exs:49-98 with every native step on the device: document encodings into an
    inner-product flat index, searched by the query encoding; the top 3 contain MaxSim's top 2."""
    from vettore_amd.index_flat import FlatGpu
    r = golden()["retrieval"]
    args = cfg_args(r["config"])
    docs = [(d[0], d[1]) for d in r["documents"]]
    status, exact = nifs.multi_vector_top_k(docs, r["query"], nifs.METRIC_CODE["inner_product"], r["exact_top"])
    assert status == "ok" and len(exact) == r["exact_top"]
    status, qfde = nifs.muvera_encode_query(r["query"], *args)
    assert status == "ok"
    fdes = []
    for _, vectors in docs:
        status, fde = nifs.muvera_encode_document(vectors, *args)
        assert status == "ok" and len(fde) == len(qfde)
        fdes.append(fde)
    status, index = FlatGpu.new("inner_product")
    assert status == "ok"
    assert nifs.flat_load_matrix(index, [d[0] for d in docs], np.asarray(fdes, dtype=np.float32)) == ("ok", ())
    status, hits = nifs.flat_search(index, qfde, r["limit"])
    assert status == "ok" and {h[0] for h in exact} <= {h[0] for h in hits}, (exact, hits)


def test_two_thousand_documents_search_like_the_reference(nifs):
    from vettore_amd.index_flat import FlatGpu
    rng = np.random.default_rng(2000)
    d, args = 64, (64, 4, 3, 99, 8, None)
    sets = [random_set(rng, int(rng.integers(8, 41)), d) for _ in range(2000)]
    ids = ["doc-%04d" % i for i in range(2000)]
    status, (matrix, reasons) = nifs.muvera_encode_batch(sets, muvera_ref.DOCUMENT, *args)
    assert status == "ok" and not any(reasons)
    want = np.stack([muvera_ref.encode_document(s, *args)[1] for s in sets])
    assert matrix.tobytes() == want.tobytes()
    indexes = []
    for m in (matrix, want):
        status, index = FlatGpu.new("inner_product")
        assert status == "ok" and nifs.flat_load_matrix(index, ids, m) == ("ok", ())
        indexes.append(index)
    for _ in range(5):
        query = random_set(rng, 32, d)
        got_q, want_q = nifs.muvera_encode_query(query, *args), muvera_ref.encode_query(query, *args)
        assert_same(got_q, want_q, "query")
        a, b = nifs.flat_search(indexes[0], got_q[1], 10), nifs.flat_search(indexes[1], list(map(float, want_q[1])), 10)
        assert a[0] == "ok" and a == b and len(a[1]) == 10
