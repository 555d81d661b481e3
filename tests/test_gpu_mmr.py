"""MMR reranking on the device (vt_mmr_rerank, vt_flat_mmr_*, K12: vt_mmr.hip) -- `-m gpu`.  The reference's MMR is
deterministic, so every assertion is equality of the chosen order and of the status with its restatement
(tests/mmr_ref.py, metric values from the CPU oracle in the lane order in force).  No tolerance anywhere.  The shapes
are the ones at which the step kernel can go wrong, not the workload's: lists that end inside a block, at its end and
one past it, rows that end inside a chunk, one candidate, more rounds than candidates."""
import ctypes as C

import numpy as np
import pytest

import mmr_ref
import support
from test_gpu_parity import bits, nifs, unwrap  # noqa: F401  (nifs: a fixture)

pytestmark = pytest.mark.gpu

METRICS = list(mmr_ref.DISTANCE_METRICS[:2]) + ["cosine", "inner_product"] + list(mmr_ref.DISTANCE_METRICS[2:])
OVERFLOW = ("error", "metric_overflow")
STATUS = {0: "ok", 4: "metric_overflow", 38: "invalid_mmr_args", 18: "unsupported"}


@pytest.fixture
def lane_order(nifs, oracle_mod):
    """Sets the library's default lane order and the oracle's together; both go back afterwards."""
    was = nifs.debug_get("reduce_order")

    def set_order(order):
        assert nifs.set_default_reduce_order(order) == "ok"
        oracle_mod.set_reduce_order(order)
    set_order(was)
    yield set_order
    nifs.set_default_reduce_order(was)
    oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


def device_order(nifs, metric, rows, scores, alpha, final_k):
    """vt_mmr_rerank as the restatement's order_of_rows answers: ("ok", [indices]) or ("error", atom)."""
    import vettore_amd._lib as L
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, d = rows.shape
    sc = np.ascontiguousarray(scores, dtype=np.float64)
    order = np.full(max(n, 1), 0xDEAD, dtype=np.uint32)
    count = C.c_size_t(12345)
    st = L.load().vt_mmr_rerank(nifs.DEVICE, mmr_ref_code(metric), n, d, rows.ctypes.data_as(C.POINTER(C.c_float)),
                                sc.ctypes.data_as(C.POINTER(C.c_double)), float(alpha), final_k,
                                order.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(count))
    if st != 0:
        assert count.value == 0
        return ("error", STATUS.get(st, st))
    assert count.value == min(final_k, n)
    return ("ok", [int(i) for i in order[:count.value]])


def mmr_ref_code(metric):
    import oracle
    return oracle.METRIC_CODE[metric]


def reference(rows, scores, metric, alpha, final_k):
    return mmr_ref.order_of_rows(np.asarray(rows, dtype=np.float32).tolist(), list(scores), metric, alpha, final_k)


def random_case(n, d, seed, ties=False):
    rng = np.random.default_rng(seed)
    if ties:
        rows = rng.integers(-1, 2, size=(n, d)).astype(np.float32)
        rows[rng.integers(0, n, size=max(1, n // 3))] = rows[rng.integers(0, n, size=max(1, n // 3))]  # duplicates
        scores = rng.choice([0.25, 0.5, 0.75], size=n)
    else:
        rows = rng.normal(size=(n, d)).astype(np.float32)
        scores = rng.uniform(-1, 1, size=n)
    return rows, [float(s) for s in scores]


def final_ks(n):
    return sorted({k for k in (1, n - 1, n, n + 5) if k >= 1})


# ------------------------------------------------------------------ shapes, metrics, lane orders
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_list_lengths_and_round_counts(nifs, lane_order, n):
    rows, scores = random_case(n, 7, 100 + n)
    for metric in ("l2", "cosine"):
        for k in final_ks(n):
            assert device_order(nifs, metric, rows, scores, 0.3, k) == reference(rows, scores, metric, 0.3, k), (metric, k)


def test_257_candidates_every_round(nifs, lane_order):
    n = 257
    rows, scores = random_case(n, 9, 7)
    # one run of the restatement: without an error the answer for final_k is the first final_k choices of a longer run
    # (do_mmr is the same recursion stopped earlier; the shorter lists above check that directly)
    full = reference(rows, scores, "manhattan", 0.5, n + 5)
    assert full[0] == "ok" and sorted(full[1]) == list(range(n))
    for k in final_ks(n):
        assert device_order(nifs, "manhattan", rows, scores, 0.5, k) == ("ok", full[1][:k]), k


@pytest.mark.parametrize("order", [3, 1, 0, 2])
@pytest.mark.parametrize("d", [1, 7, 8, 9, 64, 65])
def test_every_metric_dimension_and_lane_order(nifs, lane_order, d, order):
    lane_order(order)
    rows, scores = random_case(20, d, 1000 + d)
    for metric in METRICS:
        assert device_order(nifs, metric, rows, scores, 0.5, 20) == reference(rows, scores, metric, 0.5, 20), metric


@pytest.mark.parametrize("order", [3, 1])
def test_every_metric_at_768(nifs, lane_order, order):
    lane_order(order)
    rows, scores = random_case(12, 768, 768)
    for metric in METRICS:
        assert device_order(nifs, metric, rows, scores, 0.5, 12) == reference(rows, scores, metric, 0.5, 12), metric


# ------------------------------------------------------------------ ties, zero signs, zero vectors
def tie_rows(n, d, seed):
    """Rows of {-1, 0, 1}^d with duplicates and scores of three values: ties inside a block, across blocks and at the
    list's end.  A few rows make a zero redundancy negative (their f64 cosine to a neighbour is about -1e-60, -0.0 as an
    f32), a few are zero vectors, and the last entry ties with the first."""
    rows, scores = random_case(n, d, seed, ties=True)
    if n >= 8 and d >= 3:
        rows[1] = 0.0
        rows[2, :] = 0.0
        rows[2, :3] = [1e-30, 1.0, 0.0]
        rows[3, :] = 0.0
        rows[3, :3] = [-1e-30, 0.0, 1.0]
        rows[n - 2] = 0.0
        rows[n - 1] = rows[0]
        scores[n - 1] = scores[0]
    return rows, scores


@pytest.mark.parametrize("alpha", [0, 0.3, 0.5, 1])
def test_ties_keep_the_first_and_zero_signs_do_not_matter(nifs, lane_order, alpha):
    n = 70
    rows, scores = tie_rows(n, 5, 31)
    import oracle
    assert np.float32(oracle.cosine(rows[2], rows[3])).tobytes() == np.float32(-0.0).tobytes()
    for metric in ("cosine", "inner_product", "hamming", "jaccard", "chebyshev"):
        for k in (1, n // 2, n + 5):
            assert device_order(nifs, metric, rows, scores, alpha, k) == reference(rows, scores, metric, alpha, k), (metric, k)


def test_the_score_is_not_fused(nifs, lane_order):
    """The inputs of tests/test_mmr_ref.py on which an FMA of either product into the subtraction chooses b where the
    reference chooses c: a kernel built with contraction would fail here."""
    from test_mmr_ref import FMA_ALPHA, FMA_ROWS, FMA_SCORES
    rows = [FMA_ROWS[k] for k in "abc"]
    scores = [FMA_SCORES[k] for k in "abc"]
    assert reference(rows, scores, "cosine", FMA_ALPHA, 3) == ("ok", [0, 2, 1])
    assert device_order(nifs, "cosine", rows, scores, FMA_ALPHA, 3) == ("ok", [0, 2, 1])
    assert device_order(nifs, "cosine", rows, scores, FMA_ALPHA, 2) == ("ok", [0, 2])


def test_integers_and_the_python_mirror(nifs, lane_order):
    """nifs.mmr_rerank: the caller's own entries come back, integers are numbers, the atoms are the reference's."""
    embeddings = [("id%02d" % i, [float(i % 5), float(i % 3), 1]) for i in range(17)]
    initial = [("id%02d" % i, (i * 7) % 11) for i in (3, 16, 0, 9, 12, 5)]
    for metric in ("l2", "cosine", "negative_inner_product"):
        for alpha in (0, 1, 0.5):
            got = nifs.mmr_rerank(initial, embeddings, metric, alpha, 4)
            assert got == mmr_ref.mmr_rerank(initial, embeddings, metric, alpha, 4), (metric, alpha)
            assert all(any(g is e for e in initial) for g in got[1])
    big = [("a", [1.5e19]), ("b", [-1.5e19])]
    assert nifs.mmr_rerank([("a", 1.0), ("b", 0.5)], big, "l2_squared", 0.5, 2) == OVERFLOW
    assert nifs.mmr_rerank([("a", 1.0), ("b", 0.5)], big, "l2_squared", 0.5, 1) == ("ok", [("a", 1.0)])


# ------------------------------------------------------------------ overflow
def test_overflow_is_recovered_where_f64_can_and_reported_only_in_a_round_that_runs(nifs, lane_order):
    # the f32 chain overflows, the f64 recovery is representable: no error
    rows = [[2.0e38, 0.0, 2.0e38], [-1.0e38, 0.0, 1.0e38], [3.0e38, 1.0, -3.0e38]]
    scores = [1.0, 0.5, 0.25]
    for metric in ("l2", "inner_product", "negative_inner_product"):
        want = reference(rows, scores, metric, 0.5, 3)
        assert device_order(nifs, metric, rows, scores, 0.5, 3) == want, metric
    assert reference(rows[:2], scores[:2], "l2", 0.5, 2) == ("ok", [0, 1])
    # not representable: (c, b) overflows under l2_squared, (b, a) and (c, a) do not; chosen in the order a, b, c
    rows, scores = [[0.0], [1.5e19], [-1.5e19]], [3.0, 2.0, 1.0]
    for k in (1, 2, 3, 8):
        want = reference(rows, scores, "l2_squared", 1.0, k)
        assert want == (("ok", [0, 1][:k]) if k <= 2 else OVERFLOW)
        assert device_order(nifs, "l2_squared", rows, scores, 1.0, k) == want, k
    for metric in ("manhattan", "chebyshev", "l2"):
        rows = [[3.0e38, 3.0e38], [-3.0e38, 3.0e38], [0.0, 0.0]]
        for k in (1, 2, 3):
            assert device_order(nifs, metric, rows, scores, 0.5, k) == reference(rows, scores, metric, 0.5, k), (metric, k)


def overflow_rows(n, where, seed=5):
    """l2_squared, one coordinate: entry 0 is chosen first (the best score) and sits at 1.5e19; the entries of `where` sit
    at -1.5e19 -- their pair with entry 0 is not representable --, everything else near 0."""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-1, 1, size=(n, 1)).astype(np.float32)
    scores = [float(s) for s in rng.uniform(0, 1, size=n)]
    rows[0, 0], scores[0] = 1.5e19, 5.0
    for i in where:
        rows[i, 0] = -1.5e19
    return rows, scores


# ------------------------------------------------------------------ several blocks, the unstaged walk (hooks build)
def test_forced_block_splits_and_unstaged_rows(request, nifs, lane_order, vt_debug):
    """(test_mmr_block_rows / test_mmr_lds_dim, libvettore_hip_hooks.so only: the test re-runs itself there.)  The same
    answers whatever the split: one block, two, several with a ragged last one; a chosen row staged in LDS or walked
    where it lies."""
    if support.rerun_with_hooks_library(request):
        return
    wanted = {}

    def want(key, *args):
        if key not in wanted:
            wanted[key] = reference(*args)
        return wanted[key]
    for block_rows, lds_dim in ((0, 0), (32, 0), (64, 8), (5, 4), (2, 0)):
        vt_debug.set("test_mmr_block_rows", block_rows)
        vt_debug.set("test_mmr_lds_dim", lds_dim)
        # (block_rows = 2: 257 candidates are more than 64 blocks' worth, every block takes a second and a third pass)
        for n in (1, 2, 63, 64, 65, 129, 257):
            rows, scores = random_case(n, 9, 200 + n)
            for k in final_ks(n):
                got = device_order(nifs, "l2", rows, scores, 0.3, k)
                assert got == want(("l2", n, k), rows, scores, "l2", 0.3, k), (block_rows, lds_dim, n, k)
        # d = 9 and 65 sit above a staging limit of 8 (and 4): the unstaged walk, every metric
        for d in (9, 65):
            rows, scores = random_case(40, d, 300 + d)
            for metric in METRICS:
                got = device_order(nifs, metric, rows, scores, 0.5, 40)
                assert got == want((metric, d), rows, scores, metric, 0.5, 40), (block_rows, lds_dim, metric, d)
        # ties inside a block, across blocks and at the list's end
        rows, scores = tie_rows(130, 5, 77)
        for metric in ("cosine", "hamming"):
            for alpha in (0, 0.5, 1):
                got = device_order(nifs, metric, rows, scores, alpha, 135)
                assert got == want(("tie", metric, alpha), rows, scores, metric, alpha, 135), (block_rows, metric, alpha)
        # several overflowing candidates in one round, in different blocks; the failing round decides, not a later one
        for where in ((40, 70, 99), (99,), (1,)):
            rows, scores = overflow_rows(100, where)
            for k in (1, 2, 5):
                got = device_order(nifs, "l2_squared", rows, scores, 0.5, k)
                assert got == want(("ovf", where, k), rows, scores, "l2_squared", 0.5, k) == (("ok", [0]) if k == 1 else OVERFLOW)
        # an overflow that waits for a later round: entry 0 is chosen in round 2 only
        rows, scores = overflow_rows(100, (40, 70))
        scores[0] = -5.0
        scores[40] = scores[70] = -6.0
        for k in (1, 3, 99, 100):
            got = device_order(nifs, "l2_squared", rows, scores, 1.0, k)
            assert got == want(("late", k), rows, scores, "l2_squared", 1.0, k), (block_rows, k)
        assert wanted[("late", 3)][0] == "ok" and wanted[("late", 100)] == OVERFLOW


# ------------------------------------------------------------------ resident rows
def make_index(nifs, metric, rows, order=3):
    ref = nifs._flat_new(mmr_ref_code(metric))
    nifs.flat_set_reduce_order(ref, order)
    ids = ["row%04d" % i for i in range(len(rows))]
    unwrap(nifs.flat_insert_many(ref, [(ids[i], rows[i]) for i in range(len(rows))]))
    return ref, ids


def restated(vectors, initial, metric, alpha, k):
    """The restatement over the index's rows: ("ok", [(id, score)]) or the library's string for the error."""
    res = mmr_ref.mmr_rerank(initial, [(i, [float(v) for v in vec]) for i, vec in vectors.items()], metric, alpha, k)
    if res[0] == "ok":
        return res
    return ("error", {"metric_overflow": "metric overflow", "invalid_mmr_args": "invalid mmr args"}[res[1]])


@pytest.mark.parametrize("metric,order", [("l2", 3), ("cosine", 3), ("inner_product", 1), ("jaccard", 3)])
def test_rerank_by_ids_after_rows_have_moved(nifs, lane_order, metric, order):
    lane_order(order)
    rows, _ = random_case(90, 9, 41, ties=(metric == "jaccard"))
    ref, ids = make_index(nifs, metric, rows, order)
    vectors = {ids[i]: rows[i] for i in range(len(ids))}
    rng = np.random.default_rng(3)
    for i in (5, 17, 60):  # upserts: the row changes where it lies
        vectors[ids[i]] = rng.normal(size=9).astype(np.float32)
        unwrap(nifs.flat_insert(ref, ids[i], vectors[ids[i]]))
    for i in (0, 33, 88, 2):  # swap-deletes: the last row moves into the hole
        unwrap(nifs.flat_delete(ref, ids[i]))
        del vectors[ids[i]]
    vectors["zz-new"] = rng.normal(size=9).astype(np.float32)
    unwrap(nifs.flat_insert(ref, "zz-new", vectors["zz-new"]))
    live = sorted(vectors)
    pick = [live[i] for i in rng.permutation(len(live))[:40]]
    initial = [(i, float(s)) for i, s in zip(pick, rng.uniform(-1, 1, size=len(pick)))]
    for alpha, k in ((0.5, 40), (0.3, 7), (1, 45), (0, 1)):
        got = nifs.flat_mmr_rerank(ref, initial, alpha, k)
        assert got == restated(vectors, initial, metric, alpha, k), (alpha, k)
        assert got[0] == "ok" and all(any(g is e for e in initial) for g in got[1])
    # ids the index does not hold (one of them deleted a moment ago), ids twice, bad arguments, nothing to do
    inv = ("error", "invalid mmr args")
    assert nifs.flat_mmr_rerank(ref, initial + [(ids[0], 0.1)], 0.5, 3) == inv
    assert nifs.flat_mmr_rerank(ref, initial + [("never", 0.1)], 0.5, 3) == inv
    assert nifs.flat_mmr_rerank(ref, initial + [initial[4]], 0.5, 3) == inv
    assert nifs.flat_mmr_rerank(ref, initial, 1.5, 3) == inv
    assert nifs.flat_mmr_rerank(ref, initial, 0.5, 0) == inv
    assert nifs.flat_mmr_rerank(ref, [(pick[0], float("nan"))], 0.5, 1) == inv
    assert nifs.flat_mmr_rerank(ref, [], 0.5, 3) == ("ok", [])
    assert nifs.flat_mmr_rerank(nifs._flat_new(0), [], 0.5, 3) == ("ok", [])
    assert nifs.flat_mmr_rerank(nifs._flat_new(0), [("a", 1.0)], 0.5, 3) == inv


def test_a_batch_of_different_problems(nifs, lane_order):
    """Problems that differ in n, k and alpha in one launch chain: an empty one, failing ones, some that finish many
    launches before the longest -- every answer the lone call's."""
    rng = np.random.default_rng(11)
    rows = rng.normal(size=(120, 1)).astype(np.float32)
    rows[0, 0], rows[1, 0] = 1.5e19, -1.5e19
    ref, ids = make_index(nifs, "l2_squared", rows)
    vectors = {ids[i]: rows[i] for i in range(len(ids))}

    def initial(which):
        return [(ids[i], float(rng.uniform(0, 1))) for i in which]
    problems = [
        (initial(range(2, 100)), 0.5, 98),                      # the longest: 99 launches
        ([], 0.5, 3),                                           # empty
        (initial([0, 1, 5]), 0.5, 3),                           # fails in its second round
        (initial([7]), 1, 4),
        (initial(range(10, 75)), 0.3, 1),
        (initial([0, 1, 5]), 0.5, 1),                           # the same pair, never scored
        (initial(range(40, 105)), 0, 70),
        (initial([3, 3]), 0.5, 2),                              # an id twice
        (initial([9, 8]), 1.5, 2),                              # a bad alpha
        (initial(range(2, 66)), 0.7, 64),
    ]
    got = nifs.flat_mmr_rerank_batch(ref, problems)
    assert len(got) == len(problems)
    for p, (init, alpha, k) in enumerate(problems):
        assert got[p] == restated(vectors, init, "l2_squared", alpha, k), p
        assert got[p] == nifs.flat_mmr_rerank(ref, init, alpha, k), p
    assert [g[0] for g in got] == ["ok", "ok", "error", "ok", "ok", "ok", "ok", "error", "error", "ok"]
    assert got[2] == ("error", "metric overflow")


@pytest.mark.parametrize("metric,score_mode", [("cosine", "raw"), ("cosine", "similarity"), ("l2", "raw"), ("l2", "similarity"),
                                               ("negative_inner_product", "similarity"), ("hamming", "similarity")])
def test_mmr_search_is_search_then_rerank(nifs, lane_order, metric, score_mode):
    from vettore_amd.index_flat import result_values
    rows, _ = random_case(300, 24, 51, ties=(metric == "hamming"))
    ref, ids = make_index(nifs, metric, rows)
    vectors = {ids[i].encode(): rows[i] for i in range(len(ids))}
    rng = np.random.default_rng(8)
    queries = rng.normal(size=(5, 24)).astype(np.float32)

    def piped(hits, alpha, limit):
        initial = [(i, result_values(metric, raw, score_mode)[0]) for i, raw in hits]
        res = mmr_ref.order_of(initial, [(i, [float(v) for v in vectors[i]]) for i, _ in hits], metric, alpha, limit)
        assert res[0] == "ok"
        return res[1]
    for candidates, limit, alpha in ((40, 10, 0.5), (65, 65, 0.3), (7, 20, 1), (300, 3, 0)):
        lone = []
        for q in queries:
            hits = unwrap(nifs.flat_search(ref, q, candidates))
            got_hits, order = unwrap(nifs.flat_mmr_search(ref, q, candidates, limit, alpha, score_mode))
            assert bits(got_hits) == bits(hits)  # the candidate list is flat_search's, byte for byte
            assert order == piped(hits, alpha, limit), (candidates, limit, alpha)
            lone.append((bits(hits), order))
        batch = unwrap(nifs.flat_mmr_search_batch(ref, queries, candidates, limit, alpha, score_mode))
        batch_hits = unwrap(nifs.flat_search_batch(ref, queries, candidates))
        for b, res in enumerate(batch):
            assert res[0] == "ok"
            assert bits(res[1][0]) == bits(batch_hits[b]) == lone[b][0]
            assert res[1][1] == lone[b][1], (b, candidates, limit, alpha)
    inv = ("error", "invalid mmr args")
    assert nifs.flat_mmr_search(ref, queries[0], 10, 0, 0.5) == inv
    assert nifs.flat_mmr_search(ref, queries[0], 10, 3, -0.5) == inv
    assert nifs.flat_mmr_search_batch(ref, queries, 10, 3, 2) == inv
    assert nifs.flat_mmr_search(ref, queries[0][:5], 10, 3, 0.5) == nifs.flat_search(ref, queries[0][:5], 10)  # the search's own error
    assert nifs.flat_mmr_search(ref, queries[0], 0, 3, 0.5) == ("ok", ([], []))
    empty = nifs._flat_new(mmr_ref_code(metric))
    assert nifs.flat_mmr_search(empty, queries[0], 10, 3, 0.5) == ("ok", ([], []))
    assert unwrap(nifs.flat_mmr_search_batch(empty, queries, 10, 3, 0.5)) == [("ok", ([], []))] * 5


def test_mmr_search_reports_a_querys_own_overflow(nifs, lane_order):
    """Two rows whose pair is not representable under l2_squared, far from a cluster: a query between them has both
    among its candidates and fails once a second round runs; a query near the cluster never sees them."""
    rows = np.zeros((10, 2), np.float32)
    rows[0], rows[1] = [1.5e19, 0.0], [-1.5e19, 0.0]
    for i in range(2, 10):
        rows[i] = [i * 1.0e15, 1.4e19]
    ref, ids = make_index(nifs, "l2_squared", rows)
    between = np.array([0.0, -4.0e18], np.float32)
    near = np.array([0.0, 8.0e18], np.float32)
    assert {i for i, _ in unwrap(nifs.flat_search(ref, between, 5))} >= {b"row0000", b"row0001"}
    assert not {i for i, _ in unwrap(nifs.flat_search(ref, near, 5))} & {b"row0000", b"row0001"}
    assert len(unwrap(nifs.flat_mmr_search(ref, near, 5, 5, 0.5))[1]) == 5
    assert len(unwrap(nifs.flat_mmr_search(ref, between, 5, 1, 0.5))[1]) == 1   # one round: no pair is scored
    assert nifs.flat_mmr_search(ref, between, 5, 5, 0.5) == ("error", "metric overflow")
    batch = unwrap(nifs.flat_mmr_search_batch(ref, np.stack([near, between, near]), 5, 5, 0.5))
    assert [b[0] for b in batch] == ["ok", "error", "ok"] and batch[1] == ("error", "metric overflow")
    assert batch[0] == batch[2] == nifs.flat_mmr_search(ref, near, 5, 5, 0.5)


def test_a_sharded_handle_refuses(nifs):
    ref = nifs.flat_new_sharded(0, [0, 0])
    unwrap(nifs.flat_insert_many(ref, [("a", [1.0, 0.0]), ("b", [0.0, 1.0]), ("c", [1.0, 1.0])]))
    q = np.array([1.0, 0.0], np.float32)
    for res in (nifs.flat_mmr_rerank(ref, [("a", 1.0), ("b", 0.5)], 0.5, 2), nifs.flat_mmr_search(ref, q, 3, 2, 0.5),
                nifs.flat_mmr_search_batch(ref, q.reshape(1, 2), 3, 2, 0.5),
                nifs.flat_mmr_rerank_batch(ref, [([("a", 1.0)], 0.5, 1)])):
        assert res[0] == "error" and res[1].startswith("unsupported on device") and "sharded" in res[1], res
    assert unwrap(nifs.flat_search(ref, q, 2))[0][0] == b"a"
