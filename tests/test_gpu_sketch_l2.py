"""GPU parity tests for K1q on L2 and squared-L2 handles: lone searches nominated from the int8 sketch of the rows, whose
column keeps ||x||^2 beside the dot's bounds (vettore_amd/csrc/vt_sketch.hip).

As in tests/test_gpu_sketch.py the sketch is an accelerator and must never show in a result: every hit equals the oracle's
restatement of flat.rs:96-124 bit for bit -- on adversarial corpora (norms spread over decades, near-copies of the query
where q.q + x.x - 2 q.x cancels), after mutations that leave the column to be patched or rebuilt, when the search declines
(magnitudes near 2^62, "metric overflow" included), when the card "has no room", on a multi-shard handle, under concurrent
readers, and beside cosine and dot handles whose searches stay what they were.  force_sketch sends these small corpora
where the cost model sends rows of 256 MB and more.  The corpora of the first test are the ones
tests/test_sketch8_l2_model.py certifies in the model.
"""
import threading

import numpy as np
import pytest

import sketch8_l2_ref as ref
import support
from test_gpu_parity import GpuIndex, bits, nifs, unwrap  # noqa: F401  (nifs: fixture)
from test_gpu_sketch import make_corpus as dot_corpus
from test_gpu_sketch import queries as dot_queries

pytestmark = pytest.mark.gpu

L2, L2SQ, COS, IP = 0, 1, 2, 3
METRICS = [L2, L2SQ]


def check(nifs, oracle_mod, handle, metric, x, ids, qs, k, note=""):
    packed = oracle_mod.pack_ids(ids)
    for i, q in enumerate(qs):
        got = unwrap(nifs.flat_search(handle, q, k))
        assert bits(got) == bits(oracle_mod.matrix_search(metric, x, packed, q, k)), (note, metric, k, i)


def loaded(nifs, metric, ids, x, profiling=True):
    g = GpuIndex(nifs, metric)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    if profiling:
        nifs.flat_set_profiling(g.ref, True)
    return g


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [1, 10, 100])
def test_lone_l2_searches_from_the_sketch_equal_the_oracle(nifs, oracle_mod, metric, k, vt_debug):
    """Tie blocks, 1 % duplicate rows, d on and off the 128-byte grid, two queries that are stored rows; the pass must serve
    (almost) all of them.  (Without the L2 family in the sketch's predicate no search launches the pass.)"""
    vt_debug.set("force_sketch", 1)
    for d, n in ref.E2E_SHAPES:
        x, ids, qs = ref.e2e_case(metric, k, d, n)
        g = loaded(nifs, metric, ids, x)
        check(nifs, oracle_mod, g.ref, metric, x, ids, qs, k, "d=%d" % d)
        prof = nifs.flat_get_profile(g.ref)
        assert prof["sketch_builds"] == 1, prof
        assert prof["sketch_launches"] == len(qs) == 12, prof
        assert prof["sketch_fallbacks"] <= 1, prof
        assert prof["sketch_candidates"] >= (len(qs) - prof["sketch_fallbacks"]) * min(k, n), prof


@pytest.mark.parametrize("metric", METRICS)
def test_adversarial_rows(nifs, oracle_mod, metric, vt_debug):
    """Norms over four decades, spiky rows, zero rows, duplicates, near-copies of three queries at relative distance
    10^-7 .. 10^-3."""
    vt_debug.set("force_sketch", 1)
    x, ids, qs = ref.spread_corpus(12000, 160, 910 + metric)
    g = loaded(nifs, metric, ids, x)
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs, 10)
    assert nifs.flat_get_profile(g.ref)["sketch_launches"] > 0


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("big", [3e37, 1e18])
def test_magnitudes_near_2_to_the_62_decline(nifs, oracle_mod, metric, big, vt_debug):
    """(||q|| + max ||x||) >= 2^62: a squared difference of K1's can overflow f32, so K1's own scan must decide (its f64
    recovery or "metric overflow"), and the sketch pass declines before it launches.  3e37: the squares overflow; 1e18: they
    do not, the search only declines."""
    vt_debug.set("force_sketch", 1)
    n, d = 5000, 64
    x, ids = ref.corpus(n, d, 77)
    x[10] = np.float32(big)
    g = loaded(nifs, metric, ids, x)
    packed = oracle_mod.pack_ids(ids)
    for q in (np.full(d, 2.0, np.float32), x[10].copy()):
        got = nifs.flat_search(g.ref, q, 5)
        try:
            want = bits(oracle_mod.matrix_search(metric, x, packed, q, 5))
        except oracle_mod.OracleError as e:  # ("metric overflow": the search must fail the same way)
            assert got[0] == "error" and "overflow" in str(got[1]), (got, e)
        else:
            assert got[0] == "ok" and bits(got[1]) == want, (got, want)
    assert nifs.flat_get_profile(g.ref)["sketch_launches"] == 0


def test_mutations_patch_then_rebuild_the_sketch(nifs, oracle_mod, vt_debug):
    """Upserts, deletes (swap with the last row) and appends are patched row by row, xx with them; more than
    kMaxDerivedDirty mutated rows rebuild the column; an emptied index gives it back and a new dimension starts anew."""
    vt_debug.set("force_sketch", 1)
    metric, n, d = L2, 9000, 128
    x, ids = ref.corpus(n, d, 4243, tie_block=20)
    ids = list(ids)
    g = loaded(nifs, metric, ids, x)
    qs = ref.queries(6, x, 6)
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs, 10, "fresh")
    for r in (0, 17, n - 1, 4500):  # upserts that become query 2's best hits: only a patched xx lets them through
        x[r] = (qs[2] * (1.0 + 0.001 * (1 + r % 5))).astype(np.float32)
        unwrap(nifs.flat_insert(g.ref, ids[r], x[r]))
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs, 10, "upserts")
    for r in (5, 6000):  # swap-deletes
        unwrap(nifs.flat_delete(g.ref, ids[r]))
        last = len(ids) - 1
        x[r], ids[r] = x[last], ids[last]
        x, ids = x[:last], ids[:last]
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs, 10, "deletes")
    new = (qs[3] * 1.0005).astype(np.float32)
    unwrap(nifs.flat_insert(g.ref, b"zz-new", new))
    x, ids = np.vstack([x, new[None]]), ids + [b"zz-new"]
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs, 10, "append")
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch_builds"] == 1 and prof["sketch_patched_rows"] >= 6, prof
    assert prof["sketch_launches"] >= 2 * len(qs), prof  # (fresh and upserts at the least: an append may leave the ranks lazy)
    # a bulk replacement of more rows than kMaxDerivedDirty: rebuilt, not patched
    m = 70000
    y, _ = ref.corpus(m, d, 99)
    yids = [b"zz-x%08d" % i for i in range(m)]  # (new ids, after every id so far: the ranks stay strictly current)
    unwrap(nifs.flat_load_matrix(g.ref, yids, y))
    x, ids = np.vstack([x, y]), ids + list(yids)
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs[:3], 10, "bulk")
    assert nifs.flat_get_profile(g.ref)["sketch_builds"] == 2
    for i in list(ids):
        unwrap(nifs.flat_delete(g.ref, i))
    assert len(g.ref) == 0
    x, ids = ref.corpus(3000, 40, 5)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    check(nifs, oracle_mod, g.ref, metric, x, ids, ref.queries(8, x, 3), 7, "new dimension")
    assert nifs.flat_get_profile(g.ref)["sketch_builds"] == 3


def test_no_room_for_the_sketch_means_scanning_the_rows(nifs, oracle_mod, request, vt_debug):
    """(test_refuse_sketch, libvettore_hip_hooks.so only: the test re-runs itself there.)"""
    if support.rerun_with_hooks_library(request):
        return
    vt_debug.set("test_refuse_sketch", 1)
    vt_debug.set("force_sketch", 1)
    x, ids = ref.corpus(8000, 96, 12)
    g = loaded(nifs, L2SQ, ids, x)
    check(nifs, oracle_mod, g.ref, L2SQ, x, ids, ref.queries(2, x, 4), 10)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch_launches"] == 0 and prof["sketch_builds"] == 0 and prof["scan_launches"] == 4, prof


def test_switched_off_the_rows_are_scanned(nifs, oracle_mod, vt_debug):
    vt_debug.set("force_sketch", 1)
    vt_debug.set("sketch", 0)
    x, ids = ref.corpus(8000, 96, 13)
    g = loaded(nifs, L2, ids, x)
    check(nifs, oracle_mod, g.ref, L2, x, ids, ref.queries(3, x, 3), 10)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch_launches"] == 0 and prof["sketch_builds"] == 0, prof


def test_a_multi_shard_handle(nifs, oracle_mod, vt_debug):
    vt_debug.set("force_sketch", 1)
    x, ids = ref.corpus(20000, 128, 14, tie_block=16)
    handle = nifs.flat_new_sharded(L2, [0, 0, 0])
    unwrap(nifs.flat_load_matrix(handle, ids, x))
    nifs.flat_set_profiling(handle, True)
    check(nifs, oracle_mod, handle, L2, x, ids, ref.queries(4, x, 5), 10)
    assert nifs.flat_get_profile(handle)["sketch_launches"] >= 5 * 3 - 1


def test_concurrent_readers(nifs, oracle_mod, vt_debug):
    """Readers on their own contexts (coalescing off) run the pass side by side, each with its own scratch."""
    vt_debug.set("force_sketch", 1)
    vt_debug.set("coalesce", 0)
    metric = L2SQ
    x, ids = ref.corpus(20000, 128, 15)
    g = loaded(nifs, metric, ids, x, profiling=False)
    qs = ref.queries(5, x, 24)
    unwrap(nifs.flat_search(g.ref, qs[0], 10))  # (builds the sketch)
    packed = oracle_mod.pack_ids(ids)
    want = [bits(oracle_mod.matrix_search(metric, x, packed, q, 10)) for q in qs]
    errors = []

    def run(t):
        for rep in range(3):
            for i in range(t, len(qs), 6):
                got = bits(unwrap(nifs.flat_search(g.ref, qs[i], 10)))
                if got != want[i]:
                    errors.append((t, rep, i))

    ths = [threading.Thread(target=run, args=(t,)) for t in range(6)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors, errors[:5]


def test_cosine_and_dot_handles_beside_the_l2_one(nifs, oracle_mod, vt_debug):
    """Three handles in one process, their searches interleaved: each column is its own handle's (the cosine and dot
    images are built without xx: tests/test_gpu_sketch_l2_kernels.py reads them back), and the cosine and dot counters are
    what tests/test_gpu_sketch.py expects of them."""
    vt_debug.set("force_sketch", 1)
    n, d, k = 9000, 100, 10
    cases = []
    for metric in (COS, L2, IP, L2SQ):
        if metric in (COS, IP):
            x, ids = dot_corpus(n, d, 7100 + metric + d, metric == COS, oracle_mod, tie_block=48)
            qs = dot_queries(np.random.default_rng(k + d), x, 12, metric, oracle_mod)
        else:
            x, ids, qs = ref.e2e_case(metric, k, d, n)
        cases.append((metric, x, ids, qs, loaded(nifs, metric, ids, x), oracle_mod.pack_ids(ids)))
    for i in range(12):
        for metric, x, ids, qs, g, packed in cases:
            got = unwrap(nifs.flat_search(g.ref, qs[i], k))
            assert bits(got) == bits(oracle_mod.matrix_search(metric, x, packed, qs[i], k)), (metric, i)
    for metric, x, ids, qs, g, packed in cases:
        prof = nifs.flat_get_profile(g.ref)
        assert prof["sketch_builds"] == 1 and prof["sketch_launches"] == 12 and prof["sketch_fallbacks"] <= 1, (metric, prof)
        assert prof["sketch_candidates"] >= (12 - prof["sketch_fallbacks"]) * k, (metric, prof)
        assert prof["sketch6_launches"] == 0 and prof["sketch5_launches"] == 0 and prof["sketch4_launches"] == 0, (metric, prof)


def test_a_headline_shaped_l2_search_reads_the_sketch(nifs, oracle_mod):
    """No forcing: L2 rows past the size cut take the pass by default, and the bytes it is priced at are the sketch's
    (whole 64-row tiles of ld8 + 16 bytes per row: xx costs no byte), counted in scan_bytes too."""
    import torch
    from bench import build_shard, doc_ids
    rows, dim = 400_000, 768  # 1.2 GB of f32 rows
    x = build_shard(torch, torch.device("cuda", 0), rows, dim, 4243, normalize=False)
    g = GpuIndex(nifs, L2)
    assert nifs.flat_load_device_matrix(g.ref, doc_ids(0, rows), x.data_ptr(), rows, dim) == ("ok", ())
    q = x[123].cpu().numpy().copy()
    del x
    unwrap(nifs.flat_search(g.ref, q, 10))  # (builds the sketch)
    nifs.flat_set_profiling(g.ref, True)
    for _ in range(5):
        hits = unwrap(nifs.flat_search(g.ref, q, 10))
    assert hits[0][0] == doc_ids(123, 1)[0] and hits[0][1] == 0.0
    prof = nifs.flat_get_profile(g.ref)
    tile_bytes = (dim // 16 + 1) * 1024
    assert prof["sketch_launches"] == 5 and prof["sketch_fallbacks"] == 0, prof
    assert prof["sketch_bytes"] == 5 * ((rows + 63) // 64) * tile_bytes, prof
    assert prof["scan_launches"] == 5 and prof["scan_bytes"] == prof["sketch_bytes"], prof
