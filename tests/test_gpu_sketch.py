"""GPU parity tests for K1q: lone cosine / dot searches nominated from the int8 sketch of the rows
(vettore_amd/csrc/vt_sketch.hip).

The sketch is an accelerator and must never show in a result: every hit equals the oracle's restatement of
flat.rs:96-124 bit for bit -- on adversarial corpora, after mutations that leave it to be patched or rebuilt, when it
declines (magnitudes near f32 overflow), when the card "has no room" for it, on a multi-shard handle and under
concurrent readers.  force_sketch sends these small corpora where the cost model sends rows of 256 MB and more.
"""
import threading

import numpy as np
import pytest

import support
from test_gpu_parity import GpuIndex, bits, nifs, unwrap
from test_gpu_parity import make_corpus as _corpus  # noqa: F401  (nifs: fixture)

pytestmark = pytest.mark.gpu

COS, IP, NIP = 2, 3, 4


def make_corpus(n, d, seed, normalize, oracle_mod, **kw):
    """test_gpu_parity's corpus with ids that arrive in ascending byte order: the rank column stays strictly current
    (the pass never serves a lazily ranked shard)."""
    x, _ = _corpus(n, d, seed, normalize, oracle_mod, **kw)
    return x, [b"doc-%08d" % i for i in range(n)]


def check(nifs, oracle_mod, ref, metric, x, ids, qs, k, note=""):
    packed = oracle_mod.pack_ids(ids)
    for i, q in enumerate(qs):
        got = unwrap(nifs.flat_search(ref, q, k))
        assert bits(got) == bits(oracle_mod.matrix_search(metric, x, packed, q, k)), (note, metric, k, i)


def queries(rng, x, nq, metric, oracle_mod):
    d = x.shape[1]
    qs = rng.uniform(-1, 1, size=(nq, d)).astype(np.float32)
    qs[0] = x[len(x) // 2]  # sits on the block of identical rows
    qs[1] = x[3]
    if metric == COS:
        qs = np.stack([oracle_mod.normalize_l2(q) for q in qs])
    return qs


@pytest.mark.parametrize("metric", [COS, IP, NIP])
@pytest.mark.parametrize("k", [1, 10, 100])
def test_lone_searches_from_the_sketch_equal_the_oracle(nifs, oracle_mod, metric, k, vt_debug):
    """Tie blocks, 1 % duplicate rows, d on and off the 128-byte grid; the pass must serve (almost) all of them."""
    vt_debug.set("force_sketch", 1)
    for d, n in ((192, 30000), (100, 9000)):
        x, ids = make_corpus(n, d, 7100 + metric + d, metric == COS, oracle_mod, tie_block=48)
        g = GpuIndex(nifs, metric)
        unwrap(nifs.flat_load_matrix(g.ref, ids, x))
        nifs.flat_set_profiling(g.ref, True)
        qs = queries(np.random.default_rng(k + d), x, 12, metric, oracle_mod)
        check(nifs, oracle_mod, g.ref, metric, x, ids, qs, k, "d=%d" % d)
        prof = nifs.flat_get_profile(g.ref)
        assert prof["sketch_builds"] == 1, prof
        assert prof["sketch_launches"] == len(qs), prof
        assert prof["sketch_fallbacks"] <= 1, prof
        assert prof["sketch_candidates"] >= (len(qs) - prof["sketch_fallbacks"]) * min(k, n), prof


@pytest.mark.parametrize("metric", [COS, IP, NIP])
def test_adversarial_rows(nifs, oracle_mod, metric, vt_debug):
    """Un-normalised rows scaled by U(8, 24), spiky rows with one large coordinate, zero rows, duplicates."""
    vt_debug.set("force_sketch", 1)
    n, d = 12000, 160
    rng = np.random.default_rng(31 + metric)
    x, ids = make_corpus(n, d, 900 + metric, False, oracle_mod, tie_block=30)
    if metric != COS:
        x *= rng.uniform(8, 24, size=(n, 1)).astype(np.float32)
    spiky = rng.integers(0, n, 200)
    x[spiky, rng.integers(0, d, 200)] = rng.choice([-1, 1], 200) * rng.uniform(50, 400, 200).astype(np.float32)
    x[rng.integers(0, n, 50)] = 0.0
    if metric == COS:
        x = np.stack([oracle_mod.normalize_l2(r) for r in x])
    g = GpuIndex(nifs, metric)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    nifs.flat_set_profiling(g.ref, True)
    qs = queries(rng, x, 10, metric, oracle_mod)
    qs[2] = x[spiky[0]]
    qs[3] = 0.0
    qs[3, 5] = 1.0
    for k in (1, 10, 64):
        check(nifs, oracle_mod, g.ref, metric, x, ids, qs, k)
    assert nifs.flat_get_profile(g.ref)["sketch_launches"] > 0


@pytest.mark.parametrize("metric", [IP, NIP])
def test_magnitudes_near_overflow_decline(nifs, oracle_mod, metric, vt_debug):
    """A dot of these rows can overflow f32: K1's own scan must decide (its f64 recovery or "metric overflow"), and the
    sketch pass declines before it launches."""
    vt_debug.set("force_sketch", 1)
    n, d = 5000, 64
    x, ids = make_corpus(n, d, 77, False, oracle_mod)
    x[10] = 3e37
    g = GpuIndex(nifs, metric)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    nifs.flat_set_profiling(g.ref, True)
    packed = oracle_mod.pack_ids(ids)
    q = np.full(d, 2.0, np.float32)
    got = nifs.flat_search(g.ref, q, 5)
    try:
        want = bits(oracle_mod.matrix_search(metric, x, packed, q, 5))
    except oracle_mod.OracleError as e:  # ("metric overflow": the search must fail the same way)
        assert got[0] == "error" and "overflow" in str(got[1]), (got, e)
    else:
        assert got[0] == "ok" and bits(got[1]) == want, (got, want)
    assert nifs.flat_get_profile(g.ref)["sketch_launches"] == 0


def test_mutations_patch_then_rebuild_the_sketch(nifs, oracle_mod, vt_debug):
    """Upserts, deletes (swap with the last row) and appends are patched row by row; more than kMaxDerivedDirty
    mutated rows rebuild it; an emptied index gives it back and a new dimension starts anew."""
    vt_debug.set("force_sketch", 1)
    metric, n, d = IP, 9000, 128
    x, ids = make_corpus(n, d, 4243, False, oracle_mod, tie_block=20)
    x, ids = x.copy(), list(ids)
    g = GpuIndex(nifs, metric)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    nifs.flat_set_profiling(g.ref, True)
    rng = np.random.default_rng(6)
    qs = queries(rng, x, 6, metric, oracle_mod)
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs, 10, "fresh")
    for r in (0, 17, n - 1, 4500):  # upserts that become query 2's best hits
        x[r] = (qs[2] * (3.0 + r % 5)).astype(np.float32)
        unwrap(nifs.flat_insert(g.ref, ids[r], x[r]))
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs, 10, "upserts")
    for r in (5, 6000):  # swap-deletes
        unwrap(nifs.flat_delete(g.ref, ids[r]))
        last = len(ids) - 1
        x[r], ids[r] = x[last], ids[last]
        x, ids = x[:last], ids[:last]
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs, 10, "deletes")
    new = (qs[3] * 9.0).astype(np.float32)
    unwrap(nifs.flat_insert(g.ref, b"zz-new", new))
    x, ids = np.vstack([x, new[None]]), ids + [b"zz-new"]
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs, 10, "append")
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch_builds"] == 1 and prof["sketch_patched_rows"] >= 6, prof
    # a bulk replacement of more rows than kMaxDerivedDirty: rebuilt, not patched
    m = 70000
    y, _ = make_corpus(m, d, 99, False, oracle_mod)
    yids = [b"zz-x%08d" % i for i in range(m)]  # (new ids, after every id so far: the ranks stay strictly current)
    unwrap(nifs.flat_load_matrix(g.ref, yids, y))
    x, ids = np.vstack([x, y]), ids + list(yids)
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs[:3], 10, "bulk")
    assert nifs.flat_get_profile(g.ref)["sketch_builds"] == 2
    for i in list(ids):
        unwrap(nifs.flat_delete(g.ref, i))
    assert len(g.ref) == 0
    x, ids = make_corpus(3000, 40, 5, False, oracle_mod)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    check(nifs, oracle_mod, g.ref, metric, x, ids, queries(rng, x, 3, metric, oracle_mod), 7, "new dimension")
    assert nifs.flat_get_profile(g.ref)["sketch_builds"] == 3


def test_no_room_for_the_sketch_means_scanning_the_rows(nifs, oracle_mod, request, vt_debug):
    """(test_refuse_sketch, libvettore_hip_hooks.so only: the test re-runs itself there.)"""
    if support.rerun_with_hooks_library(request):
        return
    vt_debug.set("test_refuse_sketch", 1)
    vt_debug.set("force_sketch", 1)
    x, ids = make_corpus(8000, 96, 12, True, oracle_mod)
    g = GpuIndex(nifs, COS)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    nifs.flat_set_profiling(g.ref, True)
    check(nifs, oracle_mod, g.ref, COS, x, ids, queries(np.random.default_rng(2), x, 4, COS, oracle_mod), 10)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch_launches"] == 0 and prof["sketch_builds"] == 0 and prof["scan_launches"] == 4, prof


def test_switched_off_the_rows_are_scanned(nifs, oracle_mod, vt_debug):
    vt_debug.set("force_sketch", 1)
    vt_debug.set("sketch", 0)
    x, ids = make_corpus(8000, 96, 13, False, oracle_mod)
    g = GpuIndex(nifs, IP)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    nifs.flat_set_profiling(g.ref, True)
    check(nifs, oracle_mod, g.ref, IP, x, ids, queries(np.random.default_rng(3), x, 3, IP, oracle_mod), 10)
    assert nifs.flat_get_profile(g.ref)["sketch_launches"] == 0


def test_a_multi_shard_handle(nifs, oracle_mod, vt_debug):
    vt_debug.set("force_sketch", 1)
    x, ids = make_corpus(20000, 128, 14, True, oracle_mod, tie_block=16)
    ref = nifs.flat_new_sharded(COS, [0, 0, 0])
    unwrap(nifs.flat_load_matrix(ref, ids, x))
    nifs.flat_set_profiling(ref, True)
    check(nifs, oracle_mod, ref, COS, x, ids, queries(np.random.default_rng(4), x, 5, COS, oracle_mod), 10)
    assert nifs.flat_get_profile(ref)["sketch_launches"] >= 5 * 3 - 1


def test_concurrent_readers(nifs, oracle_mod, vt_debug):
    """Readers on their own contexts (coalescing off) run the pass side by side, each with its own scratch."""
    vt_debug.set("force_sketch", 1)
    vt_debug.set("coalesce", 0)
    metric = COS
    x, ids = make_corpus(20000, 128, 15, True, oracle_mod)
    g = GpuIndex(nifs, metric)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    qs = queries(np.random.default_rng(5), x, 24, metric, oracle_mod)
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


def test_a_headline_shaped_search_reads_the_sketch(nifs, oracle_mod):
    """No forcing: rows past the size cut take the pass by default, and the bytes it is priced at are the sketch's
    (whole 64-row tiles of ld8 + 16 bytes per row), counted in scan_bytes too."""
    import torch
    from bench import build_shard, doc_ids
    rows, dim = 400_000, 768  # 1.2 GB of f32 rows
    x = build_shard(torch, torch.device("cuda", 0), rows, dim, 4243)
    g = GpuIndex(nifs, COS)
    assert nifs.flat_load_device_matrix(g.ref, doc_ids(0, rows), x.data_ptr(), rows, dim) == ("ok", ())
    q = x[123].cpu().numpy().copy()
    del x
    unwrap(nifs.flat_search(g.ref, q, 10))  # (builds the sketch)
    nifs.flat_set_profiling(g.ref, True)
    for _ in range(5):
        hits = unwrap(nifs.flat_search(g.ref, q, 10))
    assert hits[0][0] == doc_ids(123, 1)[0]
    prof = nifs.flat_get_profile(g.ref)
    tile_bytes = (dim // 16 + 1) * 1024
    assert prof["sketch_launches"] == 5 and prof["sketch_fallbacks"] == 0, prof
    assert prof["sketch_bytes"] == 5 * ((rows + 63) // 64) * tile_bytes, prof
    assert prof["scan_launches"] == 5 and prof["scan_bytes"] == prof["sketch_bytes"], prof
