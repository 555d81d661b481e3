"""GPU parity tests for K1s: lone cosine / dot searches with limits up to 32 nominated from the 6-bit sketch of the rows
in two planes (sketch6_scan_kernel, vettore_amd/csrc/vt_sketch.hip), with the int8 sketch (K1q) as its
fallback and the f32 rows behind both.

Like the int8 sketch it is an accelerator and must never show in a result: every hit equals the oracle's restatement of
flat.rs:96-124 bit for bit.  force_sketch6 sends these small corpora where the cost model sends rows of GBs.
"""
import threading

import numpy as np
import pytest

import support
from test_gpu_parity import GpuIndex, bits, nifs, unwrap  # noqa: F401  (nifs: fixture)
from test_gpu_sketch import COS, IP, NIP, check, make_corpus, queries

pytestmark = pytest.mark.gpu

CAND_CAP = 32768  # the 6-bit tier's cand_cap (host/vt_sketchtiers.h)
MISS_LIMIT = 4    # ... and its miss_limit


def tile_bytes(d):
    ld8 = (d + 127) // 128 * 128
    return (3 * ld8 // 64 + 1) * 1024


def loaded(nifs, metric, x, ids, order=3):
    g = GpuIndex(nifs, metric, order)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    nifs.flat_set_profiling(g.ref, True)
    return g


def with_copies(x, row, every):
    at = np.arange(row % every, len(x), every)
    x[at] = x[row]
    return at


@pytest.mark.parametrize("metric", [COS, IP, NIP])
@pytest.mark.parametrize("k", [1, 10, 32])
def test_lone_searches_from_the_6bit_sketch_equal_the_oracle(nifs, oracle_mod, metric, k, vt_debug):
    """A tie block, 1 % duplicate rows, d off the 32-, 64- and 128-element grids and on them; the pass serves (almost)
    all of them and is priced at whole tiles of both planes and the metadata."""
    vt_debug.set("force_sketch6", 1)
    for d, n in ((129, 9000), (192, 30000), (768, 4096)):
        x, ids = make_corpus(n, d, 7600 + metric + d, metric == COS, oracle_mod, tie_block=48)
        g = loaded(nifs, metric, x, ids)
        qs = queries(np.random.default_rng(k + d), x, 8, metric, oracle_mod)
        check(nifs, oracle_mod, g.ref, metric, x, ids, qs, k, "d=%d" % d)
        prof = nifs.flat_get_profile(g.ref)
        assert prof["sketch6_builds"] == 1, prof
        assert prof["sketch6_launches"] == len(qs), prof
        assert prof["sketch6_fallbacks"] <= 1, prof
        assert prof["sketch6_bytes"] == len(qs) * ((n + 63) // 64) * tile_bytes(d), prof
        assert prof["sketch6_candidates"] >= (len(qs) - prof["sketch6_fallbacks"]) * min(k, n), prof
        assert prof["sketch_launches"] == prof["sketch6_fallbacks"], prof  # (the int8 pass: only behind a miss)


@pytest.mark.parametrize("d", [128, 129, 191, 193, 255, 256, 257])
def test_tile_ends_and_plane_widths(nifs, oracle_mod, d, vt_debug):
    """One row to just past two tiles, at both plane widths.  A tile of ld8 = 128 is seven loads, fewer than the ring of
    eight: the 6-bit path declines d <= 128 and the int8 sketch serves as ever."""
    vt_debug.set("force_sketch6", 1)
    for n in (1, 63, 64, 65, 129):
        x, ids = make_corpus(n, d, 7700 + d + n, True, oracle_mod, dup_frac=0.0)
        g = loaded(nifs, COS, x, ids)
        qs = queries(np.random.default_rng(d + n), x, 3, COS, oracle_mod) if n > 3 else x[:1].copy()
        check(nifs, oracle_mod, g.ref, COS, x, ids, qs, 10, "d=%d n=%d" % (d, n))
        prof = nifs.flat_get_profile(g.ref)
        if d <= 128:
            assert prof["sketch6_launches"] == 0 and prof["sketch6_builds"] == 0 and prof["sketch_launches"] == len(qs), prof
        else:
            assert prof["sketch6_launches"] == len(qs), prof


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_every_reduce_order(nifs, oracle_mod, order, vt_debug):
    vt_debug.set("force_sketch6", 1)
    oracle_mod.set_reduce_order(order)
    try:
        n, d = 7000, 193
        for metric in (COS, IP):
            x, ids = make_corpus(n, d, 7800 + order + metric, metric == COS, oracle_mod, tie_block=20)
            g = loaded(nifs, metric, x, ids, order)
            qs = queries(np.random.default_rng(order), x, 5, metric, oracle_mod)
            check(nifs, oracle_mod, g.ref, metric, x, ids, qs, 10, "order=%d" % order)
            prof = nifs.flat_get_profile(g.ref)
            assert prof["sketch6_launches"] == len(qs) and prof["sketch6_fallbacks"] <= 1, prof
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


@pytest.mark.parametrize("metric", [COS, IP, NIP])
def test_adversarial_rows(nifs, oracle_mod, metric, vt_debug):
    """Un-normalised rows scaled by U(8, 24), spiky rows with one large coordinate, zero rows, duplicates."""
    vt_debug.set("force_sketch6", 1)
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
    g = loaded(nifs, metric, x, ids)
    qs = queries(rng, x, 8, metric, oracle_mod)
    qs[2] = x[spiky[0]]
    qs[3] = 0.0
    qs[3, 5] = 1.0
    for k in (1, 10, 32):
        check(nifs, oracle_mod, g.ref, metric, x, ids, qs, k)
    assert nifs.flat_get_profile(g.ref)["sketch6_launches"] > 0


@pytest.mark.parametrize("metric", [IP, NIP])
def test_magnitudes_near_overflow_decline(nifs, oracle_mod, metric, vt_debug):
    """A dot of these rows can overflow f32: K1's own scan decides, and neither sketch pass is launched."""
    vt_debug.set("force_sketch6", 1)
    n, d = 5000, 192
    x, ids = make_corpus(n, d, 77, False, oracle_mod)
    x[10] = 3e37
    g = loaded(nifs, metric, x, ids)
    packed = oracle_mod.pack_ids(ids)
    q = np.full(d, 2.0, np.float32)
    got = nifs.flat_search(g.ref, q, 5)
    try:
        want = bits(oracle_mod.matrix_search(metric, x, packed, q, 5))
    except oracle_mod.OracleError as e:  # ("metric overflow": the search must fail the same way)
        assert got[0] == "error" and "overflow" in str(got[1]), (got, e)
    else:
        assert got[0] == "ok" and bits(got[1]) == want, (got, want)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch6_launches"] == 0 and prof["sketch_launches"] == 0, prof


def test_uncertified_passes_fall_back_and_then_stop(nifs, oracle_mod, vt_debug):
    """Every third row is a copy of the query's row: every block's list fills with ties.  The int8 sketch or the rows
    serve each search, the misses are counted, and after four in a row the shard stops taking the 6-bit path."""
    vt_debug.set("force_sketch6", 1)
    n, d, k = 30000, 192, 10
    x, ids = make_corpus(n, d, 9300, True, oracle_mod)
    x = x.copy()
    at = with_copies(x, 4242, 3)
    q = x[4242].copy()
    want = oracle_mod.matrix_search(COS, x, oracle_mod.pack_ids(ids), q, k)
    assert [h[0] for h in want] == [ids[r] for r in at[:k]]
    g = loaded(nifs, COS, x, ids)
    seen = []
    for _ in range(MISS_LIMIT + 3):
        assert bits(unwrap(nifs.flat_search(g.ref, q, k))) == bits(want)
        seen.append(nifs.flat_get_profile(g.ref)["sketch6_launches"])
    prof = nifs.flat_get_profile(g.ref)
    assert seen == [1, 2, 3, 4, 4, 4, 4], seen
    assert prof["sketch6_fallbacks"] == MISS_LIMIT and prof["sketch6_launches"] == MISS_LIMIT, prof
    assert prof["sketch_launches"] + prof["scan_launches"] >= len(seen), prof


@pytest.mark.parametrize("metric", [COS, IP, NIP])
def test_hundreds_of_scattered_ties_are_served_in_one_chain(nifs, oracle_mod, metric, vt_debug):
    """300 copies of the query's row, every 100th row: all tie the k-th key, no block's list fills -- the 6-bit pass, its
    certifying tail, the gathered K1 and its select serve the search; neither the int8 pass nor a scan of the rows runs."""
    vt_debug.set("force_sketch6", 1)
    n, d, k = 30000, 192, 10
    x, ids = make_corpus(n, d, 9100 + metric, metric == COS, oracle_mod)
    x = x.copy()
    at = with_copies(x, 4242, 100)
    assert len(at) == 300
    q = x[4242].copy()
    want = oracle_mod.matrix_search(metric, x, oracle_mod.pack_ids(ids), q, k)
    assert [h[0] for h in want] == [ids[r] for r in at[:k]]
    g = loaded(nifs, metric, x, ids)
    nq = 3
    for _ in range(nq):
        assert bits(unwrap(nifs.flat_search(g.ref, q, k))) == bits(want)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch6_launches"] == nq and prof["sketch6_fallbacks"] == 0, prof
    assert 300 * nq <= prof["sketch6_candidates"] <= CAND_CAP * nq, prof
    assert prof["sketch_launches"] == 0 and prof["scan_launches"] == nq and prof["scan_bytes"] == prof["sketch6_bytes"], prof


def test_limit_33_takes_the_int8_sketch(nifs, oracle_mod, vt_debug):
    vt_debug.set("force_sketch6", 1)
    x, ids = make_corpus(9000, 192, 21, True, oracle_mod, tie_block=16)
    g = loaded(nifs, COS, x, ids)
    qs = queries(np.random.default_rng(9), x, 4, COS, oracle_mod)
    check(nifs, oracle_mod, g.ref, COS, x, ids, qs, 33)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch6_launches"] == 0 and prof["sketch_launches"] == len(qs), prof


def test_force_sketch_alone_never_selects_the_6bit_path(nifs, oracle_mod, vt_debug):
    vt_debug.set("force_sketch", 1)
    x, ids = make_corpus(9000, 192, 22, True, oracle_mod, tie_block=16)
    g = loaded(nifs, COS, x, ids)
    qs = queries(np.random.default_rng(10), x, 4, COS, oracle_mod)
    check(nifs, oracle_mod, g.ref, COS, x, ids, qs, 10)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch6_launches"] == 0 and prof["sketch6_builds"] == 0 and prof["sketch_launches"] == len(qs), prof


def test_switched_off_the_int8_sketch_serves(nifs, oracle_mod, vt_debug):
    vt_debug.set("force_sketch6", 1)
    vt_debug.set("sketch6", 0)
    x, ids = make_corpus(9000, 192, 23, False, oracle_mod)
    g = loaded(nifs, IP, x, ids)
    qs = queries(np.random.default_rng(11), x, 3, IP, oracle_mod)
    check(nifs, oracle_mod, g.ref, IP, x, ids, qs, 10)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch6_launches"] == 0 and prof["sketch6_builds"] == 0 and prof["sketch_launches"] == len(qs), prof


def test_mutations_patch_then_rebuild_the_6bit_sketch(nifs, oracle_mod, vt_debug):
    """Upserts, swap-deletes and an append are patched row by row; more than kMaxDerivedDirty mutated rows rebuild."""
    vt_debug.set("force_sketch6", 1)
    metric, n, d = IP, 9000, 160
    x, ids = make_corpus(n, d, 4243, False, oracle_mod, tie_block=20)
    x, ids = x.copy(), list(ids)
    g = loaded(nifs, metric, x, ids)
    rng = np.random.default_rng(6)
    qs = queries(rng, x, 5, metric, oracle_mod)
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
    assert prof["sketch6_builds"] == 1 and prof["sketch6_patched_rows"] >= 6, prof
    assert prof["sketch6_launches"] >= 4 * len(qs) - 4, prof
    m = 70000  # a bulk load of more rows than kMaxDerivedDirty: rebuilt, not patched
    y, _ = make_corpus(m, d, 99, False, oracle_mod)
    yids = [b"zz-x%08d" % i for i in range(m)]
    unwrap(nifs.flat_load_matrix(g.ref, yids, y))
    x, ids = np.vstack([x, y]), ids + list(yids)
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs[:3], 10, "bulk")
    assert nifs.flat_get_profile(g.ref)["sketch6_builds"] == 2


def test_no_room_for_the_6bit_sketch_means_the_int8_one(nifs, oracle_mod, request, vt_debug):
    """(test_refuse_sketch6, libvettore_hip_hooks.so only: the test re-runs itself there.)"""
    if support.rerun_with_hooks_library(request):
        return
    vt_debug.set("test_refuse_sketch6", 1)
    vt_debug.set("force_sketch6", 1)
    x, ids = make_corpus(8000, 192, 12, True, oracle_mod)
    g = loaded(nifs, COS, x, ids)
    check(nifs, oracle_mod, g.ref, COS, x, ids, queries(np.random.default_rng(2), x, 4, COS, oracle_mod), 10)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch6_launches"] == 0 and prof["sketch6_builds"] == 0 and prof["sketch_launches"] == 4, prof


def test_concurrent_readers(nifs, oracle_mod, vt_debug):
    """Four readers on their own contexts (coalescing off), each with its own lists, candidate rows and result block."""
    vt_debug.set("force_sketch6", 1)
    vt_debug.set("coalesce", 0)
    metric = COS
    x, ids = make_corpus(20000, 136, 15, True, oracle_mod, tie_block=20)
    g = GpuIndex(nifs, metric)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    qs = queries(np.random.default_rng(5), x, 16, metric, oracle_mod)
    unwrap(nifs.flat_search(g.ref, qs[0], 10))  # (builds both sketches)
    packed = oracle_mod.pack_ids(ids)
    want = [bits(oracle_mod.matrix_search(metric, x, packed, q, 10)) for q in qs]
    nifs.flat_set_profiling(g.ref, True)
    errors = []

    def run(t):
        for rep in range(3):
            for i in range(t, len(qs), 4):
                got = bits(unwrap(nifs.flat_search(g.ref, qs[i], 10)))
                if got != want[i]:
                    errors.append((t, rep, i))

    ths = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors, errors[:5]
    assert nifs.flat_get_profile(g.ref)["sketch6_launches"] > 0


def test_a_two_shard_handle(nifs, oracle_mod, vt_debug):
    vt_debug.set("force_sketch6", 1)
    x, ids = make_corpus(20000, 160, 14, True, oracle_mod, tie_block=16)
    ref = nifs.flat_new_sharded(COS, [0, 0])
    unwrap(nifs.flat_load_matrix(ref, ids, x))
    nifs.flat_set_profiling(ref, True)
    check(nifs, oracle_mod, ref, COS, x, ids, queries(np.random.default_rng(4), x, 5, COS, oracle_mod), 10)
    assert nifs.flat_get_profile(ref)["sketch6_launches"] >= 5 * 2 - 2
