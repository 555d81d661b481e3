"""GPU parity tests for K1f: lone cosine / dot searches with limits up to 10 nominated from the 5-bit sketch of the rows
(sketch5_scan_kernel, vettore_amd/csrc/vt_sketch_nibble.hip), with the 6-bit sketch (K1s), the int8 sketch (K1q)
and the f32 rows behind it, in that order.

Like the other sketches it is an accelerator and must never show in a result: every hit equals the oracle's restatement of
flat.rs:96-124 bit for bit.  force_sketch6 = 2 sends these small corpora where the cost model sends rows of GBs (= 1 forces
the 6-bit path alone; VT_SKETCH6=2 switches the 5-bit path off and leaves the 6-bit one).
"""
import threading

import numpy as np
import pytest

import support
from test_gpu_parity import GpuIndex, bits, nifs, unwrap  # noqa: F401  (nifs: fixture)
from test_gpu_sketch import COS, IP, NIP, check, make_corpus, queries
from test_gpu_sketch6 import loaded

pytestmark = pytest.mark.gpu

MAX_LIMIT = 10    # the 5-bit tier's max_limit (host/vt_sketchtiers.h)
CAND_CAP = 65536  # ... its cand_cap
MISS_LIMIT = 4    # ... and its miss_limit


def tile_bytes(d):
    ld8 = (d + 127) // 128 * 128
    return (5 * ld8 // 128 + 1) * 1024


@pytest.mark.parametrize("metric", [COS, IP, NIP])
@pytest.mark.parametrize("k", sorted({1, 10, MAX_LIMIT}))
def test_lone_searches_from_the_5bit_sketch_equal_the_oracle(nifs, oracle_mod, metric, k, vt_debug):
    """A tie block, 1 % duplicate rows, d off the 32- and 128-element grids and on them; the pass serves (almost) all of
    them and is priced at whole tiles of 5 ld8 / 128 + 1 KiB; the 6-bit pass runs only behind a miss."""
    vt_debug.set("force_sketch6", 2)
    for d, n in ((129, 9000), (192, 30000), (768, 4096)):
        x, ids = make_corpus(n, d, 8600 + metric + d, metric == COS, oracle_mod, tie_block=48)
        g = loaded(nifs, metric, x, ids)
        qs = queries(np.random.default_rng(k + d), x, 8, metric, oracle_mod)
        check(nifs, oracle_mod, g.ref, metric, x, ids, qs, k, "d=%d" % d)
        prof = nifs.flat_get_profile(g.ref)
        assert prof["sketch5_builds"] == 1, prof
        assert prof["sketch5_launches"] == len(qs), prof
        assert prof["sketch5_fallbacks"] <= 1, prof
        assert prof["sketch5_bytes"] == len(qs) * ((n + 63) // 64) * tile_bytes(d), prof
        assert prof["sketch5_candidates"] >= (len(qs) - prof["sketch5_fallbacks"]) * min(k, n), prof
        assert prof["sketch6_launches"] == prof["sketch5_fallbacks"], prof


@pytest.mark.parametrize("d", [128, 129, 255, 256, 257, 384, 385])
def test_tile_ends_and_plane_widths(nifs, oracle_mod, d, vt_debug):
    """One row to just past two tiles, at one, two and three L-runs.  A tile of ld8 = 128 is six loads, fewer than the ring
    of eight: the 5-bit path declines d <= 128 (as the 6-bit path does) and the int8 sketch serves."""
    vt_debug.set("force_sketch6", 2)
    for n in (1, 63, 64, 65, 129):
        x, ids = make_corpus(n, d, 8700 + d + n, True, oracle_mod, dup_frac=0.0)
        g = loaded(nifs, COS, x, ids)
        qs = queries(np.random.default_rng(d + n), x, 3, COS, oracle_mod) if n > 3 else x[:1].copy()
        check(nifs, oracle_mod, g.ref, COS, x, ids, qs, 10, "d=%d n=%d" % (d, n))
        prof = nifs.flat_get_profile(g.ref)
        if d <= 128:
            assert prof["sketch5_launches"] == 0 and prof["sketch5_builds"] == 0, prof
            assert prof["sketch6_launches"] == 0 and prof["sketch_launches"] == len(qs), prof
        else:
            assert prof["sketch5_launches"] == len(qs), prof


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_every_reduce_order(nifs, oracle_mod, order, vt_debug):
    vt_debug.set("force_sketch6", 2)
    oracle_mod.set_reduce_order(order)
    try:
        n, d = 7000, 193
        x, ids = make_corpus(n, d, 8800 + order, True, oracle_mod, tie_block=20)
        g = loaded(nifs, COS, x, ids, order)
        qs = queries(np.random.default_rng(order), x, 5, COS, oracle_mod)
        check(nifs, oracle_mod, g.ref, COS, x, ids, qs, 10, "order=%d" % order)
        prof = nifs.flat_get_profile(g.ref)
        assert prof["sketch5_launches"] == len(qs) and prof["sketch5_fallbacks"] <= 1, prof
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


def test_thousands_of_candidates_in_one_chain(nifs, oracle_mod, vt_debug):
    """6 000 scattered copies of one row, d = 256, the query that row, k = 10: all tie the k-th key and all are candidates --
    the per-wave collect, a count far above what the certifying block rescores itself, and a Kt that over a thousand
    entries tie with.  One chain serves each search: no fallback, neither older pass, K1 only as the gathered rescoring.
    (20 000 rows are 313 tiles, one per block list on this corpus: about 19 copies among a list's 64 rows.)"""
    vt_debug.set("force_sketch6", 2)
    n, d, k = 20000, 256, 10
    x, ids = make_corpus(n, d, 9500, True, oracle_mod, dup_frac=0.0)
    x = x.copy()
    at = np.sort(np.random.default_rng(95).choice(n, 6000, replace=False))
    x[at] = x[at[17]]
    q = x[at[17]].copy()
    want = oracle_mod.matrix_search(COS, x, oracle_mod.pack_ids(ids), q, k)
    assert [h[0] for h in want] == [ids[r] for r in at[:k]]
    g = loaded(nifs, COS, x, ids)
    nq = 2
    for _ in range(nq):
        assert bits(unwrap(nifs.flat_search(g.ref, q, k))) == bits(want)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch5_launches"] == nq and prof["sketch5_fallbacks"] == 0, prof
    assert 6000 * nq <= prof["sketch5_candidates"] <= CAND_CAP * nq, prof
    assert prof["sketch6_launches"] == 0 and prof["sketch_launches"] == 0, prof
    assert prof["scan_launches"] == nq and prof["scan_bytes"] == prof["sketch5_bytes"], prof


def test_uncertified_passes_fall_back_and_then_stop(nifs, oracle_mod, vt_debug):
    """Spiky rows: one coordinate -- the same one in every row -- 10^3 times the rest, so every other one quantises to 0
    in five bits (and in six, and in eight) and no interval separates two rows: every list fills with candidates.  K1s,
    K1q or the rows serve each search; after four misses in a row the shard stops taking the 5-bit path, and a rebuild of
    the column starts it again."""
    vt_debug.set("force_sketch6", 2)
    n, d, k = 9000, 192, 10
    rng = np.random.default_rng(41)
    x = rng.uniform(-1e-3, 1e-3, (n, d)).astype(np.float32)
    x[:, 7] = 1.0
    x = np.stack([oracle_mod.normalize_l2(r) for r in x])
    ids = [b"id-%08d" % i for i in range(n)]
    g = loaded(nifs, COS, x, ids)
    q = oracle_mod.normalize_l2(rng.uniform(-1, 1, d).astype(np.float32))
    want = bits(oracle_mod.matrix_search(COS, x, oracle_mod.pack_ids(ids), q, k))
    seen = []
    for _ in range(MISS_LIMIT + 2):
        assert bits(unwrap(nifs.flat_search(g.ref, q, k))) == want
        seen.append(nifs.flat_get_profile(g.ref)["sketch5_launches"])
    prof = nifs.flat_get_profile(g.ref)
    assert seen == [1, 2, 3, 4, 4, 4], seen
    assert prof["sketch5_fallbacks"] == MISS_LIMIT and prof["sketch5_builds"] == 1, prof
    assert prof["sketch6_launches"] + prof["sketch_launches"] + prof["scan_launches"] >= len(seen), prof
    m = 70000  # more rows than kMaxDerivedDirty at once: the column is rebuilt, and its misses start over
    y = rng.uniform(-1e-3, 1e-3, (m, d)).astype(np.float32)
    y[:, 7] = 1.0
    y = np.stack([oracle_mod.normalize_l2(r) for r in y])
    yids = [b"zz-%08d" % i for i in range(m)]
    unwrap(nifs.flat_load_matrix(g.ref, yids, y))
    x, ids = np.vstack([x, y]), ids + yids
    assert bits(unwrap(nifs.flat_search(g.ref, q, k))) == bits(oracle_mod.matrix_search(COS, x, oracle_mod.pack_ids(ids), q, k))
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch5_builds"] == 2 and prof["sketch5_launches"] == MISS_LIMIT + 1, prof


def test_force_sketch6_at_1_never_selects_the_5bit_path(nifs, oracle_mod, vt_debug):
    vt_debug.set("force_sketch6", 1)
    x, ids = make_corpus(9000, 192, 31, True, oracle_mod, tie_block=16)
    g = loaded(nifs, COS, x, ids)
    qs = queries(np.random.default_rng(10), x, 4, COS, oracle_mod)
    check(nifs, oracle_mod, g.ref, COS, x, ids, qs, 10)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch5_launches"] == 0 and prof["sketch5_builds"] == 0 and prof["sketch6_launches"] == len(qs), prof


def test_a_limit_above_the_maximum_takes_the_6bit_sketch(nifs, oracle_mod, vt_debug):
    vt_debug.set("force_sketch6", 2)
    x, ids = make_corpus(9000, 192, 32, True, oracle_mod, tie_block=16)
    g = loaded(nifs, COS, x, ids)
    qs = queries(np.random.default_rng(9), x, 4, COS, oracle_mod)
    check(nifs, oracle_mod, g.ref, COS, x, ids, qs, MAX_LIMIT + 1)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch5_launches"] == 0 and prof["sketch6_launches"] == len(qs), prof


def test_switched_off_the_6bit_sketch_serves(nifs, oracle_mod, vt_debug):
    vt_debug.set("force_sketch6", 2)
    vt_debug.set("sketch6", 2)
    x, ids = make_corpus(9000, 192, 33, False, oracle_mod)
    g = loaded(nifs, IP, x, ids)
    qs = queries(np.random.default_rng(11), x, 3, IP, oracle_mod)
    check(nifs, oracle_mod, g.ref, IP, x, ids, qs, 10)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch5_launches"] == 0 and prof["sketch5_builds"] == 0 and prof["sketch6_launches"] == len(qs), prof


def test_no_room_for_the_5bit_sketch_means_the_6bit_one(nifs, oracle_mod, request, vt_debug):
    """(test_refuse_sketch5, libvettore_hip_hooks.so only: the test re-runs itself there.)"""
    if support.rerun_with_hooks_library(request):
        return
    vt_debug.set("test_refuse_sketch5", 1)
    vt_debug.set("force_sketch6", 2)
    x, ids = make_corpus(8000, 192, 12, True, oracle_mod)
    g = loaded(nifs, COS, x, ids)
    check(nifs, oracle_mod, g.ref, COS, x, ids, queries(np.random.default_rng(2), x, 4, COS, oracle_mod), 10)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch5_launches"] == 0 and prof["sketch5_builds"] == 0 and prof["sketch6_launches"] == 4, prof


def test_mutations_patch_then_rebuild_the_5bit_sketch(nifs, oracle_mod, vt_debug):
    """Upserts, swap-deletes and an append are patched row by row; more than kMaxDerivedDirty mutated rows rebuild."""
    vt_debug.set("force_sketch6", 2)
    metric, n, d = IP, 9000, 160
    x, ids = make_corpus(n, d, 5243, False, oracle_mod, tie_block=20)
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
    assert prof["sketch5_builds"] == 1 and prof["sketch5_patched_rows"] >= 6, prof
    assert prof["sketch5_launches"] >= 4 * len(qs) - 4, prof
    m = 70000  # a bulk load of more rows than kMaxDerivedDirty: rebuilt, not patched
    y, _ = make_corpus(m, d, 99, False, oracle_mod)
    yids = [b"zz-x%08d" % i for i in range(m)]
    unwrap(nifs.flat_load_matrix(g.ref, yids, y))
    x, ids = np.vstack([x, y]), ids + list(yids)
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs[:3], 10, "bulk")
    assert nifs.flat_get_profile(g.ref)["sketch5_builds"] == 2


def test_concurrent_readers(nifs, oracle_mod, vt_debug):
    """Four readers on their own contexts (coalescing off), each with its own lists, candidate rows and result block."""
    vt_debug.set("force_sketch6", 2)
    vt_debug.set("coalesce", 0)
    metric = COS
    x, ids = make_corpus(20000, 136, 15, True, oracle_mod, tie_block=20)
    g = GpuIndex(nifs, metric)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    qs = queries(np.random.default_rng(5), x, 16, metric, oracle_mod)
    unwrap(nifs.flat_search(g.ref, qs[0], 10))  # (builds the three sketches)
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
    assert nifs.flat_get_profile(g.ref)["sketch5_launches"] > 0


def test_a_two_shard_handle(nifs, oracle_mod, vt_debug):
    vt_debug.set("force_sketch6", 2)
    x, ids = make_corpus(20000, 160, 14, True, oracle_mod, tie_block=16)
    ref = nifs.flat_new_sharded(COS, [0, 0])
    unwrap(nifs.flat_load_matrix(ref, ids, x))
    nifs.flat_set_profiling(ref, True)
    check(nifs, oracle_mod, ref, COS, x, ids, queries(np.random.default_rng(4), x, 5, COS, oracle_mod), 10)
    assert nifs.flat_get_profile(ref)["sketch5_launches"] >= 5 * 2 - 2
