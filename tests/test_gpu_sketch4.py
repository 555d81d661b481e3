"""GPU parity tests for K1n: lone cosine / dot searches with limits up to 10 nominated from the 4-bit sketch of the rows
(sketch4_scan_kernel, vettore_amd/csrc/vt_sketch_nibble.hip) with the threshold taken from the exact keys of k
rows (sketch_refine_kernel, vt_sketch.hip), and the 5-bit sketch (K1f), the 6-bit sketch (K1s), the int8 sketch (K1q) and
the f32 rows behind it, in that order.

Like the other sketches it is an accelerator and must never show in a result: every hit equals the oracle's restatement of
flat.rs:96-124 bit for bit.  force_sketch6 = 3 sends these small corpora where the cost model sends rows of GBs (= 2 forces
the 5-bit and 6-bit paths alone, = 1 the 6-bit one; VT_SKETCH6=3 switches the 4-bit path off and leaves the other two).
"""
import numpy as np
import pytest

import support
from test_gpu_parity import GpuIndex, bits, nifs, unwrap  # noqa: F401  (nifs: fixture)
from test_gpu_sketch import COS, IP, check, make_corpus, queries
from test_gpu_sketch6 import loaded

pytestmark = pytest.mark.gpu

CAND_CAP = 131072  # the 4-bit tier's cand_cap (host/vt_sketchtiers.h)
MISS_LIMIT = 4     # ... and its miss_limit


def tile_bytes(d):
    ld8 = (d + 127) // 128 * 128
    return (ld8 // 32 + 1) * 1024


@pytest.mark.parametrize("metric", [COS, IP])
@pytest.mark.parametrize("k", [1, 10])
def test_lone_searches_from_the_4bit_sketch_equal_the_oracle(nifs, oracle_mod, metric, k, vt_debug):
    """n = 5 (fewer rows than k = 10: the exact threshold stands aside), 4 133 (a partial last tile) and 20 000 with a block
    of identical rows; d off the 32- and 128-element grids and on them.  The pass serves (almost) all of them, is priced at
    whole tiles of ld8 / 32 + 1 KiB, and the 5-bit pass runs only behind a miss."""
    vt_debug.set("force_sketch6", 3)
    for d, n, tie in ((200, 5, 0), (193, 4133, 20), (256, 20000, 48)):
        x, ids = make_corpus(n, d, 8400 + metric + d, metric == COS, oracle_mod, **({"tie_block": tie} if tie else {"dup_frac": 0.0}))
        g = loaded(nifs, metric, x, ids)
        qs = queries(np.random.default_rng(k + d), x, 6, metric, oracle_mod) if n > 6 else x[:2].copy()
        check(nifs, oracle_mod, g.ref, metric, x, ids, qs, k, "d=%d n=%d" % (d, n))
        prof = nifs.flat_get_profile(g.ref)
        assert prof["sketch4_builds"] == 1, prof
        assert prof["sketch4_launches"] == len(qs), prof
        assert prof["sketch4_fallbacks"] <= 1, prof
        assert prof["sketch4_bytes"] == len(qs) * ((n + 63) // 64) * tile_bytes(d), prof
        assert prof["sketch4_candidates"] >= (len(qs) - prof["sketch4_fallbacks"]) * min(k, n), prof
        assert prof["sketch5_launches"] == prof["sketch4_fallbacks"], prof


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_every_reduce_order(nifs, oracle_mod, order, vt_debug):
    """The refine kernel rescores in the index's reduce order: a threshold from another order's sums could sit one f32 step
    below the k-th key and lose it.  d = 203: full chunks, and a scalar tail of three."""
    vt_debug.set("force_sketch6", 3)
    oracle_mod.set_reduce_order(order)
    try:
        n, d = 7000, 203
        x, ids = make_corpus(n, d, 8450 + order, True, oracle_mod, tie_block=20)
        g = loaded(nifs, COS, x, ids, order)
        qs = queries(np.random.default_rng(order), x, 5, COS, oracle_mod)
        check(nifs, oracle_mod, g.ref, COS, x, ids, qs, 10, "order=%d" % order)
        prof = nifs.flat_get_profile(g.ref)
        assert prof["sketch4_launches"] == len(qs) and prof["sketch4_fallbacks"] <= 1, prof
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


def test_the_exact_threshold_leaves_fewer_candidates_than_the_sketchs_own(nifs, oracle_mod, vt_debug):
    """Uniform unit rows, d = 768, the 4-bit and the 5-bit chains on the same queries.  The 4-bit intervals are 2.14 times as
    wide (test_sketch4_model.py), but its band is one interval e4 = 1.98 sigma where the 5-bit chain's is two, 2 e5 = 1.84
    sigma.  The 10th of 20 000 sits near 3.3 sigma, so the counts stand as P(z > 1.32) / P(z > 1.46) = 1.30; with the
    sketch's own threshold the 4-bit band would be 3.96 sigma and three quarters of the corpus a candidate, ten times the
    5-bit count.  The bound is 2 x: between the two, far from both."""
    n, d, k = 20000, 768, 10
    x, ids = make_corpus(n, d, 8470, True, oracle_mod, dup_frac=0.0)
    qs = queries(np.random.default_rng(3), x, 6, COS, oracle_mod)[1:]
    cands = {}
    for force in (3, 2):
        vt_debug.set("force_sketch6", force)
        g = loaded(nifs, COS, x, ids)
        check(nifs, oracle_mod, g.ref, COS, x, ids, qs, k)
        prof = nifs.flat_get_profile(g.ref)
        name = "sketch4" if force == 3 else "sketch5"
        assert prof[name + "_launches"] == len(qs) and prof[name + "_fallbacks"] == 0, prof
        cands[force] = prof[name + "_candidates"]
    print("candidates over %d queries: 4-bit %d, 5-bit %d" % (len(qs), cands[3], cands[2]))
    assert cands[3] <= 2 * cands[2], cands


def test_thousands_of_candidates_in_one_chain(nifs, oracle_mod, vt_debug):
    """6 000 scattered copies of one row, d = 256, the query that row, k = 10: all tie the k-th key -- the exact threshold
    is that key -- and all are candidates.  One chain serves each search: no fallback, no older pass."""
    vt_debug.set("force_sketch6", 3)
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
    assert prof["sketch4_launches"] == nq and prof["sketch4_fallbacks"] == 0, prof
    assert 6000 * nq <= prof["sketch4_candidates"] <= CAND_CAP * nq, prof
    assert prof["sketch5_launches"] == 0 and prof["sketch6_launches"] == 0 and prof["sketch_launches"] == 0, prof
    assert prof["scan_launches"] == nq and prof["scan_bytes"] == prof["sketch4_bytes"], prof


def test_a_tile_of_copies_is_refused_and_the_5bit_sketch_answers(nifs, oracle_mod, vt_debug):
    """64 copies of the query's row fill one tile, which is one list: all its slots are candidates, the certificate is
    refused and K1f answers (its own list fills too; what lies behind it serves).  Four misses in a row and the shard stops
    taking the 4-bit path."""
    vt_debug.set("force_sketch6", 3)
    n, d, k = 9000, 192, 10
    x, ids = make_corpus(n, d, 9600, True, oracle_mod, dup_frac=0.0)
    x = x.copy()
    x[64 * 31:64 * 32] = x[64 * 31 + 5]
    q = x[64 * 31 + 5].copy()
    want = bits(oracle_mod.matrix_search(COS, x, oracle_mod.pack_ids(ids), q, k))
    g = loaded(nifs, COS, x, ids)
    seen = []
    for _ in range(MISS_LIMIT + 2):
        assert bits(unwrap(nifs.flat_search(g.ref, q, k))) == want
        seen.append(nifs.flat_get_profile(g.ref)["sketch4_launches"])
    prof = nifs.flat_get_profile(g.ref)
    assert seen == [1, 2, 3, 4, 4, 4], seen
    assert prof["sketch4_fallbacks"] == MISS_LIMIT and prof["sketch4_builds"] == 1, prof
    assert prof["sketch5_launches"] >= 1, prof


def test_state_across_100_calls(nifs, oracle_mod, vt_debug):
    """The chain's shared words (claim, fail, ticket, the published threshold) start over with every call: 100 searches,
    every fifth a query whose threshold is far from the one before."""
    vt_debug.set("force_sketch6", 3)
    n, d, k = 4133, 256, 10
    x, ids = make_corpus(n, d, 9700, True, oracle_mod, tie_block=12)
    g = loaded(nifs, COS, x, ids)
    qs = queries(np.random.default_rng(97), x, 5, COS, oracle_mod)
    packed = oracle_mod.pack_ids(ids)
    want = [bits(oracle_mod.matrix_search(COS, x, packed, q, k)) for q in qs]
    for i in range(100):
        assert bits(unwrap(nifs.flat_search(g.ref, qs[i % 5], k))) == want[i % 5], i
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == 100 and prof["sketch4_fallbacks"] <= 20, prof


def test_switched_off_the_5bit_sketch_serves(nifs, oracle_mod, vt_debug):
    vt_debug.set("force_sketch6", 3)
    vt_debug.set("sketch6", 3)
    x, ids = make_corpus(9000, 192, 33, False, oracle_mod)
    g = loaded(nifs, IP, x, ids)
    qs = queries(np.random.default_rng(11), x, 3, IP, oracle_mod)
    check(nifs, oracle_mod, g.ref, IP, x, ids, qs, 10)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == 0 and prof["sketch4_builds"] == 0 and prof["sketch5_launches"] == len(qs), prof


def test_no_room_for_the_4bit_sketch_means_the_5bit_one(nifs, oracle_mod, request, vt_debug):
    """(test_refuse_sketch4, libvettore_hip_hooks.so only: the test re-runs itself there.)"""
    if support.rerun_with_hooks_library(request):
        return
    vt_debug.set("test_refuse_sketch4", 1)
    vt_debug.set("force_sketch6", 3)
    x, ids = make_corpus(8000, 192, 12, True, oracle_mod)
    g = loaded(nifs, COS, x, ids)
    check(nifs, oracle_mod, g.ref, COS, x, ids, queries(np.random.default_rng(2), x, 4, COS, oracle_mod), 10)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == 0 and prof["sketch4_builds"] == 0 and prof["sketch5_launches"] == 4, prof


def test_force_sketch6_at_2_never_selects_the_4bit_path(nifs, oracle_mod, vt_debug):
    vt_debug.set("force_sketch6", 2)
    x, ids = make_corpus(9000, 192, 31, True, oracle_mod, tie_block=16)
    g = loaded(nifs, COS, x, ids)
    qs = queries(np.random.default_rng(10), x, 4, COS, oracle_mod)
    check(nifs, oracle_mod, g.ref, COS, x, ids, qs, 10)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == 0 and prof["sketch4_builds"] == 0 and prof["sketch5_launches"] == len(qs), prof


def test_a_limit_above_the_maximum_and_a_short_row_take_the_older_paths(nifs, oracle_mod, vt_debug):
    """Limit 11 goes to the 6-bit sketch as before; d = 128 is five loads a tile, fewer than the ring of eight: declined."""
    vt_debug.set("force_sketch6", 3)
    x, ids = make_corpus(9000, 192, 32, True, oracle_mod, tie_block=16)
    g = loaded(nifs, COS, x, ids)
    qs = queries(np.random.default_rng(9), x, 3, COS, oracle_mod)
    check(nifs, oracle_mod, g.ref, COS, x, ids, qs, 11)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == 0 and prof["sketch6_launches"] == len(qs), prof
    x, ids = make_corpus(3000, 128, 34, True, oracle_mod)
    g = loaded(nifs, COS, x, ids)
    qs = queries(np.random.default_rng(8), x, 3, COS, oracle_mod)
    check(nifs, oracle_mod, g.ref, COS, x, ids, qs, 10)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == 0 and prof["sketch4_builds"] == 0 and prof["sketch_launches"] == len(qs), prof


def test_a_dirty_row_patch_then_a_search(nifs, oracle_mod, vt_debug):
    """Upserts that become a query's best hits, a swap-delete and an append are patched into the column row by row."""
    vt_debug.set("force_sketch6", 3)
    metric, n, d = IP, 9000, 160
    x, ids = make_corpus(n, d, 5244, False, oracle_mod, tie_block=20)
    x, ids = x.copy(), list(ids)
    g = loaded(nifs, metric, x, ids)
    qs = queries(np.random.default_rng(6), x, 4, metric, oracle_mod)
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs, 10, "fresh")
    for r in (0, 17, n - 1, 4500):
        x[r] = (qs[2] * (3.0 + r % 5)).astype(np.float32)
        unwrap(nifs.flat_insert(g.ref, ids[r], x[r]))
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs, 10, "upserts")
    unwrap(nifs.flat_delete(g.ref, ids[5]))
    last = len(ids) - 1
    x[5], ids[5] = x[last], ids[last]
    x, ids = x[:last], ids[:last]
    new = (qs[3] * 9.0).astype(np.float32)
    unwrap(nifs.flat_insert(g.ref, b"zz-new", new))
    x, ids = np.vstack([x, new[None]]), ids + [b"zz-new"]
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs, 10, "delete and append")
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_builds"] == 1 and prof["sketch4_patched_rows"] >= 5, prof
    assert prof["sketch4_launches"] >= 3 * len(qs) - 3, prof
