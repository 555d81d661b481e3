"""K1n's chain end to end with its exact threshold taken from each list's best rows, inside the pass: blit,
pass, rescore, one wait -- no threshold and no refine launch.  The chain is taken from the smallest corpus that gives every
wave of the pass a tile, multi_processor_count x 16 tiles of 64 rows (262 144 rows at 256 CUs); one tile fewer keeps the
chain as it was.  Every hit equals the oracle's restatement of flat.rs:96-124 bit for bit; `sketch4_best` counts the searches
served this way.
"""
import numpy as np
import pytest
import torch

from test_gpu_parity import GpuIndex, bits, nifs, unwrap  # noqa: F401  (nifs: fixture)
from test_gpu_sketch import COS, IP
from test_gpu_sketch6 import loaded

pytestmark = pytest.mark.gpu

_corpora = {}


def rows_for_the_chain():
    return torch.cuda.get_device_properties(0).multi_processor_count * 16 * 64


def corpus(d, normalize):
    """n rows, a tie block of 48 in the middle and 1 % verbatim duplicates; computed once, shared, never written to."""
    key = (d, normalize)
    if key not in _corpora:
        n = rows_for_the_chain()
        rng = np.random.default_rng(9100 + d + int(normalize))
        x = rng.uniform(-1.0, 1.0, size=(n, d)).astype(np.float32)
        ndup = n // 100
        x[rng.integers(0, n, ndup)] = x[rng.integers(0, n, ndup)]
        x[n // 2:n // 2 + 48] = x[n // 2]
        if normalize:
            x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
        x.setflags(write=False)
        _corpora[key] = (x, [b"doc-%08d" % i for i in range(n)])
    return _corpora[key]


def some_queries(rng, x, nq, metric, oracle_mod):
    qs = rng.uniform(-1, 1, size=(nq, x.shape[1])).astype(np.float32)
    qs[0] = x[len(x) // 2]  # sits on the block of identical rows
    qs[1] = x[3]
    return np.stack([oracle_mod.normalize_l2(q) for q in qs]) if metric == COS else qs


def search_all(nifs, oracle_mod, g, metric, x, ids, qs, ks, note):
    packed = oracle_mod.pack_ids(ids)
    for k in ks:
        for i, q in enumerate(qs):
            assert bits(unwrap(nifs.flat_search(g.ref, q, k))) == bits(oracle_mod.matrix_search(metric, x, packed, q, k)), (note, k, i)
    return len(ks) * len(qs)


@pytest.mark.parametrize("metric", [COS, IP])
def test_the_chain_is_taken_where_every_wave_owns_a_tile(nifs, oracle_mod, metric, vt_debug):
    """d = 160, k = 1 and 10: at n every search takes the new chain; at n - 64 none does, and both give the oracle's hits."""
    vt_debug.set("force_sketch6", 3)
    x, ids = corpus(160, metric == COS)
    n = len(x)
    qs = some_queries(np.random.default_rng(n + metric), x, 4, metric, oracle_mod)
    for rows, best in ((n, True), (n - 64, False)):
        g = loaded(nifs, metric, x[:rows], ids[:rows])
        nq = search_all(nifs, oracle_mod, g, metric, x[:rows], ids[:rows], qs, (1, 10), "n=%d" % rows)
        prof = nifs.flat_get_profile(g.ref)
        assert prof["sketch4_launches"] == nq and prof["sketch4_fallbacks"] <= 1, prof
        assert prof["sketch4_best"] == (nq if best else 0), prof
        assert prof["sketch4_finished"] == nq - prof["sketch4_fallbacks"], prof
        del g


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_rows_with_a_scalar_tail_in_each_reduce_order(nifs, oracle_mod, order, vt_debug):
    """d = 203 (full chunks and a scalar tail of three): the best rows' keys are formed in the index's reduce order."""
    vt_debug.set("force_sketch6", 3)
    oracle_mod.set_reduce_order(order)
    try:
        x, ids = corpus(203, True)
        g = loaded(nifs, COS, x, ids, order)
        qs = some_queries(np.random.default_rng(order), x, 3, COS, oracle_mod)
        nq = search_all(nifs, oracle_mod, g, COS, x, ids, qs, (10,), "order %d" % order)
        prof = nifs.flat_get_profile(g.ref)
        assert prof["sketch4_launches"] == nq and prof["sketch4_best"] == nq and prof["sketch4_fallbacks"] <= 1, prof
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


def test_thousands_of_ties_take_the_second_wait(nifs, oracle_mod, vt_debug):
    """2 000 scattered copies of the query's row tie the k-th key: more survivors than the short list holds.  The collect runs
    over the pass's lists behind the second wait with the word the rescoring kernel published, then the lists and the
    select: the oracle's hits, no fallback, one scan a search."""
    vt_debug.set("force_sketch6", 3)
    k = 10
    x, ids = corpus(160, True)
    x = x.copy()
    n = len(x)
    at = np.sort(np.random.default_rng(59).choice(n, 2000, replace=False))
    x[at] = x[at[3]]
    q = x[at[3]].copy()
    packed = oracle_mod.pack_ids(ids)
    want = oracle_mod.matrix_search(COS, x, packed, q, k)
    assert [h[0] for h in want] == [ids[r] for r in at[:k]]
    g = loaded(nifs, COS, x, ids)
    for _ in range(2):
        assert bits(unwrap(nifs.flat_search(g.ref, q, k))) == bits(want)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == 2 and prof["sketch4_best"] == 2 and prof["sketch4_finished"] == 0, prof
    assert prof["sketch4_fallbacks"] == 0 and prof["sketch5_launches"] == 0 and prof["scan_launches"] == 2, prof
    assert prof["sketch4_candidates"] >= 2 * 2000, prof
    plain = oracle_mod.normalize_l2(np.random.default_rng(58).uniform(-1, 1, x.shape[1]).astype(np.float32))
    assert bits(unwrap(nifs.flat_search(g.ref, plain, k))) == bits(oracle_mod.matrix_search(COS, x, packed, plain, k))
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == 3 and prof["sketch4_best"] == 3 and prof["sketch4_finished"] == 1, prof


def test_the_shared_words_start_over_with_every_call(nifs, oracle_mod, vt_debug):
    """50 calls alternating two far-apart queries on one handle: a best word, a threshold or a ticket left by the call before
    would hand one query the other's threshold."""
    vt_debug.set("force_sketch6", 3)
    x, ids = corpus(160, True)
    packed = oracle_mod.pack_ids(ids)
    qa = oracle_mod.normalize_l2(x[17])
    qb = oracle_mod.normalize_l2(-x[17])
    want = [bits(oracle_mod.matrix_search(COS, x, packed, q, 10)) for q in (qa, qb)]
    g = loaded(nifs, COS, x, ids)
    for i in range(50):
        assert bits(unwrap(nifs.flat_search(g.ref, (qa, qb)[i % 2], 10))) == want[i % 2], i
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == 50 and prof["sketch4_best"] == 50 and prof["sketch4_fallbacks"] == 0, prof
