"""K1n's chain end to end with its two-kernel finish: behind the 4-bit pass the threshold and its refinement
are one launch, and the gathered K1 keeps only the rows whose rank word is <= the exact threshold Kt' and writes the sorted
result itself (vt_scan_filter.hip) -- no select, one host wait.  Every hit still equals the oracle's restatement of
flat.rs:96-124 bit for bit; `sketch4_finished` counts the searches the filtered K1 delivered, so a test can tell that finish
from the second-wait route (more survivors than its short list holds: the lists and the select as before, not a fallback).
"""
import threading

import numpy as np
import pytest

from test_gpu_parity import GpuIndex, bits, nifs, unwrap  # noqa: F401  (nifs: fixture)
from test_gpu_sketch import COS, IP, make_corpus, queries
from test_gpu_sketch6 import loaded

pytestmark = pytest.mark.gpu

N = 20000
_corpora = {}


def corpus(oracle_mod, d, normalize, dup_frac=0.0):
    """Computed once, shared, never written to."""
    key = (d, normalize, dup_frac)
    if key not in _corpora:
        x, ids = make_corpus(N, d, 9900 + d + int(normalize), normalize, oracle_mod, dup_frac=dup_frac)
        x.setflags(write=False)
        _corpora[key] = (x, ids, oracle_mod.pack_ids(ids))
    return _corpora[key]


def copies_corpus(oracle_mod):
    """6 000 scattered copies of one row among 20 000, d = 256: (x, ids, packed ids, the row's query)."""
    if "copies" not in _corpora:
        x, ids, packed = corpus(oracle_mod, 256, True)
        x = x.copy()
        at = np.sort(np.random.default_rng(95).choice(N, 6000, replace=False))
        x[at] = x[at[17]]
        x.setflags(write=False)
        _corpora["copies"] = (x, ids, packed, x[at[17]].copy())
    return _corpora["copies"]


@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("metric", [COS, IP])
def test_the_filtered_k1_delivers_the_oracles_hits(nifs, oracle_mod, metric, order, vt_debug):
    """20 000 x 768 and 20 000 x 256, k = 1 and 10: every search is served by the 4-bit chain and delivered by the filtered
    K1 -- the survivors are the k hits and what ties the k-th, a dozen keys at most."""
    vt_debug.set("force_sketch6", 3)
    oracle_mod.set_reduce_order(order)
    try:
        for d in (768, 256):
            x, ids, packed = corpus(oracle_mod, d, metric == COS)
            g = loaded(nifs, metric, x, ids, order)
            qs = queries(np.random.default_rng(order + d), x, 4, metric, oracle_mod)
            for k in (1, 10):
                for i, q in enumerate(qs):
                    got = unwrap(nifs.flat_search(g.ref, q, k))
                    assert bits(got) == bits(oracle_mod.matrix_search(metric, x, packed, q, k)), (d, k, i)
            prof = nifs.flat_get_profile(g.ref)
            assert prof["sketch4_launches"] == 2 * len(qs) and prof["sketch4_fallbacks"] == 0, prof
            assert prof["sketch4_finished"] == prof["sketch4_launches"], prof
            assert prof["sketch5_launches"] == 0, prof
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


def test_duplicates_at_the_kth_key_are_ordered_by_id(nifs, oracle_mod, vt_debug):
    """1 % verbatim duplicates; the query is a row that stands three times or more, k below and at that number: the copies
    share a rank word, all survive the filter, and the id bytes decide among them -- still delivered."""
    vt_debug.set("force_sketch6", 3)
    x, ids, packed = corpus(oracle_mod, 256, True, dup_frac=0.01)
    _, inverse, counts = np.unique(x, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    twice = np.nonzero(counts[inverse] >= 2)[0]
    assert len(twice) >= 100
    g = loaded(nifs, COS, x, ids)
    nq = 0
    for row in twice[:6]:
        copies = int(counts[inverse[row]])
        for k in (1, copies - 1, copies, 10):
            if k < 1:
                continue
            want = oracle_mod.matrix_search(COS, x, packed, x[row], k)
            m = min(k, copies)  # (the copies lead, in the order of their id bytes)
            assert [h[0] for h in want[:m]] == sorted(ids[r] for r in np.nonzero(inverse == inverse[row])[0])[:m]
            assert bits(unwrap(nifs.flat_search(g.ref, x[row], k))) == bits(want), (row, k)
            nq += 1
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == nq and prof["sketch4_finished"] == nq and prof["sketch4_fallbacks"] == 0, prof


def test_thousands_of_ties_take_the_second_wait(nifs, oracle_mod, vt_debug):
    """6 000 copies of the query's row tie the k-th key: more survivors than the short list holds.  The lists and the select
    run behind a second wait on the candidates still on the device -- the hits are right, nothing falls back, and the
    search is not counted as finished by the filtered K1."""
    vt_debug.set("force_sketch6", 3)
    x, ids, packed, q = copies_corpus(oracle_mod)
    want = bits(oracle_mod.matrix_search(COS, x, packed, q, 10))
    g = loaded(nifs, COS, x, ids)
    for _ in range(3):
        assert bits(unwrap(nifs.flat_search(g.ref, q, 10))) == want
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == 3 and prof["sketch4_finished"] == 0 and prof["sketch4_fallbacks"] == 0, prof
    assert prof["sketch5_launches"] == 0 and prof["scan_launches"] == 3, prof


def test_100_calls_alternating_the_two_finishes(nifs, oracle_mod, vt_debug):
    """One handle, the delivered finish and the second wait in turn: the zero words ride in every call's blit, so neither
    the tickets nor the survivor count and overflow word carry over."""
    vt_debug.set("force_sketch6", 3)
    x, ids, packed, q_ties = copies_corpus(oracle_mod)
    q_plain = oracle_mod.normalize_l2(np.random.default_rng(4).uniform(-1, 1, 256).astype(np.float32))
    want = [bits(oracle_mod.matrix_search(COS, x, packed, q, 10)) for q in (q_ties, q_plain)]
    g = loaded(nifs, COS, x, ids)
    for i in range(100):
        assert bits(unwrap(nifs.flat_search(g.ref, (q_ties, q_plain)[i % 2], 10))) == want[i % 2], i
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == 100 and prof["sketch4_finished"] == 50 and prof["sketch4_fallbacks"] == 0, prof


def test_four_threads_on_one_handle(nifs, oracle_mod, vt_debug):
    """Each caller has a context of its own -- its own query image and zero words, its own survivor list."""
    vt_debug.set("force_sketch6", 3)
    x, ids, packed, q_ties = copies_corpus(oracle_mod)
    rng = np.random.default_rng(44)
    qs = [q_ties] + [oracle_mod.normalize_l2(rng.uniform(-1, 1, 256).astype(np.float32)) for _ in range(3)]
    want = [bits(oracle_mod.matrix_search(COS, x, packed, q, 10)) for q in qs]
    g = loaded(nifs, COS, x, ids)
    assert bits(unwrap(nifs.flat_search(g.ref, qs[1], 10))) == want[1]  # (the column is built before the threads start)
    bad = []

    def caller(t):
        for i in range(12):
            j = (t + i) % 4
            if bits(unwrap(nifs.flat_search(g.ref, qs[j], 10))) != want[j]:
                bad.append((t, i))

    threads = [threading.Thread(target=caller, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not bad, bad
    prof = nifs.flat_get_profile(g.ref)
    # (callers that meet may be served together by another path: how many searches took the chain is not fixed)
    assert 0 < prof["sketch4_finished"] <= prof["sketch4_launches"] <= 49 and prof["sketch4_fallbacks"] == 0, prof
