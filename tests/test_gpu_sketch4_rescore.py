"""K1n's chain end to end with its last link rescoring straight from the pass's lists (DESIGN.md 4.10;
vt_sketch4_rescore.hip): blit, pass, threshold, refine, and one kernel that takes the candidates under the exact threshold
Kt' from the lists, rescores them, keeps the rows whose rank word is <= Kt' and writes the sorted result itself -- no collect,
no gathered K1, one host wait.  Every hit equals the oracle's restatement of flat.rs:96-124 bit for bit; `sketch4_finished`
counts the searches that kernel delivered.  With more survivors than its short list holds, the collect, the lists and the
select run over the pass's lists behind a second wait: not a fallback, no miss counted.
"""
import numpy as np
import pytest

from test_gpu_parity import GpuIndex, bits, nifs, unwrap  # noqa: F401  (nifs: fixture)
from test_gpu_sketch import COS, IP, check, make_corpus, queries
from test_gpu_sketch6 import loaded

pytestmark = pytest.mark.gpu

_corpora = {}


def corpus(oracle_mod, n, d, normalize, **kw):
    """Computed once, shared, never written to."""
    key = (n, d, normalize, tuple(sorted(kw.items())))
    if key not in _corpora:
        x, ids = make_corpus(n, d, 7300 + d + int(normalize), normalize, oracle_mod, **kw)
        x.setflags(write=False)
        _corpora[key] = (x, ids)
    return _corpora[key]


@pytest.mark.parametrize("metric,n,d,order", [(COS, 20000, 768, 3), (IP, 40000, 200, 3), (COS, 20000, 321, 1)])
def test_random_rows_are_delivered_from_the_lists(nifs, oracle_mod, metric, n, d, order, vt_debug):
    """Rows of three segments, of one padded one, and of two with a scalar tail of one, the default order and another:
    k = 1 and 10, every search delivered by the rescoring kernel."""
    vt_debug.set("force_sketch6", 3)
    oracle_mod.set_reduce_order(order)
    try:
        x, ids = corpus(oracle_mod, n, d, metric == COS, dup_frac=0.0)
        g = loaded(nifs, metric, x, ids, order)
        qs = queries(np.random.default_rng(n + d), x, 5, metric, oracle_mod)
        for k in (1, 10):
            check(nifs, oracle_mod, g.ref, metric, x, ids, qs, k, "k=%d" % k)
        prof = nifs.flat_get_profile(g.ref)
        # (a certificate may refuse once, as in test_gpu_sketch4.py; whatever it grants is delivered, none by a second wait)
        assert prof["sketch4_launches"] == 2 * len(qs) and prof["sketch4_fallbacks"] <= 1, prof
        assert prof["sketch4_finished"] == prof["sketch4_launches"] - prof["sketch4_fallbacks"], prof
        assert prof["sketch4_candidates"] >= 11 * (len(qs) - 1), prof
        assert prof["sketch5_launches"] == prof["sketch4_fallbacks"], prof
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


def test_a_tie_block_is_ordered_by_id(nifs, oracle_mod, vt_debug):
    """48 identical rows in 20 000 and a query that finds them: they tie the k-th rank word, all survive the filter, and the
    id ranks decide -- delivered."""
    vt_debug.set("force_sketch6", 3)
    x, ids = corpus(oracle_mod, 20000, 256, True, tie_block=48)
    row = len(x) // 2  # (the block's first row)
    assert np.all(x[row:row + 48] == x[row]) and not np.all(x[row + 48] == x[row])
    g = loaded(nifs, COS, x, ids)
    packed = oracle_mod.pack_ids(ids)
    nq = 0
    for k in (1, 7, 10):
        assert bits(unwrap(nifs.flat_search(g.ref, x[row], k))) == bits(oracle_mod.matrix_search(COS, x, packed, x[row], k)), k
        nq += 1
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == nq and prof["sketch4_finished"] == nq and prof["sketch4_fallbacks"] == 0, prof


def test_after_upserts_a_delete_and_an_append(nifs, oracle_mod, vt_debug):
    """The lists name rows of the column as patched: upserts that become a query's best hits, a swap-delete and an append."""
    vt_debug.set("force_sketch6", 3)
    metric, n, d = IP, 20000, 160
    x, ids = corpus(oracle_mod, n, d, False, tie_block=20)
    x, ids = x.copy(), list(ids)
    g = loaded(nifs, metric, x, ids)
    qs = queries(np.random.default_rng(61), x, 4, metric, oracle_mod)
    check(nifs, oracle_mod, g.ref, metric, x, ids, qs, 10, "fresh")
    finished = nifs.flat_get_profile(g.ref)["sketch4_finished"]
    assert finished >= len(qs) - 1
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
    # (whether the column was patched or rebuilt is test_gpu_sketch4.py's business: here, that the chain went on delivering)
    assert prof["sketch4_finished"] > finished and prof["sketch4_fallbacks"] <= 3, prof


def test_thousands_of_ties_take_the_second_wait_over_the_lists(nifs, oracle_mod, vt_debug):
    """5 000 scattered copies of the query's row in 30 000 tie the k-th key: more survivors than the short list holds.  No
    candidate array was left: the collect runs over the pass's lists behind the second wait, then the lists and the select.
    The hits are the oracle's, no miss is counted, and the search is not counted as finished by the rescoring kernel; the
    next search on the same handle is delivered again."""
    vt_debug.set("force_sketch6", 3)
    n, d, k = 30000, 256, 10
    x, ids = corpus(oracle_mod, n, d, True, dup_frac=0.0)
    x = x.copy()
    at = np.sort(np.random.default_rng(59).choice(n, 5000, replace=False))
    x[at] = x[at[3]]
    q = x[at[3]].copy()
    packed = oracle_mod.pack_ids(ids)
    want = oracle_mod.matrix_search(COS, x, packed, q, k)
    assert [h[0] for h in want] == [ids[r] for r in at[:k]]
    g = loaded(nifs, COS, x, ids)
    for _ in range(2):
        assert bits(unwrap(nifs.flat_search(g.ref, q, k))) == bits(want)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == 2 and prof["sketch4_finished"] == 0 and prof["sketch4_fallbacks"] == 0, prof
    assert prof["sketch4_candidates"] >= 2 * 5000 and prof["sketch5_launches"] == 0 and prof["scan_launches"] == 2, prof
    plain = oracle_mod.normalize_l2(np.random.default_rng(58).uniform(-1, 1, d).astype(np.float32))
    assert bits(unwrap(nifs.flat_search(g.ref, plain, k))) == bits(oracle_mod.matrix_search(COS, x, packed, plain, k))
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch4_launches"] == 3 and prof["sketch4_finished"] == 1 and prof["sketch4_fallbacks"] == 0, prof
