"""GPU parity tests for the tail behind K1q's pass (sketch_tail_kernel, vettore_amd/csrc/vt_sketch.hip):
one block certifies the pass and, when the candidates are few, rescores them itself with K1's arithmetic and selects
the hits; longer candidate lists go through the gathered K1, and what cannot be certified through a scan of the rows.

Whichever of the three served a search, every hit equals the oracle's restatement of flat.rs:96-124 bit for bit.
"""
import threading

import numpy as np
import pytest

from test_gpu_parity import GpuIndex, bits, nifs, unwrap  # noqa: F401  (nifs: fixture)
from test_gpu_sketch import COS, IP, NIP, check, make_corpus, queries

pytestmark = pytest.mark.gpu

FUSE_MAX = 256  # kTailFuseMax: candidates the tail's block rescored itself at most
CAND_CAP = 4096  # the int8 tier's cand_cap (host/vt_sketchtiers.h)


def with_copies(x, row, every):
    """Every `every`-th row becomes a verbatim copy of x[row]; returns the rows that hold one."""
    at = np.arange(row % every, len(x), every)
    x[at] = x[row]
    return at


@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("metric", [COS, IP, NIP])
def test_the_tail_rescored_with_k1_arithmetic(nifs, oracle_mod, metric, order, vt_debug):
    """Limits 1, 10, 100, 128 and n < k, every reduce order, d with and without a scalar tail: the candidates of the small
    limits are rescored by the tail itself, and its sums are K1's (the oracle's for that order)."""
    vt_debug.set("force_sketch", 1)
    oracle_mod.set_reduce_order(order)
    try:
        for d, n in ((192, 30000), (100, 9000), (203, 7)):
            x, ids = make_corpus(n, d, 8100 + 10 * metric + order + d, metric == COS, oracle_mod, tie_block=min(48, n // 2))
            g = GpuIndex(nifs, metric, order)
            unwrap(nifs.flat_load_matrix(g.ref, ids, x))
            nifs.flat_set_profiling(g.ref, True)
            qs = queries(np.random.default_rng(order + d), x, 6, metric, oracle_mod)
            for k in (1, 10, 100, 128):
                nifs.flat_get_profile(g.ref, reset=True)
                check(nifs, oracle_mod, g.ref, metric, x, ids, qs, k, "d=%d n=%d order=%d" % (d, n, order))
                prof = nifs.flat_get_profile(g.ref)
                assert prof["sketch_launches"] == len(qs), prof
                assert prof["sketch_fallbacks"] <= 1, prof
                served = len(qs) - prof["sketch_fallbacks"]
                assert prof["sketch_candidates"] >= served * min(k, n), prof
                if k <= 10:  # (a few dozen candidates at the most: none of them may need the gathered K1)
                    assert prof["sketch_tail_rescored"] == served, prof
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


@pytest.mark.parametrize("metric", [COS, IP, NIP])
def test_hundreds_of_scattered_ties_go_through_the_gathered_k1(nifs, oracle_mod, metric, vt_debug):
    """300 copies of the query's row, every 100th row: all of them tie the k-th key, so the candidates exceed what the
    tail rescored itself, but no block's list fills with them -- served from the sketch, and the ten hits are the ten
    copies first in id order."""
    vt_debug.set("force_sketch", 1)
    n, d, k = 30000, 192, 10
    x, ids = make_corpus(n, d, 9100 + metric, metric == COS, oracle_mod)
    x = x.copy()
    at = with_copies(x, 4242, 100)
    assert len(at) == 300
    q = x[4242].copy()  # (its own row is the best hit under all three metrics: the largest dot)
    packed = oracle_mod.pack_ids(ids)
    want = oracle_mod.matrix_search(metric, x, packed, q, k)
    assert [h[0] for h in want] == [ids[r] for r in at[:k]]  # the oracle alone: the copies, in id-byte order
    g = GpuIndex(nifs, metric)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    nifs.flat_set_profiling(g.ref, True)
    nq = 3
    for _ in range(nq):
        assert bits(unwrap(nifs.flat_search(g.ref, q, k))) == bits(want)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch_launches"] == nq and prof["sketch_fallbacks"] == 0, prof
    assert prof["sketch_candidates"] >= 300 * nq and prof["sketch_candidates"] <= CAND_CAP * nq, prof
    assert prof["sketch_tail_rescored"] == 0, prof  # (more than FUSE_MAX candidates)
    assert 300 > FUSE_MAX


@pytest.mark.parametrize("metric", [COS, IP, NIP])
def test_thousands_of_ties_are_not_certified(nifs, oracle_mod, metric, vt_debug):
    """5 000 copies, every 6th row: over the candidate cap and over every block's list -- counted as a fall-back, and the
    scan of the rows gives the oracle's hits."""
    vt_debug.set("force_sketch", 1)
    n, d, k = 30000, 192, 10
    x, ids = make_corpus(n, d, 9200 + metric, metric == COS, oracle_mod)
    x = x.copy()
    at = with_copies(x, 4242, 6)
    assert len(at) == 5000 and len(at) > CAND_CAP
    q = x[4242].copy()
    packed = oracle_mod.pack_ids(ids)
    want = oracle_mod.matrix_search(metric, x, packed, q, k)
    assert [h[0] for h in want] == [ids[r] for r in at[:k]]
    g = GpuIndex(nifs, metric)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    nifs.flat_set_profiling(g.ref, True)
    nq = 3
    for _ in range(nq):
        assert bits(unwrap(nifs.flat_search(g.ref, q, k))) == bits(want)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch_launches"] == nq and prof["sketch_fallbacks"] == nq, prof
    assert prof["sketch_tail_rescored"] == 0, prof


@pytest.mark.parametrize("metric", [IP, NIP])
def test_rows_that_leave_k1s_f32_path_never_reach_the_tail(nifs, oracle_mod, metric, vt_debug):
    """Rows whose dot with the query leaves f32 (K1's f64 recovery or "metric overflow") make the pass decline before any
    launch, so the tail never sees such a candidate: K1's own scan answers, as the oracle does."""
    vt_debug.set("force_sketch", 1)
    n, d = 6000, 72
    x, ids = make_corpus(n, d, 78, False, oracle_mod)
    x = x.copy()
    x[11] = 2.5e37
    x[4000] = -2.5e37
    g = GpuIndex(nifs, metric)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    nifs.flat_set_profiling(g.ref, True)
    packed = oracle_mod.pack_ids(ids)
    for q in (np.full(d, 1.5, np.float32), np.full(d, 16.0, np.float32)):
        got = nifs.flat_search(g.ref, q, 5)
        try:
            want = bits(oracle_mod.matrix_search(metric, x, packed, q, 5))
        except oracle_mod.OracleError as e:
            assert got[0] == "error" and "overflow" in str(got[1]), (got, e)
        else:
            assert got[0] == "ok" and bits(got[1]) == want, (got, want)
    assert nifs.flat_get_profile(g.ref)["sketch_launches"] == 0


def test_concurrent_readers_through_the_tail(nifs, oracle_mod, vt_debug):
    """Six readers on their own contexts, three rounds: each context has its own lists, candidate rows and result block."""
    vt_debug.set("force_sketch", 1)
    vt_debug.set("coalesce", 0)
    metric = COS
    x, ids = make_corpus(20000, 136, 16, True, oracle_mod, tie_block=20)
    g = GpuIndex(nifs, metric)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    qs = queries(np.random.default_rng(8), x, 24, metric, oracle_mod)
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
