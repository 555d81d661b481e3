"""GPU parity tests for the certification behind K1s's and K1f's passes, spread over the card in two kernels
(sketch_thresh_kernel, sketch_collect_kernel, vettore_amd/csrc/vt_sketch.hip): every block's k smallest
key(lo) words, then Kt from those, the candidates of every block's own lists, one claim per block and the last block's
count.

The lists are 1 024 x 64 slots whatever n is, so the shapes here are the smallest at which the two kernels can go wrong:
a handful of live slots among slices that are otherwise empty, more than k equal words inside one slice and around the
k-th overall, the shared claim / fail / ticket words across many calls of both chains on one context, and a list that
consists of candidates alone.  The yardstick is the oracle, bit for bit, as for every other path.
"""
import functools

import numpy as np
import pytest

from test_gpu_parity import bits, nifs, unwrap  # noqa: F401  (nifs: fixture)
from test_gpu_sketch import COS, IP, check, make_corpus, queries
from test_gpu_sketch6 import loaded

pytestmark = pytest.mark.gpu

D = 192


@pytest.mark.parametrize("metric", [COS, IP])
@pytest.mark.parametrize("force,limits", [(2, (1, 10)), (1, (1, 10, 32))])
def test_few_live_entries(nifs, oracle_mod, metric, force, limits, vt_debug):
    """Live total below k, equal to k and k + 1 (Kt is the empty word or the largest live word), and slices -- nearly
    all of them -- with no live word at all.  Every search is served by its chain: no fallback, no int8 pass."""
    vt_debug.set("force_sketch6", force)
    name = "sketch5" if force == 2 else "sketch6"
    for n in (1, 9, 10, 11, 64 * 5 + 3):
        x, ids = make_corpus(n, D, 9700 + metric + n, metric == COS, oracle_mod, dup_frac=0.0)
        g = loaded(nifs, metric, x, ids)
        qs = queries(np.random.default_rng(n), x, 3, metric, oracle_mod) if n > 3 else x[:1].copy()
        for k in limits:
            check(nifs, oracle_mod, g.ref, metric, x, ids, qs, k, "n=%d" % n)
        prof = nifs.flat_get_profile(g.ref)
        print(name, metric, n, {f: prof[f] for f in (name + "_launches", name + "_fallbacks", name + "_candidates")})
        assert prof[name + "_launches"] == len(qs) * len(limits), prof
        assert prof[name + "_fallbacks"] == 0 and prof["sketch_launches"] == 0, prof


@functools.lru_cache(maxsize=None)
def tied_corpus(oracle_mod):
    """20 000 rows of d = 192 (15 MB).  Row A copied to 3 000 random places; row B copied to exactly 10 places inside one
    64-row tile (tile 100, none of A's places).  Queries: A, B and a random unit vector; the oracle's hits at 10 and 32."""
    n = 20000
    x, ids = make_corpus(n, D, 9800, True, oracle_mod, dup_frac=0.0)
    x = x.copy()
    rng = np.random.default_rng(98)
    tile = np.arange(6400, 6464)
    free = np.setdiff1d(np.arange(n), tile)
    at_a = np.sort(rng.choice(free, 3000, replace=False))
    x[at_a] = x[at_a[0]]
    at_b = np.sort(rng.choice(tile, 10, replace=False))
    x[at_b] = x[at_b[0]]
    qs = np.stack([x[at_a[0]], x[at_b[0]], oracle_mod.normalize_l2(rng.uniform(-1, 1, D).astype(np.float32))])
    packed = oracle_mod.pack_ids(ids)
    want = {k: [bits(oracle_mod.matrix_search(COS, x, packed, q, k)) for q in qs] for k in (10, 32)}
    assert [h[0] for h in want[10][0]] == [ids[r] for r in at_a[:10]]
    assert sorted(h[0] for h in want[10][1]) == sorted(ids[r] for r in at_b)
    return x, ids, qs, want


def test_multiplicity_inside_a_slice(nifs, oracle_mod, vt_debug):
    """More than k equal words sit in single slices and around the k-th overall: 3 000 copies of the first query's row
    (about ten a list, 160 a slice of the threshold kernel), ten copies of the second's inside one list.  On this seed all
    three queries certify (no list is filled by copies): 3 launches, 0 fallbacks; the assertion the issue sets is
    launches - fallbacks >= 1, and a query that fell back would still have to equal the oracle."""
    vt_debug.set("force_sketch6", 2)
    x, ids, qs, want = tied_corpus(oracle_mod)
    g = loaded(nifs, COS, x, ids)
    seen = []
    for i, q in enumerate(qs):
        assert bits(unwrap(nifs.flat_search(g.ref, q, 10))) == want[10][i], i
        prof = nifs.flat_get_profile(g.ref)
        seen.append((prof["sketch5_launches"], prof["sketch5_fallbacks"], prof["sketch5_candidates"]))
    print("launches, fallbacks, candidates after each query:", seen)
    assert seen[1][1] == seen[0][1], seen  # (the second query's list holds ten copies among 64 rows: it certifies)
    assert seen[2][0] == 3 and seen[2][0] - seen[2][1] >= 1, seen
    assert seen[0][2] >= 3000 or seen[0][1] == 1, seen


def test_state_between_calls(nifs, oracle_mod, vt_debug):
    """The same query 20 times, then limits 10 and 32 alternately ten times -- the 5-bit and the 6-bit chain in turn on one
    context and its shared count, claim, fail and ticket words.  Every answer is the first one and the oracle's, and the
    candidates grow by the same amount at every repeat: a word that is not zeroed again shows here."""
    vt_debug.set("force_sketch6", 2)
    x, ids, qs, want = tied_corpus(oracle_mod)
    g = loaded(nifs, COS, x, ids)

    def step(i, k):
        before = nifs.flat_get_profile(g.ref)
        got = bits(unwrap(nifs.flat_search(g.ref, qs[i], k)))
        after = nifs.flat_get_profile(g.ref)
        assert got == want[k][i], (i, k)
        return got, tuple(after[f] - before[f] for f in ("sketch5_candidates", "sketch6_candidates",
                                                         "sketch5_fallbacks", "sketch6_fallbacks"))

    for i in range(len(qs)):
        first = step(i, 10)
        assert first[1][0] >= 10 and first[1][1:] == (0, 0, 0), (i, first[1])
        for rep in range(19):
            assert step(i, 10) == first, (i, rep)
    for i in (0, 2):
        first10, first32 = step(i, 10), step(i, 32)
        assert first10[1][0] >= 10 and first10[1][1:] == (0, 0, 0), (i, first10[1])
        assert first32[1][1] >= 32 and first32[1][0] == 0 and first32[1][2:] == (0, 0), (i, first32[1])
        for rep in range(9):
            assert step(i, 10) == first10 and step(i, 32) == first32, (i, rep)
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch5_launches"] == 3 * 20 + 2 * 10 and prof["sketch6_launches"] == 2 * 10, prof
    assert prof["sketch_launches"] == 0, prof


def test_a_full_list_still_refuses(nifs, oracle_mod, vt_debug):
    """64 copies of one row fill one 64-row tile, so one list consists of candidates alone: the pass is not certified, the
    6-bit and the int8 pass behind it refuse for the same reason and the exact scan answers (one launch more than the
    passes booked).  The next, ordinary query on the same handle certifies: the zero count did not stick."""
    vt_debug.set("force_sketch6", 2)
    n = 64 * 9
    x, ids = make_corpus(n, D, 9900, True, oracle_mod, dup_frac=0.0)
    x = x.copy()
    x[192:256] = x[192]
    g = loaded(nifs, COS, x, ids)
    packed = oracle_mod.pack_ids(ids)
    q = x[192].copy()
    want = oracle_mod.matrix_search(COS, x, packed, q, 10)
    assert [h[0] for h in want] == ids[192:202]
    assert bits(unwrap(nifs.flat_search(g.ref, q, 10))) == bits(want)
    prof = nifs.flat_get_profile(g.ref)
    print({f: prof[f] for f in prof if f.startswith("sketch") and f.endswith(("launches", "fallbacks"))}, prof["scan_launches"])
    assert prof["sketch5_launches"] == 1 and prof["sketch5_fallbacks"] == 1, prof
    passes = prof["sketch5_launches"] + prof["sketch6_launches"] + prof["sketch_launches"]
    assert prof["scan_launches"] == passes + 1, prof  # (every pass books one launch; the exact scan one more)
    r = np.random.default_rng(99).uniform(-1, 1, D).astype(np.float32)
    q2 = oracle_mod.normalize_l2((r - (np.dot(r, q) + 3.0) * q).astype(np.float32))  # (the copies score well below zero)
    assert bits(unwrap(nifs.flat_search(g.ref, q2, 10))) == bits(oracle_mod.matrix_search(COS, x, packed, q2, 10))
    after = nifs.flat_get_profile(g.ref)
    assert after["sketch5_launches"] == 2 and after["sketch5_fallbacks"] == 1, after
    assert after["scan_launches"] == prof["scan_launches"] + 1 and after["sketch6_launches"] == prof["sketch6_launches"], after
