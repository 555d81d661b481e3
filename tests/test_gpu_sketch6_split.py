"""GPU parity tests for the 6-bit pass with its third query level kept off the L plane, its operands read through the scalar
cache and its loop of wave-uniform branches (sketch6_scan_kernel, vettore_amd/csrc/vt_sketch_nibble.hip), and for the tail that
reads the pass's word arrays (sketch_tail_kernel, vt_sketch.hip): DESIGN.md 4.10.

Every hit equals the oracle's bit for bit and no search falls back: rows built so that the dropped term sits at an end of
its range, a plane width that is no multiple of the load ring, a corpus on which every wave owns two or three tiles, and
the list sizes at which the tail's first sweep ends inside a group of loads."""
import numpy as np
import pytest

import sketch6_split_ref as split
from test_gpu_parity import GpuIndex, bits, nifs, unwrap  # noqa: F401  (nifs: fixture)
from test_gpu_sketch import COS, IP, check, make_corpus, queries
from test_gpu_sketch6 import CAND_CAP, loaded

pytestmark = pytest.mark.gpu

WAVES = 4096  # 256 CUs x 4 blocks x 4 waves: what the host launches, whatever n


def no_fallback(nifs, g, nq):
    prof = nifs.flat_get_profile(g.ref)
    assert prof["sketch6_launches"] == nq and prof["sketch6_fallbacks"] == 0, prof
    assert prof["sketch_launches"] == 0, prof
    assert prof["sketch6_tail_words"] == nq, prof  # (every tail read the pass's word arrays, not the lists)
    return prof


@pytest.mark.parametrize("metric", [COS, IP])
@pytest.mark.parametrize("d", [192, 768])
def test_the_dropped_term_at_either_end_of_its_range(nifs, oracle_mod, metric, d, vt_debug):
    vt_debug.set("force_sketch6", 1)
    rng = np.random.default_rng(50 + d)
    q = rng.uniform(-1, 1, d).astype(np.float32)
    if metric == COS:
        q = oracle_mod.normalize_l2(q)
    n = 64 * 5 + 3
    for mirror in (False, True):
        x, _ = split.adversarial_rows(q, n, 3 * d + metric, mirror)
        ids = [b"doc-%08d" % i for i in range(n)]
        g = loaded(nifs, metric, x, ids)
        qs = np.stack([q, x[n // 2], -q])
        for k in (1, 10, 32):
            check(nifs, oracle_mod, g.ref, metric, x, ids, qs, k, "mirror=%s" % mirror)
        no_fallback(nifs, g, 3 * len(qs))


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_a_plane_width_that_is_no_multiple_of_the_ring(nifs, oracle_mod, n, vt_debug):
    """d = 320: ld8 = 384, twelve H-runs and six L-runs."""
    vt_debug.set("force_sketch6", 1)
    d = 320
    x, ids = make_corpus(n, d, 8100 + n, True, oracle_mod, dup_frac=0.0)
    g = loaded(nifs, COS, x, ids)
    qs = queries(np.random.default_rng(n), x, 3, COS, oracle_mod) if n > 3 else x[:1].copy()
    check(nifs, oracle_mod, g.ref, COS, x, ids, qs, 10, "n=%d" % n)
    no_fallback(nifs, g, len(qs))


@pytest.fixture(scope="module")
def ring_corpus(oracle_mod):
    """Waves own two and three tiles: n = 2 * 4096 * 64 + 65 rows of d = 192 (0.4 GB), 40 verbatim copies of one row spread
    over the first, the middle and the last tile."""
    n, d = 2 * WAVES * 64 + 65, 192
    rng = np.random.default_rng(8200)
    x = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    x /= np.sqrt((x.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)
    src = n // 3
    mid = (n // 64 // 2) * 64
    at = np.concatenate([np.arange(0, 56, 4), mid + np.arange(0, 52, 4), n - 1 - np.arange(0, 52, 4)])
    assert len(at) == 40 and src not in at
    at = np.sort(np.concatenate([at, [src]]))  # the row and its 40 copies
    x[at] = x[src]
    ids = [b"doc-%08d" % i for i in range(n)]
    return x, ids, at, src, oracle_mod.pack_ids(ids)


def test_the_ring_runs_across_tile_ends(nifs, oracle_mod, ring_corpus, vt_debug):
    vt_debug.set("force_sketch6", 1)
    x, ids, at, src, packed = ring_corpus
    n = len(x)
    assert (n + 63) // 64 == 2 * WAVES + 2
    g = loaded(nifs, COS, x, ids)
    rng = np.random.default_rng(8201)
    qs = np.stack([x[src], oracle_mod.normalize_l2(rng.uniform(-1, 1, x.shape[1]).astype(np.float32)), x[n - 1]])
    k = 32
    for i, q in enumerate(qs):
        want = oracle_mod.matrix_search(COS, x, packed, q, k)
        if i == 0:
            assert [h[0] for h in want] == [ids[r] for r in at[:k]]
        assert bits(unwrap(nifs.flat_search(g.ref, q, k))) == bits(want), i
    prof = no_fallback(nifs, g, len(qs))
    # the tail's counters: at least k candidates a query, at most the cap; one gathered K1 behind every pass
    assert k * len(qs) <= prof["sketch6_candidates"] <= CAND_CAP * len(qs), prof
    assert prof["scan_launches"] == len(qs), prof


@pytest.mark.parametrize("k", [1, 32])
def test_the_tails_first_sweep_boundary(nifs, oracle_mod, k, vt_debug):
    """n = 4096 * 64 + 1: every wave owns a tile and one owns two; the lists hold 1 024 x 64 slots whatever k is."""
    vt_debug.set("force_sketch6", 1)
    n, d = WAVES * 64 + 1, 192
    rng = np.random.default_rng(8300)
    x = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    x /= np.sqrt((x.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)
    x[n - 1] = x[7]
    ids = [b"doc-%08d" % i for i in range(n)]
    g = loaded(nifs, COS, x, ids)
    qs = np.stack([x[7], oracle_mod.normalize_l2(rng.uniform(-1, 1, d).astype(np.float32))])
    check(nifs, oracle_mod, g.ref, COS, x, ids, qs, k)
    no_fallback(nifs, g, len(qs))
