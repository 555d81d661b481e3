"""K1n's threshold from each list's best rows against the refine's rule it replaces, on the CPU (tests/sketch4_best_ref.py;
DESIGN.md 4.10).  100 000 uniform unit rows of d = 768 quantised to 4 bits as the column is (s = max|x| / 7, rho = ||x - s X||),
a row's interval a -+ ||q|| rho about the sketch's dot a = (s X) . q, 32 queries; the rows dealt to 128 lists tile by tile as
the pass deals them (64 blocks), 64 slots a list.  Both rules' words are sound, the candidate set holds the true top k and
its ties, and the new rule leaves no more candidates than the refine's in the mean, never more than 1.10 x on one query."""
import numpy as np
import pytest

import sketch4_best_ref as best
import sketch6_ref as ref6

N, D, K, QUERIES, BLOCKS = 100_000, 768, 10, 32, 64


@pytest.fixture(scope="module")
def modelled():
    """exact[q][n], hi[q][n], lo[q][n]: the orderable words of the cosine key 1 - dot: exact, optimistic, pessimistic."""
    rng = np.random.default_rng(20260723)
    qs = rng.uniform(-1, 1, (QUERIES, D)).astype(np.float32)
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    qn = np.linalg.norm(qs.astype(np.float64), axis=1)
    exact, hi, lo = (np.zeros((QUERIES, N), np.uint32) for _ in range(3))
    for at in range(0, N, 20_000):
        x = rng.uniform(-1, 1, (20_000, D)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        s = np.abs(x).max(axis=1) / np.float32(7)
        xa = (s[:, None] * np.rint(x / s[:, None])).astype(np.float32)
        rho = np.linalg.norm((x - xa).astype(np.float64), axis=1) * (1 + 2.0 ** -20)
        ex = (x @ qs.T).astype(np.float64).T
        a = (xa @ qs.T).astype(np.float64).T
        e = qn[:, None] * rho[None, :] + 1e-6      # (the f32 matrix products' own rounding, well inside)
        assert np.all(np.abs(ex - a) <= e)
        sl = slice(at, at + 20_000)
        exact[:, sl] = ref6.orderable((1.0 - ex).astype(np.float32))
        hi[:, sl] = ref6.orderable(np.nextafter((1.0 - (a + e)).astype(np.float32), np.float32(-np.inf)))
        lo[:, sl] = ref6.orderable(np.nextafter((1.0 - (a - e)).astype(np.float32), np.float32(np.inf)))
    assert np.all(hi <= exact) and np.all(exact <= lo)
    return exact, hi, lo


def test_the_best_rows_threshold_is_sound_and_no_looser_than_the_refines(modelled):
    exact, hi, lo = modelled
    owner = best.owner_lists(N, BLOCKS)
    nlists = 2 * BLOCKS
    counts = []
    for q in range(QUERIES):
        rows, lhi, llo, lex = best.deal(owner, nlists, hi[q], lo[q], exact[q])
        assert (rows >= 0).all()  # every list is full: each owns some 780 rows
        kt_refine = best.refine_threshold(llo, lex, K)
        kt_best = best.best_threshold(best.best_words(llo, lex), K)
        kth = int(np.sort(exact[q])[K - 1])
        assert kt_best >= kth and kt_refine >= kth, (q, hex(kt_best), hex(kt_refine), hex(kth))
        needed = exact[q] <= np.uint32(kth)  # the top k and every tie of the k-th
        per_rule = []
        for kt in (kt_best, kt_refine):
            # (the candidates among ALL rows: at a hundredth of the headline's rows the band is a far larger share of a list's
            # rows, lists of 64 fill with candidates and would be refused -- what a list keeps is the kernel tests' matter)
            cand = hi[q] <= np.uint32(kt)
            assert cand[needed].all(), q
            retained, refused = best.candidates(lhi, kt)
            assert refused or set(np.nonzero(needed)[0].tolist()) <= set(rows[retained].tolist()), q
            per_rule.append(int(cand.sum()))
        counts.append(per_rule)
    counts = np.array(counts, np.float64)
    ratio = counts[:, 0] / counts[:, 1]
    print("candidates: best rows mean %.0f, refine mean %.0f; ratio of means %.3f, per query %.3f .. %.3f"
          % (counts[:, 0].mean(), counts[:, 1].mean(), counts[:, 0].mean() / counts[:, 1].mean(), ratio.min(), ratio.max()))
    assert counts[:, 0].mean() <= counts[:, 1].mean()
    assert ratio.max() <= 1.10, ratio.max()


def test_fewer_than_k_live_words_give_the_open_threshold():
    """Lists with k - 1 live slots in all: k - 1 live best words, so Kt'' is the empty word and every live slot a candidate;
    one more live slot closes it at the largest of the k exact words."""
    rng = np.random.default_rng(7)
    lo = np.full((8, best.KP), best.EMPTY, np.uint32)
    ex = lo.copy()
    at = [(b, 0) for b in range(8)] + [(3, 1)]                      # nine slots, at most two a list
    for b, s in at:
        lo[b, s] = 0xC0000000 + rng.integers(0, 1000)
        ex[b, s] = 0xBFFF0000 + rng.integers(0, 1000)
    words = best.best_words(lo, ex)
    assert (words != best.EMPTY).sum() == K - 1
    assert best.best_threshold(words, K) == 0xFFFFFFFF
    cand, refused = best.candidates(ex, 0xFFFFFFFF)
    assert cand.sum() == K - 1 and not refused
    lo[5, 1], ex[5, 1] = 0xC0000500, 0xBFFF0500
    words = best.best_words(lo, ex)
    assert best.best_threshold(words, K) == int(ex[ex != best.EMPTY].max())
    # a third live slot of a list adds no word: two a list are rescored, the two of smallest key(lo) word
    lo[5, 2], ex[5, 2] = 0xC0000001, 0xBFFF0001
    words = best.best_words(lo, ex)
    assert (words != best.EMPTY).sum() == K and words[5, 0] == 0xBFFF0001
    assert best.best_threshold(np.zeros(K - 1, np.uint32), K) == 0xFFFFFFFF
