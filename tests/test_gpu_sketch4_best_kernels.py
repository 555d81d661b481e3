"""K1n's threshold from each list's best rows, kernel by kernel, through tests/sketch4_best_probe.cpp
(libvt_sketch4_best_probe.so: vt_sketch_nibble.hip, vt_sketch4_rescore.hip and nothing else of the library), against the
numpy restatement in tests/sketch4_best_ref.py on the oracle's dot:

  A  the 4-bit pass asked for its lists' best words: per list the exact rank words of the two live slots of smallest key(lo)
     word, byte for byte, in the three dot metrics and the four reduce orders; its lists and word arrays byte-equal to a
     launch that was not asked; a list with one live slot, an empty list, a row whose value is not finite.
  B  the rescoring kernel handed best words in place of a threshold: the word it publishes, info[2] and the candidate total
     are the k-th smallest word's with multiplicity, and everything else it writes equals a launch handed that word.
"""
import ctypes as C
import os

import numpy as np
import pytest

import sketch4_best_ref as best
from test_gpu_sketch4_rescore_kernels import A5, KP, RescoreProbe, corpus, random_lists, rank_words
from test_gpu_sketch_kernels import COS, IP, NIP, Probe, Query, padded_dim, strided
from test_sketch5_model import unit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32P = C.POINTER(C.c_uint32)
EMPTY = 0xFFFFFFFF


class BestProbe:
    def __init__(self):
        path = os.environ.get("VT_SKETCH4_BEST_PROBE_LIB") or os.path.join(ROOT, "vettore_amd", "lib", "libvt_sketch4_best_probe.so")
        assert os.path.exists(path), "build it with `make` (%s)" % os.path.basename(path)
        F = self.lib = C.CDLL(path)
        u8p, f32p, u64p = C.POINTER(C.c_ubyte), C.POINTER(C.c_float), C.POINTER(C.c_uint64)
        for name in ("vtbp_block_lists", "vtbp_best_rows", "vtbp_max_words", "vtbp_max_k", "vtbp_delivered"):
            getattr(F, name).restype = C.c_uint32
        assert (F.vtbp_block_lists(), F.vtbp_best_rows()) == (2, best.BEST_ROWS)
        F.vtbp_scan.argtypes = [u8p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int, U32P, u8p, C.c_size_t, f32p, C.c_double, C.c_double,
                                C.c_double, C.c_uint32, C.c_uint32, f32p, C.c_size_t, C.c_size_t, f32p, C.c_int, C.c_int, u64p, U32P,
                                U32P, U32P, U32P]
        F.vtbp_rescore.argtypes = [f32p, C.c_size_t, C.c_size_t, C.c_uint32, f32p, C.c_uint32, C.c_int, C.c_int, U32P, U32P, U32P,
                                   C.c_uint32, C.c_uint32, U32P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, U32P, u64p, U32P, U32P,
                                   U32P, U32P, C.POINTER(C.c_int), U32P]

    @staticmethod
    def _p(a, ctype):
        return a.ctypes.data_as(C.POINTER(ctype))

    def scan(self, img, n, d, metric, qy, blocks, xbuf, stride, order, want_best, k=KP):
        img = np.ascontiguousarray(img, np.uint8).reshape(-1)
        qimg = np.ascontiguousarray(qy.image).view(np.uint8).reshape(-1)
        t = np.ascontiguousarray(qy.t, np.float32)
        q = np.ascontiguousarray(qy.q, np.float32)
        lists = 2 * blocks
        keys, pay = np.zeros((lists, k), np.uint64), np.zeros((lists, k, 2), np.uint32)
        lo, hi, bw = np.zeros((lists, k), np.uint32), np.zeros((lists, k), np.uint32), np.zeros((lists, best.BEST_ROWS), np.uint32)
        rc = self.lib.vtbp_scan(self._p(img, C.c_ubyte), img.size, n, d, metric, None, self._p(qimg, C.c_ubyte), qimg.size,
                                self._p(t, C.c_float), qy.qn, qy.eta, qy.kerr, k, blocks, self._p(xbuf, C.c_float), xbuf.size, stride,
                                self._p(q, C.c_float), order, int(want_best), self._p(keys, C.c_uint64), self._p(pay, C.c_uint32),
                                self._p(lo, C.c_uint32), self._p(hi, C.c_uint32), self._p(bw, C.c_uint32))
        assert rc == 0, "vtbp_scan: hipError_t %d" % rc
        return keys, pay, lo, hi, bw

    def rescore(self, xbuf, stride, n_rows, q, metric, order, id_rank, hi, rows, blocks, kp, words, k, cap, runs=2, expect=0):
        q = np.ascontiguousarray(q, np.float32)
        rank = None if id_rank is None else np.ascontiguousarray(id_rank, np.uint32)
        hi, rows = np.ascontiguousarray(hi, np.uint32), np.ascontiguousarray(rows, np.uint32)
        words = np.ascontiguousarray(words, np.uint32).reshape(-1)
        out = dict(head=np.zeros((runs, 2), np.uint32), keys=np.zeros((runs, k), np.uint64), rows=np.zeros((runs, k), np.uint32),
                   raws=np.zeros((runs, k), np.uint32), info=np.zeros((runs, 4), np.uint32), words=np.zeros((runs, 2), np.uint32),
                   status=np.zeros(runs, np.int32), kt=np.zeros(runs, np.uint32))
        rc = self.lib.vtbp_rescore(self._p(xbuf, C.c_float), xbuf.size, stride, n_rows, self._p(q, C.c_float), len(q), metric, order,
                                   None if rank is None else self._p(rank, C.c_uint32), self._p(hi, C.c_uint32), self._p(rows, C.c_uint32),
                                   blocks, kp, self._p(words, C.c_uint32), words.size, k, cap, runs, self._p(out["head"], C.c_uint32),
                                   self._p(out["keys"], C.c_uint64), self._p(out["rows"], C.c_uint32), self._p(out["raws"], C.c_uint32),
                                   self._p(out["info"], C.c_uint32), self._p(out["words"], C.c_uint32), self._p(out["status"], C.c_int),
                                   self._p(out["kt"], C.c_uint32))
        assert rc == expect, "vtbp_rescore: hipError_t %d" % rc
        return out


@pytest.fixture(scope="module")
def probe():
    return BestProbe()


@pytest.fixture(scope="module")
def builder():
    return Probe()


@pytest.fixture(scope="module")
def word_probe():
    return RescoreProbe()


# ---- A. the pass ---------------------------------------------------------------------------------------------------------------
def check_pass(probe, builder, oracle_mod, x, q, metric, order, blocks, what, not_finite=()):
    n, d = x.shape
    stride = padded_dim(d)
    xbuf = strided(x, stride)
    img, _ = builder.build(4, xbuf, stride, n, (n + 63) // 64 * 64, d)
    qy = Query(4, q)
    plain = probe.scan(img, n, d, metric, qy, blocks, xbuf, stride, order, False)
    asked = probe.scan(img, n, d, metric, qy, blocks, xbuf, stride, order, True)
    for got, want, name in zip(asked[:4], plain[:4], ("keys", "pay", "lo_words", "hi_words")):
        assert got.tobytes() == want.tobytes(), (what, name)  # (an empty slot's payload is never written: the prefill in both)
    assert np.all(plain[4] == A5), what
    _, pay, lo, _, bw = asked
    _, word, _ = rank_words(oracle_mod, metric, order, x, q)
    rows = pay[:, :, 0].astype(np.int64)
    live = lo != np.uint32(EMPTY)
    exact = np.where(live, word[np.where(live, rows, 0)], np.uint32(EMPTY)).astype(np.uint32)
    finite = ~np.isin(rows, list(not_finite))
    want = best.best_words(lo, exact, finite)
    assert np.array_equal(bw, want), (what, [hex(v) for v in bw.reshape(-1)[:6]], [hex(v) for v in want.reshape(-1)[:6]])
    return lo, rows, bw


@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("d", [203, 160])
def test_pass_leaves_each_lists_best_words(probe, builder, oracle_mod, order, d):
    """Two blocks (four lists, eight waves), 1 024 + 37 rows -- a partial last tile, every list full --, d = 203 (full chunks
    and a scalar tail of three) and d = 160, the three metrics."""
    n = 1024 + 37
    rng = np.random.default_rng(1000 * d + order)
    x = unit(rng.uniform(-1, 1, (n, d)).astype(np.float32))
    q = unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0]
    for metric in (COS, IP, NIP):
        lo, _, bw = check_pass(probe, builder, oracle_mod, x, q, metric, order, 2, "d %d order %d metric %d" % (d, order, metric))
        assert np.all(lo != np.uint32(EMPTY)) and np.all(bw != np.uint32(EMPTY))


def test_pass_lists_with_one_slot_and_none(probe, builder, oracle_mod):
    """65 rows on two blocks: tile 0 fills list 0, the one row of tile 1 is list 2's only slot -- its second word is empty --,
    lists 1 and 3 own no tile: both words empty."""
    d = 160
    rng = np.random.default_rng(65)
    x = unit(rng.uniform(-1, 1, (65, d)).astype(np.float32))
    lo, rows, bw = check_pass(probe, builder, oracle_mod, x, x[9].copy(), COS, 3, 2, "65 rows")
    assert [int((l != np.uint32(EMPTY)).sum()) for l in lo] == [64, 0, 1, 0]
    assert [[int(w != EMPTY) for w in b] for b in bw] == [[1, 1], [0, 0], [1, 0], [0, 0]]


def test_pass_leaves_a_word_empty_for_a_row_that_is_not_finite(probe, builder, oracle_mod):
    """Row 70's first product overflows f32 in any order, so its value is +inf and its rank is not finite: its interval's
    ends are infinite too, it is its list's best slot by key(lo), and the word it would give stays empty."""
    n, d = 1024 + 37, 160
    rng = np.random.default_rng(70)
    x = unit(rng.uniform(-1, 1, (n, d)).astype(np.float32))
    q = unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0]
    q[0] = np.float32(2.0)
    x[70, 0] = np.float32(3.0e38)
    safe = x.copy()
    safe[70] = 0  # (the oracle is not asked for that row's dot)
    stride = padded_dim(d)
    xbuf = strided(x, stride)
    img, _ = builder.build(4, xbuf, stride, n, (n + 63) // 64 * 64, d)
    _, pay, lo, _, bw = probe.scan(img, n, d, IP, Query(4, q), 2, xbuf, stride, 0, True)
    _, word, _ = rank_words(oracle_mod, IP, 0, safe, q)
    rows = pay[:, :, 0].astype(np.int64)
    exact = word[rows]
    want = best.best_words(lo, exact, rows != 70)
    assert np.array_equal(bw, want)
    at = np.argwhere(rows == 70)
    assert len(at) == 1
    b, s = at[0]
    assert lo[b, s] == lo[b].min() and bw[b, 0] == EMPTY and bw[b, 1] != EMPTY


# ---- B. the rescoring kernel's head ------------------------------------------------------------------------------------------
def check_head(probe, word_probe, x, q, metric, order, hi, rows, blocks, words, k, what):
    """A launch handed `words` against a launch handed their k-th smallest: every output equal, and the word published."""
    d = x.shape[1]
    stride = padded_dim(d)
    xbuf = strided(x, stride)
    kt = best.best_threshold(words, k)
    got = probe.rescore(xbuf, stride, len(x), q, metric, order, None, hi, rows, blocks, KP, words, k, 1 << 17)
    want = word_probe.rescore(xbuf, stride, len(x), q, metric, order, None, hi, rows, blocks, KP, kt, k, 1 << 17)
    cand = (np.asarray(hi, np.uint32) != np.uint32(EMPTY)) & (np.asarray(hi, np.uint32) <= np.uint32(kt))
    for r in range(2):
        assert int(got["kt"][r]) == kt, (what, r, hex(int(got["kt"][r])), hex(kt))
        assert int(got["info"][r][2]) == kt and int(got["info"][r][1]) == int(cand.sum()), (what, r, list(got["info"][r]))
        for f in ("head", "keys", "rows", "raws", "info", "words", "status"):
            assert np.array_equal(got[f][r], want[f][r]), (what, r, f)
    return kt, int(cand.sum())


@pytest.mark.parametrize("k", [1, 10])
def test_head_finds_the_kth_smallest_best_word(probe, word_probe, oracle_mod, k):
    """Best words of 33 blocks (132 words, no multiple of a thread's sixteen) and of the most a launch takes (4 096): random
    exact words with a share of them empty; fewer than k live, exactly k, copies of the k-th word across the cut, all empty."""
    n, blocks, d = 2400, 33, 100
    rng, x, q = corpus(500 + k, n, d)
    _, word, _ = rank_words(oracle_mod, COS, 3, x, q)
    mid = int(np.sort(word)[n // 3])
    hi, rows = random_lists(rng, blocks, n, word, mid)
    lists = 2 * blocks
    for count in (lists * 2, probe.lib.vtbp_max_words()):
        words = word[rng.integers(0, n, count)].astype(np.uint32)
        words[rng.random(count) < 0.3] = EMPTY
        kt, total = check_head(probe, word_probe, x, q, COS, 3, hi, rows, blocks, words, k, "random %d" % count)
        assert kt != EMPTY and total >= 1
        # copies of the k-th word on both sides of the cut: with multiplicity the k-th smallest is still that word
        tied = words.copy()
        tied[rng.choice(count, 3 * k + 2, replace=False)] = np.uint32(kt)
        assert check_head(probe, word_probe, x, q, COS, 3, hi, rows, blocks, tied, k, "copies %d" % count)[0] == kt
        low = tied.copy()
        low[rng.choice(count, k, replace=False)] = np.uint32(int(np.sort(word)[0]))  # k copies of one smaller word: Kt'' is it
        assert check_head(probe, word_probe, x, q, COS, 3, hi, rows, blocks, low, k, "k copies %d" % count)[0] == int(np.sort(word)[0])
        for live in (k - 1, k):
            few = np.full(count, EMPTY, np.uint32)
            few[rng.choice(count, live, replace=False)] = words[words != EMPTY][:live]
            kt, total = check_head(probe, word_probe, x, q, COS, 3, hi, rows, blocks, few, k, "live %d of %d" % (live, count))
            assert (kt == EMPTY) == (live < k)
            if live < k:
                assert total == int((hi != EMPTY).sum())  # the open threshold: every live slot a candidate
        assert check_head(probe, word_probe, x, q, COS, 3, hi, rows, blocks, np.full(count, EMPTY, np.uint32), k, "all empty")[0] == EMPTY
    # fewer words than k, and a single word
    assert check_head(probe, word_probe, x, q, IP, 1, hi, rows, blocks, word[:1].copy(), k, "one word")[0] == (int(word[0]) if k == 1 else EMPTY)


def test_head_refuses_what_it_cannot_select(probe, oracle_mod):
    """More words than a thread's sixteen times the block, or a k whose smaller words may not fit a word a thread: invalid
    value, nothing launched."""
    n, blocks, d = 300, 2, 65
    rng, x, q = corpus(3, n, d)
    hi = np.full(blocks * 2 * KP, EMPTY, np.uint32)
    rows = np.zeros(blocks * 2 * KP, np.uint32)
    stride = padded_dim(d)
    words = np.zeros(probe.lib.vtbp_max_words() + 1, np.uint32)
    probe.rescore(strided(x, stride), stride, n, q, COS, 3, None, hi, rows, blocks, KP, words, 10, 1 << 17, expect=1)
    probe.rescore(strided(x, stride), stride, n, q, COS, 3, None, hi, rows, blocks, KP, words[:64], probe.lib.vtbp_max_k() + 1, 1 << 17,
                  expect=1)
