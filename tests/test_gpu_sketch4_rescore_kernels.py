"""K1n's last link, launched through tests/sketch4_rescore_probe.cpp (libvt_sketch4_rescore_probe.so:
vt_sketch4_rescore.hip and nothing else of the library) on hand-made lists, against a numpy restatement on the oracle's dot
in the order under test:

  candidates  the slots whose key(hi) word h is live (!= 0xffffffff) and <= Kt'; the certificate refuses when some list's
              kp slots are all candidates or the candidates number more than cap;
  survivors   the candidates' rows that are valid and whose exact rank word is <= Kt'; the result their first k by
              (rank word, id rank), delivered when the certificate holds and at most 1 024 rows survive;
  info        {3 delivered / 2 certified only / 0 refused, candidates, Kt', 1}.

Every comparison is byte equality.  Every case runs twice on the same device buffers, nothing re-zeroed by the test: the
probe queues the zero words in a copy in front of each launch, as the search does inside the query's blit.
"""
import ctypes as C
import os

import numpy as np
import pytest

import sketch6_ref as ref6
from test_gpu_sketch4_finish_kernels import all_dots
from test_gpu_sketch_kernels import COS, IP, NIP, padded_dim, strided
from test_sketch5_model import unit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32P = C.POINTER(C.c_uint32)
EMPTY = 0xFFFFFFFF
A5, A5_64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
OVERFLOW = 4  # VT_ERR_OVERFLOW
KP = 64       # the pass's list length


class RescoreProbe:
    def __init__(self):
        path = os.environ.get("VT_SKETCH4_RESCORE_PROBE_LIB") or os.path.join(ROOT, "vettore_amd", "lib", "libvt_sketch4_rescore_probe.so")
        assert os.path.exists(path), "build it with `make` (%s)" % os.path.basename(path)
        F = self.lib = C.CDLL(path)
        f32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
        for name in ("vtpr_filter_cap", "vtpr_delivered", "vtpr_block_lists"):
            getattr(F, name).restype = C.c_uint32
        F.vtpr_lds_bytes.restype = C.c_size_t
        F.vtpr_lds_bytes.argtypes = [C.c_uint32, C.c_uint32]
        F.vtpr_rescore.argtypes = [f32p, C.c_size_t, C.c_size_t, C.c_uint32, f32p, C.c_uint32, C.c_int, C.c_int, U32P, U32P, U32P,
                                   C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, U32P, u64p, U32P, U32P, U32P,
                                   U32P, C.POINTER(C.c_int)]
        self.cap, self.delivered, self.block_lists = F.vtpr_filter_cap(), F.vtpr_delivered(), F.vtpr_block_lists()

    @staticmethod
    def _p(a, ctype):
        return a.ctypes.data_as(C.POINTER(ctype))

    def rescore(self, xbuf, stride, n_rows, q, metric, order, id_rank, hi, rows, blocks, kp, kt, k, cap, runs=2):
        q = np.ascontiguousarray(q, np.float32)
        rank = None if id_rank is None else np.ascontiguousarray(id_rank, np.uint32)
        hi, rows = np.ascontiguousarray(hi, np.uint32), np.ascontiguousarray(rows, np.uint32)
        assert hi.size == rows.size == blocks * self.block_lists * kp
        out = dict(head=np.zeros((runs, 2), np.uint32), keys=np.zeros((runs, k), np.uint64), rows=np.zeros((runs, k), np.uint32),
                   raws=np.zeros((runs, k), np.uint32), info=np.zeros((runs, 4), np.uint32), words=np.zeros((runs, 2), np.uint32),
                   status=np.zeros(runs, np.int32))
        rc = self.lib.vtpr_rescore(self._p(xbuf, C.c_float), xbuf.size, stride, n_rows, self._p(q, C.c_float), len(q), metric, order,
                                   None if rank is None else self._p(rank, C.c_uint32), self._p(hi, C.c_uint32), self._p(rows, C.c_uint32),
                                   blocks, kp, int(kt), k, cap, runs, self._p(out["head"], C.c_uint32), self._p(out["keys"], C.c_uint64),
                                   self._p(out["rows"], C.c_uint32), self._p(out["raws"], C.c_uint32), self._p(out["info"], C.c_uint32),
                                   self._p(out["words"], C.c_uint32), self._p(out["status"], C.c_int))
        assert rc == 0, "vtpr_rescore: hipError_t %d" % rc
        return out


@pytest.fixture(scope="module")
def probe():
    return RescoreProbe()


def rank_words(oracle_mod, metric, order, x, q, special=None):
    """(raw as f32, exact rank word, valid) of every row of x, K1's way.  `special`: {row: raw or None} for rows the oracle
    would refuse -- a dot whose f32 sum is not finite: the f64 value where it fits an f32, invalid (None) where not."""
    special = special or {}
    xs = x.copy()
    for r in special:
        xs[r] = 0
    oracle_mod.set_reduce_order(order)
    try:
        dots = all_dots(oracle_mod, xs, q)
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)
    valid = np.ones(len(x), bool)
    for r, v in special.items():
        valid[r] = v is not None
        dots[r] = np.float32(0.0 if v is None else v)
    raw = (-dots if metric == NIP else dots).astype(np.float32)
    for r, v in special.items():  # (the recovery hands back the metric's own value: -(f64 dot) for the negative dot)
        if v is not None:
            raw[r] = np.float32(-v if metric == NIP else v)
    rank = (np.float32(1.0) - raw) if metric == COS else (-raw if metric == IP else raw)
    return raw, ref6.orderable(rank.astype(np.float32)), valid


def restate(raw, word, valid, id_rank, hi, rows, kp, kt, k, cap):
    """(candidates, some list full of them, survivors, [(key, row, raw bits)] of the first k)."""
    hi, rows = np.asarray(hi, np.uint32), np.asarray(rows, np.int64)
    cand = (hi != np.uint32(EMPTY)) & (hi <= np.uint32(kt))
    full = cand.reshape(-1, kp).all(axis=1).any()
    total = int(cand.sum())
    crow = rows[cand]
    keep = crow[valid[crow] & (word[crow] <= np.uint32(kt))]
    r = (np.arange(len(raw)) if id_rank is None else id_rank).astype(np.uint64)
    key = (word.astype(np.uint64) << np.uint64(32)) | r
    first = keep[np.argsort(key[keep], kind="stable")][:k]
    return total, bool(full), len(keep), [(int(key[i]), int(i), int(raw[i:i + 1].view(np.uint32)[0])) for i in first]


def check(probe, oracle_mod, x, q, metric, order, id_rank, hi, rows, blocks, kt, k, what, kp=KP, cap=1 << 17, special=None,
          status=0):
    d = x.shape[1]
    stride = padded_dim(d)
    raw, word, valid = rank_words(oracle_mod, metric, order, x, q, special)
    total, full, nsurv, want = restate(raw, word, valid, id_rank, hi, rows, kp, kt, k, cap)
    refused = full or total > cap
    out = probe.rescore(strided(x, stride), stride, len(x), q, metric, order, id_rank, hi, rows, blocks, kp, kt, k, cap)
    for r in range(2):
        tag = (what, "run %d" % r)
        assert out["words"][r][0] == nsurv, (tag, out["words"][r][0], nsurv)
        assert list(out["info"][r][1:]) == [total, kt, 1], (tag, list(out["info"][r]), total)
        if refused or nsurv > probe.cap:  # not delivered: the block stays as it was, the status word stays on the device
            assert out["info"][r][0] == (0 if refused else 2), (tag, list(out["info"][r]))
            assert list(out["head"][r]) == [A5, A5] and np.all(out["keys"][r] == A5_64), tag
            assert out["status"][r] == status, tag
            assert bool(out["words"][r][1] & 2) == full and bool(out["words"][r][1] & 1) == (nsurv > probe.cap), tag
        else:
            assert out["info"][r][0] == probe.delivered, (tag, list(out["info"][r]))
            assert list(out["head"][r]) == [status, min(nsurv, k)], (tag, list(out["head"][r]))
            got = list(zip(out["keys"][r].tolist(), out["rows"][r].tolist(), out["raws"][r].tolist()))[:len(want)]
            assert got == want, (tag, got[:3], want[:3])
            assert np.all(out["keys"][r][len(want):] == A5_64), tag
            assert out["status"][r] == 0 and out["words"][r][1] == 0, tag
    return total, refused, nsurv


def random_lists(rng, blocks, n_rows, word, kt, kp=KP, fill=0.4, lists=2):
    """Lists over distinct rows: a slot is empty with probability 1 - fill; a live slot's key(hi) word lies under the row's
    exact word (as the pass leaves it), at Kt' itself for a few, and over Kt' for a share of the rows that would survive."""
    slots = blocks * lists * kp
    live = rng.random(slots) < fill
    live[rng.integers(0, slots)] = True
    assert live.sum() <= n_rows
    rows = np.full(slots, A5, np.uint32)
    rows[live] = rng.permutation(n_rows)[:live.sum()]
    hi = np.full(slots, EMPTY, np.uint32)
    w = word[rows[live]].astype(np.int64)
    h = np.maximum(w - rng.integers(0, 1 << 22, live.sum()), 0)
    pick = rng.random(live.sum())
    h = np.where(pick < 0.15, kt, h)                                   # the candidate rule's boundary
    h = np.where((pick > 0.85) & (kt < EMPTY - 1), min(kt + 1, EMPTY - 1), h)  # just past it: no candidate, whatever the row
    hi[live] = h.astype(np.uint32)
    return hi, rows


def corpus(seed, n, d):
    rng = np.random.default_rng(seed)
    x = unit(rng.uniform(-1, 1, (n, d)).astype(np.float32))
    q = unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0]
    return rng, x, q


@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("d", [64, 65, 100, 768])
def test_rescore_random_lists(probe, oracle_mod, order, d):
    """1, 2, 8 and 33 blocks (33 is no multiple of the 32 ticket groups), the three metrics, id ranks absent and permuted,
    k = 1 and 10; Kt' is the exact word of one listed row, so the filter's boundary is met, and a share of the slots carry
    Kt' itself as their key(hi) word, so the candidate rule's is.  Slots are empty between live ones throughout."""
    n = 2400
    rng, x, q = corpus(100 * d + order, n, d)
    perm = rng.permutation(n).astype(np.uint32)
    for metric, id_rank in ((COS, None), (IP, perm), (NIP, perm)):
        _, word, _ = rank_words(oracle_mod, metric, order, x, q)
        for blocks in (1, 2, 8, 33):
            star = int(np.argsort(word, kind="stable")[n // 3])
            kt = int(word[star])  # a third of the rows would survive; row `star` by `<=` alone
            hi, rows = random_lists(rng, blocks, n, word, kt)
            if star not in rows[hi != EMPTY]:
                rows[np.flatnonzero(hi != EMPTY)[0]] = star
            at = np.flatnonzero((hi != EMPTY) & (rows == star))[0]
            hi[at] = min(int(hi[at]), kt)
            for k in (1, 10):
                total, refused, nsurv = check(probe, oracle_mod, x, q, metric, order, id_rank, hi, rows, blocks, kt, k,
                                              "blocks %d metric %d k %d" % (blocks, metric, k))
                assert not refused and total >= 1 and nsurv >= 1


@pytest.mark.parametrize("order,metric,d", [(3, COS, 768), (1, IP, 100), (0, NIP, 65)])
def test_rescore_blocks_without_and_full_of_candidates(probe, oracle_mod, order, metric, d):
    """Eight blocks: block 2 has live slots and no candidate, block 3 no live slot at all.  Then block 5's two lists are both
    full of candidates -- 128 rows, 32 a wave, several load rounds each -- and the certificate must refuse while every row is
    still rescored (the survivor count says so); then one list alone is full and all of it candidates: refused; the same
    list with one slot just over Kt': certified."""
    n, blocks = 1500, 8
    rng, x, q = corpus(7 + d, n, d)
    _, word, _ = rank_words(oracle_mod, metric, order, x, q)
    kt = int(np.sort(word)[n // 2])
    hi, rows = random_lists(rng, blocks, n, word, kt, fill=0.3)
    b2, b3 = slice(2 * 2 * KP, 3 * 2 * KP), slice(3 * 2 * KP, 4 * 2 * KP)
    hi[b2] = np.where(hi[b2] != EMPTY, np.uint32(min(kt + 7, EMPTY - 1)), hi[b2])
    hi[b3] = EMPTY
    total, refused, _ = check(probe, oracle_mod, x, q, metric, order, None, hi, rows, blocks, kt, 10, "no candidate")
    assert not refused
    # block 5 full: rows not listed elsewhere
    free = np.setdiff1d(np.arange(n), rows[hi != EMPTY])
    b5 = slice(5 * 2 * KP, 6 * 2 * KP)
    full_hi, full_rows = hi.copy(), rows.copy()
    full_rows[b5] = free[:2 * KP]
    full_hi[b5] = np.minimum(word[full_rows[b5]], np.uint32(kt))
    total, refused, nsurv = check(probe, oracle_mod, x, q, metric, order, None, full_hi, full_rows, blocks, kt, 10, "both lists full")
    assert refused and nsurv >= (word[full_rows[b5]] <= kt).sum() >= 1
    one_hi = full_hi.copy()
    one_hi[5 * 2 * KP + KP:6 * 2 * KP:2] = EMPTY  # the block's second list: every other slot empty
    total, refused, _ = check(probe, oracle_mod, x, q, metric, order, None, one_hi, full_rows, blocks, kt, 10, "one list full")
    assert refused
    one_hi[5 * 2 * KP + KP - 1] = min(kt + 1, EMPTY - 1)  # the full list's last slot: live, no candidate
    total, refused, _ = check(probe, oracle_mod, x, q, metric, order, None, one_hi, full_rows, blocks, kt, 10, "kp - 1 of kp")
    assert not refused


def test_rescore_more_candidates_than_cap(probe, oracle_mod):
    """total == cap is certified, total == cap + 1 is not; the total is exact either way."""
    n, blocks, d = 900, 8, 100
    rng, x, q = corpus(31, n, d)
    _, word, _ = rank_words(oracle_mod, COS, 3, x, q)
    kt = int(np.sort(word)[n // 2])
    hi, rows = random_lists(rng, blocks, n, word, kt)
    total = int(((hi != EMPTY) & (hi <= kt)).sum())
    for cap, want in ((total, False), (total - 1, True)):
        got_total, refused, _ = check(probe, oracle_mod, x, q, COS, 3, None, hi, rows, blocks, kt, 10, "cap %d" % cap, cap=cap)
        assert got_total == total and refused == want


@pytest.mark.parametrize("live", [0, 1, 7, 10])
def test_rescore_every_live_slot_with_the_open_threshold(probe, oracle_mod, live):
    """Kt' = 0xffffffff with k or fewer live slots (the refine publishes it then): every live slot is a candidate and every
    valid row survives; with no live slot the result is empty and delivered."""
    n, blocks, d, k = 300, 2, 65, 10
    rng, x, q = corpus(live, n, d)
    hi = np.full(blocks * 2 * KP, EMPTY, np.uint32)
    rows = np.full(blocks * 2 * KP, A5, np.uint32)
    at = rng.permutation(len(hi))[:live]
    hi[at] = rng.integers(0, EMPTY - 1, live).astype(np.uint32)
    rows[at] = rng.permutation(n)[:live]
    total, refused, nsurv = check(probe, oracle_mod, x, q, COS, 2, None, hi, rows, blocks, EMPTY, k, "live %d" % live)
    assert (total, refused, nsurv) == (live, False, live)


def test_rescore_at_the_survivor_lists_bound(probe, oracle_mod):
    """Exactly 1 024 survivors are sorted and delivered; 1 025 are not, and info[0] says certified only (2).  The
    survivors are copies of one row and tie the k-th rank word: the id rank alone orders them."""
    n, blocks, d = 3000, 33, 100
    rng, x, q0 = corpus(1024, n, d)
    q = x[7].copy()
    perm = rng.permutation(n).astype(np.uint32)
    for copies in (1024, 1025):
        xc = x.copy()
        at = rng.choice(np.setdiff1d(np.arange(n), [7]), copies - 1, replace=False)  # (row 7 itself is the first copy)
        xc[at] = x[7]
        _, word, _ = rank_words(oracle_mod, COS, 3, xc, q)
        kt = int(word.min())
        assert (word == kt).sum() == copies
        # every row in a slot of its own, no list full: 33 * 2 lists of 64, 3 000 rows
        slots = blocks * 2 * KP
        place = np.concatenate([rng.permutation(KP)[:46] + KP * l for l in range(blocks * 2)])[:n]
        assert len(place) == n
        hi = np.full(slots, EMPTY, np.uint32)
        rows = np.full(slots, A5, np.uint32)
        rows[place] = rng.permutation(n)
        hi[place] = np.where(word[rows[place]] == kt, np.uint32(kt), np.uint32(min(kt + 1, EMPTY - 1)))
        hi[place[:200]] = np.minimum(hi[place[:200]], np.uint32(kt))  # (candidates that do not survive, too)
        total, refused, nsurv = check(probe, oracle_mod, xc, q, COS, 3, perm, hi, rows, blocks, kt, 10, "%d copies" % copies)
        assert nsurv == copies and not refused and total >= copies


@pytest.mark.parametrize("metric", [COS, IP, NIP])
def test_rescore_overflowing_rows(probe, oracle_mod, metric):
    """A row whose f32 dot is not finite while its f64 value fits an f32 is recovered and ranked by that value; one whose f64
    value does not fit is left out and raises the status word: the delivered block carries VT_ERR_OVERFLOW."""
    n, blocks, d = 400, 2, 100
    rng, x, q = corpus(77, n, d)
    x = (x * np.float32(4.0)).astype(np.float32)
    q = np.ones(d, np.float32)
    big = np.float32(3.0e38)
    x[11] = 0
    x[11, :8], x[11, 8:16], x[11, 16] = big, -big, np.float32(2.5)   # chunk sums +inf, -inf: NaN; in f64: 2.5
    x[12] = 0
    x[12, 90:100] = big                                               # the scalar tail's own sum: +inf; in f64: 3e39
    special = {11: 2.5, 12: None}
    _, word, valid = rank_words(oracle_mod, metric, 3, x, q, special)
    kt = int(np.sort(word[valid])[n // 2])
    kt = max(kt, int(word[11]))
    hi, rows = random_lists(rng, blocks, n, word, kt, fill=0.5)
    keep = ~np.isin(rows, [11, 12])
    hi, rows = np.where(keep, hi, np.uint32(EMPTY)), np.where(keep, rows, np.uint32(A5))
    empty = np.flatnonzero(hi == EMPTY)[:2]
    rows[empty], hi[empty] = [11, 12], [0, 0]
    total, refused, nsurv = check(probe, oracle_mod, x, q, metric, 3, None, hi, rows, blocks, kt, 10, "overflow", special=special,
                                  status=OVERFLOW)
    assert not refused and nsurv >= 1
    # without the row that cannot be recovered: the status stays clear
    hi[empty[1]] = EMPTY
    check(probe, oracle_mod, x, q, metric, 3, None, hi, rows, blocks, kt, 10, "recovered only", special=special)


def test_rescore_short_lists_and_long_rows(probe, oracle_mod):
    """Lists of 16 slots (k' follows the pass), and rows of four to six 1-KiB segments: the slots of a load round name
    their rows and segments at run time there, and a round holds fewer rows."""
    for d, kp, order in ((900, 16, 3), (1030, 64, 1), (1500, 64, 3)):
        assert probe.lib.vtpr_lds_bytes(d, kp) != 0
        n, blocks = 700, 3
        rng, x, q = corpus(d, n, d)
        _, word, _ = rank_words(oracle_mod, IP, order, x, q)
        kt = int(np.sort(word)[n // 2])
        hi, rows = random_lists(rng, blocks, n, word, kt, kp=kp, fill=0.7)
        total, refused, nsurv = check(probe, oracle_mod, x, q, IP, order, None, hi, rows, blocks, kt, 10, "d %d" % d, kp=kp)
        assert total >= 4 and nsurv >= 1
    assert probe.lib.vtpr_lds_bytes(6000, 64) == 0  # (rows too long for the block: the search keeps the collect and the filtered K1)
