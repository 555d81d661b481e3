"""The kernel that finishes K1n's chain, launched through tests/sketch4_finish_probe.cpp
(libvt_sketch4_finish_probe.so: vt_scan_filter.hip and nothing else of the library): the gathered K1 in filter mode against
a numpy restatement on the oracle's dot in the order under test -- survivors = the listed rows whose rank word is <= the
word given, the result their first k by (rank word, id rank).

Every case runs twice on the same device buffers, nothing re-zeroed by the test: the probe queues the zero words in a copy
in front of each launch, as the search does inside the query's blit.
"""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import sketch6_ref as ref6
from test_gpu_sketch_kernels import COS, IP, NIP, padded_dim, strided
from test_sketch5_model import unit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32P = C.POINTER(C.c_uint32)


class FinishProbe:
    def __init__(self):
        path = os.environ.get("VT_SKETCH4_FINISH_PROBE_LIB") or os.path.join(ROOT, "vettore_amd", "lib", "libvt_sketch4_finish_probe.so")
        assert os.path.exists(path), "build it with `make` (%s)" % os.path.basename(path)
        F = self.fin = C.CDLL(path)
        f32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
        F.vtpf_filter_cap.restype = C.c_uint32
        F.vtpf_delivered.restype = C.c_uint32
        F.vtpf_filter.argtypes = [f32p, C.c_size_t, C.c_size_t, C.c_uint32, f32p, C.c_uint32, C.c_int, C.c_int, U32P, U32P, C.c_uint32,
                                  C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, U32P, U32P, u64p, U32P, U32P, U32P, U32P,
                                  C.POINTER(C.c_int)]

    @staticmethod
    def _p(a, ctype):
        return a.ctypes.data_as(C.POINTER(ctype))

    def filter(self, xbuf, stride, n_rows, q, metric, order, id_rank, rows, dev_count, hi_word, k, blocks, info_in=(2, 0, 0, 1), runs=2):
        rows = np.ascontiguousarray(rows, np.uint32)
        cap = max(len(rows), 1)
        if len(rows) == 0:
            rows = np.zeros(1, np.uint32)
        q = np.ascontiguousarray(q, np.float32)
        rank = None if id_rank is None else np.ascontiguousarray(id_rank, np.uint32)
        info_in = np.array(info_in, np.uint32)
        out = dict(head=np.zeros((runs, 2), np.uint32), keys=np.zeros((runs, k), np.uint64), rows=np.zeros((runs, k), np.uint32),
                   raws=np.zeros((runs, k), np.uint32), info=np.zeros((runs, 4), np.uint32), survivors=np.zeros(runs, np.uint32),
                   status=np.zeros(runs, np.int32))
        rc = self.fin.vtpf_filter(self._p(xbuf, C.c_float), xbuf.size, stride, n_rows, self._p(q, C.c_float), len(q), metric, order,
                                  None if rank is None else self._p(rank, C.c_uint32), self._p(rows, C.c_uint32), cap, dev_count,
                                  int(hi_word), k, blocks, runs, self._p(info_in, C.c_uint32), self._p(out["head"], C.c_uint32),
                                  self._p(out["keys"], C.c_uint64), self._p(out["rows"], C.c_uint32), self._p(out["raws"], C.c_uint32),
                                  self._p(out["info"], C.c_uint32), self._p(out["survivors"], C.c_uint32), self._p(out["status"], C.c_int))
        assert rc == 0, "vtpf_filter: hipError_t %d" % rc
        return out


@pytest.fixture(scope="module")
def probe():
    return FinishProbe()


def all_dots(oracle_mod, x, q):
    """The oracle's dot of q with every row of x, in the reduce order in force: one matrix_search that returns every row."""
    ids = [struct.pack(">I", i) for i in range(len(x))]
    hits = oracle_mod.matrix_search(IP, x, oracle_mod.pack_ids(ids), q, len(x))
    out = np.zeros(len(x), np.float32)
    for id_, raw in hits:
        out[struct.unpack(">I", id_)[0]] = np.float32(raw)
    assert len(hits) == len(x)
    return out


def restate(metric, dots, rows, id_rank, hi_word, k):
    """(survivors, [(key, row, raw bits)] of the first k) over the candidate list `rows`."""
    raw = -dots if metric == NIP else dots
    rank = (np.float32(1.0) - raw) if metric == COS else (-raw if metric == IP else raw)
    word = ref6.orderable(rank.astype(np.float32))
    cand = np.asarray(rows, np.int64)
    keep = cand[word[cand] <= np.uint32(hi_word)]
    r = (np.arange(len(dots)) if id_rank is None else id_rank).astype(np.uint64)
    key = (word.astype(np.uint64) << np.uint64(32)) | r
    first = keep[np.argsort(key[keep], kind="stable")][:k]
    return len(keep), [(int(key[i]), int(i), int(raw[i:i + 1].view(np.uint32)[0])) for i in first]


def check_filter(probe, oracle_mod, x, q, metric, order, id_rank, rows, hi_word, k, blocks, what, dev_count=None):
    d = x.shape[1]
    stride = padded_dim(d)
    oracle_mod.set_reduce_order(order)
    try:
        dots = all_dots(oracle_mod, x, q)
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)
    count = len(rows) if dev_count is None else dev_count
    nsurv, want = restate(metric, dots, rows[:count], id_rank, hi_word, k)
    info_in = (2, count, int(hi_word), 1)
    out = probe.filter(strided(x, stride), stride, len(x), q, metric, order, id_rank, rows, count, hi_word, k, blocks, info_in)
    cap, delivered = probe.fin.vtpf_filter_cap(), probe.fin.vtpf_delivered()
    for r in range(2):
        tag = (what, "run %d" % r)
        assert out["survivors"][r] == nsurv, (tag, out["survivors"][r], nsurv)
        if count == 0:  # nothing handed over: the count alone is written
            assert list(out["head"][r]) == [0xA5A5A5A5, 0] and list(out["info"][r]) == list(info_in), tag
            assert np.all(out["keys"][r] == 0xA5A5A5A5A5A5A5A5), tag
        elif nsurv > cap:  # not delivered: the block, info and the status word stay as they were
            assert list(out["head"][r]) == [0xA5A5A5A5, 0xA5A5A5A5] and list(out["info"][r]) == list(info_in), tag
            assert np.all(out["keys"][r] == 0xA5A5A5A5A5A5A5A5), tag
        else:
            assert list(out["head"][r]) == [0, min(nsurv, k)], (tag, list(out["head"][r]))
            assert list(out["info"][r]) == [delivered] + list(info_in[1:]), tag
            got = list(zip(out["keys"][r].tolist(), out["rows"][r].tolist(), out["raws"][r].tolist()))[:len(want)]
            assert got == want, (tag, got[:3], want[:3])
            assert np.all(out["keys"][r][len(want):] == 0xA5A5A5A5A5A5A5A5), tag
        assert out["status"][r] == 0, tag
    return nsurv


def kth_word(oracle_mod, metric, order, x, q, rows, j):
    """The j-th smallest rank word (1-based) among the rows listed."""
    oracle_mod.set_reduce_order(order)
    try:
        dots = all_dots(oracle_mod, x, q)
    finally:
        oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)
    raw = -dots if metric == NIP else dots
    rank = (np.float32(1.0) - raw) if metric == COS else (-raw if metric == IP else raw)
    return int(np.sort(ref6.orderable(rank.astype(np.float32))[np.asarray(rows, np.int64)])[j - 1])


@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("d", [136, 200, 768])
def test_filter_short_lists(probe, oracle_mod, order, d):
    """Candidate lists of 0, 1, 7, 8 and 9 rows (a tile is 8 rows) out of 300, on 3 blocks (blocks without a tile still
    draw their ticket); the word given lets everything, about half, and nothing through; id ranks absent and permuted."""
    rng = np.random.default_rng(order * 17 + d)
    x = unit(rng.uniform(-1, 1, (300, d)).astype(np.float32))
    q = unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0]
    perm = rng.permutation(300).astype(np.uint32)
    for metric, id_rank in ((COS, None), (IP, perm), (NIP, perm)):
        for n in (0, 1, 7, 8, 9):
            rows = rng.choice(300, n, replace=False).astype(np.uint32)
            words = [0xFFFFFFFF, 0] + ([kth_word(oracle_mod, metric, order, x, q, rows, (n + 1) // 2)] if n else [])
            for hw in words:
                for k in (1, 10):
                    check_filter(probe, oracle_mod, x, q, metric, order, id_rank, rows, hw, k, 3, "n %d word %x k %d metric %d" % (n, hw, k, metric))


@pytest.mark.parametrize("order,metric", [(3, COS), (1, IP)])
def test_filter_forty_thousand_rows_a_dozen_survivors(probe, oracle_mod, order, metric):
    """The headline's proportions: 40 000 candidates (with repeats of 6 000 rows' worth of memory: the list names rows, the
    same row may stand twice), 64 blocks, and a word that leaves twelve of them."""
    d, n = 264, 6000
    rng = np.random.default_rng(4100 + order)
    x = unit(rng.uniform(-1, 1, (n, d)).astype(np.float32))
    q = unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0]
    rows = np.concatenate([rng.permutation(n), rng.permutation(n), rng.permutation(n), rng.permutation(n), rng.permutation(n),
                           rng.permutation(n), rng.permutation(n)[:4000]]).astype(np.uint32)
    assert len(rows) == 40000
    hw = kth_word(oracle_mod, metric, order, x, q, rows, 12)
    perm = rng.permutation(n).astype(np.uint32)
    nsurv = check_filter(probe, oracle_mod, x, q, metric, order, perm, rows, hw, 10, 64, "40 000")
    assert 12 <= nsurv <= 24, nsurv


def test_filter_at_the_survivor_lists_bound(probe, oracle_mod):
    """Exactly 1 024 survivors are sorted and delivered; 1 025 are not, and info stays as it was.  Copies of one row tie
    the word: the id rank alone orders them."""
    d, n = 136, 3000
    rng = np.random.default_rng(1024)
    x = unit(rng.uniform(-1, 1, (n, d)).astype(np.float32))
    q = x[7].copy()
    perm = rng.permutation(n).astype(np.uint32)
    for copies in (1024, 1025):
        xc = x.copy()
        at = rng.choice(np.setdiff1d(np.arange(n), [7]), copies - 1, replace=False)  # (row 7 itself is the first copy)
        xc[at] = x[7]
        rows = rng.permutation(n).astype(np.uint32)
        hw = kth_word(oracle_mod, COS, 3, xc, q, rows, 1)
        nsurv = check_filter(probe, oracle_mod, xc, q, COS, 3, perm, rows, hw, 10, 16, "%d copies" % copies)
        assert nsurv == copies


def test_filter_with_a_device_count_of_zero(probe, oracle_mod):
    """A refused collect leaves *count = 0 over a list that still holds the last call's rows: nothing is scanned, nothing is
    written but count = 0, info stays the collect's."""
    d = 200
    rng = np.random.default_rng(5)
    x = unit(rng.uniform(-1, 1, (100, d)).astype(np.float32))
    rows = rng.permutation(100)[:50].astype(np.uint32)
    out = probe.filter(strided(x, padded_dim(d)), padded_dim(d), 100, x[3], COS, 3, None, rows, 0, 0xFFFFFFFF, 10, 8, (0, 77, 5, 1))
    for r in range(2):
        assert list(out["head"][r]) == [0xA5A5A5A5, 0] and list(out["info"][r]) == [0, 77, 5, 1] and out["survivors"][r] == 0
        assert np.all(out["keys"][r] == 0xA5A5A5A5A5A5A5A5)
