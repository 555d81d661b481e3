"""The chain behind K1n's pass against its numpy model.  K1n's builders and pass are a width of
test_gpu_sketch_kernels.py's parametrised tests (A and B there); here, through tests/sketch4_probe.cpp
(libvt_sketch4_probe.so: vt_sketch.hip, vt_sketch_nibble.hip and nothing else of the library):

  C  the chain with the exact threshold (sketch_thresh_kernel filing slots, sketch_refine_kernel, sketch_collect_kernel
     taking the published word) on synthetic arrays: the k rows picked, Kt' against a numpy restatement on the oracle's dot
     in each reduce order, the candidates, and the state two calls share.
"""
import ctypes as C
import os

import numpy as np
import pytest

import sketch6_ref as ref6
from test_gpu_sketch_kernels import COS, EMPTY, IP, padded_dim, strided
from test_sketch5_model import unit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP = 64


class Probe4:
    def __init__(self):
        path = os.environ.get("VT_SKETCH4_PROBE_LIB") or os.path.join(ROOT, "vettore_amd", "lib", "libvt_sketch4_probe.so")
        assert os.path.exists(path), "build it with `make` (%s)" % os.path.basename(path)
        L = self.lib = C.CDLL(path)
        u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
        L.vtp4_thresh_blocks.restype = C.c_uint32
        L.vtp4_thresh_blocks.argtypes = [C.c_uint32, C.c_uint32]
        L.vtp4_certify.argtypes = [u32p, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, f32p, C.c_size_t, C.c_size_t,
                                   C.c_uint32, f32p, C.c_uint32, C.c_int, C.c_int, C.c_uint32] + [u32p] * 7

    @staticmethod
    def _p(a, ctype):
        return a.ctypes.data_as(C.POINTER(ctype))

    def certify(self, lo, hi, rows, lists, k, cap, xbuf, stride, n_rows, q, metric, order, runs=2):
        lo, hi = np.ascontiguousarray(lo, np.uint32), np.ascontiguousarray(hi, np.uint32)
        pay = np.zeros((lists * KP, 2), np.uint32)
        pay[:, 0] = rows
        pay[:, 1] = 0x7FC00000  # (the payload's float is not read)
        tb = self.lib.vtp4_thresh_blocks(lists, KP)
        out = dict(parts=np.zeros((runs, tb, k), np.uint32), slots=np.zeros((runs, tb, k), np.uint32), kt=np.zeros(runs, np.uint32),
                   picked=np.zeros((runs, k), np.uint32), rows=np.zeros((runs, cap), np.uint32), count=np.zeros(runs, np.uint32),
                   info=np.zeros((runs, 4), np.uint32))
        q = np.ascontiguousarray(q, np.float32)
        rc = self.lib.vtp4_certify(self._p(lo, C.c_uint32), self._p(hi, C.c_uint32), self._p(pay, C.c_uint32), lists, KP, k, cap,
                                   self._p(xbuf, C.c_float), xbuf.size, stride, n_rows, self._p(q, C.c_float), len(q), metric, order,
                                   runs, *(self._p(out[f], C.c_uint32) for f in ("parts", "slots", "kt", "picked", "rows", "count", "info")))
        assert rc == 0, "vtp4_certify: hipError_t %d" % rc
        return out


@pytest.fixture(scope="module")
def probe():
    return Probe4()


# ---- C. the chain behind the pass, with the exact threshold ------------------------------------------------------------------
def exact_words(oracle_mod, metric, q, x):
    out = np.zeros(len(x), np.float32)
    for i, row in enumerate(x):
        dot = oracle_mod.compute(IP, q, row)
        out[i] = oracle_mod.rank_value(COS, dot) if metric == COS else oracle_mod.rank_value(IP, dot)
    return ref6.orderable(out)


def check_refine(probe, oracle_mod, lo, hi, lists, k, x, q, metric, order, what):
    """The slots name distinct rows (a permutation), so the rows picked tell the slots picked."""
    slots = lists * KP
    d = x.shape[1]
    assert len(x) >= slots
    rng = np.random.default_rng(slots + k)
    rows = rng.permutation(len(x))[:slots].astype(np.uint32)
    stride = padded_dim(d)
    out = probe.certify(lo, hi, rows, lists, k, slots, strided(x, stride), stride, len(x), q, metric, order, runs=2)
    live = np.nonzero(lo != EMPTY)[0]
    slot_of_row = {int(r): i for i, r in enumerate(rows)}
    for r in range(2):  # (the same answer from the same buffers, whatever the call before left)
        tag = (what, "run %d" % r)
        # the threshold kernel's slots really hold the words filed beside them, and are distinct
        pw, ps = out["parts"][r].reshape(-1), out["slots"][r].reshape(-1)
        real = pw != EMPTY
        assert np.array_equal(lo[ps[real]], pw[real]), tag
        assert len(set(ps[real].tolist())) == real.sum(), tag
        if len(live) <= k:
            assert out["kt"][r] == 0xFFFFFFFF and np.all(out["picked"][r] == EMPTY), tag
            ktp = 0xFFFFFFFF
        else:
            kt = int(np.sort(lo[live])[k - 1])
            picked = [slot_of_row[int(p)] for p in out["picked"][r]]
            assert len(set(picked)) == k, tag
            assert np.array_equal(np.sort(lo[picked]), np.sort(lo[live])[:k]), (tag, "not the k smallest key(lo) words")
            oracle_mod.set_reduce_order(order)
            try:
                ex = exact_words(oracle_mod, metric, q, x[rows[picked]])
            finally:
                oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)
            ktp = min(kt, int(ex.max()))
            assert int(out["kt"][r]) == ktp, (tag, hex(int(out["kt"][r])), hex(ktp), hex(kt))
        cand = (hi != EMPTY) & (hi <= np.uint32(ktp))
        fail = bool(cand.reshape(lists, KP).all(axis=1).any())
        assert list(out["info"][r]) == [0 if fail else 2, cand.sum(), ktp, 1], (tag, list(out["info"][r]), cand.sum())
        assert out["count"][r] == (0 if fail else cand.sum()), tag
        if not fail:
            assert np.array_equal(np.sort(out["rows"][r][:cand.sum()]), np.sort(rows[cand])), tag
    return int(out["kt"][0])


@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("k", [1, 10])
def test_refine_publishes_the_exact_threshold(probe, oracle_mod, order, k):
    """33 lists (three threshold slices, the last partial), rows of d = 203 (full chunks and a scalar tail of three), the
    words consistent with the rows -- key(hi) <= the exact word <= key(lo), the band 40 000 words wide -- so Kt' is the
    largest exact word of the k rows picked and lies below Kt; and once with the exact words above every key(lo) word, where
    Kt' must stay Kt."""
    lists, d = 33, 203
    slots = lists * KP
    rng = np.random.default_rng(order * 31 + k)
    x = unit(rng.uniform(-1, 1, (slots + 50, d)).astype(np.float32))
    q = unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0]
    for metric in (COS, IP):
        probe_rows = np.random.default_rng(slots + k).permutation(len(x))[:slots]
        oracle_mod.set_reduce_order(order)
        try:
            ex = exact_words(oracle_mod, metric, q, x[probe_rows])
        finally:
            oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)
        lo = (ex + rng.integers(0, 40000, slots).astype(np.uint32)).astype(np.uint32)
        hi = (ex - rng.integers(0, 40000, slots).astype(np.uint32)).astype(np.uint32)
        dead = rng.uniform(size=slots) < 0.3
        lo[dead] = EMPTY
        hi[dead] = EMPTY
        kt = int(np.sort(lo[~dead])[k - 1])
        ktp = check_refine(probe, oracle_mod, lo, hi, lists, k, x, q, metric, order, "consistent metric %d" % metric)
        assert ktp <= kt
        low = np.where(dead, EMPTY, np.uint32(0x10000000) + rng.integers(0, 5000, slots).astype(np.uint32)).astype(np.uint32)
        assert check_refine(probe, oracle_mod, low, low, lists, k, x, q, metric, order, "exact above Kt") == int(np.sort(low[~dead])[k - 1])


@pytest.mark.parametrize("k", [1, 10])
def test_refine_edges(probe, oracle_mod, k):
    """Copies of the word at Kt inside one slice and spread over the slices (the k picked must be distinct slots that hold
    it); live = k - 1, k (plain Kt = 0xffffffff, nothing picked) and k + 1; all slots empty."""
    lists, d = 33, 256
    slots = lists * KP
    rng = np.random.default_rng(900 + k)
    x = unit(rng.uniform(-1, 1, (slots, d)).astype(np.float32))
    q = x[5].copy()
    empty = np.full(slots, EMPTY, np.uint32)
    assert check_refine(probe, oracle_mod, empty, empty, lists, k, x, q, COS, 3, "all empty") == 0xFFFFFFFF
    for live in (k - 1, k, k + 1):
        lo, hi = empty.copy(), empty.copy()
        at = rng.choice(slots, live, replace=False)
        lo[at] = (0xC0001000 + rng.integers(0, 50, live)).astype(np.uint32)
        hi[at] = 0x00001000
        ktp = check_refine(probe, oracle_mod, lo, hi, lists, k, x, q, COS, 3, "live=%d" % live)
        assert (ktp == 0xFFFFFFFF) == (live <= k)
    for name, where in (("one slice", np.arange(100, 100 + 3 * k + 5)), ("spread", np.arange(3 * k + 5) * (slots // (3 * k + 5)))):
        lo = (0xC0002000 + rng.integers(0, 1000, slots)).astype(np.uint32)
        hi = np.full(slots, 0x00002000, np.uint32)
        lo[where] = 0xC0001234
        smaller = rng.choice(np.setdiff1d(np.arange(slots), where), k // 2, replace=False)
        lo[smaller] = 0xC0001000
        check_refine(probe, oracle_mod, lo, hi, lists, k, x, q, COS, 3, "copies at Kt, " + name)
