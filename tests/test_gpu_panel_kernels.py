"""The row-panel kernels against the oracle, cell by cell (csrc/vt_panel.cuh).

K1p (vt_prefix_multi.hip), K6bm and K6b (vt_cosine.hip) run stage 1 of every funnel group and every prefix sweep of a batch.
The funnel and sweep tests compare final hits and tolerate a threshold that misses: a sample cell off by one tile, a count
that forgets the rows past the cap, a maximum taken over the wrong tile would pass them and only make the product slower.
Here the kernels are launched one at a time through tests/panel_probe.cpp (libvt_panel_probe.so: vt_cosine.o,
vt_prefix_multi.o and nothing else of the library), with ONE block of four waves, and everything is read back:

  dense    every sample cell is the oracle's value in the kernel's "larger is better" orientation (-rank_value for K1p, raw
           for K6bm), bit for bit; rows past n hold -inf; cells outside sample_rows and of queries >= nq keep their fill;
  maxima   one value per query and sampled tile: the maximum of that tile's dense values; nothing else is written;
  lists    tau near the median with rows scoring exactly tau: the count is the number of rows < n at or above tau, the
           listed (key, row, raw bits) set is the expected one (append order is the atomics': compared as sets), with the cap
           below the count the count is still full and exactly cap slots are written, slots of queries >= nq keep their fill;
  overflow a pair that recovers in f64 is listed with the recovered bits, one that does not sets the status word in sweep
           mode and is not listed, and in dense mode gives -inf with the status word 0;
  K6b      the block's list is the oracle's vector_top_k on the prefix (k = 5 and 70: both wave buffers), the key column
           holds the same keys, has_lo excludes keys <= lo_key.

Shapes: n = 549 = 2 * 4 * 64 + 37 gives every wave of the one block a second tile (the "next tile, panel 0" prefetch) and a
partial last tile (the clamp; rows >= n never listed, never counted); d = 1 .. 70 is only a scalar tail, one whole chunk, a
partial panel with a tail, exactly one panel, a second panel of one float, a tail that starts a panel, two panels, a third
panel with a tail.  Each axis is walked against the base shape (n = 549, d = 70, nq = 3); dot walks every d in both modes.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
G = 8
K1P, K6BM = 0, 1
SWEEP, DENSE, MAXIMA = 0, 1, 2
L2, L2SQ, COS, IP, NIP, L1, LINF = 0, 1, 2, 3, 4, 5, 6
ERR_OVERFLOW = 4
SENT32 = np.uint32(0xA5A5A5A5)
SENT64 = np.uint64(0xA5A5A5A5A5A5A5A5)
NINF = np.float32(-np.inf)
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
NS = (1, 63, 64, 549)
DS = (1, 7, 8, 31, 32, 33, 36, 64, 70)
BASE = dict(n=549, d=70, nq=3)


class VppGroup(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("mode", C.c_int32), ("metric", C.c_int32), ("order", C.c_int32),
                ("n", C.c_uint32), ("d", C.c_uint32), ("nq", C.c_uint32), ("q_stride", C.c_uint32),
                ("sample_stride", C.c_uint32), ("sample_rows", C.c_uint32), ("cand_cap", C.c_uint32), ("blocks", C.c_uint32),
                ("X", C.c_void_p), ("x_floats", C.c_uint64), ("stride", C.c_uint64),
                ("Q", C.c_void_p), ("q_floats", C.c_uint64),
                ("id_rank", C.c_void_p), ("rank_len", C.c_uint64),
                ("tau", C.c_void_p), ("tau_len", C.c_uint64),
                ("sample", C.c_void_p), ("sample_len", C.c_uint64),
                ("cand_keys", C.c_void_p), ("cand_rows", C.c_void_p), ("cand_raw", C.c_void_p), ("cand_len", C.c_uint64),
                ("cand_count", C.c_void_p), ("count_len", C.c_uint64),
                ("status", C.c_void_p)]


def ptr(a):
    return None if a is None else a.ctypes.data


class Probe:
    def __init__(self):
        # VT_PANEL_PROBE_LIB: another build of the same probe (a deliberately broken kernel, to see these tests fail)
        path = os.environ.get("VT_PANEL_PROBE_LIB") or os.path.join(ROOT, "vettore_amd", "lib", "libvt_panel_probe.so")
        assert os.path.exists(path), "build it with `make` (%s)" % os.path.basename(path)
        L = self.lib = C.CDLL(path)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.vpp_group_max.restype = u32
        L.vpp_padded_dim.restype = u32
        L.vpp_padded_dim.argtypes = [u32]
        L.vpp_group_lds_bytes.restype = C.c_size_t
        L.vpp_group_blocks_per_cu.argtypes = [C.c_int]
        L.vpp_group.argtypes = [C.POINTER(VppGroup)]
        L.vpp_cosine_scan.argtypes = [vp, u64, u64, u32, u32, vp, u64, vp, u64, u32, C.c_int, u64, u32, vp, vp, vp, u64, vp, u64, vp]
        assert L.vpp_group_max() == G

    def group(self, kernel, mode, case, metric=COS, order=0, tau=None, cap=0, id_rank=None, sample_stride=1, sample_rows=0, expect=0):
        """One launch on one block.  Dense modes: sample[G][sample_rows]; sweep: (keys, rows, raw bits)[G][cap], count[G]."""
        p = VppGroup(kernel=kernel, mode=mode, metric=metric, order=order, n=case.n, d=case.d, nq=case.nq, q_stride=case.q_stride,
                     sample_stride=sample_stride, sample_rows=sample_rows, cand_cap=cap, blocks=1,
                     X=ptr(case.xbuf), x_floats=case.xbuf.size, stride=case.stride, Q=ptr(case.qbuf), q_floats=case.qbuf.size)
        status = np.full(1, -1, np.int32)
        p.status = ptr(status)
        if id_rank is not None:
            p.id_rank, p.rank_len = ptr(id_rank), id_rank.size
        keep = [status, id_rank]
        if mode == SWEEP:
            tau = np.ascontiguousarray(tau, np.float32)
            keys, rows, raw = np.zeros((G, cap), np.uint64), np.zeros((G, cap), np.uint32), np.zeros((G, cap), np.uint32)
            count = np.full(G, 77, np.uint32)
            p.tau, p.tau_len = ptr(tau), tau.size
            p.cand_keys, p.cand_rows, p.cand_raw, p.cand_len = ptr(keys), ptr(rows), ptr(raw), keys.size
            p.cand_count, p.count_len = ptr(count), count.size
            keep += [tau]
        else:
            sample = np.zeros((G, sample_rows), np.float32)
            p.sample, p.sample_len = ptr(sample), sample.size
        rc = self.lib.vpp_group(C.byref(p))
        assert rc == expect, "vpp_group: hipError_t %d" % rc
        if mode == SWEEP:
            return keys, rows, raw, count, int(status[0])
        return sample, int(status[0])

    def cosine_scan(self, case, q, k, id_rank=None, lo_key=None, key_column=False, expect=0):
        q = np.ascontiguousarray(q, np.float32)
        status = np.full(1, -1, np.int32)
        keys, rows, raw = np.zeros(k, np.uint64), np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        col = np.zeros(case.n, np.uint64) if key_column else None
        rc = self.lib.vpp_cosine_scan(ptr(case.xbuf), case.xbuf.size, case.stride, case.n, case.d, ptr(q), q.size, ptr(id_rank),
                                      0 if id_rank is None else id_rank.size, k, int(lo_key is not None), int(lo_key or 0), 1,
                                      ptr(keys), ptr(rows), ptr(raw), keys.size, ptr(col), 0 if col is None else col.size, ptr(status))
        assert rc == expect, "vpp_cosine_scan: hipError_t %d" % rc
        return (col if key_column else (keys, rows, raw)), int(status[0])


@pytest.fixture(scope="module")
def probe():
    return Probe()


def padded_dim(d):
    return (d + 63) // 64 * 64


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def orderable(f):
    u = bits(f).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)


class Case:
    """A seed-fixed corpus: n rows of d meaningful floats `stride` apart, nq queries.  Every row stands in the corpus twice
    (row i and row i + ceil(n / 2)), so every score is met at least twice: a threshold taken from the scores has rows exactly
    on it.  What lies behind column d -- the rest of the rows and of the query rows -- is NaN: nothing may read it into a sum."""

    def __init__(self, n, d, nq, stride=None, seed=0):
        rng = np.random.default_rng(1000 * n + 10 * d + nq + seed)
        self.n, self.d, self.nq = n, d, nq
        self.stride = stride or padded_dim(d)
        self.q_stride = (max(d, 8) + 7) // 8 * 8
        half = (n + 1) // 2
        rows = rng.standard_normal((half, d)).astype(np.float32)
        self.X = np.concatenate([rows, rows])[:n].copy()
        self.Qs = rng.standard_normal((nq, d)).astype(np.float32)
        self.pack()

    def pack(self):
        x = np.full((self.n, self.stride), np.nan, np.float32)
        x[:, :self.d] = self.X
        self.xbuf = x.reshape(-1)
        q = np.full((G, self.q_stride), np.nan, np.float32)
        q[:, :self.d] = 0.0      # (the unused query rows are readable and finite: K1p sums them too)
        q[:self.nq, :self.d] = self.Qs
        self.qbuf = q.reshape(-1)


_CASES, _EXPECT = {}, {}


def case_of(n=BASE["n"], d=BASE["d"], nq=BASE["nq"], stride=None):
    key = (n, d, nq, stride)
    if key not in _CASES:
        _CASES[key] = Case(n, d, nq, stride)
    return _CASES[key]


def expected(om, case, kernel, metric=COS, order=0, tag=None):
    """(good[nq][n] f32 with -inf where a pair has no value, rank[nq][n] f32, raw[nq][n] f32, valid[nq][n]) from the oracle,
    computed once per (corpus, kernel, metric, order) and never changed."""
    key = (id(case), tag, kernel, metric, order)
    if key in _EXPECT:
        return _EXPECT[key]
    nq, n = case.nq, case.n
    raw, valid = np.zeros((nq, n), np.float32), np.ones((nq, n), bool)
    rank = np.zeros((nq, n), np.float32)
    om.set_reduce_order(order)
    try:
        for q in range(nq):
            for r in range(n):
                try:
                    if kernel == K6BM:
                        raw[q, r] = om.cosine(case.Qs[q], case.X[r])
                        rank[q, r] = np.float32(1.0) - raw[q, r]
                    else:
                        raw[q, r] = om.compute(metric, case.Qs[q], case.X[r])
                        rank[q, r] = om.rank_value(metric, raw[q, r])
                except om.OracleError:
                    valid[q, r] = False
    finally:
        om.set_reduce_order(3)
    good = raw.copy() if kernel == K6BM else -rank
    good[~valid] = NINF
    out = _EXPECT[key] = (good, rank, raw, valid)
    for a in out:
        a.setflags(write=False)
    return out


def tiles_of(n, step=1):
    return ((n + 63) // 64 + step - 1) // step


def dense_expected(good, n, step, sample_rows):
    """What dense mode writes of sample[q][0 .. sample_rows): cell ti * 64 + lane is row ti * step * 64 + lane; -inf past n."""
    nq = good.shape[0]
    want = np.full((nq, tiles_of(n, step) * 64), NINF, np.float32)
    for ti in range(tiles_of(n, step)):
        lo = ti * step * 64
        hi = min(n, lo + 64)
        want[:, ti * 64:ti * 64 + hi - lo] = good[:, lo:hi]
    return want[:, :sample_rows]


def check_dense(probe, om, case, kernel, metric=COS, order=0, tag=None, steps=(1, 2)):
    good = expected(om, case, kernel, metric, order, tag)[0]
    for step in steps:
        if step > (case.n + 63) // 64:
            continue
        full = tiles_of(case.n, step) * 64
        for sample_rows in (full, max(1, full - 27))[:3 - step]:   # (the second: the last cells fall outside the sample)
            sample, status = probe.group(kernel, DENSE, case, metric, order, sample_stride=step, sample_rows=sample_rows)
            want = dense_expected(good, case.n, step, sample_rows)
            assert status == 0
            assert np.array_equal(bits(sample[:case.nq]), bits(want)), (step, sample_rows, np.argwhere(bits(sample[:case.nq]) != bits(want))[:5])
            assert np.all(bits(sample[case.nq:]) == SENT32), "cells of queries >= nq were written"
        tiles = tiles_of(case.n, step)
        maxima, status = probe.group(kernel, MAXIMA, case, metric, order, sample_stride=step, sample_rows=tiles)
        want = dense_expected(good, case.n, step, full).reshape(case.nq, tiles, 64).max(axis=2)
        assert status == 0
        assert np.array_equal(bits(maxima[:case.nq]), bits(want)), (step, np.argwhere(bits(maxima[:case.nq]) != bits(want))[:5])
        assert np.all(bits(maxima[case.nq:]) == SENT32)


def median_tau(good):
    """tau[G]: per query a score near the median of its finite scores (every score is met twice: rows sit exactly on it)."""
    tau = np.full(G, np.inf, np.float32)
    for q in range(good.shape[0]):
        finite = np.sort(good[q][np.isfinite(good[q])])
        tau[q] = finite[finite.size // 2]
    return tau


def check_lists(probe, om, case, kernel, metric=COS, order=0, id_rank=None, tag=None, want_status=0):
    good, rank, raw, valid = expected(om, case, kernel, metric, order, tag)
    tau = median_tau(good)
    hit = valid & (good >= tau[:case.nq, None])
    counts = hit.sum(axis=1).astype(np.uint32)
    if case.n > 2 and tag is None:
        assert all((good[q] == tau[q]).sum() >= 2 for q in range(case.nq)), "the corpus must put rows exactly on tau"
    low = np.arange(case.n, dtype=np.uint64) if id_rank is None else id_rank.astype(np.uint64)
    cap = int(counts.max()) + 3
    keys, rows, rawb, count, status = probe.group(kernel, SWEEP, case, metric, order, tau=tau, cap=cap, id_rank=id_rank)
    assert status == want_status
    assert np.array_equal(count[:case.nq], counts), (count, counts)
    assert np.all(count[case.nq:] == 0), "a count of a query >= nq moved"
    for q in range(case.nq):
        r = np.flatnonzero(hit[q])
        want = set(zip(((orderable(rank[q, r]) << np.uint64(32)) | low[r]).tolist(), r.tolist(), bits(raw[q, r]).tolist()))
        c = int(counts[q])
        got = set(zip(keys[q, :c].tolist(), rows[q, :c].tolist(), rawb[q, :c].tolist()))
        assert got == want, (q, sorted(got ^ want)[:4])
        assert np.all(keys[q, c:] == SENT64) and np.all(rows[q, c:] == SENT32), "slots past the count were written"
    assert np.all(keys[case.nq:] == SENT64) and np.all(rows[case.nq:] == SENT32) and np.all(rawb[case.nq:] == SENT32)
    # the cap below the count: the count is still the full count, exactly cap slots are written, each a listed pair
    small = max(1, int(counts.min()) // 2)
    if small < int(counts.min()):
        keys, rows, rawb, count, status = probe.group(kernel, SWEEP, case, metric, order, tau=tau, cap=small, id_rank=id_rank)
        assert np.array_equal(count[:case.nq], counts)
        for q in range(case.nq):
            r = np.flatnonzero(hit[q])
            want = set(zip(((orderable(rank[q, r]) << np.uint64(32)) | low[r]).tolist(), r.tolist(), bits(raw[q, r]).tolist()))
            got = set(zip(keys[q].tolist(), rows[q].tolist(), rawb[q].tolist()))
            assert len(got) == small and got <= want, (q, sorted(got - want)[:4])
        assert np.all(keys[case.nq:] == SENT64)


# ---- K1p ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
def test_k1p_dot_every_prefix(probe, oracle_mod, d):
    case = case_of(d=d)
    check_dense(probe, oracle_mod, case, K1P, IP, 3)
    check_lists(probe, oracle_mod, case, K1P, IP, 3)


@pytest.mark.parametrize("metric", (L2, L2SQ, NIP, L1, LINF))
def test_k1p_metrics(probe, oracle_mod, metric):
    case = case_of()
    check_dense(probe, oracle_mod, case, K1P, metric, 3)
    check_lists(probe, oracle_mod, case, K1P, metric, 3)


@pytest.mark.parametrize("metric", (IP, L2))
@pytest.mark.parametrize("order", (0, 1, 2))
def test_k1p_lane_orders(probe, oracle_mod, metric, order):
    case = case_of()
    check_dense(probe, oracle_mod, case, K1P, metric, order, steps=(2,))
    check_lists(probe, oracle_mod, case, K1P, metric, order)


@pytest.mark.parametrize("n", NS[:3])
def test_k1p_rows(probe, oracle_mod, n):
    case = case_of(n=n)
    check_dense(probe, oracle_mod, case, K1P, L2, 3)
    check_lists(probe, oracle_mod, case, K1P, L2, 3)


@pytest.mark.parametrize("nq", (1, 8))
def test_k1p_queries(probe, oracle_mod, nq):
    case = case_of(nq=nq)
    check_dense(probe, oracle_mod, case, K1P, IP, 3, steps=(1,))
    check_lists(probe, oracle_mod, case, K1P, IP, 3)


def test_k1p_wide_rows_and_id_rank(probe, oracle_mod):
    case = case_of(stride=192)
    check_dense(probe, oracle_mod, case, K1P, L2, 3)
    rank = np.random.default_rng(5).permutation(case.n).astype(np.uint32)
    check_lists(probe, oracle_mod, case, K1P, L2, 3, id_rank=rank)


def overflow_case(metric):
    """The base shape with three rows and query 0 made large: row 0 recovers in f64, row 1 does not, row 2 is its twin
    behind the panel boundary."""
    case = Case(BASE["n"], BASE["d"], BASE["nq"], seed=metric + 1)
    case.Qs[0, :] = 0.0
    case.X[0:3, :] = 0.0
    if metric == IP:
        case.Qs[0, 0:2] = 3e38
        case.X[0, 0:2] = (2.0, -1.5)      # inf + -inf in f32; 1.5e38 in f64
        case.X[1, 0:2] = (3e38, 3e38)     # 1.8e77: no f32
        case.X[2, 40:42] = (3e38, 3e38)   # finite: the query is zero there
    else:
        case.Qs[0, 0] = 3e38
        case.X[0, 0] = 2.9e38             # (1e37)^2 overflows f32; the f64 root is 1e37
        case.X[1, 0] = -3e38              # 6e38: no f32
        case.X[2, 40] = 1e38              # finite: the f64 root stays below FLT_MAX
    case.pack()
    return case


@pytest.mark.parametrize("metric", (IP, L2))
def test_k1p_overflow(probe, oracle_mod, metric):
    case = overflow_case(metric)
    good, rank, raw, valid = expected(oracle_mod, case, K1P, metric, 3, tag="overflow")
    assert valid[0, 0] and np.isfinite(raw[0, 0]) and not valid[0, 1] and valid[0, 2]
    check_dense(probe, oracle_mod, case, K1P, metric, 3, tag="overflow")   # -inf in the cell, status 0
    check_lists(probe, oracle_mod, case, K1P, metric, 3, tag="overflow", want_status=ERR_OVERFLOW)
    # the recovered pair, listed with the recovered bits: a threshold below everything lists every pair that has a value
    tau = np.full(G, -np.inf, np.float32)
    keys, rows, rawb, count, status = probe.group(K1P, SWEEP, case, metric, 3, tau=tau, cap=case.n)
    assert status == ERR_OVERFLOW and np.array_equal(count[:case.nq], valid.sum(axis=1))
    listed = dict(zip(rows[0, :count[0]].tolist(), rawb[0, :count[0]].tolist()))
    assert 1 not in listed and listed[0] == int(bits(raw[0, 0]).ravel()[0])


# ---- K6bm ---------------------------------------------------------------------------------------------------------------
def cosine_case(**kw):
    return case_of(**kw)


@pytest.mark.parametrize("d", (1, 8, 33, 70))
def test_k6bm_prefixes(probe, oracle_mod, d):
    case = cosine_case(d=d)
    check_dense(probe, oracle_mod, case, K6BM)
    check_lists(probe, oracle_mod, case, K6BM)


@pytest.mark.parametrize("n,nq", ((1, 3), (63, 3), (64, 3), (549, 1), (549, 8)))
def test_k6bm_rows_and_queries(probe, oracle_mod, n, nq):
    case = cosine_case(n=n, nq=nq)
    check_dense(probe, oracle_mod, case, K6BM, steps=(1,))
    check_lists(probe, oracle_mod, case, K6BM)


def zero_case():
    case = Case(BASE["n"], BASE["d"], BASE["nq"], stride=192, seed=99)
    case.Qs[1, :] = 0.0          # a zero prefix query: 0.0 against every row
    case.X[5, :] = 0.0           # a zero row: 0.0 against every query
    case.X[300, :] = 0.0
    case.pack()
    return case


def test_k6bm_zero_vectors_wide_rows_and_id_rank(probe, oracle_mod):
    case = zero_case()
    good = expected(oracle_mod, case, K6BM, tag="zero")[0]
    assert np.all(good[1] == 0.0) and np.all(good[:, 5] == 0.0)
    check_dense(probe, oracle_mod, case, K6BM, tag="zero")
    rank = np.random.default_rng(6).permutation(case.n).astype(np.uint32)
    check_lists(probe, oracle_mod, case, K6BM, id_rank=rank, tag="zero")


def test_k6bm_overflow(probe, oracle_mod):
    """A similarity that is not finite (an infinite row entry: the oracle refuses such a vector) has no value."""
    case = Case(BASE["n"], BASE["d"], BASE["nq"], seed=7)
    case.X[70, 3] = np.inf
    case.pack()
    good, rank, raw, valid = expected(oracle_mod, case, K6BM, tag="inf")
    assert not valid[:, 70].any() and valid.sum() == case.nq * (case.n - 1)
    check_dense(probe, oracle_mod, case, K6BM, tag="inf")
    check_lists(probe, oracle_mod, case, K6BM, tag="inf", want_status=ERR_OVERFLOW)


# ---- K6b ----------------------------------------------------------------------------------------------------------------
def k6b_query(case, q):
    out = np.zeros(padded_dim(case.d), np.float32)
    out[:case.d] = case.Qs[q]
    return out


def k6b_expected(om, case, q, id_rank, k):
    """[(key, row, raw bits)] of the oracle's vector_top_k on the prefix, ids ranked as id_rank ranks the rows."""
    vectors = [(b"%08d" % int(id_rank[r]), case.X[r]) for r in range(case.n)]
    hits = om.vector_top_k(vectors, case.Qs[q], COS, case.d, k)
    row_of = {int(id_rank[r]): r for r in range(case.n)}
    out = []
    for id_, raw in hits:
        raw = np.float32(raw)
        key = (int(orderable(np.float32(1.0) - raw).ravel()[0]) << 32) | int(id_)
        out.append((key, row_of[int(id_)], int(bits(raw).ravel()[0])))
    return out


@pytest.mark.parametrize("k", (5, 70))
@pytest.mark.parametrize("n,d", ((549, 70), (63, 33), (549, 32)))
def test_k6b_top_k_key_column_and_lo(probe, oracle_mod, k, n, d):
    case = zero_case() if (n, d) == (549, 70) else cosine_case(n=n, d=d)
    id_rank = np.random.default_rng(8).permutation(case.n).astype(np.uint32)
    kk = min(k, case.n)
    for q in range(2 if (n, d) == (549, 70) else 1):
        want = k6b_expected(oracle_mod, case, q, id_rank, case.n)        # every row, in the oracle's order
        (keys, rows, rawb), status = probe.cosine_scan(case, k6b_query(case, q), k, id_rank)
        assert status == 0
        order = np.argsort(keys, kind="stable")[:kk]
        got = list(zip(keys[order].tolist(), rows[order].tolist(), rawb[order].tolist()))
        assert got == want[:kk], (q, got[:3], want[:3])
        assert (keys != EMPTY_KEY).sum() == kk
        col, status = probe.cosine_scan(case, k6b_query(case, q), k, id_rank, key_column=True)
        assert status == 0
        assert col.tolist() == [key for key, _ in sorted(((key, row) for key, row, _ in want), key=lambda t: t[1])]
        # has_lo: only keys above the kk-th best of the first list -- the next page
        lo = want[kk - 1][0]
        (keys, rows, rawb), status = probe.cosine_scan(case, k6b_query(case, q), k, id_rank, lo_key=lo)
        rest = [w for w in want if w[0] > lo][:k]
        order = np.argsort(keys, kind="stable")[:len(rest)]
        assert (keys != EMPTY_KEY).sum() == len(rest)
        assert list(zip(keys[order].tolist(), rows[order].tolist(), rawb[order].tolist())) == rest
        col, status = probe.cosine_scan(case, k6b_query(case, q), k, id_rank, lo_key=lo, key_column=True)
        by_row = sorted(((key, row) for key, row, _ in want), key=lambda t: t[1])
        assert col.tolist() == [key if key > lo else int(EMPTY_KEY) for key, _ in by_row]


# ---- the probe's own checks ------------------------------------------------------------------------------------------------
def test_probe_refuses_what_the_kernels_would_overrun(probe):
    case = case_of(n=64, d=33)
    tau = np.zeros(G, np.float32)
    short = Case(64, 33, 3)
    short.xbuf = short.xbuf[:-1]
    probe.group(K1P, SWEEP, short, IP, 3, tau=tau, cap=8, expect=HIP_INVALID_VALUE)
    probe.group(K1P, SWEEP, case, IP, 3, tau=tau, cap=8, id_rank=np.zeros(63, np.uint32), expect=HIP_INVALID_VALUE)
    probe.group(K1P, DENSE, case, IP, 3, sample_stride=2, sample_rows=64, expect=HIP_INVALID_VALUE)   # one tile: no second
    probe.group(K1P, SWEEP, case, COS, 3, tau=tau, cap=8, expect=HIP_INVALID_VALUE)                   # the launcher's own check
    probe.cosine_scan(case, np.zeros(63, np.float32), 5, expect=HIP_INVALID_VALUE)
    probe.cosine_scan(case, np.zeros(64, np.float32), 257, expect=HIP_INVALID_VALUE)
    assert probe.lib.vpp_group_lds_bytes() == 4 * 64 * 36 * 4
    assert probe.lib.vpp_group_blocks_per_cu(IP) == 2 and probe.lib.vpp_group_blocks_per_cu(COS) == 0
