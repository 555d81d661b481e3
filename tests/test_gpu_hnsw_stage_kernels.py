"""K15, the two scoring kernels behind an HNSW collection's staged searches (vt_hnsw_stage.hip: hnsw_stage_bits_kernel,
hnsw_stage_score_kernel), launched through tests/hnsw_stage_probe.cpp (libvt_hnsw_stage_probe.so: vt_hnsw_stage.hip and
nothing else of the library) on hand-made slabs, against the numpy model in tests/hnsw_stage_ref.py (which
tests/test_hnsw_stage_model.py holds to the oracle on the CPU).

Every key and every payload of a column is compared bit for bit; the columns are EXTRA entries longer than the contract
and start as 0xA5 bytes, so a write past the scanned positions shows; the slab's pad floats are NaN."""
import ctypes as C
import os

import numpy as np
import pytest

import hnsw_stage_ref as ref
from hnsw_stage_ref import COSINE, DIMS, INNER_PRODUCT, L2, ROWS
from test_gpu_parity import nifs  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = 5
FILL_KEY = np.uint64(0xA5A5A5A5A5A5A5A5)
METRICS = (L2, COSINE, INNER_PRODUCT)


class StageProbe:
    def __init__(self):
        path = os.environ.get("VT_HNSW_STAGE_PROBE_LIB") or os.path.join(ROOT, "vettore_amd", "lib", "libvt_hnsw_stage_probe.so")
        assert os.path.exists(path), "build it with `make` (%s)" % os.path.basename(path)
        F = self.lib = C.CDLL(path)
        f32p, u32p, u64p, vp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_void_p
        F.vths_no_row.restype = F.vths_lds_dim.restype = C.c_uint32
        F.vths_empty_key.restype = C.c_uint64
        F.vths_bits.argtypes = [f32p, C.c_uint32, C.c_uint32, C.c_uint32, u32p, f32p, C.c_uint32, u64p, vp]
        F.vths_score.argtypes = [f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, f32p, u32p, u32p, C.c_uint32, C.c_int, C.c_int,
                                 C.c_uint32, u64p, vp, C.POINTER(C.c_int)]
        assert F.vths_no_row() == ref.NO_ROW and F.vths_empty_key() == int(ref.EMPTY_KEY) and F.vths_lds_dim() == 4096

    @staticmethod
    def _p(a, t):
        return a.ctypes.data_as(C.POINTER(t))

    def bits(self, X, d, id_rank, q):
        X, rk, q = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(id_rank, np.uint32), np.ascontiguousarray(q, np.float32)
        rows, stride = X.shape
        keys, pay = np.zeros(rows + EXTRA, np.uint64), np.zeros(rows + EXTRA, ref.PAYLOAD)
        rc = self.lib.vths_bits(self._p(X, C.c_float), rows, stride, d, self._p(rk, C.c_uint32), self._p(q, C.c_float), EXTRA,
                                self._p(keys, C.c_uint64), pay.ctypes.data)
        return rc, keys, pay

    def score(self, X, d, p, id_rank, q, metric, order, rows=None):
        X, rk, q = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(id_rank, np.uint32), np.ascontiguousarray(q, np.float32)
        nrows, stride = X.shape
        lst = None if rows is None else np.ascontiguousarray(rows, np.uint32)
        n = nrows if lst is None else len(lst)
        keys, pay, status = np.zeros(n + EXTRA, np.uint64), np.zeros(n + EXTRA, ref.PAYLOAD), C.c_int(-1)
        one = np.zeros(1, np.uint32)
        rc = self.lib.vths_score(self._p(X, C.c_float), nrows, stride, d, p, self._p(q, C.c_float), self._p(rk, C.c_uint32),
                                 None if lst is None else self._p(lst if n else one, C.c_uint32), n, metric, order, EXTRA,
                                 self._p(keys, C.c_uint64), pay.ctypes.data, C.byref(status))
        return rc, keys, pay, status.value


@pytest.fixture(scope="module")
def probe():
    import vettore_amd._lib as L
    assert L.load().vt_device_count() >= 1, "no HIP device: GPU tests need the real hardware"
    return StageProbe()


@pytest.fixture
def order(nifs):
    return nifs.debug_get("reduce_order")


def assert_column(got_keys, got_pay, want_keys, want_pay, what):
    n = len(want_keys)
    assert len(got_keys) == n + EXTRA
    bad = np.flatnonzero(got_keys[:n] != want_keys)
    assert bad.size == 0, (what, "key", int(bad[0]), hex(int(got_keys[bad[0]])), hex(int(want_keys[bad[0]])))
    g, w = got_pay[:n].view(np.uint32).reshape(-1), want_pay.view(np.uint32).reshape(-1)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, "payload word", int(bad[0]), hex(int(g[bad[0]])), hex(int(w[bad[0]])))
    # bytes outside the contract keep the probe's fill
    assert (got_keys[n:] == FILL_KEY).all() and (got_pay[n:].view(np.uint64) == FILL_KEY).all(), what


def prefixes(d):
    return sorted({p for p in (1, 7, 8, 9, d - 1, d) if 1 <= p <= d})


@pytest.mark.parametrize("d", DIMS)
def test_bits_column_every_key_and_payload(probe, d):
    rng = np.random.default_rng(100 + d)
    for rows in ROWS:
        for kind in ("normal", "zeros", "two"):
            X = ref.make_slab(rng, rows, d, kind)
            q = ref.make_slab(rng, 1, d, "zeros" if kind == "zeros" else "normal")[0, :d]
            for name, dead in ref.dead_sets(rows).items():
                if kind != "normal" and name not in ("none", "every third"):
                    continue
                _, rk = ref.ranks_with_dead(rows, dead)
                rc, keys, pay = probe.bits(X, d, rk, q)
                assert rc == 0
                assert_column(keys, pay, *ref.bits_column(X, d, rk, q), (rows, d, kind, name))


def test_bits_of_zero_rows_launches_nothing(probe):
    rc, keys, pay = probe.bits(np.zeros((0, 8), np.float32), 8, np.zeros(0, np.uint32), np.ones(8, np.float32))
    assert rc == 0 and (keys == FILL_KEY).all()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_score_column_all_rows(probe, order, d, metric):
    rng = np.random.default_rng(200 + d * 7 + metric)
    q = rng.standard_normal(d).astype(np.float32)
    ps = prefixes(d)
    for rows in ROWS:
        X = ref.make_slab(rng, rows, d)
        for name, dead in ref.dead_sets(rows).items():
            _, rk = ref.ranks_with_dead(rows, dead)
            # every prefix where a row dies in every third place and at 65 rows; the shortest and the full one everywhere
            for p in (ps if name == "every third" or rows == 65 else sorted({ps[0], ps[-1]})):
                rc, keys, pay, status = probe.score(X, d, p, rk, q, metric, order)
                wk, wp, ws = ref.score_column(X, d, p, rk, q, metric, order)
                assert rc == 0 and status == ws == 0
                assert_column(keys, pay, wk, wp, (rows, d, p, name))


@pytest.mark.parametrize("lane_order", [0, 1, 2, 3])
def test_score_column_in_every_lane_order(probe, lane_order):
    rng = np.random.default_rng(17)
    X, q = ref.make_slab(rng, 65, 100), rng.standard_normal(100).astype(np.float32)
    _, rk = ref.ranks_with_dead(65, [3])
    for metric in (L2, INNER_PRODUCT):
        for p in (9, 100):
            rc, keys, pay, status = probe.score(X, 100, p, rk, q, metric, lane_order)
            wk, wp, _ = ref.score_column(X, 100, p, rk, q, metric, lane_order)
            assert rc == 0 and status == 0
            assert_column(keys, pay, wk, wp, (metric, p))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [3, 100, 130, 768])
def test_score_column_of_a_list(probe, order, d, metric):
    rng = np.random.default_rng(300 + d + metric)
    rows = 257
    X, q = ref.make_slab(rng, rows, d), rng.standard_normal(d).astype(np.float32)
    _, rk = ref.ranks_with_dead(rows, range(0, rows, 3))
    lists = {"repeated": [5, 5, 200, 5, 200, 256, 1], "descending": list(range(rows - 1, -1, -1)), "one": [77], "none": [],
             "many": list(rng.integers(0, rows, 300))}
    for name, lst in lists.items():
        for p in sorted({prefixes(d)[0], min(7, d), d}):
            rc, keys, pay, status = probe.score(X, d, p, rk, q, metric, order, lst)
            wk, wp, ws = ref.score_column(X, d, p, rk, q, metric, order, lst)
            assert rc == 0 and status == ws == 0
            assert_column(keys, pay, wk, wp, (name, p))


@pytest.mark.parametrize("metric", METRICS)
def test_rows_past_the_lds_tile_are_walked_where_they_lie(probe, order, metric):
    rng = np.random.default_rng(400 + metric)
    d = 4100
    X, q = ref.make_slab(rng, 8, d), rng.standard_normal(d).astype(np.float32)
    _, rk = ref.ranks_with_dead(8, [2])
    for p in (4096, 4097, d):  # the narrowest tile (two rows), then no tile at all
        for lst in (None, [7, 2, 0, 0]):
            rc, keys, pay, status = probe.score(X, d, p, rk, q, metric, order, lst)
            wk, wp, _ = ref.score_column(X, d, p, rk, q, metric, order, lst)
            assert rc == 0 and status == 0
            assert_column(keys, pay, wk, wp, (p, lst))


def test_a_zero_prefix_under_cosine_follows_cosine_raw(probe, order):
    rng = np.random.default_rng(9)
    X = ref.make_slab(rng, 70, 12)
    X[::2, :7] = 0.0
    X[1, :7] = -0.0
    q = rng.standard_normal(12).astype(np.float32)
    _, rk = ref.ranks_with_dead(70, [])
    for qq, p in ((q, 7), (q, 12), (np.concatenate([np.zeros(8, np.float32), q[8:]]), 8)):
        rc, keys, pay, status = probe.score(X, 12, p, rk, qq, COSINE, order)
        wk, wp, _ = ref.score_column(X, 12, p, rk, qq, COSINE, order)
        assert rc == 0 and status == 0
        assert_column(keys, pay, wk, wp, p)
        if p != 12:
            assert (wp["raw"][::2] == 0.0).all()


def test_a_nan_raw_value_raises_the_status_word(probe, order):
    X = np.zeros((66, 8), np.float32)
    X[:, 1] = 1.0
    X[65, 0] = X[3, 0] = 3e38
    rk = np.arange(66, dtype=np.uint32)
    big = np.asarray([3e38, 1, 0, 0, 0, 0, 0, 0], np.float32)
    # l2: the f32 chain overflows, the f64 recovery is finite -- no status, a key for every row
    rc, keys, pay, status = probe.score(X, 8, 8, rk, 0 * big, L2, order)
    wk, wp, ws = ref.score_column(X, 8, 8, rk, 0 * big, L2, order)
    assert rc == 0 and status == ws == 0 and (wk != ref.EMPTY_KEY).all() and wp["raw"][3] == np.float32(3e38)
    assert_column(keys, pay, wk, wp, "recovered")
    # inner product: the recovery is not finite either -- "metric overflow"
    rc, keys, pay, status = probe.score(X, 8, 8, rk, big, INNER_PRODUCT, order)
    wk, wp, ws = ref.score_column(X, 8, 8, rk, big, INNER_PRODUCT, order)
    assert rc == 0 and status == ws == ref.ERR_OVERFLOW and wk[3] == wk[65] == ref.EMPTY_KEY
    assert_column(keys, pay, wk, wp, "overflow")


def test_the_probe_refuses_what_a_kernel_would_index_with(probe, order):
    X, rk, q = np.zeros((4, 8), np.float32), np.arange(4, dtype=np.uint32), np.ones(8, np.float32)
    assert probe.score(X, 8, 8, rk, q, L2, order, [0, 4])[0] != 0   # a list entry beyond the slab
    assert probe.score(X, 8, 9, rk, q, L2, order)[0] != 0           # a prefix beyond d
    assert probe.score(X, 8, 0, rk, q, L2, order)[0] != 0
