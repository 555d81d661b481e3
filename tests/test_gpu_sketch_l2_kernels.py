"""The int8 sketch's L2 family, kernel by kernel, against its numpy model and the oracle.

tests/test_sketch8_l2_model.py shows on the CPU that the model's two words hold the oracle's f32 distance;
tests/test_gpu_sketch_l2.py shows that a search's hits are the oracle's.  Here the kernels themselves are launched through
tests/sketch_l2_probe.cpp (libvt_sketch_l2_probe.so: vt_sketch.hip and nothing else of the library):

  A  the builders' images with xx and without it, byte for byte against the model (rho, nu and xx inside their bands; the
     fourth dword zero when xx is not asked for -- a cosine or dot handle's image is what it was);
  B  the pass's lists: every row's two words equal the model's bit for bit, and hold the oracle's value;
  C  the tail: outcome, Kt, the candidate set, and the rescored block bit for bit what the oracle gives those rows -- in all
     three outcomes (rescored by the block, left for the gathered K1, refused) and every lane order.

Geometry of B: the pass numbers its waves block by block, so with blocks = tiles / 4 and lists of 256 block b owns tiles
4 b .. 4 b + 3 and its list holds every one of their rows.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import sketch6_ref as ref6
import sketch8_l2_ref as ref
import sketch8_ref as ref8
from test_gpu_sketch_kernels import assert_band, edge_rows, exact_norms, max_norm_bits, padded_dim, strided

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2, L2SQ = ref.M_L2, ref.M_L2SQ
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
SIZES = (63, 64, 65, 9001)
DIMS = (100, 192)
FLT_MAX = float(np.finfo(np.float32).max)


class Probe:
    def __init__(self):
        path = os.environ.get("VT_SKETCH_L2_PROBE_LIB") or os.path.join(ROOT, "vettore_amd", "lib", "libvt_sketch_l2_probe.so")
        assert os.path.exists(path), "build it with `make` (%s)" % os.path.basename(path)
        L = self.lib = C.CDLL(path)
        u8p, u32p, u64p, f32p, i32p = (C.POINTER(t) for t in (C.c_ubyte, C.c_uint32, C.c_uint64, C.c_float, C.c_int))
        L.vtl_image_bytes.restype = C.c_size_t
        L.vtl_image_bytes.argtypes = [C.c_uint32, C.c_uint32]
        L.vtl_build.argtypes = [C.c_int, f32p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, u8p, C.c_size_t, u64p]
        L.vtl_rows.argtypes = [C.c_int, f32p, C.c_size_t, C.c_size_t, u32p, C.c_uint32, C.c_uint32, C.c_uint32, u8p, C.c_size_t, u64p]
        L.vtl_scan.argtypes = [u8p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int, u32p, u8p, C.c_size_t, f32p] + [C.c_double] * 5 + \
                              [C.c_uint32, C.c_uint32, u64p, u32p]
        L.vtl_tail.argtypes = [u64p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, f32p, C.c_size_t, C.c_uint32, f32p, u32p,
                               C.c_uint32, C.c_int, C.c_int, u32p, u32p, u32p, i32p, i32p, u64p, u32p, f32p]

    @staticmethod
    def _p(a, ctype):
        return a.ctypes.data_as(C.POINTER(ctype))

    def build(self, with_xx, xbuf, stride, n_src, rows_img, d):
        img = np.zeros(self.lib.vtl_image_bytes(rows_img, d), np.uint8)
        mx = np.zeros(1, np.uint64)
        rc = self.lib.vtl_build(int(with_xx), self._p(xbuf, C.c_float), xbuf.size, stride, n_src, rows_img, d,
                                self._p(img, C.c_ubyte), img.size, self._p(mx, C.c_uint64))
        assert rc == 0, "vtl_build: hipError_t %d" % rc
        return img, int(mx[0])

    def rows(self, with_xx, xbuf, stride, rowlist, rows_img, d, img, max_norm):
        img = img.copy()
        mx = np.array([max_norm], np.uint64)
        rowlist = np.ascontiguousarray(rowlist, np.uint32)
        rc = self.lib.vtl_rows(int(with_xx), self._p(xbuf, C.c_float), xbuf.size, stride, self._p(rowlist, C.c_uint32), rowlist.size,
                               rows_img, d, self._p(img, C.c_ubyte), img.size, self._p(mx, C.c_uint64))
        assert rc == 0, "vtl_rows: hipError_t %d" % rc
        return img, int(mx[0])

    def scan(self, img, n, d, metric, id_rank, qy, k, blocks):
        img = np.ascontiguousarray(img, np.uint8).reshape(-1)
        qimg = np.ascontiguousarray(qy.image).view(np.uint8).reshape(-1)
        t = np.ascontiguousarray(qy.t, np.float32)
        keys = np.zeros((blocks, k), np.uint64)
        pay = np.zeros((blocks, k, 2), np.uint32)
        rank = None if id_rank is None else np.ascontiguousarray(id_rank, np.uint32)
        rc = self.lib.vtl_scan(self._p(img, C.c_ubyte), img.size, n, d, metric, None if rank is None else self._p(rank, C.c_uint32),
                               self._p(qimg, C.c_ubyte), qimg.size, self._p(t, C.c_float), qy.qn, qy.eta, qy.kerr, qy.qq_lo, qy.qq_hi,
                               k, blocks, self._p(keys, C.c_uint64), self._p(pay, C.c_uint32))
        assert rc == 0, "vtl_scan: hipError_t %d" % rc
        return keys, pay

    def tail(self, keys, pay, k, cap, x, q, id_rank, metric, order):
        lists, kp = keys.shape
        n, d = x.shape
        stride = padded_dim(d)
        xbuf = strided(x, stride)
        qbuf = np.zeros(stride, np.float32)
        qbuf[:d] = q
        keys, pay = np.ascontiguousarray(keys, np.uint64), np.ascontiguousarray(pay, np.uint32)
        rank = None if id_rank is None else np.ascontiguousarray(id_rank, np.uint32)
        out = dict(rows=np.zeros(cap, np.uint32), count=np.zeros(1, np.uint32), info=np.zeros(4, np.uint32),
                   status=np.zeros(1, np.int32), head=np.zeros(2, np.int32), keys=np.zeros(k, np.uint64),
                   res_rows=np.zeros(k, np.uint32), raw=np.zeros(k, np.float32))
        rc = self.lib.vtl_tail(self._p(keys, C.c_uint64), self._p(pay, C.c_uint32), lists, kp, k, cap, self._p(xbuf, C.c_float),
                               stride, n, self._p(qbuf, C.c_float), None if rank is None else self._p(rank, C.c_uint32), d, metric,
                               order, self._p(out["rows"], C.c_uint32), self._p(out["count"], C.c_uint32),
                               self._p(out["info"], C.c_uint32), self._p(out["status"], C.c_int), self._p(out["head"], C.c_int),
                               self._p(out["keys"], C.c_uint64), self._p(out["res_rows"], C.c_uint32), self._p(out["raw"], C.c_float))
        assert rc == 0, "vtl_tail: hipError_t %d" % rc
        return out


@pytest.fixture(scope="module")
def probe():
    return Probe()


# ---- A. the builders -------------------------------------------------------------------------------------------------------
def builder_corpus(d, n):
    """Rows of any scale with the quantiser's edge rows among them (a zero row, subnormals, an element near the largest f32
    -- whose xx is infinite --, exact ties) and a few of the L2 family's own (unit rows, one spike)."""
    rng = np.random.default_rng(7100 + d)
    x = (rng.uniform(-1, 1, (n, d)) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)
    e = np.concatenate([edge_rows(d, 127), ref.unit(rng.uniform(-1, 1, (3, d)))])
    at = np.arange(len(e)) * 5 % n
    x[at] = e
    return x


def exact_sq(x):
    return np.array([math.fsum((r.astype(np.float64) ** 2).tolist()) for r in x])


def check_image(img, x, n_src, rows_img, d, with_xx, what):
    """The image equals the model's of x[:n_src] byte for byte, rho, nu and xx apart, which lie in their bands; without xx
    the fourth dword is zero in every row."""
    Xm, sm, _, _ = ref8.quantise_rows(x[:n_src])
    assert img.size == (ref8.chunks_of(d) + 1) * 1024 * rows_img // 64
    img3 = img.reshape(rows_img // 64, ref8.chunks_of(d) + 1, 64, 16)
    Xd, sd, rhod, nud, xxd = ref.unpack_tiles(img3, n_src, d)
    assert np.array_equal(Xd, Xm), what
    assert np.array_equal(sd.view(np.uint32), sm.view(np.uint32)), what
    R, N = exact_norms(x[:n_src], Xm, sm)
    assert_band(rhod, R, what + " rho")
    assert_band(nud, N, what + " nu")
    if with_xx:
        sq = exact_sq(x[:n_src])
        fits = sq * (1.0 + 2.0 ** -29) < FLT_MAX
        assert_band(xxd[fits], sq[fits], what + " xx")
        assert np.all(np.isposinf(xxd[~fits])), what  # (past the largest f32: rounded up to infinity, and the search declines)
    else:
        assert not xxd.view(np.uint32).any(), what
    want = np.zeros(img.size, np.uint8)
    model = ref.pack_tiles(Xm, sm, rhod, nud, xxd if with_xx else None).reshape(-1)
    want[:model.size] = model
    assert np.array_equal(img, want), (what, np.nonzero(img != want)[0][:8])
    return rhod, nud


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("with_xx", [True, False])
def test_builders_write_the_models_image(probe, d, with_xx):
    full = builder_corpus(d, 9001)
    for n in SIZES:
        rows_img = (n + 63) // 64 * 64 + (64 if n == 65 else 0)  # (n = 65: an empty tile beyond)
        stride = padded_dim(d) + (64 if n == 63 else 0)
        what = "xx %d d %d n %d" % (with_xx, d, n)
        img, mx = probe.build(with_xx, strided(full[:n], stride), stride, n, rows_img, d)
        rhod, nud = check_image(img, full, n, rows_img, d, with_xx, what)
        assert mx == max_norm_bits(rhod, nud), what
        if with_xx and n == 65:  # the two builders differ in the fourth dword alone
            plain, mx0 = probe.build(False, strided(full[:n], stride), stride, n, rows_img, d)
            meta = np.zeros(img.size, bool).reshape(rows_img // 64, -1, 64, 16)
            meta[:, -1, :, 12:] = True
            assert mx0 == mx and np.array_equal(plain[~meta.reshape(-1)], img[~meta.reshape(-1)]), what


@pytest.mark.parametrize("with_xx", [True, False])
def test_builders_patch_rows_in_place(probe, with_xx):
    d, n, rows_img = 100, 130, 192
    stride = padded_dim(d) + 64
    old = builder_corpus(d, n)
    img0, mx0 = probe.build(with_xx, strided(old, stride), stride, n, rows_img, d)
    rng = np.random.default_rng(72)
    new = old.copy()
    touched = np.array([77, 0, 129, 64, 63, 5, 100])
    new[touched] = (rng.uniform(-1, 1, (len(touched), d)) * 3.0).astype(np.float32)
    rowlist = np.array([77, 0, rows_img, 129, 64, 0xFFFFFFF0, 63, 5, rows_img + 63, 100], np.uint32)  # (>= rows_img: ignored)
    img1, mx1 = probe.rows(with_xx, strided(new, stride), stride, rowlist, rows_img, d, img0, mx0)
    rhod, nud = check_image(img1, new, n, rows_img, d, with_xx, "rows xx %d" % with_xx)
    keep = np.setdiff1d(np.arange(n), touched)
    shape = (rows_img // 64, ref8.chunks_of(d) + 1, 64, 16)
    for before, after in zip(ref.unpack_tiles(img0.reshape(shape), n, d), ref.unpack_tiles(img1.reshape(shape), n, d)):
        assert before[keep].tobytes() == after[keep].tobytes()
    assert mx1 == max(mx0, max_norm_bits(rhod[touched], nud[touched]))


# ---- B. the pass ------------------------------------------------------------------------------------------------------------
def pass_corpus(d, n, q, seed):
    """Uniform rows with the adversarial ones of the model test among them: norms over 10^-3 .. 10^3, a zero row, the query,
    near-copies of it, 48 identical rows, spikes."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    adv = np.vstack(list(ref.adversarial(d, q, seed + 1, n_each=8 if n < 200 else 24).values()))[:n]
    at = rng.permutation(n)[:len(adv)]
    x[at] = adv
    return x


def device_image(probe, x):
    n, d = x.shape
    rows_img = (n + 63) // 64 * 64
    img, mx = probe.build(True, strided(x, padded_dim(d)), padded_dim(d), n, rows_img, d)
    return img.reshape(rows_img // 64, ref8.chunks_of(d) + 1, 64, 16), mx


def check_lists(keys, pay, first, second, rank, blocks, kp, what):
    """Block b's list is exactly the kp smallest (kmin word, id rank) keys of the rows it owns with the model's kmax word
    beside each, and every other slot is empty."""
    lo, hi, rows = ref.block_lists(first, second, rank, blocks, kp)
    lo, hi, rows = lo.reshape(blocks, kp), hi.reshape(blocks, kp), rows.reshape(blocks, kp)
    want_key = (hi.astype(np.uint64) << np.uint64(32)) | np.asarray(rank, np.uint64)[rows]
    for b in range(blocks):
        nlive = int((hi[b] != ref.EMPTY).sum())
        live = keys[b] != EMPTY_KEY
        assert live.sum() == nlive, (what, b, live.sum(), nlive)
        order = np.argsort(keys[b][live], kind="stable")
        assert np.array_equal(keys[b][live][order], want_key[b][:nlive]), (what, b, "kmin words or id ranks differ from the model's")
        assert np.array_equal(pay[b][live][:, 0][order], rows[b][:nlive]), (what, b)
        got = ref6.orderable(pay[b][live][:, 1].copy().view(np.float32))[order]
        assert np.array_equal(got, lo[b][:nlive]), (what, b, "kmax words differ from the model's")


@pytest.mark.parametrize("metric", [L2, L2SQ])
@pytest.mark.parametrize("d", DIMS)
def test_the_pass_gives_every_row_the_models_words(probe, oracle_mod, d, metric):
    rng = np.random.default_rng(300 + d + metric)
    for n in SIZES:
        q = (rng.uniform(-1, 1, d) * (3.0 if n == 64 else 1.0)).astype(np.float32)
        x = pass_corpus(d, n, q, 500 + n + d)
        img, mx = device_image(probe, x)
        X, s, rho, nu, xx = ref.unpack_tiles(img, n, d)
        qy = ref.Query(q)
        assert not ref.declines(qy.qn, float(np.array([mx], np.uint64).view(np.float64)[0]))
        first, second = ref.pass_words(metric, X, s, rho, nu, xx, qy)
        assert np.all(first <= second)
        id_rank = None if n == 63 else rng.permutation(n).astype(np.uint32)
        rank = np.arange(n) if id_rank is None else id_rank
        tiles = (n + 63) // 64
        blocks = (tiles + 3) // 4
        what = "metric %d d %d n %d" % (metric, d, n)
        keys, pay = probe.scan(img, n, d, metric, id_rank, qy, 256, blocks)   # every row retained
        check_lists(keys, pay, first, second, rank, blocks, 256, what)
        # the oracle's value inside the two words (every row of the small shapes, every ninth of the large one)
        at = np.arange(n) if n < 200 else np.arange(0, n, 9)
        word = ref6.orderable(np.array([oracle_mod.compute(metric, q, x[r]) for r in at], np.float32))
        assert np.all((first[at] <= word) & (word <= second[at])), what
    # the search's own geometry at the largest shape: lists of k' = 26 on more blocks than tiles and on fewer
    for blocks in (256, 5):
        keys, pay = probe.scan(img, n, d, metric, id_rank, qy, 26, blocks)
        check_lists(keys, pay, first, second, rank, blocks, 26, what + " blocks %d" % blocks)


# ---- C. the tail ------------------------------------------------------------------------------------------------------------
def oracle_block(oracle_mod, metric, q, x, rank, cand, k):
    """What the tail's block must deliver for these candidates: K1's value per row, keyed and sorted as K1's select does."""
    raw = np.array([oracle_mod.compute(metric, q, x[r]) for r in cand], np.float32)
    key = (ref6.orderable(raw).astype(np.uint64) << np.uint64(32)) | np.asarray(rank, np.uint64)[cand]
    order = np.argsort(key, kind="stable")[:k]
    return key[order], np.asarray(cand, np.uint32)[order], raw[order]


def run_tail(probe, oracle_mod, metric, x, q, id_rank, k, blocks, order, what, expect):
    n, d = x.shape
    img, _ = device_image(probe, x)
    qy = ref.Query(q)
    kp = ref.list_k(k)
    rank = np.arange(n) if id_rank is None else id_rank
    keys, pay = probe.scan(img, n, d, metric, id_rank, qy, kp, blocks)
    hi = np.where(keys == EMPTY_KEY, ref.EMPTY, (keys >> np.uint64(32)).astype(np.uint32)).reshape(-1)
    lo = np.where(keys == EMPTY_KEY, ref.EMPTY, ref6.orderable(pay[:, :, 1].copy().view(np.float32))).reshape(-1)
    cert = ref.certify(lo, hi, pay[:, :, 0].reshape(-1), blocks, kp, k)
    outcome = ref.tail_outcome(cert, blocks, kp, d)
    assert outcome == expect, (what, outcome, cert["cnt"])
    saved = oracle_mod.get_reduce_order()
    oracle_mod.set_reduce_order(order)
    try:
        out = probe.tail(keys, pay, k, ref.CAND_CAP, x, q, id_rank, metric, order)
        assert list(out["info"]) == [outcome, cert["cnt"], cert["kt"], 0], (what, list(out["info"]), cert["cnt"], cert["kt"])
        assert out["count"][0] == (cert["cnt"] if outcome else 0), what
        if outcome:
            assert np.array_equal(np.sort(out["rows"][:cert["cnt"]]), cert["rows"]), what
            # the certificate is sound: the oracle's k best of ALL rows are among the candidates
            allkey, allrows, _ = oracle_block(oracle_mod, metric, q, x, rank, np.arange(n), k)
            assert set(allrows.tolist()) <= set(cert["rows"].tolist()), what
        if outcome == 1:
            wkey, wrows, wraw = oracle_block(oracle_mod, metric, q, x, rank, cert["rows"], k)
            m = len(wkey)
            assert list(out["head"]) == [0, m] and out["status"][0] == 0, (what, list(out["head"]))
            assert np.array_equal(out["keys"][:m], wkey), what
            assert np.array_equal(out["res_rows"][:m], wrows), what
            assert out["raw"][:m].tobytes() == wraw.tobytes(), what
            assert np.array_equal(wkey, allkey), what  # and that is the search's answer
    finally:
        oracle_mod.set_reduce_order(saved)


def tail_corpus(rng, d, n):
    """Uniform rows around a query with the rows that decide its search among them."""
    q = rng.uniform(-1, 1, d).astype(np.float32)
    x = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    at = rng.permutation(n)[:12]
    x[at[0]] = q                                                    # c = 0 exactly
    x[at[1:7]] = (q.astype(np.float64) * (1.0 + 10.0 ** rng.uniform(-7, -3, (6, 1)) * rng.uniform(-1, 1, (6, d)))).astype(np.float32)
    x[at[7]] = 0.0
    x[at[8:10]] = x[at[8:10]] * np.float32(1e-3)
    x[at[10], d // 2] = np.float32(300.0)                           # a spike
    x[at[11]] = x[at[1]]                                            # a tie decided by the id rank
    return q, x


def long_corpora(metric):
    """(query, 300 copies of one near row thirty rows apart, 48 copies of it side by side) over 9 001 uniform rows."""
    d, n = 100, 9001
    rng = np.random.default_rng(77 + metric)
    q = rng.uniform(-1, 1, d).astype(np.float32)
    x = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    near = (q + rng.uniform(-1, 1, d) * 0.01).astype(np.float32)
    spread = x.copy()
    spread[np.arange(300) * 30] = near
    packed = x.copy()
    packed[4000:4048] = near
    return q, spread, packed


@pytest.mark.parametrize("metric", [L2, L2SQ])
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("d", DIMS)
def test_the_tail_rescores_what_the_oracle_computes(probe, oracle_mod, d, k, metric):
    rng = np.random.default_rng(40 + d + k + metric)
    for n in SIZES:
        order = oracle_mod.ORDERS[(n + k) % 4]
        q, x = tail_corpus(rng, d, n)
        id_rank = None if n == 64 else rng.permutation(n).astype(np.uint32)
        blocks = 1 if n < 200 else 40
        # one block over at most 65 rows: a list of k' >= 17 slots none of which may be all candidates
        run_tail(probe, oracle_mod, metric, x, q, id_rank, k, blocks, order, "d %d k %d n %d order %d" % (d, k, n, order), 1)


@pytest.mark.parametrize("metric", [L2, L2SQ])
def test_the_tail_leaves_long_lists_and_refuses_full_ones(probe, oracle_mod, metric):
    k = 10
    q, spread, packed = long_corpora(metric)
    # 300 copies spread thirty rows apart: more candidates than the block rescores, no list full of them
    run_tail(probe, oracle_mod, metric, spread, q, None, k, 36, 3, "spread", 2)
    # 48 copies side by side: one block's list of k' = 26 holds candidates alone
    run_tail(probe, oracle_mod, metric, packed, q, None, k, 36, 3, "packed", 0)
