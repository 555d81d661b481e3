"""The sketch kernels against their numpy models, row by row (the third link of the certificate).

The model tests (test_sketch8_model.py, test_sketch6_split_model.py, test_sketch5_model.py) show on the CPU that the
model's interval holds the oracle's dot; test_gpu_sketch*.py show that a search's hits are the oracle's.  Here the kernels
themselves are launched through tests/sketch_probe.cpp (libvt_sketch_probe.so: vt_sketch.hip, vt_sketch_nibble.hip and
nothing else of the library) and what no search returns is read back:

  A  the builders' images, byte for byte against pack_tiles, and rho / nu against the exact norms;
  B  the passes' lists and word arrays: every row's two words equal the model's (sketch*_ref.pass_words) bit for bit and hold
     the oracle's f32 rank value, on one block per tile (every row read out) and on one block walking ten tiles;
  C  the spread certification (sketch_thresh_kernel, sketch_collect_kernel) on synthetic word arrays: Kt, the candidates,
     the count, the full-list refusal, and the state two calls share.

Geometry of B.  The 5-bit pass numbers its waves across the blocks first, so with blocks = tiles block b owns tile b alone
and a list of 64 holds all its rows.  The 4-bit pass numbers them likewise (wave = wave-in-block * blocks + block) and
leaves two lists a block, waves 0-1 and waves 2-3: tile t goes to wave w = t mod 4 blocks, which is wave-in-block
w div blocks of block w mod blocks; with blocks = tiles every tile has the first list of its block to itself and the second
lists stay empty.  The int8 pass numbers them block by block: with blocks = tiles / 4 and lists of 256
block b owns tiles 4 b .. 4 b + 3.  The 6-bit pass numbers them block by block too but takes lists of at most 64, so no
launch over several tiles returns every row: it is launched once per tile, on that tile's slice of the image, and meets
several tiles per wave in the ring tests.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import sketch4_ref as ref4
import sketch5_ref as ref5
import sketch6_ref as ref6
import sketch6_split_ref as split6
import sketch8_ref as ref8
from test_sketch5_model import corpora, unit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (8, 6, 5, 4)
NIBBLE_WIDTHS = (6, 5, 4)
HALF = {8: 127, 6: 31, 5: 15, 4: 7}
MODEL = {8: ref8, 6: ref6, 5: ref5, 4: ref4}
COS, IP, NIP = ref6.M_COS, ref6.M_IP, ref6.M_NIP
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
EMPTY = np.uint32(0xFFFFFFFF)
HIP_INVALID_VALUE = 1
UP = ref6.UP


# ---- the probe ----------------------------------------------------------------------------------------------------------
class Probe:
    def __init__(self):
        # VT_SKETCH_PROBE_LIB: another build of the same probe (a deliberately broken kernel, to see these tests fail)
        path = os.environ.get("VT_SKETCH_PROBE_LIB") or os.path.join(ROOT, "vettore_amd", "lib", "libvt_sketch_probe.so")
        assert os.path.exists(path), "build it with `make` (%s)" % os.path.basename(path)
        L = self.lib = C.CDLL(path)
        u8p, u32p, u64p, f32p = C.POINTER(C.c_ubyte), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
        L.vtp_image_bytes.restype = C.c_size_t
        L.vtp_image_bytes.argtypes = [C.c_int, C.c_uint32, C.c_uint32]
        L.vtp_thresh_blocks.restype = C.c_uint32
        L.vtp_thresh_blocks.argtypes = [C.c_uint32, C.c_uint32]
        L.vtp_block_lists.restype = C.c_uint32
        L.vtp_block_lists.argtypes = [C.c_int]
        assert [L.vtp_block_lists(w) for w in WIDTHS] == [1, 1, 1, 2]
        L.vtp_build.argtypes = [C.c_int, f32p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, u8p, C.c_size_t, u64p]
        L.vtp_rows.argtypes = [C.c_int, f32p, C.c_size_t, C.c_size_t, u32p, C.c_uint32, C.c_uint32, C.c_uint32, u8p, C.c_size_t, u64p]
        L.vtp_scan.argtypes = [C.c_int, u8p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int, u32p, u8p, C.c_size_t, f32p,
                               C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_uint32, u64p, u32p, u32p, u32p]
        L.vtp_certify.argtypes = [u32p, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u32p, C.c_uint32,
                                  u32p, u32p, u32p, u32p, u32p, u32p]
        L.vtp_level_words.restype = C.c_uint32
        L.vtp_level_words.argtypes = [C.c_uint32]
        L.vtp_query_levels.restype = None
        L.vtp_query_levels.argtypes = [f32p, C.c_uint32, u32p, C.POINTER(C.c_double), f32p, C.POINTER(C.c_double)]
        L.vtp_level_sums.restype = None
        L.vtp_level_sums.argtypes = [u32p, C.c_uint32] + [C.POINTER(C.c_longlong)] * 3
        L.vtp_level_bound5.restype = None
        L.vtp_level_bound5.argtypes = [u32p, C.c_uint32, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_double)]

    @staticmethod
    def _p(a, ctype):
        return a.ctypes.data_as(C.POINTER(ctype))

    def build(self, width, xbuf, stride, n_src, rows_img, d, expect=0):
        img = np.zeros(self.lib.vtp_image_bytes(width, rows_img, d), np.uint8)
        mx = np.zeros(1, np.uint64)
        rc = self.lib.vtp_build(width, self._p(xbuf, C.c_float), xbuf.size, stride, n_src, rows_img, d, self._p(img, C.c_ubyte),
                                img.size, self._p(mx, C.c_uint64))
        assert rc == expect, "vtp_build: hipError_t %d" % rc
        return img, int(mx[0])

    def rows(self, width, xbuf, stride, rowlist, rows_img, d, img, max_norm):
        img = img.copy()
        mx = np.array([max_norm], np.uint64)
        rowlist = np.ascontiguousarray(rowlist, np.uint32)
        rc = self.lib.vtp_rows(width, self._p(xbuf, C.c_float), xbuf.size, stride, self._p(rowlist, C.c_uint32), rowlist.size,
                               rows_img, d, self._p(img, C.c_ubyte), img.size, self._p(mx, C.c_uint64))
        assert rc == 0, "vtp_rows: hipError_t %d" % rc
        return img, int(mx[0])

    def scan(self, width, img, n, d, metric, id_rank, qimg, t, qn, eta, kerr, c3, w3, k, blocks, expect=0):
        img = np.ascontiguousarray(img, np.uint8).reshape(-1)
        qimg = np.ascontiguousarray(qimg).view(np.uint8).reshape(-1)
        t = np.ascontiguousarray(t, np.float32)
        lists = blocks * self.lib.vtp_block_lists(width)
        keys = np.zeros((lists, k), np.uint64)
        pay = np.zeros((lists, k, 2), np.uint32)
        lo, hi = np.zeros((lists, k), np.uint32), np.zeros((lists, k), np.uint32)
        rank = None if id_rank is None else np.ascontiguousarray(id_rank, np.uint32)
        rc = self.lib.vtp_scan(width, self._p(img, C.c_ubyte), img.size, n, d, metric,
                               None if rank is None else self._p(rank, C.c_uint32), self._p(qimg, C.c_ubyte), qimg.size,
                               self._p(t, C.c_float), qn, eta, kerr, c3, w3, k, blocks, self._p(keys, C.c_uint64),
                               self._p(pay, C.c_uint32), self._p(lo, C.c_uint32), self._p(hi, C.c_uint32))
        assert rc == expect, "vtp_scan: hipError_t %d" % rc
        return keys, pay, lo, hi

    def certify(self, lo, hi, rows, lists, kp, k, cap, prefill, runs=2, expect=0):
        lo, hi = np.ascontiguousarray(lo, np.uint32), np.ascontiguousarray(hi, np.uint32)
        pay = np.zeros((lists * kp, 2), np.uint32)
        pay[:, 0] = rows
        pay[:, 1] = 0x7FC00000  # (the payload's float is not read)
        tb = self.lib.vtp_thresh_blocks(lists, kp)
        out = dict(parts=np.zeros((runs, tb, k), np.uint32), live=np.zeros((runs, tb), np.uint32),
                   rows=np.zeros((runs, cap), np.uint32), count=np.zeros(runs, np.uint32), info=np.zeros((runs, 4), np.uint32),
                   sync=np.zeros((runs, 4), np.uint32))
        prefill = np.ascontiguousarray(prefill, np.uint32)
        assert prefill.size == 4
        rc = self.lib.vtp_certify(self._p(lo, C.c_uint32), self._p(hi, C.c_uint32), self._p(pay, C.c_uint32), lists, kp, k, cap,
                                  self._p(prefill, C.c_uint32), runs, *(self._p(out[f], C.c_uint32)
                                                                       for f in ("parts", "live", "rows", "count", "info", "sync")))
        assert rc == expect, "vtp_certify: hipError_t %d" % rc
        return out


@pytest.fixture(scope="module")
def probe():
    return Probe()


# ---- one interface over the four models ----------------------------------------------------------------------------------
def quantise(width, x):
    return MODEL[width].quantise_rows(x)


def pack(width, X, s, rho, nu):
    return MODEL[width].pack_tiles(X, s, rho, nu).view(np.uint8).reshape(-1)


def runs_of(width, d):
    return ref8.chunks_of(d) + 1 if width == 8 else MODEL[width].runs_of(d)


def unpack(width, img, n, d):
    tiles = img.size // (runs_of(width, d) * 1024)
    if width == 8:
        return ref8.unpack_tiles(img.reshape(tiles, -1, 64, 16), n, d)
    shaped = img.view(np.uint32).reshape(tiles, -1, 64, 4)
    return MODEL[width].unpack_tiles(shaped, n, d)


def query_levels(width, q):
    return ref8.query_levels(q) if width == 8 else ref6.query_levels(q)


def nibble_image(Q, d):
    """[levels][ld8 / 8] dwords: nibble i of dword g is element 8 g + i (host/vt_sketch6.h)."""
    img = np.zeros((len(Q), ref6.ld8_of(d) // 8), np.uint32)
    for i in range(d):
        img[:, i >> 3] |= ((Q[:, i] & 0xF) << (4 * (i & 7))).astype(np.uint32)
    return img


def query_image(width, Q, d):
    return ref8.query_image(Q, d) if width == 8 else nibble_image(np.asarray(Q, np.int64), d)


def level_bound(width, Q, t):
    if width in (8, 4):  # (no level kept off a plane)
        return 0.0, 0.0
    return (split6 if width == 6 else ref5).level_bound(Q[2], t[2])


def pass_words(width, metric, X, s, rho, nu, Q, t, qn, eta, kerr, c3, w3):
    if width == 8:
        return ref8.pass_words(metric, X, s, rho, nu, Q, t, qn, eta, kerr)
    return {6: split6, 5: ref5, 4: ref4}[width].pass_words(metric, X, s, rho, nu, Q, t, qn, eta, kerr, c3, w3)


def padded_dim(d):
    return (d + 63) // 64 * 64


def strided(x, stride):
    buf = np.zeros(max(1, len(x)) * stride, np.float32)
    buf.reshape(-1, stride)[:len(x), :x.shape[1]] = x
    return buf


def edge_rows(d, half, seed=0):
    """The rows a quantiser goes wrong on, nine of them (at small d some coincide)."""
    rng = np.random.default_rng(900 + d + seed)
    rows = []
    z = np.zeros(d, np.float32)
    z[::2] = -0.0
    rows.append(z)                                                                # all zero, with -0.0 entries
    rows.append((rng.integers(-90, 91, d) * 1e-40).astype(np.float32))           # subnormals: half / m is infinite
    rows[-1][rng.integers(0, d)] = np.float32(9e-39)
    big = (rng.uniform(-1, 1, d) * 1e30).astype(np.float32)
    big[rng.integers(0, d)] = np.float32(-3e38)                                   # m near the largest f32
    rows.append(big)
    rows.append(rng.uniform(-1.0, -0.125, d).astype(np.float32))                  # the row's maximum is negative
    rows.append(rng.choice(np.array([-0.37, 0.37], np.float32), d))               # +-m only
    rows.append(np.full(d, -1.0, np.float32))
    for sign in (1, -1):                                                          # x / s = K + 0.5 exactly: rintf meets ties
        K = rng.integers(-half, half, d)
        x = (K + 0.5) * 2.0 ** -9 * sign
        x[rng.integers(0, d)] = half * 2.0 ** -9
        rows.append(x.astype(np.float32))
        assert np.array_equal(rows[-1].astype(np.float64), x)
    hot = np.zeros(d, np.float32)
    hot[d // 3] = 2.5
    rows.append(hot)
    return np.stack(rows)


def next_f32_above(v):
    """The least f32 greater than the f64 v, element-wise."""
    f = ref6.f32_up_v(v)
    return np.where(f.astype(np.float64) > np.asarray(v, np.float64), f, np.nextafter(f, np.float32(np.inf))).astype(np.float32)


def exact_norms(x, X, s):
    """||x - s X|| and s ||X|| per row: the residual is exact in f64, its squares are summed exactly (fsum)."""
    s64 = s.astype(np.float64)
    r = x.astype(np.float64) - s64[:, None] * X
    R = np.array([math.sqrt(math.fsum((r[i] * r[i]).tolist())) for i in range(len(x))])
    N = s64 * np.sqrt((X.astype(np.int64) ** 2).sum(axis=1).astype(np.float64))
    return R, N


def assert_band(dev, exact, what):
    """exact (1 + 2^-31) <= dev <= the f32 above exact (1 + 2^-29): the kernel applies 1 + 2^-30 to f64 sums that carry at most
    d 2^-53 <= 2^-38 relative error and then rounds up by less than one f32 step.  Rounding to nearest, or no margin, falls
    below the lower bound on about half the rows."""
    dev64 = dev.astype(np.float64)
    low = exact * (1.0 + 2.0 ** -31)
    high = next_f32_above(exact * (1.0 + 2.0 ** -29)).astype(np.float64)
    bad = np.nonzero(~((low <= dev64) & (dev64 <= high)))[0]
    assert bad.size == 0, (what, bad[:5], dev64[bad[:5]], exact[bad[:5]])


def check_image(width, img, x, n_src, rows_img, d, what):
    """The image of rows_img rows equals the model's of x[:n_src] byte for byte, rho and nu apart, which lie in the band."""
    Xm, sm, _, _ = quantise(width, x[:n_src])
    assert img.size == runs_of(width, d) * 1024 * rows_img // 64
    Xd, sd, rhod, nud = unpack(width, img, n_src, d)
    assert np.array_equal(Xd, Xm), what
    assert np.array_equal(sd.view(np.uint32), sm.view(np.uint32)), what
    R, N = exact_norms(x[:n_src], Xm, sm)
    assert_band(rhod, R, what + " rho")
    assert_band(nud, N, what + " nu")
    # everything else: the planes' padding columns, the rows at or past n_src (zero rows, zero metadata), the fourth
    # metadata word, and no byte of the 0xA5 fill left -- the model's image with the device's rho and nu is the image
    want = np.zeros(img.size, np.uint8)
    model = pack(width, Xm, sm, rhod, nud)
    want[:model.size] = model
    assert np.array_equal(img, want), (what, np.nonzero(img != want)[0][:8])
    return rhod, nud


def max_norm_bits(rho, nu):
    bound = (rho.astype(np.float64) + nu.astype(np.float64)) * ref6.SLACK
    return int(np.array([bound.max() if len(bound) else 0.0], np.float64).view(np.uint64)[0])


# ---- A. the builders -------------------------------------------------------------------------------------------------------
def builder_corpus(d, half, n):
    rng = np.random.default_rng(7000 + d)
    x = (rng.uniform(-1, 1, (n, d)) * rng.uniform(0.01, 30, (n, 1))).astype(np.float32)
    e = edge_rows(d, half)
    at = np.arange(len(e)) * 7 % n if n >= 64 else np.arange(min(n, len(e)))
    x[at] = e[:len(at)]
    return x


@pytest.mark.parametrize("d", [1, 7, 128, 129, 200, 256, 320, 768, 8320])
@pytest.mark.parametrize("width", WIDTHS)
def test_builders_write_the_models_image(probe, width, d):
    """d = 8320: nch = 520, nl = 130 and 65 and the 4-bit sketch's nh = 260 are all over 64, so a lane takes a second turn of
    the per-row loop at every width (a fifth at four bits)."""
    full = builder_corpus(d, HALF[width], 130)
    shapes = [(1, 64, 0), (63, 64, 64), (64, 64, 0), (65, 128, 0), (130, 192, 64), (65, 192, 0)]  # (the last: an empty tile beyond)
    if d == 8320:
        shapes = [(65, 128, 0), (130, 192, 64)]
    for n_src, rows_img, extra in shapes:
        # (the smaller corpora: the edge rows first, all nine of them where n_src allows)
        x = full[:n_src] if n_src == 130 else np.concatenate([edge_rows(d, HALF[width]), full])[:n_src]
        stride = padded_dim(d) + extra
        what = "width %d d %d n_src %d rows_img %d stride %d" % (width, d, n_src, rows_img, stride)
        img, mx = probe.build(width, strided(x, stride), stride, n_src, rows_img, d)
        rhod, nud = check_image(width, img, x, n_src, rows_img, d, what)
        assert mx == max_norm_bits(rhod, nud), what


@pytest.mark.parametrize("width", WIDTHS)
def test_builders_edge_rows_quantise_as_the_model_says(probe, width):
    """What the model gives the edge rows is what this test means them to meet (so that a change of the model is noticed)."""
    d, half = 200, HALF[width]
    x = edge_rows(d, half)
    X, s, rho, nu = quantise(width, x)
    assert s[0] == 0 and not X[0].any() and rho[0] == 0 and nu[0] == 0                     # the zero row
    assert s[1] == 0 and not X[1].any() and rho[1] > 0 and nu[1] == 0                      # subnormals: nothing quantised
    assert abs(float(rho[1]) / math.sqrt(math.fsum((x[1].astype(np.float64) ** 2).tolist())) - 1) < 1e-3
    assert np.abs(X[2]).max() == half and np.count_nonzero(X[2]) == 1                      # the huge row
    assert X[3].max() < 0 and X[3].min() == -half
    assert set(np.unique(X[4])) == {-half, half} and set(np.unique(X[5])) == {-half}
    for i in (6, 7):                                                                        # ties go to the even integer
        v = x[i].astype(np.float64) * 2.0 ** 9
        ties = v != np.rint(v)
        assert ties.sum() >= d - 1 and not (X[i][ties] & 1).any()
    assert np.count_nonzero(X[8]) == 1 and rho[8] < 1e-6
    img, _ = probe.build(width, strided(x, padded_dim(d)), padded_dim(d), len(x), 64, d)
    check_image(width, img, x, len(x), 64, d, "edge rows, width %d" % width)


@pytest.mark.parametrize("d", [129, 320, 8320])
@pytest.mark.parametrize("width", WIDTHS)
def test_builders_patch_rows_in_place(probe, width, d):
    n, rows_img, stride = 130, 192, padded_dim(d) + 64
    old = builder_corpus(d, HALF[width], n)
    img0, mx0 = probe.build(width, strided(old, stride), stride, n, rows_img, d)
    rng = np.random.default_rng(71 + d)
    new = old.copy()
    touched = np.array([77, 0, 129, 64, 63, 5, 100])
    new[touched] = (rng.uniform(-1, 1, (len(touched), d)) * 3.0).astype(np.float32)
    new[5] = edge_rows(d, HALF[width])[6]
    rowlist = np.array([77, 0, rows_img, 129, 64, 0xFFFFFFF0, 63, 5, rows_img + 63, 100], np.uint32)  # (>= rows_img: ignored)
    img1, mx1 = probe.rows(width, strided(new, stride), stride, rowlist, rows_img, d, img0, mx0)
    what = "rows, width %d d %d" % (width, d)
    rhod, nud = check_image(width, img1, new, n, rows_img, d, what)
    # rows not in the list: byte for byte what they were (check_image allows their rho and nu a band; here they may not move)
    keep = np.setdiff1d(np.arange(n), touched)
    for before, after in zip(unpack(width, img0, n, d), unpack(width, img1, n, d)):
        assert before[keep].tobytes() == after[keep].tobytes(), what
    # max_norm only ever rises: the old bound, or a patched row's
    assert mx1 == max(mx0, max_norm_bits(rhod[touched], nud[touched])), what


# ---- B. the passes ---------------------------------------------------------------------------------------------------------
def owner_list(width, tile, blocks):
    """The list a tile's rows go to: waves = 4 blocks, tile t goes to wave t mod waves; the 5-bit and 4-bit passes number
    their waves across the blocks first (wave = wave-in-block * blocks + block), the other two block by block; the 4-bit
    pass leaves two lists a block, one per pair of waves."""
    w = tile % (4 * blocks)
    if width == 4:
        return 2 * (w % blocks) + (w // blocks) // 2
    return w % blocks if width == 5 else w // 4


class Query:
    """A query as a pass takes it: the integer levels, their scales and the bounds the host computes beside them."""

    def __init__(self, width, q, arbitrary=None):
        self.q = np.asarray(q, np.float32)
        d = len(self.q)
        Q, t, eta_v = query_levels(width, self.q)
        if arbitrary is not None:
            # any integers in range and any positive scales: the bound holds as long as eta is formed from them
            top = 127 if width == 8 else 7
            Q = np.clip(Q + arbitrary.integers(-1, 2, Q.shape), -top, top)
            t = (np.maximum(t, np.float32(2.0 ** -20)) * arbitrary.uniform(0.9, 1.1, t.shape)).astype(np.float32)
            eta_v = self.q.astype(np.float64) - sum(np.float64(t[j]) * Q[j] for j in range(len(t)))
        self.Q, self.t = Q, t
        self.qn = math.sqrt(math.fsum((self.q.astype(np.float64) ** 2).tolist())) * UP
        self.eta = math.sqrt(math.fsum((eta_v ** 2).tolist())) * UP
        self.kerr = 8.0 * d * 2.0 ** -24
        self.c3, self.w3 = level_bound(width, Q, t)
        self.image = query_image(width, Q, d)


def rank_words(oracle_mod, metric, q, x):
    """The orderable word of K1's f32 rank value per row: the oracle's dot, then its rank function (both dot metrics rank by
    minus the dot, cosine by one minus it)."""
    out = np.zeros(len(x), np.float32)
    for i, row in enumerate(x):
        dot = oracle_mod.compute(IP, q, row)
        out[i] = oracle_mod.rank_value(COS, dot) if metric == COS else oracle_mod.rank_value(IP, dot)
    return ref6.orderable(out)


def model_words(width, metric, img, n, d, qy):
    X, s, rho, nu = unpack(width, img, n, d)
    first, second = pass_words(width, metric, X, s, rho, nu, qy.Q, qy.t, qy.qn, qy.eta, qy.kerr, qy.c3, qy.w3)
    assert np.all(first <= second)
    return first, second, (rho.astype(np.float64) + nu.astype(np.float64))


def run_scan(probe, width, img, n, d, metric, id_rank, qy, k, blocks):
    """One launch; the lists checked slot by slot against the model: list b is exactly the k smallest
    (key(hi) word, id rank) keys of the rows it owns, with both model words, and every other slot is empty.
    Returns {row: (first word, second word)} as the device has them."""
    first, second, _ = model_words(width, metric, img, n, d, qy)
    rank = np.arange(n, dtype=np.uint64) if id_rank is None else id_rank.astype(np.uint64)
    key = (first.astype(np.uint64) << np.uint64(32)) | rank
    keys, pay, lo, hi = probe.scan(width, img, n, d, metric, id_rank, qy.image, qy.t, qy.qn, qy.eta, qy.kerr, qy.c3, qy.w3, k, blocks)
    owner = np.array([owner_list(width, r // 64, blocks) for r in range(n)])
    seen = {}
    for b in range(len(keys)):
        mine = np.nonzero(owner == b)[0]
        want = mine[np.argsort(key[mine], kind="stable")][:k]
        live = keys[b] != EMPTY_KEY
        assert live.sum() == len(want), (b, live.sum(), len(want))
        if width != 8:
            assert np.all(lo[b][~live] == EMPTY) and np.all(hi[b][~live] == EMPTY), b
            assert np.array_equal(hi[b][live], (keys[b][live] >> np.uint64(32)).astype(np.uint32)), b
            assert np.array_equal(lo[b][live], ref6.orderable(pay[b][live][:, 1].copy().view(np.float32))), b
        got_rows = pay[b][live][:, 0]
        order = np.argsort(keys[b][live], kind="stable")
        assert np.array_equal(got_rows[order], want), (b, got_rows[order][:8], want[:8])
        assert np.array_equal(keys[b][live][order], key[want]), (b, "key(hi) words or id ranks differ from the model's")
        got_second = ref6.orderable(pay[b][live][:, 1].copy().view(np.float32))[order]
        assert np.array_equal(got_second, second[want]), (b, "key(lo) words differ from the model's")
        for r, f2, s2 in zip(want, (keys[b][live][order] >> np.uint64(32)).astype(np.uint32), got_second):
            assert int(r) not in seen
            seen[int(r)] = (int(f2), int(s2))
    return seen


def read_every_row(probe, width, img, n, d, metric, id_rank, qy):
    """Geometry G1 (the module's docstring): every row's two words as the device has them."""
    tiles = (n + 63) // 64
    if width in (5, 4):
        seen = run_scan(probe, width, img, n, d, metric, id_rank, qy, 64, tiles)
    elif width == 8:
        seen = run_scan(probe, 8, img, n, d, metric, id_rank, qy, 256, (tiles + 3) // 4)
    else:
        seen, per = {}, img.size // tiles
        for t in range(tiles):
            rows = min(64, n - 64 * t)
            part = run_scan(probe, 6, img[t * per:(t + 1) * per], rows, d, metric,
                            None if id_rank is None else id_rank[64 * t:64 * t + rows], qy, 64, 1)
            seen.update({64 * t + r: w for r, w in part.items()})
    assert sorted(seen) == list(range(n))  # every row below n once, none at or past n
    return seen


def assert_sound(oracle_mod, seen, metric, qy, x, norms, what, exempt=()):
    """K1's rank value lies inside every row's two words under f32's total order -- for every row the premise of the bound
    covers: sketch_search declines a corpus on which ||q|| (rho + nu) could reach 2^126 (K1's overflow flag is K1's to
    raise), which here is the one row with an element near the largest f32."""
    covered = qy.qn * norms * ref6.SLACK * UP < 2.0 ** 126
    assert sorted(np.nonzero(~covered)[0]) == sorted(exempt), (what, np.nonzero(~covered)[0])
    at = np.nonzero(covered)[0]
    for r, word in zip(at, rank_words(oracle_mod, metric, qy.q, x[at])):
        assert seen[r][0] <= int(word) <= seen[r][1], (what, r, seen[r], int(word))


def lean_rows(q, half, count, rng, scale):
    """Rows whose rounding residual is parallel to the query: x = scale (K + 0.49 sign(q) sigma) / half, one element exactly
    `scale` (so s = scale / half and X = K): q . (x - s X) is then 0.49 s ||q||_1, most of e_r's leading term ||q|| rho_r."""
    d = len(q)
    K = rng.integers(-(half - 1), half, (count, d)).astype(np.float64)
    sigma = np.where(np.arange(count) % 2 == 0, 1.0, -1.0)[:, None]
    x = scale * (K + 0.49 * np.sign(q.astype(np.float64)) * sigma) / half
    x[np.arange(count), rng.integers(0, d, count)] = scale
    return x.astype(np.float32)


def adversarial5(q, n, seed, mirror, scale=2.0 ** -9):
    """sketch6_split_ref.adversarial_rows for the one-bit plane: L = X mod 2 is 1 exactly where Q3 > 0 and 0 where Q3 < 0 (or
    the mirror image), so that Q3.L sits at an end of [N3, P3]."""
    q = np.asarray(q, np.float32)
    d = len(q)
    Q3 = ref6.query_levels(q)[0][2]
    rng = np.random.default_rng(seed)
    up, down = (Q3 < 0, Q3 > 0) if mirror else (Q3 > 0, Q3 < 0)
    L = rng.integers(0, 2, (n, d))
    L[:, up] = 1
    L[:, down] = 0
    X = 2 * rng.integers(-7, 8, (n, d)) + L
    pin = np.nonzero(~down)[0]
    assert pin.size
    X[np.arange(n), pin[rng.integers(0, pin.size, n)]] = 15
    assert np.abs(X).max() == 15
    return (X * scale).astype(np.float32)


def pass_corpus(width, d, metric, q):
    """The four corpora of the model tests, the builders' edge rows, the rows that lean on the bound and, for the passes that
    keep level 3 off the L plane, the rows that put its share at either end of its range: 233 rows, four tiles."""
    rng = np.random.default_rng(4000 + 10 * d + width)
    parts = [c[:40] for c in corpora(d, n=40, seed=width).values()]
    if metric != COS:  # rows of any length
        parts = [(p * rng.uniform(0.05, 24, (len(p), 1)).astype(np.float32)).astype(np.float32) for p in parts]
    parts.append(edge_rows(d, HALF[width]))
    lean_at = sum(len(p) for p in parts)
    parts.append(lean_rows(q, HALF[width], 32, rng, 1.7 / math.sqrt(d) if metric == COS else 3.0))
    if width == 6:
        parts += [split6.adversarial_rows(q, 16, 3 * d, False)[0], split6.adversarial_rows(q, 16, 3 * d + 1, True)[0]]
    elif width == 5:
        parts += [adversarial5(q, 16, 3 * d, False), adversarial5(q, 16, 3 * d + 1, True)]
    x = np.concatenate(parts)
    huge = 4 * 40 + 2  # (edge_rows' third row)
    assert np.abs(x[huge]).max() > 1e38
    return x, huge, slice(lean_at, lean_at + 32)


PASS_DIMS = {8: (7, 128, 129, 200, 256, 320, 768), 6: (129, 200, 256, 320, 768), 5: (129, 200, 256, 320, 768),
             4: (129, 200, 256, 320, 768)}
PASS_CASES = [(w, d) for w in WIDTHS for d in PASS_DIMS[w]]
# the share of e_r the leaning rows must use on the model (it prints 0.82-0.88 for the int8 sketch, 0.83-0.87 for the two
# 6- and 5-bit sketches, 0.85-0.89 for the 4-bit one)
LEAN_FLOOR = 0.8


@pytest.mark.parametrize("width,d", PASS_CASES)
def test_passes_give_every_row_the_models_interval(probe, oracle_mod, width, d):
    """G1 on images packed by numpy from the model: each row's words equal the model's bit for bit (run_scan) and hold K1's
    rank value (assert_sound), for the three metrics, id ranks absent and permuted, the host's own levels and arbitrary ones.
    The leaning rows use at least LEAN_FLOOR of e_r on the model (printed), so a bound narrowed by a few percent is seen."""
    rng = np.random.default_rng(600 + d + width)
    q_unit = unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0]
    for metric in (COS, IP, NIP):
        q = q_unit if metric == COS else (q_unit * np.float32(7.5)).astype(np.float32)
        x, huge, lean = pass_corpus(width, d, metric, q)
        n = len(x)
        X, s, rho, nu = quantise(width, x)
        img = pack(width, X, s, rho, nu)
        perm = rng.permutation(n).astype(np.uint32)
        hot = np.zeros(d, np.float32)
        hot[d // 3] = -0.75
        plans = [(Query(width, q), None), (Query(width, q, arbitrary=rng), perm), (Query(width, hot), perm),
                 (Query(width, (-x[7]).astype(np.float32)), None)]
        for i, (qy, id_rank) in enumerate(plans):
            what = "width %d d %d metric %d query %d" % (width, d, metric, i)
            seen = read_every_row(probe, width, img, n, d, metric, id_rank, qy)
            assert_sound(oracle_mod, seen, metric, qy, x, rho.astype(np.float64) + nu.astype(np.float64), what, exempt=[huge])
        # the leaning rows keep their teeth: on the model, |dot - a| reaches most of e
        qy = plans[0][0]
        first, second, _ = model_words(width, metric, img, n, d, qy)
        model = {8: ref8, 6: split6, 5: ref5, 4: ref4}[width]
        a, e = model.intervals(X, s, rho, nu, q)
        dots = np.array([oracle_mod.compute(IP, q, row) for row in x[lean]], np.float64)
        used = (np.abs(dots - a[lean]) / e[lean]).max()
        print("width %d d %d metric %d: the leaning rows use %.4f of e_r" % (width, d, metric, used))
        assert used >= LEAN_FLOOR, (width, d, metric, used)


@pytest.mark.parametrize("width", WIDTHS)
def test_passes_on_the_images_the_builders_wrote(probe, oracle_mod, width):
    """G1 once more per width with nothing of the model between the two kernels: the device-built image, read as it is."""
    d = 200
    rng = np.random.default_rng(650 + width)
    q = (unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0] * np.float32(2.5)).astype(np.float32)
    x, huge, _ = pass_corpus(width, d, IP, q)
    n = len(x)
    img, _ = probe.build(width, strided(x, padded_dim(d)), padded_dim(d), n, (n + 63) // 64 * 64, d)
    _, _, rho, nu = unpack(width, img, n, d)
    for metric in (COS, IP):
        qy = Query(width, q)
        seen = read_every_row(probe, width, img, n, d, metric, rng.permutation(n).astype(np.uint32), qy)
        assert_sound(oracle_mod, seen, metric, qy, x, rho.astype(np.float64) + nu.astype(np.float64),
                     "device-built, width %d metric %d" % (width, metric), exempt=[huge])


def ring_mid(width):
    """A row of a second-turn tile: tile 5 (wave 1); at four bits tile 6, wave 2's, so that the block's second list meets one."""
    return 64 * (6 if width == 4 else 5) + 9


def ring_corpus(width, d):
    n = 64 * 9 + 5
    rng = np.random.default_rng(8800 + d + width)
    x = unit(rng.uniform(-1, 1, (n, d)).astype(np.float32))
    e = edge_rows(d, HALF[width], seed=1)
    x[np.arange(len(e)) * 67 % n] = e
    x[[3, ring_mid(width), n - 2]] = unit(rng.uniform(-1, 1, (3, d)).astype(np.float32))
    return x


RING_CASES = [(8, 7), (8, 129), (8, 320), (6, 129), (6, 320), (5, 129), (5, 320), (4, 129), (4, 200), (4, 256), (4, 320), (4, 768)]


@pytest.mark.parametrize("width,d", RING_CASES)
def test_passes_walk_from_tile_to_tile(probe, width, d):
    """G2: one block, ten tiles (the four waves own 3, 3, 2, 2 of them, the last tile partial), lists of 64: every wave walks
    from a tile into the next through its load ring, its parked sums and its metadata run.  Runs per tile: int8 9, 17 and 25,
    6-bit 13 and 19, 5-bit 11 and -- a multiple of the ring of 8 -- 16 at d = 320, 4-bit 9, 9, 9, 13 and 25.  The list must be
    exactly the model's 64 smallest keys with the model's words (run_scan); the 4-bit pass leaves two, of waves 0-1's rows and
    of waves 2-3's.  The queries put a retained row in a tile of each turn: a row of the
    first tile, of a second-turn tile, of the last, partial tile, and minus a query.  Then three blocks over the same image:
    each owns more than 64 rows and returns its own 64 smallest."""
    assert runs_of(width, d) % 8 != 0 or (width, d) == (5, 320)
    x = ring_corpus(width, d)
    n = len(x)
    img = pack(width, *quantise(width, x))
    rng = np.random.default_rng(d + width)
    perm = rng.permutation(n).astype(np.uint32)
    lists, mid = probe.lib.vtp_block_lists(width), ring_mid(width)
    for i, q in enumerate((x[3], x[mid], x[n - 2], -x[3], unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0])):
        qy = Query(width, q, arbitrary=rng if i == 4 else None)
        for metric, id_rank in ((COS, None), (IP, perm)) if i < 3 else ((NIP, perm),):
            seen = run_scan(probe, width, img, n, d, metric, id_rank, qy, 64, 1)
            assert len(seen) == lists * 64
            if i < 3:  # (the query's own row, in the first, a second-turn and the last tile, is among the retained)
                assert (3, mid, n - 2)[i] in seen, (i, metric)
    qy = Query(width, x[mid])
    seen = run_scan(probe, width, img, n, d, COS, perm, qy, 64, 3)
    assert len(seen) == 3 * lists * 64


@pytest.mark.parametrize("width", NIBBLE_WIDTHS)
def test_passes_refuse_a_tile_shorter_than_the_ring(probe, width):
    """ld8 = 128: a tile of at most 7 runs, so two tiles could end in one group of the ring's loads -- the launcher refuses it
    before anything is launched (the search goes to the int8 sketch)."""
    d = 128
    assert runs_of(width, d) <= 8
    x = unit(np.random.default_rng(width).uniform(-1, 1, (64, d)).astype(np.float32))
    probe.scan(width, pack(width, *quantise(width, x)), 64, d, COS, None, Query(width, x[0]).image, np.ones(3, np.float32),
               1.0, 0.0, 0.0, 0.0, 0.0, 64, 1, expect=HIP_INVALID_VALUE)


def test_the_hosts_query_levels_are_the_models(probe):
    """host/vt_sketch6.h through the probe: the nibble image, the scales and the residual's norm equal the model's bit for
    bit, and so do the sums that bound level 3 -- the pass tests above feed the kernels what a search would."""
    for d in (129, 200, 768):
        rng = np.random.default_rng(d)
        for q in (unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0], np.eye(1, d, d // 3)[0].astype(np.float32),
                  (rng.uniform(-1, 1, d) * 40).astype(np.float32)):
            lw = probe.lib.vtp_level_words(d)
            img, resid, t, ee = np.zeros((3, lw), np.uint32), np.zeros(d), np.zeros(3, np.float32), C.c_double()
            probe.lib.vtp_query_levels(probe._p(q, C.c_float), d, probe._p(img, C.c_uint32), probe._p(resid, C.c_double),
                                       probe._p(t, C.c_float), C.byref(ee))
            Q, tm, eta_v = ref6.query_levels(q)
            assert np.array_equal(img, nibble_image(Q, d)) and np.array_equal(t.view(np.uint32), tm.view(np.uint32))
            assert np.array_equal(resid, eta_v)
            assert abs(ee.value - math.fsum((eta_v ** 2).tolist())) <= 2.0 ** -40 * ee.value
            pos, neg, l1 = C.c_longlong(), C.c_longlong(), C.c_longlong()
            probe.lib.vtp_level_sums(probe._p(img[2], C.c_uint32), lw, C.byref(pos), C.byref(neg), C.byref(l1))
            assert (pos.value, neg.value, l1.value) == ref5.level_sums(Q[2])
            c, w = C.c_double(), C.c_double()
            probe.lib.vtp_level_bound5(probe._p(img[2], C.c_uint32), lw, t[2], C.byref(c), C.byref(w))
            assert (c.value, w.value) == ref5.level_bound(Q[2], tm[2])


# ---- C. the spread certification --------------------------------------------------------------------------------------------
KP = 64


def certify_model(lo, hi, rows, lists, kp, k, cap):
    """DESIGN 4.10's tail in numpy: Kt = the k-th smallest live key(lo) word (0xffffffff when at most k are live); a slot is a
    candidate iff it is live by its key(hi) word and that word is <= Kt; a list of candidates alone refuses the certificate."""
    live = lo != EMPTY
    kt = int(np.sort(lo[live])[k - 1]) if live.sum() > k else 0xFFFFFFFF
    cand = (hi != EMPTY) & (hi <= np.uint32(kt))
    fail = bool(cand.reshape(lists, kp).all(axis=1).any())
    cnt = int(cand.sum())
    ok = not fail and cnt <= cap
    slots = lists * kp
    tb = (slots + 1023) // 1024
    padded = np.full(tb * 1024, EMPTY, np.uint32)
    padded[:slots] = lo
    parts = np.sort(padded.reshape(tb, 1024), axis=1)[:, :k]
    return dict(kt=kt, cnt=cnt, ok=ok, rows=np.sort(rows[cand]), parts=parts, live=(padded.reshape(tb, 1024) != EMPTY).sum(axis=1))


def check_certify(probe, lo, hi, lists, k, cap, what, expect_ok=None):
    slots = lists * KP
    rows = (np.arange(slots, dtype=np.uint64) * 7 + 3).astype(np.uint32)
    want = certify_model(lo, hi, rows, lists, KP, k, cap)
    if expect_ok is not None:
        assert want["ok"] == expect_ok, (what, want["cnt"], want["kt"])
    # twice on the same buffers, the three shared words garbage before the first call: both calls give the same answer
    out = probe.certify(lo, hi, rows, lists, KP, k, cap, [0xDEADBEEF, 0x1, 0xFFFFFF00, 0xA5A5A5A5], runs=2)
    for r in range(2):
        tag = (what, "run %d" % r)
        assert np.array_equal(np.sort(out["parts"][r], axis=1), want["parts"]), tag
        assert np.array_equal(out["live"][r], want["live"]), tag
        assert list(out["info"][r]) == [2 if want["ok"] else 0, want["cnt"], want["kt"], 1], (tag, list(out["info"][r]), want["cnt"], want["kt"])
        assert out["count"][r] == (want["cnt"] if want["ok"] else 0), tag
        if want["ok"]:
            assert np.array_equal(np.sort(out["rows"][r][:want["cnt"]]), want["rows"]), tag
    return want


def random_lists(rng, lists, live_frac=0.5, spread=3000, base=0x80000000):
    """Word arrays as a pass leaves them: live slots carry key(hi) <= key(lo), empty ones 0xffffffff in both; the words come
    from a narrow range, so the k-th smallest has neighbours and copies."""
    slots = lists * KP
    lo = (base + rng.integers(0, spread, slots)).astype(np.uint32)
    hi = (lo - rng.integers(0, spread // 4 + 1, slots).astype(np.uint32)).astype(np.uint32)
    dead = rng.uniform(size=slots) >= live_frac
    lo[dead] = EMPTY
    hi[dead] = EMPTY
    return lo, hi


@pytest.mark.parametrize("k", [1, 10, 32, 63])
@pytest.mark.parametrize("lists", [5, 33, 16, 17, 4097])
def test_certify_random_lists(probe, lists, k):
    """lists * 64 slots that are no multiple of the threshold kernel's 1 024 (5, 33, 17, 4097), exactly one and a bit over one
    collect block's sixteen lists (16, 17), and more lists than kCollectMaxBlocks * kCollectLists (4097: seventeen lists per
    collect block).  At 4097 lists the collect's LDS holds 257 k partial words: k = 63 is over the launcher's 48 KiB and is
    refused before anything is launched, which is what this test then asserts."""
    rng = np.random.default_rng(100 * lists + k)
    lo, hi = random_lists(rng, lists, spread=3000 if lists < 100 else 400000)
    if lists == 4097 and k == 63:
        probe.certify(lo, hi, np.zeros(lists * KP, np.uint32), lists, KP, k, 64, [0] * 4, runs=1, expect=HIP_INVALID_VALUE)
        return
    check_certify(probe, lo, hi, lists, k, lists * KP, "random lists=%d k=%d" % (lists, k))
    lo, hi = random_lists(rng, lists, live_frac=0.03, spread=50)  # few live words, many copies
    check_certify(probe, lo, hi, lists, k, lists * KP, "sparse lists=%d k=%d" % (lists, k))


@pytest.mark.parametrize("k", [1, 10, 32, 63])
def test_certify_edges(probe, k):
    rng = np.random.default_rng(k)
    lists = 33  # two whole threshold slices and a piece of a third; three collect blocks
    slots = lists * KP
    empty = np.full(slots, EMPTY, np.uint32)
    # all slots empty
    w = check_certify(probe, empty, empty, lists, k, 16, "all empty k=%d" % k, expect_ok=True)
    assert (w["kt"], w["cnt"]) == (0xFFFFFFFF, 0)
    # live = k - 1, k, k + 1: at most k live words leave Kt at 0xffffffff and every live slot a candidate
    for live in (k - 1, k, k + 1):
        lo, hi = empty.copy(), empty.copy()
        at = rng.choice(slots, live, replace=False)
        lo[at] = (0x80001000 + rng.integers(0, 50, live)).astype(np.uint32)
        hi[at] = lo[at] - np.uint32(5)
        w = check_certify(probe, lo, hi, lists, k, slots, "live=%d k=%d" % (live, k), expect_ok=None)
        assert (w["kt"] == 0xFFFFFFFF) == (live <= k) and (live > k or w["cnt"] == live)
    # more than k copies of the word at Kt: inside one slice, and spread over the slices
    for name, where in (("one slice", np.arange(100, 100 + 3 * k + 5)), ("spread", np.arange(3 * k + 5) * (slots // (3 * k + 5)))):
        lo, hi = random_lists(rng, lists, spread=1000, base=0x80002000)
        lo[where] = 0x80001234
        hi[where] = 0x80001200
        smaller = rng.choice(np.setdiff1d(np.arange(slots), where), k // 2, replace=False)
        lo[smaller] = 0x80001000
        hi[smaller] = 0x80000F00
        w = check_certify(probe, lo, hi, lists, k, slots, "copies at Kt, %s, k=%d" % (name, k))
        assert w["kt"] == 0x80001234
    # the word 0xfffffffe is a live word like any other: here it is Kt
    lo, hi = empty.copy(), empty.copy()
    at = rng.choice(slots, k + 3, replace=False)
    lo[at] = 0xFFFFFFFE
    hi[at] = 0xFFFFFFFE
    lo[at[:k - 1]] = 0x90000000
    hi[at[:k - 1]] = 0x90000000
    w = check_certify(probe, lo, hi, lists, k, slots, "0xfffffffe k=%d" % k)
    assert (w["kt"], w["cnt"]) == (0xFFFFFFFE, k + 3)
    # key(hi) == Kt is a candidate, key(hi) == Kt + 1 is not
    lo, hi = random_lists(rng, lists, spread=5000, base=0x80010000)
    kt = int(np.sort(lo[lo != EMPTY])[k - 1])
    far = np.nonzero(lo > np.uint32(kt + 1))[0]
    hi[far[:7]] = kt
    hi[far[7:16]] = kt + 1
    w = check_certify(probe, lo, hi, lists, k, slots, "hi at Kt and one above, k=%d" % k)
    assert w["kt"] == kt
    rows = (np.arange(slots, dtype=np.uint64) * 7 + 3).astype(np.uint32)
    assert set(rows[far[:7]]) <= set(w["rows"]) and not set(rows[far[7:16]]) & set(w["rows"])


@pytest.mark.parametrize("lists", [5, 33])
def test_certify_refuses_a_full_list_and_a_list_over_the_cap(probe, lists):
    rng = np.random.default_rng(lists)
    slots = lists * KP
    k = 10
    # one list whose 64 slots are all candidates: it may have dropped a row that matters
    lo, hi = random_lists(rng, lists, spread=100000, base=0x80100000)
    full = lists - 2
    lo[full * KP:(full + 1) * KP] = (0x80000100 + rng.integers(0, 64, KP)).astype(np.uint32)
    hi[full * KP:(full + 1) * KP] = 0x80000010
    w = check_certify(probe, lo, hi, lists, k, slots, "one full list", expect_ok=False)
    assert w["cnt"] >= KP
    # ... and with one slot of it far above Kt the certificate stands
    hi[full * KP + 17] = 0x80200000
    lo[full * KP + 17] = 0x80200000
    check_certify(probe, lo, hi, lists, k, slots, "one slot short of a full list", expect_ok=True)
    # the candidates number exactly the cap, and one more
    lo, hi = random_lists(rng, lists, live_frac=0.4, spread=100000, base=0x80100000)
    cnt = check_certify(probe, lo, hi, lists, k, slots, "cap probe")["cnt"]
    assert cnt >= 2
    check_certify(probe, lo, hi, lists, k, cnt, "cnt == cap", expect_ok=True)
    check_certify(probe, lo, hi, lists, k, cnt - 1, "cnt == cap + 1", expect_ok=False)
