"""The matrix-core nomination kernels against their model and their bound, score by score.

K2 (vt_batch.hip), K2b (vt_batch_bf16.hip) and K2s (vt_batch_shadow.hip) only nominate rows; batch_group_finish certifies a
query on three premises that no search result shows: (1) every score a kernel forms is within eps of the true one, (2) the
pass appends every row < n_total whose score reaches tau, and counts them all even past cand_cap, (3) tau, xnorm2[] and the
largest norm are what the host believes.  test_gpu_parity.py, test_gpu_shadow.py and test_gpu_multiquery.py compare final
hits: a dropped row, a stale LDS stage or an operand rounded differently shows there only when it hits a true top-k row.
Here the kernels are launched one at a time through tests/batch_probe.cpp (libvt_batch_probe.so: the three units and
nothing else of the library) and everything is read back:

  A  the query images, the row image and its patching, byte for byte against tests/batch_ref.py; the row norms and their maximum;
  B  dense scores: a one-hot set whose every score is a single product (any lane, chunk, swizzle or k-permutation mismatch
     shows exactly), then every input class against f64 dots within the library's own margin (host/vt_batchbound.h);
  C  the pass: with the kernel's own dense scores S, the nominated set is {row < n_total : S >= tau} exactly, bits and count
     included, rows past n_total never, whatever they score;
  D  the threshold kernels against a sort, the batched select against a stable sort.

Shapes are the smallest at which each mechanism can go wrong: ld = 64 .. 320 is 2 .. 10 chunks against rings of 3, 4 and 5
stages (the library only has ld % 64 == 0); n = 1 .. 1061 is less than a tile, partial last tiles of the 128- and 256-row
block tiles and a last wave past n_total; blocks = 1, 2, tiles, tiles + 3 is a ring that crosses tile boundaries, one tile
per block (with ld = 64 a sequence shorter than the ring) and idle blocks.  Each axis is walked at two values of the others.
tests/test_batch_model.py shows on the CPU that a plain bf16 machine meets the same bounds on the same input classes.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import batch_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
K2, K2B, K2S = 0, 1, 2
KERNELS = (K2, K2B, K2S)
NAME = {K2: "K2", K2B: "K2b", K2S: "K2s"}
PASS, DENSE, MAXIMA = 0, 1, 2
SENT32 = np.uint32(0xA5A5A5A5)
NINF = np.float32(-np.inf)
LDS = (64, 128, 192, 320)
NS = (1, 100, 256, 549, 1061)
PADS = {K2: (32, 64, 128, 256), K2B: (64, 128, 256), K2S: (64, 128, 256)}
MARGINS = {}   # (kernel, family, class) -> largest |error| / tolerance seen (recorded, not asserted: see the last test)


class VbpScores(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("mode", C.c_int32), ("ld", C.c_uint32), ("nq_pad", C.c_uint32), ("n", C.c_uint32),
                ("n_total", C.c_uint32), ("sample_stride", C.c_uint32), ("blocks", C.c_uint32), ("stages", C.c_uint32),
                ("sample_rows", C.c_uint32), ("cand_cap", C.c_uint32), ("pad_", C.c_uint32),
                ("X", C.c_void_p), ("x_floats", C.c_uint64), ("stride", C.c_uint64),
                ("shadow", C.c_void_p), ("shadow_elems", C.c_uint64),
                ("Q", C.c_void_p), ("q_floats", C.c_uint64),
                ("qimage", C.c_void_p), ("qimage_bytes", C.c_uint64),
                ("xnorm2", C.c_void_p), ("xnorm_len", C.c_uint64),
                ("sample", C.c_void_p), ("sample_len", C.c_uint64),
                ("tau", C.c_void_p), ("tau_len", C.c_uint64),
                ("cand", C.c_void_p), ("cand_len", C.c_uint64),
                ("cand_count", C.c_void_p), ("count_len", C.c_uint64)]


class Probe:
    def __init__(self):
        # VT_BATCH_PROBE_LIB: another build of the same probe (a deliberately broken kernel, to see these tests fail)
        path = os.environ.get("VT_BATCH_PROBE_LIB") or os.path.join(ROOT, "vettore_amd", "lib", "libvt_batch_probe.so")
        assert os.path.exists(path), "build it with `make` (%s)" % os.path.basename(path)
        L = self.lib = C.CDLL(path)
        vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
        L.vbp_rows_per_block.restype = u32
        L.vbp_rows_per_block.argtypes = [C.c_int]
        L.vbp_q_image_bytes.restype = sz
        L.vbp_q_image_bytes.argtypes = [C.c_int, u32]
        L.vbp_shadow_elems.restype = sz
        L.vbp_shadow_elems.argtypes = [u32, u32]
        L.vbp_shadow_index.restype = sz
        L.vbp_shadow_index.argtypes = [u32, u32, u32]
        L.vbp_sample_groups.restype = u32
        L.vbp_sample_groups.argtypes = [u32]
        L.vbp_bf16_pad.restype = u32
        L.vbp_bf16_pad.argtypes = [u32]
        L.vbp_eps.restype = C.c_double
        L.vbp_eps.argtypes = [C.c_int, C.c_int, u32, C.c_double, C.c_double]
        L.vbp_bf16_terms.restype = None
        L.vbp_bf16_terms.argtypes = [C.c_int, u32, C.c_double, C.c_double, C.POINTER(C.c_double)]
        L.vbp_magnitudes_ok.argtypes = [C.c_int, C.c_double, C.c_double]
        L.vbp_q_image.argtypes = [C.c_int, vp, sz, u32, u32, vp, sz]
        L.vbp_shadow_build.argtypes = [vp, sz, sz, u32, u32, u32, vp, sz]
        L.vbp_shadow_rows.argtypes = [vp, sz, sz, vp, u32, u32, u32, vp, sz]
        L.vbp_row_sqnorms.argtypes = [vp, sz, sz, u32, u32, vp, u32, vp, sz, vp]
        L.vbp_scores.argtypes = [C.POINTER(VbpScores)]
        L.vbp_sample_tau.argtypes = [C.c_int, vp, sz, u32, u32, u32, u32, vp]
        L.vbp_batch_select.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]
        self.tile_rows = {k: L.vbp_rows_per_block(k) for k in KERNELS}
        assert self.tile_rows == {K2: 128, K2B: 256, K2S: 256}

    @staticmethod
    def ptr(a):
        return None if a is None else a.ctypes.data

    def eps(self, l2, bf16, d, qn, xn):
        return self.lib.vbp_eps(int(l2), int(bf16), d, qn, xn)

    def terms(self, l2, d, qn, xn):
        out = (C.c_double * 3)()
        self.lib.vbp_bf16_terms(int(l2), d, qn, xn, out)
        return tuple(out)

    def q_image(self, kernel, Q, ld, nq_pad, image_bytes=None, expect=0):
        Q = np.ascontiguousarray(Q, np.float32)
        nbytes = self.lib.vbp_q_image_bytes(kernel, ld) if image_bytes is None else image_bytes
        img = np.zeros(nbytes // 2, np.uint16)
        rc = self.lib.vbp_q_image(kernel, self.ptr(Q), Q.size, ld, nq_pad, self.ptr(img), nbytes)
        assert rc == expect, "vbp_q_image: hipError_t %d" % rc
        return img

    def shadow_build(self, xbuf, stride, rows_src, rows_img, ld, expect=0):
        img = np.zeros(rows_img * ld, np.uint16)
        rc = self.lib.vbp_shadow_build(self.ptr(xbuf), xbuf.size, stride, rows_src, rows_img, ld, self.ptr(img), img.size)
        assert rc == expect, "vbp_shadow_build: hipError_t %d" % rc
        return img

    def shadow_rows(self, xbuf, stride, rowlist, n_rows, ld, img, expect=0):
        img = img.copy()
        rowlist = np.ascontiguousarray(rowlist, np.uint32)
        rc = self.lib.vbp_shadow_rows(self.ptr(xbuf), xbuf.size, stride, self.ptr(rowlist), rowlist.size, n_rows, ld, self.ptr(img), img.size)
        assert rc == expect, "vbp_shadow_rows: hipError_t %d" % rc
        return img

    def row_sqnorms(self, xbuf, stride, n, d, xnorm2, max_bits, rowlist=None, expect=0):
        xnorm2 = xnorm2.copy()
        mx = np.array([max_bits], np.uint64)
        rl = None if rowlist is None else np.ascontiguousarray(rowlist, np.uint32)
        rc = self.lib.vbp_row_sqnorms(self.ptr(xbuf), xbuf.size, stride, n, d, self.ptr(rl), 0 if rl is None else rl.size,
                                      self.ptr(xnorm2), xnorm2.size, self.ptr(mx))
        assert rc == expect, "vbp_row_sqnorms: hipError_t %d" % rc
        return xnorm2, float(mx.view(np.float64)[0])

    def scores(self, kernel, mode, ld, nq_pad, n, n_total, blocks, xbuf=None, stride=0, shadow=None, Q=None, qimage=None, xnorm2=None,
               sample_stride=1, stages=5, sample_rows=0, tau=None, cand_cap=0, expect=0, **override):
        """one launch; dense / maxima: the sample matrix [nq_pad][sample_rows]; pass: (cand [nq_pad][cand_cap][2] u32, counts)"""
        keep = [np.ascontiguousarray(a) if a is not None else None for a in (xbuf, shadow, Q, qimage, xnorm2, tau)]
        xbuf, shadow, Q, qimage, xnorm2, tau = keep
        a = VbpScores(kernel=kernel, mode=mode, ld=int(ld), nq_pad=int(nq_pad), n=int(n), n_total=int(n_total), sample_stride=int(sample_stride),
                      blocks=int(blocks), stages=int(stages), sample_rows=int(sample_rows), cand_cap=int(cand_cap))
        for name, arr, length in (("X", xbuf, "x_floats"), ("shadow", shadow, "shadow_elems"), ("Q", Q, "q_floats"),
                                  ("qimage", qimage, "qimage_bytes"), ("xnorm2", xnorm2, "xnorm_len"), ("tau", tau, "tau_len")):
            setattr(a, name, self.ptr(arr))
            setattr(a, length, 0 if arr is None else (arr.nbytes if name == "qimage" else arr.size))
        a.stride = int(stride)
        sample = cand = count = None
        if mode == PASS:
            cand = np.zeros((nq_pad, max(cand_cap, 1), 2), np.uint32)
            count = np.zeros(nq_pad, np.uint32)
            a.cand, a.cand_len, a.cand_count, a.count_len = self.ptr(cand), nq_pad * cand_cap, self.ptr(count), nq_pad
        else:
            sample = np.zeros((nq_pad, max(sample_rows, 1)), np.float32)
            a.sample, a.sample_len = self.ptr(sample), nq_pad * sample_rows
        for key, value in override.items():   # force_<field>: the refusal tests lie about one size
            assert key.startswith("force_"), key
            setattr(a, key[6:], value)
        rc = self.lib.vbp_scores(C.byref(a))
        assert rc == expect, "vbp_scores: hipError_t %d" % rc
        return (cand, count) if mode == PASS else sample

    def sample_tau(self, groups, sample, nq_real, rank, expect=0):
        sample = np.ascontiguousarray(sample, np.float32)
        nq, rows = sample.shape
        tau = np.zeros(nq, np.float32)
        rc = self.lib.vbp_sample_tau(groups, self.ptr(sample), sample.size, rows, nq, nq_real, rank, self.ptr(tau))
        assert rc == expect, "vbp_sample_tau: hipError_t %d" % rc
        return tau

    def batch_select(self, keys, pay, k, export=None, expect=0):
        keys, pay = np.ascontiguousarray(keys, np.uint64), np.ascontiguousarray(pay, np.uint32)
        nq, m = keys.shape
        ok, orow, oraw, ocnt = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.uint32), np.zeros(nq, np.uint32)
        cc_out, tau_out, st_out, st_after = np.zeros(nq, np.uint32), np.zeros(nq, np.uint32), np.zeros(1, np.int32), np.zeros(1, np.int32)
        cc, tau, status = export if export else (None, None, 0)
        rc = self.lib.vbp_batch_select(self.ptr(keys), self.ptr(pay), nq, m, k, self.ptr(ok), self.ptr(orow), self.ptr(oraw), self.ptr(ocnt),
                                       1 if export else 0, self.ptr(cc), self.ptr(tau), status, self.ptr(cc_out), self.ptr(tau_out),
                                       self.ptr(st_out), self.ptr(st_after))
        assert rc == expect, "vbp_batch_select: hipError_t %d" % rc
        return ok, orow, oraw, ocnt, cc_out, tau_out, int(st_out[0]), int(st_after[0])


@pytest.fixture(scope="module")
def probe():
    return Probe()


def round_up(v, m):
    return (v + m - 1) // m * m


def sentinel_f32(n):
    return np.full(n, SENT32, np.uint32).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- one corpus and batch, with everything the launches and the checks need, made once per shape --------------------------
class Case:
    def __init__(self, name, n, ld, nq_pad, d=None, seed=3, stride=None):
        self.name, self.n, self.ld, self.nq_pad, self.d = name, n, ld, nq_pad, ld if d is None else d
        self.X, self.Q = ref.make_class(name, seed, n, nq_pad, ld, self.d) if name != "onehot" else one_hot(n, ld, nq_pad, seed)
        self.stride = ld if stride is None else stride
        self._ref = {}

    def finish(self):
        """(after a test has edited X or Q)"""
        self.xbuf = np.zeros((self.n, self.stride), np.float32)
        self.xbuf[:, :self.ld] = self.X
        self.qn, self.xmax = ref.norms(self.Q), float(ref.norms(self.X).max())
        self.shadow = ref.shadow_image(self.X, self.n, round_up(self.n, 256), self.ld)
        self.qimage = {K2B: ref.q_image(self.Q, self.ld, self.nq_pad), K2S: ref.q_image16(self.Q, self.ld, self.nq_pad)}
        self.norm_pad = np.float32(np.nan)   # what the norm column holds past n_total: must never reach a row < n_total
        return self

    def xnorm2(self):
        col = np.full(round_up(self.n, 256), self.norm_pad, np.float32)
        col[:self.n] = ref.xnorm2_f32(self.X)
        return col

    def truth(self, l2):
        if ("t", l2) not in self._ref:
            self._ref["t", l2] = ref.scores64(self.Q, self.X, l2)
            self._ref["r", l2] = ref.scores64_rounded(self.Q, self.X, l2)
        return self._ref["t", l2], self._ref["r", l2]

    def launch(self, probe, kernel, mode, l2, blocks, n=None, **kw):
        common = dict(xnorm2=self.xnorm2() if l2 else None)
        if kernel == K2S:
            common.update(shadow=kw.pop("shadow", self.shadow), qimage=self.qimage[K2S])
        else:
            common.update(xbuf=self.xbuf, stride=self.stride)
            common.update(Q=self.Q) if kernel == K2 else common.update(qimage=self.qimage[K2B])
        common.update(kw)
        return probe.scores(kernel, mode, self.ld, self.nq_pad, self.n if n is None else n, self.n, blocks, **common)

    def dense(self, probe, kernel, l2, blocks, **kw):
        tr = probe.tile_rows[kernel]
        return self.launch(probe, kernel, DENSE, l2, blocks, sample_rows=round_up(self.n, tr), **kw)


def one_hot(n, ld, nq_pad, seed):
    """Q[b] = c_b e_j(b), X[r] = v_r e_j'(r): every score is one product.  j(b) = b mod ld and j'(r) = (5 r + 1) mod ld walk
    every column (5 is prime to every ld here) when there are at least ld of either."""
    rng = np.random.default_rng(seed)
    X, Q = np.zeros((n, ld), np.float32), np.zeros((nq_pad, ld), np.float32)
    X[np.arange(n), (5 * np.arange(n) + 1) % ld] = rng.standard_normal(n).astype(np.float32) + np.float32(3.0)
    Q[np.arange(nq_pad), np.arange(nq_pad) % ld] = rng.standard_normal(nq_pad).astype(np.float32) - np.float32(3.0)
    return X, Q


_CASES = {}


def case(name, n, ld, nq_pad, **kw):
    key = (name, n, ld, nq_pad, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = Case(name, n, ld, nq_pad, **kw).finish()
    return _CASES[key]


def tiles_of(probe, kernel, n):
    return (n + probe.tile_rows[kernel] - 1) // probe.tile_rows[kernel]


def block_counts(probe, kernel, n):
    t = tiles_of(probe, kernel, n)
    return sorted({1, 2, t, t + 3})


def axis_points(probe, kernel):
    """(n, ld, nq_pad, blocks, stages): every value of each axis at two values of the others"""
    pts = set()
    pads = PADS[kernel]
    for ld in LDS:                       # chunks against the ring: one tile per block, and a ring that crosses tiles
        pts.add((549, ld, pads[-1], tiles_of(probe, kernel, 549), 5))
        pts.add((1061, ld, pads[0], 2, 4))
    for n in NS:
        pts.add((n, 64, pads[1], 1, 5))
        pts.add((n, 192, pads[-1], 2, 4))
    for n, ld in ((1061, 64), (549, 320)):
        for blocks in block_counts(probe, kernel, n):
            pts.add((n, ld, pads[1], blocks, 5))
    for pad in pads:
        pts.add((549, 64, pad, 3, 4))
        pts.add((1061, 128, pad, 1, 5))
    if kernel != K2S:                    # (only K2s has a ring depth to choose)
        pts = {(n, ld, pad, blocks, 5) for n, ld, pad, blocks, _ in pts}
    else:
        pts |= {(549, 64, 64, 3, s) for s in (4, 5)} | {(1061, 320, 256, 2, s) for s in (4, 5)}
    return sorted(pts)


def check_scores(probe, kernel, cs, l2, S, name=None):
    """premise 1 on a dense matrix S [nq_pad][>= n]: every score within the library's margin of the f64 dot"""
    truth, rounded = cs.truth(l2)
    bf16 = kernel != K2
    got = S[:, :cs.n].astype(np.float64)
    assert np.isfinite(got).all()
    worst = worst_acc = 0.0
    for b in range(cs.nq_pad):
        full = probe.eps(l2, bf16, cs.d, cs.qn[b], cs.xmax)
        err = np.abs(got[b] - truth[b]).max()
        assert err <= full, "%s %s query %d: |S - dot64| = %g > eps = %g" % (NAME[kernel], cs.name, b, err, full)
        worst = max(worst, err / full if full > 0 else 0.0)
        if bf16:
            _, acc, flush = probe.terms(l2, cs.d, cs.qn[b], cs.xmax)
            err = np.abs(got[b] - rounded[b]).max()
            assert err <= acc + flush, "%s %s query %d: |S - dot64(rounded)| = %g > %g" % (NAME[kernel], cs.name, b, err, acc + flush)
            worst_acc = max(worst_acc, err / (acc + flush) if acc + flush > 0 else 0.0)
    key = "%s/%s/%s" % (NAME[kernel], "l2" if l2 else "dot", name or cs.name)
    MARGINS[key] = max(MARGINS.get(key, 0.0), worst)
    if bf16:   # (against the rounded operands' dot: the room in the accumulation and flush terms alone)
        MARGINS[key + "/accumulation"] = max(MARGINS.get(key + "/accumulation", 0.0), worst_acc)
    assert (S[:, cs.n:] == NINF).all(), "rows >= n_total read -inf"


# ==== A: images and norms ==================================================================================================
def awkward(Q):
    """a few elements no rounding treats like the others: ties, subnormals, -0, the largest that stays finite"""
    Q = Q.copy()
    flat = Q.reshape(-1)
    special = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1e-40, -1e-45, 5e-39, -0.0, 3.38e38, 65280.0], np.float32)
    flat[(7 + 13 * np.arange(special.size)) % flat.size] = special
    return Q


@pytest.mark.parametrize("kernel", [K2B, K2S])
@pytest.mark.parametrize("ld,nq_pad", [(ld, 128) for ld in LDS] + [(128, 64), (128, 256), (64, 256), (320, 64)])
def test_query_images_byte_for_byte(probe, kernel, ld, nq_pad):
    Q = awkward(ref.make_class("gaussian", 9, 1, nq_pad, ld)[1])
    want = (ref.q_image if kernel == K2B else ref.q_image16)(Q, ld, nq_pad)
    assert np.array_equal(probe.q_image(kernel, Q, ld, nq_pad), want)   # (what a narrow batch leaves unwritten keeps the fill)


@pytest.mark.parametrize("n,ld,extra", [(549, ld, 0) for ld in LDS] + [(n, 128, 0) for n in NS] + [(n, 64, 256) for n in (1, 1061)])
def test_shadow_image_byte_for_byte(probe, n, ld, extra):
    cs = case("gaussian", n, ld, 64, stride=ld + 64 * (n % 2))
    xbuf = cs.xbuf.copy()
    xbuf[:, :ld] = awkward(cs.X)
    rows_img = round_up(n, 256) + extra
    got = probe.shadow_build(xbuf, cs.stride, n, rows_img, ld)
    assert np.array_equal(got, ref.shadow_image(xbuf, n, rows_img, ld))   # zero rows >= rows_src included
    assert not probe.shadow_build(xbuf, cs.stride, 0, 256, ld).any()


@pytest.mark.parametrize("n,ld", [(1061, 64), (549, 320), (100, 192)])
def test_shadow_rows_patch_equals_a_fresh_build(probe, n, ld):
    cs = case("gaussian", n, ld, 64)
    rng = np.random.default_rng(n)
    rows = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, 9)])).astype(np.uint32)
    marked = int(np.setdiff1d(np.arange(n), rows)[n // 2])   # an untouched row, its bytes made recognisable
    img = cs.shadow.copy()
    col = np.arange(ld)
    img[ref.shadow_index(marked, col, ld)] = 0x1234
    X2 = cs.xbuf.copy()
    X2[rows, :ld] = awkward(rng.standard_normal((rows.size, ld)).astype(np.float32))
    got = probe.shadow_rows(X2, cs.stride, rows, n, ld, img)
    want = ref.shadow_image(X2, n, round_up(n, 256), ld)
    want[ref.shadow_index(marked, col, ld)] = 0x1234
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ref.CLASSES)
def test_row_norms_and_their_maximum(probe, name):
    """xnorm2[row] == float32(sum of squares in f64).  The kernel adds the d squares (each exact in f64: 48 bits) in its own
    order -- per lane, then a butterfly -- and numpy in another; either sum is within (d - 1) 2^-53 of the exact one,
    relatively (all terms positive), so the kernel's f64 value lies within s (1 +- 2 d 2^-53) of numpy's s, and its f32
    rounding, being monotone, between the f32 roundings of the two ends."""
    n, d, stride = 1061, 100, 128
    X, _ = ref.make_class(name, 21, n, 1, stride, d)
    X[:, d:] = 7.0   # (columns >= d are not the row's)
    s = (X[:, :d].astype(np.float64) ** 2).sum(axis=1)
    g = 2 * d * 2.0 ** -53
    got, mx = probe.row_sqnorms(X, stride, n, d, sentinel_f32(n + 5), 0)
    assert (got[:n] >= (s * (1 - g)).astype(np.float32)).all() and (got[:n] <= (s * (1 + g)).astype(np.float32)).all()
    assert (bits(got[n:]) == SENT32).all()
    assert s.max() * (1 - g) <= mx <= s.max() * (1 + g)            # the largest row's, to the same term ...
    assert (mx >= s * (1 - g)).all()                               # ... so no row's norm exceeds it by more
    # the list variant: only the listed rows are written, the maximum is never lowered
    rows = np.array([0, 17, n - 1, 500], np.uint32)
    fill = sentinel_f32(n)
    got, mx2 = probe.row_sqnorms(X, stride, n, d, fill, np.float64(s.max() * 4).view(np.uint64), rowlist=rows)
    assert mx2 == s.max() * 4
    others = np.setdiff1d(np.arange(n), rows)
    assert (bits(got[others]) == SENT32).all()
    assert (got[rows] >= (s[rows] * (1 - g)).astype(np.float32)).all() and (got[rows] <= (s[rows] * (1 + g)).astype(np.float32)).all()
    _, mx3 = probe.row_sqnorms(X, stride, n, d, fill, 0, rowlist=rows)
    assert s[rows].max() * (1 - g) <= mx3 <= s[rows].max() * (1 + g)


# ==== B: scores ============================================================================================================
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("n,ld,blocks,stages", [(549, 192, 2, 5), (1061, 64, 9, 4), (549, 320, 1, 4)])
def test_one_hot_scores_are_single_products(probe, kernel, l2, n, ld, blocks, stages):
    cs = case("onehot", n, ld, 256)
    S = cs.dense(probe, kernel, l2, blocks, stages=stages)
    Qf, Xf = (cs.Q, cs.X) if kernel == K2 else (ref.bf16_round(cs.Q), ref.bf16_round(cs.X))
    jq, jx = np.arange(256) % ld, (5 * np.arange(n) + 1) % ld
    c, v = Qf[np.arange(256), jq], Xf[np.arange(n), jx]
    # one product, rounded once to f32 (exact for two bf16 operands); every other term of the sum is a zero
    want = np.where(jq[:, None] == jx[None, :], (c[:, None].astype(np.float32) * v[None, :].astype(np.float32)).astype(np.float32), np.float32(0))
    if l2:
        want = (np.float32(2.0) * want - ref.xnorm2_f32(cs.X)[None, :]).astype(np.float32)
    assert np.array_equal(S[:, :n], want), np.argwhere(S[:, :n] != want)[:5]
    assert (S[:, n:] == NINF).all()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("name", ref.CLASSES)
def test_scores_of_every_class_within_the_margin(probe, kernel, l2, name):
    cs = case(name, 549, 192, 128)
    check_scores(probe, kernel, cs, l2, cs.dense(probe, kernel, l2, 2))
    cs = case(name, 300, 128, 64, d=100)   # rows shorter than their padded length: the margin's d is the row's
    check_scores(probe, kernel, cs, l2, cs.dense(probe, kernel, l2, 5, stages=4))


@pytest.mark.parametrize("kernel", KERNELS)
def test_scores_along_every_axis(probe, kernel):
    for n, ld, pad, blocks, stages in axis_points(probe, kernel):
        cs = case("gaussian", n, ld, pad)
        for l2 in (False, True):
            S = cs.dense(probe, kernel, l2, blocks, stages=stages)
            check_scores(probe, kernel, cs, l2, S, name="gaussian")
            # the scores do not depend on how the tiles are dealt to the blocks, nor on the ring's depth
            first = cs._ref.setdefault(("S", kernel, l2), S)
            assert np.array_equal(bits(S), bits(first)), (n, ld, pad, blocks, stages)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("l2", [False, True])
def test_dense_sample_stride_two_lands_tile_2i_in_slot_i(probe, kernel, l2):
    for n, ld, blocks in ((1061, 64, 2), (1061, 192, 7)):
        cs = case("gaussian", n, ld, 64)
        tr = probe.tile_rows[kernel]
        full = cs.dense(probe, kernel, l2, 3)
        launch_tiles = (tiles_of(probe, kernel, n) + 1) // 2
        S = cs.launch(probe, kernel, DENSE, l2, blocks, n=launch_tiles * tr, sample_stride=2, sample_rows=launch_tiles * tr + 7)
        for i in range(launch_tiles):
            assert np.array_equal(bits(S[:, i * tr:(i + 1) * tr]), bits(full[:, 2 * i * tr:(2 * i + 1) * tr])), i
        assert (bits(S[:, launch_tiles * tr:]) == SENT32).all()   # nothing written past the launch's slots


@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("stages", [4, 5])
def test_shadow_maxima_are_the_dense_matrix_group_maxima(probe, l2, stages):
    for n, ld, pad, blocks, stride in ((1061, 64, 64, 5, 1), (1061, 320, 256, 2, 2), (100, 128, 128, 1, 1), (549, 192, 64, 3, 2)):
        cs = case("gaussian", n, ld, pad)
        full = cs.dense(probe, K2S, l2, 2)
        launch_tiles = (tiles_of(probe, K2S, n) + stride - 1) // stride
        groups = probe.lib.vbp_sample_groups(launch_tiles)
        assert groups == 4 * launch_tiles
        M = cs.launch(probe, K2S, MAXIMA, l2, blocks, n=launch_tiles * 256, sample_stride=stride, sample_rows=groups + 3, stages=stages)
        for i in range(launch_tiles):
            tile = full[:, i * stride * 256:(i * stride + 1) * 256].reshape(pad, 4, 64)
            assert np.array_equal(bits(M[:, 4 * i:4 * i + 4]), bits(tile.max(axis=2))), (n, ld, i)
        assert (bits(M[:, groups:]) == SENT32).all()


@pytest.mark.parametrize("name", ref.CLASSES)
@pytest.mark.parametrize("l2", [False, True])
def test_shadow_scores_are_the_bf16_kernels_in_another_order(probe, name, l2):
    """same operands, same rounding, another order of the f32 additions: within twice the accumulation term"""
    cs = case(name, 549, 192, 128)
    a, b = cs.dense(probe, K2B, l2, 2), cs.dense(probe, K2S, l2, 3, stages=4)
    for q in range(cs.nq_pad):
        acc = probe.terms(l2, cs.d, cs.qn[q], cs.xmax)[1]
        assert np.abs(a[q, :cs.n].astype(np.float64) - b[q, :cs.n].astype(np.float64)).max() <= 2 * acc, q


# ==== C: the pass ==========================================================================================================
def spread_taus(S, n):
    """thresholds per query: equal to one of the query's scores (>= must include it), between two, above all, below all,
    the infinities and NaN"""
    nq = S.shape[0]
    tau = np.zeros(nq, np.float32)
    for b in range(nq):
        row = np.sort(S[b, :n])[::-1]
        kind = b % 8
        if kind == 0:
            tau[b] = row[min(4, n - 1)]                     # the 5th best itself
        elif kind == 1:
            tau[b] = np.nextafter(row[min(4, n - 1)], np.float32(np.inf))   # just above it
        elif kind == 2:
            tau[b] = row[n // 2]                            # the median: half of the rows pass
        elif kind == 3:
            tau[b] = row[0]                                 # the best alone (and its ties)
        elif kind == 4:
            tau[b] = NINF
        elif kind == 5:
            tau[b] = np.inf
        elif kind == 6:
            tau[b] = np.nan
        else:
            tau[b] = np.nextafter(row[0], np.float32(np.inf))   # above all: nobody
    return tau


def check_pass(S, n, tau, cand, count, cap):
    """premise 2: the list of query b is {row < n : S[b][row] >= tau[b]} exactly, each entry with the bits of S, each once;
    past the cap the count still counts and the stored ones are members"""
    for b in range(S.shape[0]):
        want = np.flatnonzero(S[b, :n] >= tau[b])
        assert count[b] == want.size, "query %d: cand_count %d, %d rows reach tau %r" % (b, count[b], want.size, tau[b])
        stored = min(want.size, cap)
        rows, sc = cand[b, :stored, 1], cand[b, :stored, 0]
        assert (rows < n).all() and np.unique(rows).size == stored, b
        assert np.isin(rows, want).all(), b
        assert np.array_equal(sc, bits(S[b])[rows]), b
        if want.size <= cap:
            assert np.array_equal(np.sort(rows), want), b
        assert (cand[b, stored:] == SENT32).all(), "query %d: written past its %d entries" % (b, stored)


def loud_last_rows(cs, probe, kernel):
    """everything at and past n_total scores above every threshold: the last row (which K2 and K2b's clamped loads repeat
    for the rows past it) is the best row of every query, K2s's image carries it in its padding rows, and the norm column's
    padding makes an L2 score there enormous"""
    shadow = cs.shadow.copy().reshape(-1)
    rows_img = round_up(cs.n, 256)
    if rows_img > cs.n:
        row, col = np.meshgrid(np.arange(cs.n, rows_img), np.arange(cs.ld), indexing="ij")
        shadow[ref.shadow_index(row, col, cs.ld)] = ref.bf16_bits(cs.X[cs.n - 1])[None, :]
    return shadow


def loud_case(n, ld, pad):
    key = ("loud", n, ld, pad)
    if key not in _CASES:
        cs = Case("positive", n, ld, pad)
        cs.X[n - 1] = np.float32(3.0) + cs.X[n - 1]     # all-positive queries: the largest row wins every one of them
        cs.finish()
        cs.norm_pad = np.float32(-1e30)                  # 2 q.x - (-1e30): far above any threshold here
        _CASES[key] = cs
    return _CASES[key]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("l2", [False, True])
def test_pass_nominates_exactly_the_rows_that_reach_tau(probe, kernel, l2):
    for n, ld, pad, blocks, stages in axis_points(probe, kernel):
        cs = loud_case(n, ld, pad)
        extra = dict(shadow=loud_last_rows(cs, probe, kernel)) if kernel == K2S else {}
        S = cs.dense(probe, kernel, l2, 2, **extra)
        assert (S[:, cs.n:] == NINF).all()
        if not l2:
            assert (S[:, :n].argmax(axis=1) == n - 1).all()   # (the row the padding repeats does beat every threshold below)
        tau = spread_taus(S, n)
        cand, count = cs.launch(probe, kernel, PASS, l2, blocks, tau=tau, cand_cap=n, stages=stages, **extra)
        check_pass(S, n, tau, cand, count, n)


@pytest.mark.parametrize("kernel", KERNELS)
def test_pass_edges_every_row_once_nobody_and_the_full_list(probe, kernel):
    n, ld, pad = 1061, 64, 64
    cs = loud_case(n, ld, pad)
    extra = dict(shadow=loud_last_rows(cs, probe, kernel)) if kernel == K2S else {}
    S = cs.dense(probe, kernel, False, 2, **extra)
    for blocks in block_counts(probe, kernel, n):
        for stages in ((4, 5) if kernel == K2S else (5,)):
            # tau = -inf: rows 0 .. n_total - 1 once each, whoever owns the tile
            tau = np.full(pad, NINF, np.float32)
            cand, count = cs.launch(probe, kernel, PASS, False, blocks, tau=tau, cand_cap=n + 3, stages=stages, **extra)
            check_pass(S, n, tau, cand, count, n + 3)
            assert (count == n).all()
    for value in (np.inf, np.nan):   # nobody; (a padding column's threshold is +inf: launch_sample_tau*)
        tau = np.full(pad, value, np.float32)
        cand, count = cs.launch(probe, kernel, PASS, False, 3, tau=tau, cand_cap=8, **extra)
        assert not count.any() and (cand == SENT32).all()
    # a list of four with hundreds of passers: the count is still the true one, the four are distinct members, the
    # neighbour's list and the space behind are untouched
    tau = spread_taus(S, n)
    tau[1::2] = NINF
    cand, count = cs.launch(probe, kernel, PASS, False, 2, tau=tau, cand_cap=4, **extra)
    check_pass(S, n, tau, cand, count, 4)
    assert (count[1::2] == n).all()


# ==== D: thresholds and the batched select =================================================================================
def tau_rows(rng, n):
    """eight sample rows in the styles of tools/tau_check.hip: plain, many ties, a handful of distinct values (several of
    the best in one thread's slots, +-0 among them), -inf entries"""
    rows = []
    for style in (0, 1, 2, 3, 0, 1, 2, 3):
        x = rng.uniform(-50, 50, n).astype(np.float32)
        if style == 1:
            x = np.round(x)
        if style == 2:
            x = (np.round(x / 25) * 25).astype(np.float32)
            x[rng.random(n) < 0.1] = np.float32(-0.0)
            x[rng.random(n) < 0.1] = np.float32(0.0)
            if n >= 64:
                x[rng.integers(0, 64, 8)] = 75.0
        if style == 3:
            x[rng.random(n) < 1 / 7] = NINF
        rows.append(x)
    rows.append(np.zeros(n, np.float32))   # a padding column
    return np.stack(rows)


def check_tau(probe, groups, sample, rank):
    nq = sample.shape[0]
    got = probe.sample_tau(groups, sample, nq - 1, rank)
    assert got[nq - 1] == np.inf                                  # columns >= nq_real
    for b in range(nq - 1):
        # fewer values than the rank: the smallest -- but sample_tau_kernel's histogram path (rank > 16) answers NaN,
        # "nothing is nominated" (its callers clamp the rank to the sample's size)
        want = ref.rank_largest(sample[b], rank, short="nan" if (not groups and rank > 16) else "smallest")
        if np.isnan(want):
            assert np.isnan(got[b]), (groups, sample.shape[1], rank, b)
        else:
            assert bits(got[b:b + 1])[0] == bits(np.array([want]))[0], (groups, sample.shape[1], rank, b, got[b], want)


def test_sample_tau_is_the_rank_th_largest(probe):
    rng = np.random.default_rng(7)
    for n in (1, 5, 63, 64, 65, 1000, 4097):
        sample = tau_rows(rng, n)
        for rank in range(1, 41):
            check_tau(probe, 0, sample, rank)
    sample = tau_rows(rng, 65536)
    for rank in (1, 6, 16, 17, 27, 40):
        check_tau(probe, 0, sample, rank)


def test_sample_tau_groups_is_the_rank_th_largest(probe):
    rng = np.random.default_rng(8)
    for n in (1, 5, 63, 64, 65, 316, 1000, 1024, 2048):
        sample = tau_rows(rng, n)
        for rank in list(range(1, 41)) + [64]:
            check_tau(probe, 1, sample, rank)


def test_threshold_kernels_serve_many_queries(probe):
    rng = np.random.default_rng(9)
    sample = rng.standard_normal((256, 700)).astype(np.float32)
    for groups, rank in ((0, 6), (0, 27), (1, 6), (1, 40)):
        got = probe.sample_tau(groups, sample, 250, rank)
        want = np.sort(sample, axis=1)[:, -rank]
        assert np.array_equal(got[:250], want[:250]) and (got[250:] == np.inf).all()


@pytest.mark.parametrize("m,k", [(1, 1), (7, 10), (80, 10), (640, 32), (4096, 10), (4096, 1)])
def test_batch_select_is_a_stable_sort_of_the_live_keys(probe, m, k):
    rng = np.random.default_rng(m + k)
    nq = 9
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    keys = rng.integers(0, 1 << 62, (nq, m)).astype(np.uint64)
    keys[1] = rng.integers(0, 3, m).astype(np.uint64)          # ties broken by position
    keys[2] = empty                                            # nothing live
    keys[3, rng.random(m) < 0.5] = empty
    keys[4, 1:] = empty                                        # one live key
    keys[5] = rng.integers(0, 5, m).astype(np.uint64)
    keys[5, rng.random(m) < 0.9] = empty
    pay = rng.integers(0, 1 << 32, (nq, m, 2)).astype(np.uint32)
    cc, tau = rng.integers(0, 1 << 32, nq).astype(np.uint32), rng.standard_normal(nq).astype(np.float32)
    ok, orow, oraw, ocnt, cc_out, tau_out, st_out, st_after = probe.batch_select(keys, pay, k, export=(cc, tau, 0x5A))
    for b in range(nq):
        live = np.flatnonzero(keys[b] != empty)
        order = live[np.argsort(keys[b][live], kind="stable")][:k]
        assert ocnt[b] == min(live.size, k) == order.size
        assert np.array_equal(ok[b, :order.size], keys[b][order]) and np.array_equal(orow[b, :order.size], pay[b, order, 0])
        assert np.array_equal(oraw[b, :order.size], pay[b, order, 1])
        assert (orow[b, order.size:] == SENT32).all() and (oraw[b, order.size:] == SENT32).all()
    assert np.array_equal(cc_out, cc) and np.array_equal(tau_out, bits(tau)) and st_out == 0x5A and st_after == 0
    # without the export words, and with the threshold not wanted
    ok2 = probe.batch_select(keys, pay, k)[0]
    assert np.array_equal(ok2, ok)
    res = probe.batch_select(keys, pay, k, export=(cc, None, 3))
    assert np.array_equal(res[4], cc) and (res[5] == SENT32).all() and res[6] == 3 and res[7] == 0


# ==== the probe's own refusals (by return code: nothing is launched) =====================================================
def test_probe_refuses_what_a_kernel_would_index_out_of_bounds(probe):
    cs = case("gaussian", 549, 64, 64)
    bad = HIP_INVALID_VALUE
    for kernel in KERNELS:
        tr = probe.tile_rows[kernel]
        rows = round_up(549, tr)
        kw = dict(sample_rows=rows)
        cs.launch(probe, kernel, DENSE, False, 2, expect=bad, force_n_total=0, **kw)                          # n_total >= 1
        cs.launch(probe, kernel, DENSE, False, 2, n=rows + 1, expect=bad, sample_rows=rows + tr)        # a tile that starts past n_total
        cs.launch(probe, kernel, DENSE, False, 2, n=rows, sample_stride=2, expect=bad, **kw)            # ... through the stride
        cs.launch(probe, kernel, DENSE, False, 2, expect=bad, sample_rows=rows - 1)                     # sample slots
        cs.launch(probe, kernel, DENSE, True, 2, expect=bad, force_xnorm_len=549, **kw)                       # the norm column's padding
        cs.launch(probe, kernel, DENSE, False, 2, expect=bad, force_nq_pad=48, **kw)
        cs.launch(probe, kernel, DENSE, False, 2, expect=bad, force_ld=96, **kw)
        cs.launch(probe, kernel, DENSE, False, 0, expect=bad, **kw)
        tau = np.zeros(64, np.float32)
        cs.launch(probe, kernel, PASS, False, 2, tau=tau, cand_cap=8, expect=bad, force_cand_len=64 * 8 - 1)
        cs.launch(probe, kernel, PASS, False, 2, tau=tau, cand_cap=8, expect=bad, force_tau_len=63)
        cs.launch(probe, kernel, PASS, False, 2, tau=tau, cand_cap=8, expect=bad, force_count_len=63)
        cs.launch(probe, kernel, PASS, False, 2, tau=tau, cand_cap=0, expect=bad)
        if kernel == K2S:
            cs.launch(probe, kernel, DENSE, False, 2, expect=bad, force_shadow_elems=549 * 64, **kw)
            cs.launch(probe, kernel, DENSE, False, 2, expect=bad, stages=3, **kw)
            cs.launch(probe, kernel, DENSE, False, 2, expect=bad, force_qimage_bytes=1024, **kw)
        else:
            cs.launch(probe, kernel, DENSE, False, 2, expect=bad, force_x_floats=549 * 64 - 1, **kw)
            cs.launch(probe, kernel, DENSE, False, 2, expect=bad, stride=32, **kw)
            cs.launch(probe, kernel, MAXIMA, False, 2, expect=bad, **kw)
        if kernel == K2:
            cs.launch(probe, kernel, DENSE, False, 2, expect=bad, force_q_floats=63 * 64, **kw)
    sample = np.zeros((4, 2049), np.float32)
    probe.sample_tau(1, sample, 4, 3, expect=bad)                      # groups <= 2048
    probe.sample_tau(0, sample, 5, 3, expect=bad)
    probe.sample_tau(0, sample, 4, 0, expect=bad)
    probe.sample_tau(0, np.zeros((1, 65537), np.float32), 1, 3, expect=bad)
    keys, pay = np.zeros((2, 4097), np.uint64), np.zeros((2, 4097, 2), np.uint32)
    probe.batch_select(keys, pay, 4, expect=bad)                       # m <= 4096
    probe.q_image(K2B, cs.Q, 64, 64, image_bytes=1024, expect=bad)
    probe.q_image(K2, cs.Q, 64, 64, expect=bad)
    probe.shadow_build(cs.xbuf, 64, 549, 512, 64, expect=bad)          # rows_src <= rows_img
    probe.shadow_build(cs.xbuf, 64, 549, 600, 64, expect=bad)          # whole block tiles
    probe.shadow_rows(cs.xbuf, 64, [549], 549, 64, cs.shadow, expect=bad)
    probe.row_sqnorms(cs.xbuf, 64, 549, 64, np.zeros(549, np.float32), 0, rowlist=[549], expect=bad)
    probe.row_sqnorms(cs.xbuf, 64, 549, 64, np.zeros(548, np.float32), 0, expect=bad)
    assert probe.lib.vbp_magnitudes_ok(1, 1e18, 1.0) == 0 and probe.lib.vbp_magnitudes_ok(1, 9e17, 9e17) == 1


def test_zz_record_the_margins_room():
    """Not a check: where VT_BATCH_MARGINS_OUT names a file, the largest |error| / tolerance seen per kernel, metric family and
    input class goes there (profiles/batch_probe/margins.json is one run's) -- how much room the bound has."""
    out = os.environ.get("VT_BATCH_MARGINS_OUT")
    if out and MARGINS:
        with open(out, "w") as f:
            json.dump({k: float("%.4g" % v) for k, v in sorted(MARGINS.items())}, f, indent=1)
            f.write("\n")
