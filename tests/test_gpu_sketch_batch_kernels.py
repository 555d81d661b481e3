"""K1qm's two kernels on their own, against the numpy model of the int8 sketch and against K1q's kernels.

tests/test_gpu_sketch_batch.py shows that a batch's hits are the lone searches'.  Here the group pass
(vt_sketch_batch.hip) and the group tail (vt_sketch.hip) are launched through tests/sketch_batch_probe.cpp
(libvt_sketch_batch_probe.so: vt_sketch.hip, vt_sketch_batch.hip and nothing else of the library):

  A  the pass, for every query g of a group: (a) every retained entry's two words are the model's for that row, bit for
     bit; (b) the k' smallest keys of the whole corpus, by the model, are all retained somewhere; (c) every list equals the
     one launch_sketch_scan leaves for query g alone on the same grid -- and on another grid the two agree wherever both
     retained a row;
  B  the tail: block g's info, candidate count, Kt, candidate rows, status and result block are the lone tail's on query
     g's slice, and an outcome-1 block holds the oracle's top k with identical raw bits.

Shapes: N in {1, 63, 65, 300 (fewer tiles than waves), 4 100}, d in {1, 7, 100, 192, 768}; groups of 2, 3 and 8 (3 runs as
the pass compiled for 4), lists of 17, 26 and 64, all five metrics; rows uniform, unit, of spread norm, zero, tied and spiky.
One query of every group of three or more is a copy of the first, one is zero.
"""
import ctypes as C
import os

import numpy as np
import pytest

import sketch6_ref as ref6
import sketch8_l2_ref as refl
import sketch8_ref as ref8
import sketch_batch_cases as cases
from test_gpu_sketch_kernels import padded_dim, strided

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
SIZES = (1, 63, 65, 300, 4100)
DIMS = (1, 7, 100, 192, 768)
GROUPS = (2, 3, 8)
LISTS = (17, 26, 64)


class Probe:
    def __init__(self):
        path = os.environ.get("VT_SKETCH_BATCH_PROBE_LIB") or os.path.join(ROOT, "vettore_amd", "lib", "libvt_sketch_batch_probe.so")
        assert os.path.exists(path), "build it with `make` (%s)" % os.path.basename(path)
        L = self.lib = C.CDLL(path)
        u8p, u32p, u64p, f32p, f64p, i32p = (C.POINTER(t) for t in (C.c_ubyte, C.c_uint32, C.c_uint64, C.c_float, C.c_double, C.c_int))
        L.vtb_image_bytes.restype = C.c_size_t
        L.vtb_image_bytes.argtypes = [C.c_uint32, C.c_uint32]
        L.vtb_compiled_group.restype = C.c_uint32
        L.vtb_compiled_group.argtypes = [C.c_uint32]
        L.vtb_multi_lds_bytes.restype = C.c_size_t
        L.vtb_multi_lds_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        L.vtb_build.argtypes = [C.c_int, f32p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, u8p, C.c_size_t, u64p]
        L.vtb_scan_both.argtypes = [u8p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int, u32p, u8p, C.c_size_t, C.c_uint32, f64p,
                                    C.c_uint32, C.c_uint32, C.c_uint32, u64p, u32p, u64p, u32p]
        L.vtb_tail.argtypes = [C.c_int, u64p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, f32p, C.c_size_t,
                               C.c_uint32, f32p, u32p, C.c_uint32, C.c_int, C.c_int, u32p, u32p, u32p, i32p, i32p, u64p, u32p, f32p]

    @staticmethod
    def _p(a, ctype):
        return a.ctypes.data_as(C.POINTER(ctype))

    def build(self, with_xx, x):
        n, d = x.shape
        stride, rows_img = padded_dim(d), (n + 63) // 64 * 64
        xbuf = strided(x, stride)
        img = np.zeros(self.lib.vtb_image_bytes(rows_img, d), np.uint8)
        mx = np.zeros(1, np.uint64)
        rc = self.lib.vtb_build(int(with_xx), self._p(xbuf, C.c_float), xbuf.size, stride, n, rows_img, d,
                                self._p(img, C.c_ubyte), img.size, self._p(mx, C.c_uint64))
        assert rc == 0, "vtb_build: hipError_t %d" % rc
        return img.reshape(rows_img // 64, ref8.chunks_of(d) + 1, 64, 16)

    def scan_both(self, img, n, d, metric, id_rank, qys, kp, blocks, lone_blocks):
        ng = len(qys)
        img = np.ascontiguousarray(img, np.uint8).reshape(-1)
        qimg = np.ascontiguousarray(np.stack([qy.image for qy in qys])).view(np.uint8).reshape(-1)
        par = np.array([[float(qy.t[0]), float(qy.t[1]), qy.qn, qy.eta, qy.kerr, qy.qq_lo, qy.qq_hi] for qy in qys], np.float64)
        rank = None if id_rank is None else np.ascontiguousarray(id_rank, np.uint32)
        mk, mp = np.zeros((ng, blocks, kp), np.uint64), np.zeros((ng, blocks, kp, 2), np.uint32)
        lk, lp = np.zeros((ng, max(lone_blocks, 1), kp), np.uint64), np.zeros((ng, max(lone_blocks, 1), kp, 2), np.uint32)
        rc = self.lib.vtb_scan_both(self._p(img, C.c_ubyte), img.size, n, d, metric, None if rank is None else self._p(rank, C.c_uint32),
                                    self._p(qimg, C.c_ubyte), qimg.size, ng, self._p(par, C.c_double), kp, blocks, lone_blocks,
                                    self._p(mk, C.c_uint64), self._p(mp, C.c_uint32), self._p(lk, C.c_uint64), self._p(lp, C.c_uint32))
        assert rc == 0, "vtb_scan_both: hipError_t %d" % rc
        return mk, mp, lk, lp

    def tail(self, group, keys, pay, k, cap, x, qs, id_rank, metric, order):
        ng, lists, kp = keys.shape
        n, d = x.shape
        stride = padded_dim(d)
        xbuf = strided(x, stride)
        qbuf = strided(np.asarray(qs, np.float32), stride)
        keys, pay = np.ascontiguousarray(keys, np.uint64), np.ascontiguousarray(pay, np.uint32)
        rank = None if id_rank is None else np.ascontiguousarray(id_rank, np.uint32)
        out = dict(rows=np.zeros((ng, cap), np.uint32), count=np.zeros(ng, np.uint32), info=np.zeros((ng, 4), np.uint32),
                   status=np.zeros(ng, np.int32), head=np.zeros((ng, 2), np.int32), keys=np.zeros((ng, k), np.uint64),
                   res_rows=np.zeros((ng, k), np.uint32), raw=np.zeros((ng, k), np.float32))
        rc = self.lib.vtb_tail(int(group), self._p(keys, C.c_uint64), self._p(pay, C.c_uint32), ng, lists, kp, k, cap,
                               self._p(xbuf, C.c_float), stride, n, self._p(qbuf, C.c_float),
                               None if rank is None else self._p(rank, C.c_uint32), d, metric, order,
                               self._p(out["rows"], C.c_uint32), self._p(out["count"], C.c_uint32), self._p(out["info"], C.c_uint32),
                               self._p(out["status"], C.c_int), self._p(out["head"], C.c_int), self._p(out["keys"], C.c_uint64),
                               self._p(out["res_rows"], C.c_uint32), self._p(out["raw"], C.c_float))
        assert rc == 0, "vtb_tail: hipError_t %d" % rc
        return out


@pytest.fixture(scope="module")
def probe():
    return Probe()


def test_the_probe_and_the_model_agree_on_the_pass_s_shape(probe):
    for ng in range(2, 9):
        assert probe.lib.vtb_compiled_group(ng) == cases.compiled_group(ng)
    for d in DIMS + (896, 897, 1536, 8192, 16128, 16129, 32768):
        for kp in LISTS + (65,):
            for group in (2, 4, 8):
                assert probe.lib.vtb_multi_lds_bytes(d, kp, group) == cases.lds_bytes(d, kp, group), (d, kp, group)


# ---- the rows and the queries ----------------------------------------------------------------------------------------------
def kernel_corpus(n, d, metric, seed):
    """Uniform rows with the others among them: unit rows, norms over 10^-3 .. 10^3, a zero row, five identical rows, rows
    with one spike (from five rows up; one row: a uniform one).  Unit rows throughout for the cosine metric."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    if n >= 5:
        at = rng.permutation(n)
        m = max(1, n // 8)
        x[at[:m]] = refl.unit(x[at[:m]])
        x[at[m:2 * m]] = (x[at[m:2 * m]] * 10.0 ** rng.uniform(-3, 3, (m, 1))).astype(np.float32)
        x[at[2 * m]] = 0.0
        x[at[2 * m + 1:2 * m + 1 + min(5, m)]] = x[at[2 * m + 1]]
        sp = at[3 * m + 1:4 * m + 1]
        x[sp, rng.integers(0, d, len(sp))] *= np.float32(1e3)
    if metric == cases.COS:
        x = refl.unit(x)
    return x


class Query(refl.Query):
    """The query as sketch_group_search hands it to the pass: the L2 family's with kerr = 0, the dot family's with K1's
    summation term."""

    def __init__(self, q, metric):
        super().__init__(q)
        if metric in cases.DOT:
            self.kerr = 8.0 * len(self.q) * 2.0 ** -24


def group_queries(ng, x, metric, seed):
    rng = np.random.default_rng(seed)
    d = x.shape[1]
    qs = rng.uniform(-1, 1, (ng, d)).astype(np.float32)
    qs[0] = x[len(x) // 2]
    if ng >= 3:
        qs[ng - 1] = qs[0]   # two identical queries
        qs[1] = 0.0          # a zero query
    if metric == cases.COS:
        qs = refl.unit(qs)
    return qs


def model_words(metric, img, n, d, qy):
    """The two words of every row for one query, from the DEVICE's column (its rho, nu and xx are inputs here: the builders
    have tests of their own)."""
    if metric in cases.DOT:
        X, s, rho, nu = ref8.unpack_tiles(img, n, d)[:4]
        return ref8.pass_words(metric, X, s, rho, nu, qy.Q, qy.t, qy.qn, qy.eta, qy.kerr)
    X, s, rho, nu, xx = refl.unpack_tiles(img, n, d)
    return refl.pass_words(metric, X, s, rho, nu, xx, qy)


def entries(keys, pay):
    """{row: (key, key(lo) word)} of the live slots of one query's lists."""
    live = keys != EMPTY_KEY
    rows = pay[..., 0][live]
    assert len(set(rows.tolist())) == len(rows), "a row retained twice"
    return dict(zip(rows.tolist(), zip(keys[live].tolist(), pay[..., 1][live].tolist())))


def shapes():
    """Every N with every d, the group size and the list length rotating through them, then the two extremes."""
    out = []
    for i, n in enumerate(SIZES):
        for j, d in enumerate(DIMS):
            out.append((n, d, GROUPS[(i + j) % 3], LISTS[(i + 2 * j) % 3]))
    # and the largest LDS layouts outright: eight queries with lists of 64 at d = 768, and at d = 896 -- the longest rows a
    # group of eight takes (eight images of 1 792 bytes beside 64 KiB of wave buffers)
    out += [(4100, 768, 8, 64), (300, 896, 8, 64)]
    return out


# ---- A. the pass -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", cases.METRICS)
def test_the_group_pass_leaves_every_query_the_lone_pass_s_lists(probe, metric):
    for n, d, ng, kp in shapes():
        what = "metric %d n %d d %d group %d lists %d" % (metric, n, d, ng, kp)
        rng = np.random.default_rng(n + d + ng)
        x = kernel_corpus(n, d, metric, 9100 + n + d)
        img = probe.build(metric not in cases.DOT, x)
        qys = [Query(q, metric) for q in group_queries(ng, x, metric, 9200 + n + d)]
        id_rank = None if n == 63 else rng.permutation(n).astype(np.uint32)
        rank = np.arange(n, dtype=np.uint64) if id_rank is None else id_rank.astype(np.uint64)
        tiles = (n + 63) // 64
        blocks = 1 if tiles < 5 else 2 if tiles < 60 else 5   # (300 rows: 5 tiles on 8 waves; 4 100: three or four tiles a wave)
        other = 0 if n < 4100 else 7                # the lone pass on another grid as well
        mk, mp, lk, lp = probe.scan_both(img, n, d, metric, id_rank, qys, kp, blocks, blocks)
        for g, qy in enumerate(qys):
            first, second = model_words(metric, img, n, d, qy)
            want_key = (first.astype(np.uint64) << np.uint64(32)) | rank
            got = entries(mk[g], mp[g])
            # (a) the model's words, row by row
            for row, (key, raw) in got.items():
                assert key == int(want_key[row]), (what, g, row, "key(hi) word or id rank")
                assert int(ref6.orderable(np.array([raw], np.uint32).view(np.float32))[0]) == int(second[row]), (what, g, row, "key(lo) word")
            # (b) the k' smallest keys of the whole corpus are retained
            best = np.argsort(want_key, kind="stable")[:kp]
            assert set(best.tolist()) <= set(got), (what, g)
            # (c) the lone pass on the same grid: the same lists, slot contents as sets per block
            for b in range(blocks):
                assert entries(mk[g, b], mp[g, b]) == entries(lk[g, b], lp[g, b]), (what, g, b)
            # every list is full or holds all its block's rows; nothing lives past the group's queries
            assert len(got) == sum(min(kp, int((refl.owner_blocks(n, blocks) == b).sum())) for b in range(blocks)), (what, g)
        if other:
            _, _, lk2, lp2 = probe.scan_both(img, n, d, metric, id_rank, qys, kp, blocks, other)
            for g in range(ng):
                a, b = entries(mk[g], mp[g]), entries(lk2[g], lp2[g])
                both = set(a) & set(b)
                assert len(both) >= kp and all(a[r] == b[r] for r in both), (what, g)
        if ng >= 3:  # the two identical queries leave identical lists
            assert np.array_equal(mk[0], mk[ng - 1]) and np.array_equal(mp[0], mp[ng - 1]), what


# ---- B. the tail -----------------------------------------------------------------------------------------------------------
def oracle_block(oracle_mod, metric, q, x, rank, k):
    """K1's value for every row, keyed and sorted as K1's select does: the search's answer."""
    raw = np.array([oracle_mod.compute(metric, q, r) for r in x], np.float32)
    word = raw if metric in (cases.L2, cases.L2SQ) else (np.float32(1.0) - raw if metric == cases.COS else
                                                         (-raw if metric == cases.IP else raw))
    key = (ref6.orderable(word.astype(np.float32)).astype(np.uint64) << np.uint64(32)) | rank
    order = np.argsort(key, kind="stable")[:k]
    return key[order], order.astype(np.uint32), raw[order]


TAIL_SHAPES = ((65, 7, 3, 1), (300, 100, 8, 10), (4100, 192, 2, 32), (63, 768, 8, 1), (300, 1, 3, 10), (4100, 100, 8, 10))


@pytest.mark.parametrize("metric", cases.METRICS)
def test_every_tail_block_is_the_lone_tail_on_its_slice(probe, oracle_mod, metric):
    order = oracle_mod.get_reduce_order()
    outcomes = set()
    for n, d, ng, k in TAIL_SHAPES:
        what = "metric %d n %d d %d group %d k %d" % (metric, n, d, ng, k)
        kp = cases.list_k(k)
        rng = np.random.default_rng(n + d + k)
        x = kernel_corpus(n, d, metric, 9300 + n + d)
        img = probe.build(metric not in cases.DOT, x)
        qs = group_queries(ng, x, metric, 9400 + n + d)
        qys = [Query(q, metric) for q in qs]
        id_rank = None if n == 63 else rng.permutation(n).astype(np.uint32)
        rank = np.arange(n, dtype=np.uint64) if id_rank is None else id_rank.astype(np.uint64)
        blocks = max(1, min((n + 63) // 64, 40))
        mk, mp, _, _ = probe.scan_both(img, n, d, metric, id_rank, qys, kp, blocks, 0)
        cap = refl.CAND_CAP
        grp = probe.tail(1, mk, mp, k, cap, x, qs, id_rank, metric, order)
        one = probe.tail(0, mk, mp, k, cap, x, qs, id_rank, metric, order)
        for g in range(ng):
            outcome, cnt, kt = (int(v) for v in grp["info"][g][:3])
            assert list(grp["info"][g]) == list(one["info"][g]), (what, g, list(grp["info"][g]), list(one["info"][g]))
            assert grp["count"][g] == one["count"][g] == (cnt if outcome else 0), (what, g)
            assert grp["status"][g] == one["status"][g] == 0, (what, g)
            # the model's certificate on the same lists: the same Kt, count and outcome
            hi = np.where(mk[g] == EMPTY_KEY, refl.EMPTY, (mk[g] >> np.uint64(32)).astype(np.uint32)).reshape(-1)
            lo = np.where(mk[g] == EMPTY_KEY, refl.EMPTY, ref6.orderable(mp[g][:, :, 1].copy().view(np.float32))).reshape(-1)
            cert = refl.certify(lo, hi, mp[g][:, :, 0].reshape(-1), blocks, kp, k)
            assert [outcome, cnt, kt] == [refl.tail_outcome(cert, blocks, kp, d), cert["cnt"], cert["kt"]], (what, g)
            if outcome:
                assert np.array_equal(np.sort(grp["rows"][g][:cnt]), cert["rows"]), (what, g)
                assert np.array_equal(np.sort(one["rows"][g][:cnt]), cert["rows"]), (what, g)
            if outcome == 1:
                m = int(grp["head"][g][1])
                assert list(grp["head"][g]) == list(one["head"][g]) == [0, min(k, n)], (what, g, list(grp["head"][g]))
                for name in ("keys", "res_rows", "raw"):
                    assert grp[name][g][:m].tobytes() == one[name][g][:m].tobytes(), (what, g, name)
                if n <= 300:  # the oracle's top k of ALL rows, raw bits included
                    wkey, wrows, wraw = oracle_block(oracle_mod, metric, qs[g], x, rank, k)
                    assert np.array_equal(grp["keys"][g][:m], wkey), (what, g)
                    assert np.array_equal(grp["res_rows"][g][:m], wrows), (what, g)
                    assert grp["raw"][g][:m].tobytes() == wraw.tobytes(), (what, g)
        outcomes |= set(int(v) for v in grp["info"][:, 0])
    assert 1 in outcomes, outcomes  # (blocks did rescore)
