"""K1n's kernels against their numpy model, row by row, as test_gpu_sketch_kernels.py has the other three
sketches': launched through tests/sketch4_probe.cpp (libvt_sketch4_probe.so: vt_sketch.hip, vt_sketch4.hip and nothing else
of the library), and what no search returns is read back:

  A  the builders' images, byte for byte against sketch4_ref.pack_tiles, and rho / nu against the exact norms;
  B  the pass's lists and word arrays: every row's two words equal the model's (sketch4_ref.pass_words) bit for bit and hold
     the oracle's f32 rank value, with one list per tile (every row read out) and with one block walking ten tiles;
  C  the chain behind the pass with the exact threshold (sketch_thresh_kernel filing slots, sketch_refine_kernel,
     sketch_collect_kernel taking the published word) on synthetic arrays: the k rows picked, Kt' against a numpy
     restatement on the oracle's dot in each reduce order, the candidates, and the state two calls share.

Geometry of B.  The pass numbers its waves across the blocks first (wave = wave-in-block * blocks + block) and leaves two
lists a block, waves 0-1 and waves 2-3: tile t goes to wave w = t mod 4 blocks, which is wave-in-block w div blocks of block
w mod blocks.  With blocks = tiles every tile has the first list of its block to itself and the second lists stay empty.
"""
import ctypes as C
import os

import numpy as np
import pytest

import sketch4_ref as ref4
import sketch6_ref as ref6
from test_gpu_sketch_kernels import (COS, EMPTY, EMPTY_KEY, IP, NIP, Query, assert_band, assert_sound, builder_corpus, edge_rows,
                                     exact_norms, lean_rows, max_norm_bits, padded_dim, strided)
from test_sketch5_model import corpora, unit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = 7
KP = 64


class Probe4:
    def __init__(self):
        path = os.environ.get("VT_SKETCH4_PROBE_LIB") or os.path.join(ROOT, "vettore_amd", "lib", "libvt_sketch4_probe.so")
        assert os.path.exists(path), "build it with `make` (%s)" % os.path.basename(path)
        L = self.lib = C.CDLL(path)
        u8p, u32p, u64p, f32p = C.POINTER(C.c_ubyte), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
        L.vtp4_image_bytes.restype = C.c_size_t
        L.vtp4_image_bytes.argtypes = [C.c_uint32, C.c_uint32]
        L.vtp4_thresh_blocks.restype = C.c_uint32
        L.vtp4_thresh_blocks.argtypes = [C.c_uint32, C.c_uint32]
        L.vtp4_block_lists.restype = C.c_uint32
        L.vtp4_build.argtypes = [f32p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, u8p, C.c_size_t, u64p]
        L.vtp4_rows.argtypes = [f32p, C.c_size_t, C.c_size_t, u32p, C.c_uint32, C.c_uint32, C.c_uint32, u8p, C.c_size_t, u64p]
        L.vtp4_scan.argtypes = [u8p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int, u32p, u8p, C.c_size_t, f32p, C.c_double, C.c_double,
                                C.c_double, C.c_uint32, C.c_uint32, u64p, u32p, u32p, u32p]
        L.vtp4_certify.argtypes = [u32p, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, f32p, C.c_size_t, C.c_size_t,
                                   C.c_uint32, f32p, C.c_uint32, C.c_int, C.c_int, C.c_uint32] + [u32p] * 7
        assert L.vtp4_block_lists() == 2

    @staticmethod
    def _p(a, ctype):
        return a.ctypes.data_as(C.POINTER(ctype))

    def build(self, xbuf, stride, n_src, rows_img, d):
        img = np.zeros(self.lib.vtp4_image_bytes(rows_img, d), np.uint8)
        mx = np.zeros(1, np.uint64)
        rc = self.lib.vtp4_build(self._p(xbuf, C.c_float), xbuf.size, stride, n_src, rows_img, d, self._p(img, C.c_ubyte), img.size,
                                 self._p(mx, C.c_uint64))
        assert rc == 0, "vtp4_build: hipError_t %d" % rc
        return img, int(mx[0])

    def rows(self, xbuf, stride, rowlist, rows_img, d, img, max_norm):
        img = img.copy()
        mx = np.array([max_norm], np.uint64)
        rowlist = np.ascontiguousarray(rowlist, np.uint32)
        rc = self.lib.vtp4_rows(self._p(xbuf, C.c_float), xbuf.size, stride, self._p(rowlist, C.c_uint32), rowlist.size, rows_img, d,
                                self._p(img, C.c_ubyte), img.size, self._p(mx, C.c_uint64))
        assert rc == 0, "vtp4_rows: hipError_t %d" % rc
        return img, int(mx[0])

    def scan(self, img, n, d, metric, id_rank, qy, k, blocks, expect=0):
        img = np.ascontiguousarray(img, np.uint8).reshape(-1)
        qimg = np.ascontiguousarray(qy.image).view(np.uint8).reshape(-1)
        t = np.ascontiguousarray(qy.t, np.float32)
        lists = 2 * blocks
        keys = np.zeros((lists, k), np.uint64)
        pay = np.zeros((lists, k, 2), np.uint32)
        lo, hi = np.zeros((lists, k), np.uint32), np.zeros((lists, k), np.uint32)
        rank = None if id_rank is None else np.ascontiguousarray(id_rank, np.uint32)
        rc = self.lib.vtp4_scan(self._p(img, C.c_ubyte), img.size, n, d, metric, None if rank is None else self._p(rank, C.c_uint32),
                                self._p(qimg, C.c_ubyte), qimg.size, self._p(t, C.c_float), qy.qn, qy.eta, qy.kerr, k, blocks,
                                self._p(keys, C.c_uint64), self._p(pay, C.c_uint32), self._p(lo, C.c_uint32), self._p(hi, C.c_uint32))
        assert rc == expect, "vtp4_scan: hipError_t %d" % rc
        return keys, pay, lo, hi

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


def pack(X, s, rho, nu):
    return ref4.pack_tiles(X, s, rho, nu).view(np.uint8).reshape(-1)


def unpack(img, n, d):
    tiles = img.size // (ref4.runs_of(d) * 1024)
    return ref4.unpack_tiles(img.view(np.uint32).reshape(tiles, -1, 64, 4), n, d)


def check_image(img, x, n_src, rows_img, d, what):
    """The image of rows_img rows equals the model's of x[:n_src] byte for byte, rho and nu apart, which lie in the band."""
    Xm, sm, _, _ = ref4.quantise_rows(x[:n_src])
    assert img.size == ref4.runs_of(d) * 1024 * rows_img // 64
    Xd, sd, rhod, nud = unpack(img, n_src, d)
    assert np.array_equal(Xd, Xm), what
    assert np.array_equal(sd.view(np.uint32), sm.view(np.uint32)), what
    R, N = exact_norms(x[:n_src], Xm, sm)
    assert_band(rhod, R, what + " rho")
    assert_band(nud, N, what + " nu")
    want = np.zeros(img.size, np.uint8)  # (padding columns, rows at or past n_src, the fourth metadata word: all zero)
    model = pack(Xm, sm, rhod, nud)
    want[:model.size] = model
    assert np.array_equal(img, want), (what, np.nonzero(img != want)[0][:8])
    return rhod, nud


# ---- A. the builders -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [200, 256, 768, 8320])
def test_builders_write_the_models_image(probe, d):
    """d = 8320: 260 runs, so a lane takes a fifth turn of the per-row loop; n_src below, at and past a tile's end, an empty
    tile beyond, a stride wider than the row."""
    full = builder_corpus(d, HALF, 130)
    shapes = [(65, 128, 0), (130, 192, 64)] if d == 8320 else [(1, 64, 0), (63, 64, 64), (64, 64, 0), (130, 192, 64), (65, 192, 0)]
    for n_src, rows_img, extra in shapes:
        x = full[:n_src] if n_src == 130 else np.concatenate([edge_rows(d, HALF), full])[:n_src]
        stride = padded_dim(d) + extra
        what = "d %d n_src %d rows_img %d stride %d" % (d, n_src, rows_img, stride)
        img, mx = probe.build(strided(x, stride), stride, n_src, rows_img, d)
        rhod, nud = check_image(img, x, n_src, rows_img, d, what)
        assert mx == max_norm_bits(rhod, nud), what


def test_builders_patch_rows_in_place(probe):
    d, n, rows_img = 320, 130, 192
    stride = padded_dim(d) + 64
    old = builder_corpus(d, HALF, n)
    img0, mx0 = probe.build(strided(old, stride), stride, n, rows_img, d)
    rng = np.random.default_rng(71 + d)
    new = old.copy()
    touched = np.array([77, 0, 129, 64, 63, 5, 100])
    new[touched] = (rng.uniform(-1, 1, (len(touched), d)) * 3.0).astype(np.float32)
    new[5] = edge_rows(d, HALF)[6]
    rowlist = np.array([77, 0, rows_img, 129, 64, 0xFFFFFFF0, 63, 5, rows_img + 63, 100], np.uint32)  # (>= rows_img: ignored)
    img1, mx1 = probe.rows(strided(new, stride), stride, rowlist, rows_img, d, img0, mx0)
    rhod, nud = check_image(img1, new, n, rows_img, d, "rows")
    keep = np.setdiff1d(np.arange(n), touched)
    for before, after in zip(unpack(img0, n, d), unpack(img1, n, d)):
        assert before[keep].tobytes() == after[keep].tobytes()
    assert mx1 == max(mx0, max_norm_bits(rhod[touched], nud[touched]))


# ---- B. the pass -----------------------------------------------------------------------------------------------------------
def owner_list(tile, blocks):
    w = tile % (4 * blocks)
    return 2 * (w % blocks) + (w // blocks) // 2


def run_scan(probe, img, n, d, metric, id_rank, qy, k, blocks):
    """One launch; every list checked slot by slot against the model: it is exactly the k smallest (key(hi) word, id rank)
    keys of the rows it owns, with both model words, and every other slot is empty.  {row: (first word, second word)}."""
    X, s, rho, nu = unpack(img, n, d)
    first, second = ref4.pass_words(metric, X, s, rho, nu, qy.Q, qy.t, qy.qn, qy.eta, qy.kerr)
    assert np.all(first <= second)
    rank = np.arange(n, dtype=np.uint64) if id_rank is None else id_rank.astype(np.uint64)
    key = (first.astype(np.uint64) << np.uint64(32)) | rank
    keys, pay, lo, hi = probe.scan(img, n, d, metric, id_rank, qy, k, blocks)
    owner = np.array([owner_list(r // 64, blocks) for r in range(n)])
    seen = {}
    for b in range(2 * blocks):
        mine = np.nonzero(owner == b)[0]
        want = mine[np.argsort(key[mine], kind="stable")][:k]
        live = keys[b] != EMPTY_KEY
        assert live.sum() == len(want), (b, live.sum(), len(want))
        assert np.all(lo[b][~live] == EMPTY) and np.all(hi[b][~live] == EMPTY), b
        assert np.array_equal(hi[b][live], (keys[b][live] >> np.uint64(32)).astype(np.uint32)), b
        assert np.array_equal(lo[b][live], ref6.orderable(pay[b][live][:, 1].copy().view(np.float32))), b
        order = np.argsort(keys[b][live], kind="stable")
        assert np.array_equal(pay[b][live][:, 0][order], want), (b, pay[b][live][:, 0][order][:8], want[:8])
        assert np.array_equal(keys[b][live][order], key[want]), (b, "key(hi) words or id ranks differ from the model's")
        got_second = lo[b][live][order]
        assert np.array_equal(got_second, second[want]), (b, "key(lo) words differ from the model's")
        for r, f2, s2 in zip(want, hi[b][live][order], got_second):
            assert int(r) not in seen
            seen[int(r)] = (int(f2), int(s2))
    return seen


def pass_corpus(d, metric, q, n):
    """The model tests' corpora, the builders' edge rows and the rows that lean on the bound; n rows: n = 64 m + 37."""
    rng = np.random.default_rng(4000 + 10 * d + 4)
    parts = [c[:48] for c in corpora(d, n=48, seed=4).values()]
    if metric != COS:
        parts = [(p * rng.uniform(0.05, 24, (len(p), 1)).astype(np.float32)).astype(np.float32) for p in parts]
    huge = sum(len(p) for p in parts) + 2  # (edge_rows' third row)
    parts.append(edge_rows(d, HALF))
    parts.append(lean_rows(q, HALF, 32, rng, 1.7 / np.sqrt(d) if metric == COS else 3.0))
    x = np.concatenate(parts)
    assert len(x) >= n > huge
    assert np.abs(x[huge]).max() > 1e38
    return x[:n], huge


@pytest.mark.parametrize("d", [256, 200, 768])
def test_the_pass_gives_every_row_the_models_interval(probe, oracle_mod, d):
    """d = 256 is the smallest the path takes (nine loads a tile), d = 200 has padding and K1's scalar tail, d = 768 is the
    headline's.  n = 64 * 3 + 37: the last tile is partial.  A list per tile: each row's words equal the model's bit for bit
    and hold K1's rank value, for the three metrics, id ranks absent and permuted, the host's levels and arbitrary ones."""
    rng = np.random.default_rng(600 + d + 4)
    q_unit = unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0]
    n = 64 * 3 + 37
    for metric in (COS, IP, NIP):
        q = q_unit if metric == COS else (q_unit * np.float32(7.5)).astype(np.float32)
        x, huge = pass_corpus(d, metric, q, n)
        X, s, rho, nu = ref4.quantise_rows(x)
        img = pack(X, s, rho, nu)
        perm = rng.permutation(n).astype(np.uint32)
        for i, (qy, id_rank) in enumerate([(Query(6, q), None), (Query(6, q, arbitrary=rng), perm),
                                           (Query(6, (-x[7]).astype(np.float32)), perm)]):
            seen = run_scan(probe, img, n, d, metric, id_rank, qy, 64, 4)
            assert sorted(seen) == list(range(n))
            assert_sound(oracle_mod, seen, metric, qy, x, rho.astype(np.float64) + nu.astype(np.float64),
                         "d %d metric %d query %d" % (d, metric, i), exempt=[huge])


@pytest.mark.parametrize("d", [256, 200, 768])
def test_the_pass_walks_from_tile_to_tile(probe, d):
    """One block, ten tiles, the last partial (n = 64 * 9 + 37): waves 0-3 own tiles {0, 4, 8}, {1, 5, 9}, {2, 6}, {3, 7};
    list 0 is the 64 smallest of waves 0-1's rows, list 1 of waves 2-3's -- each wave walks from a tile into the next through
    its load ring, its parked sums and its metadata run (9, 9 and 25 runs a tile: never a multiple of the ring of 8).  Then
    three blocks over the same image."""
    assert ref4.runs_of(d) % 8 != 0
    n = 64 * 9 + 37
    rng = np.random.default_rng(8800 + d)
    x = unit(rng.uniform(-1, 1, (n, d)).astype(np.float32))
    e = edge_rows(d, HALF, seed=1)
    x[np.arange(len(e)) * 67 % n] = e
    x[[3, 64 * 6 + 9, n - 2]] = unit(rng.uniform(-1, 1, (3, d)).astype(np.float32))
    img = pack(*ref4.quantise_rows(x))
    perm = rng.permutation(n).astype(np.uint32)
    for i, q in enumerate((x[3], x[64 * 6 + 9], x[n - 2], -x[3])):
        qy = Query(6, q)
        for metric, id_rank in ((COS, None), (IP, perm)) if i < 3 else ((NIP, perm),):
            seen = run_scan(probe, img, n, d, metric, id_rank, qy, 64, 1)
            assert len(seen) == 128
            if i < 3:  # (the query's own row -- first tile, a second-turn tile of waves 2-3, the last, partial tile)
                assert (3, 64 * 6 + 9, n - 2)[i] in seen, (i, metric)
    seen = run_scan(probe, img, n, d, COS, perm, Query(6, x[64 * 6 + 9]), 64, 3)
    assert len(seen) == 6 * 64  # (twelve waves: lists of tiles {0, 3}, {6, 9}, {1, 4}, {7}, {2, 5}, {8}, each returns its 64 smallest)


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
