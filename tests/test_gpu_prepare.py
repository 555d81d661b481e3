"""K14 "prepare rows" on the device: the kernel through vt_prepare_device_rows on torch tensors, the host form through
vt_prepare_rows, and the pipeline into an index.  Every comparison is tobytes() equality with tests/prepare_ref.py, the
model of distances.rs:350-423."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

import prepare_ref
import support

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = prepare_ref.MODES
# the kernel's tile, restated (csrc/vt_device.h): a test below holds the header to it
WAVE_ROWS, PANEL, BLOCK_ROWS = 64, 64, 128
NS = (1, 63, 64, 65, 130, BLOCK_ROWS - 1, BLOCK_ROWS + 1)
DS = (1, 3, PANEL - 1, PANEL, PANEL + 1, 2 * PANEL + 5)
MAX_N = max(NS)
FLT_MAX = np.float32(3.4028234663852886e38)
SENTINEL = np.float32(7.5)
WORD_SENTINEL = 0x0123456789ABCDEF


def test_the_restated_tile_is_the_kernels():
    text = open(os.path.join(ROOT, "vettore_amd", "csrc", "vt_device.h")).read()
    for name, value in (("kPrepWaveRows", WAVE_ROWS), ("kPrepPanel", PANEL), ("kPrepBlockRows", BLOCK_ROWS)):
        assert re.search(r"constexpr uint32_t %s = %d;" % (name, value), text), name


def contents(n, d, seed):
    """Rows of every kind the arithmetic can go wrong on, cycling: random, constant, all-zero, one huge value among small
    ones, [-FLT_MAX, FLT_MAX], subnormals, wide-range random.  (d == 1 makes every row a one-element row: z-score and
    minmax give 0.)  No row holds zeros of both signs: minmax stays pinned."""
    rng = np.random.default_rng(seed)
    m = np.empty((n, d), dtype=np.float32)
    for i in range(n):
        kind = i % 7
        if kind == 0:
            row = rng.standard_normal(d)
        elif kind == 1:
            row = np.full(d, rng.standard_normal())
        elif kind == 2:
            row = np.zeros(d)
        elif kind == 3:
            row = rng.standard_normal(d) * 1e-30
            row[rng.integers(d)] = 3e38
        elif kind == 4:
            row = np.where(np.arange(d) % 2 == 0, -FLT_MAX, FLT_MAX)
        elif kind == 5:
            row = rng.integers(-(2 ** 22), 2 ** 22, d) * np.float64(2.0 ** -149)
        else:
            row = rng.standard_normal(d) * 10.0 ** rng.integers(-30, 30, d)
        m[i] = row.astype(np.float32)
    assert all(prepare_ref.minmax_is_pinned(r) for r in m)
    return m


_REFERENCE = {}


def reference(d, mode):
    """(input, normalized, words) of MAX_N rows of length d, computed once: rows are independent, so the first n rows
    are the reference of every smaller batch."""
    if (d, mode) not in _REFERENCE:
        x = contents(MAX_N, d, 1000 + d)
        out, words = prepare_ref.prepare_rows(x, mode)
        for a in (x, out, words):
            a.setflags(write=False)
        _REFERENCE[d, mode] = (x, out, words)
    return _REFERENCE[d, mode]


def device_call(mode, x, ld, in_place, with_words):
    """One vt_prepare_device_rows call on a [n][ld] image of x whose padding columns hold NaN.
    Returns (result, out image, in image after the call, words or None)."""
    import torch
    from vettore_amd import nifs
    n, d = x.shape
    W = (d + 63) // 64
    host = np.full((n, ld), np.nan, dtype=np.float32)
    host[:, :d] = x
    t_in = torch.from_numpy(host.copy()).cuda()
    if in_place:
        t_out = t_in
    else:
        blank = np.full((n, ld), np.nan, dtype=np.float32)
        blank[:, :d] = SENTINEL
        t_out = torch.from_numpy(blank).cuda()
    t_words = torch.full((n, W), WORD_SENTINEL, dtype=torch.int64, device="cuda") if with_words else None
    torch.cuda.synchronize()
    res = nifs.prepare_device_rows(mode, n, d, t_in.data_ptr(), ld, t_out.data_ptr(), ld,
                                   t_words.data_ptr() if with_words else 0)
    words = t_words.cpu().numpy().view(np.uint64) if with_words else None
    return res, t_out.cpu().numpy(), t_in.cpu().numpy(), words


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", DS)
def test_kernel_shapes_are_bit_identical_to_the_model(d, mode):
    x_all, want_all, words_all = reference(d, mode)
    for n in NS:
        x, want, want_words = x_all[:n], want_all[:n], words_all[:n]
        for ld in (d, d + 3):
            for in_place in (False, True):
                for with_words in (True, False):
                    where = (n, d, ld, in_place, with_words)
                    res, out, after, words = device_call(mode, x, ld, in_place, with_words)
                    assert res == ("ok", ()), where
                    assert out[:, :d].tobytes() == want.tobytes(), where
                    # the padding columns are neither read (they hold NaN: a read would refuse the row) nor written
                    assert np.isnan(out[:, d:]).all() and np.isnan(after[:, d:]).all(), where
                    if not in_place:
                        assert after[:, :d].tobytes() == x.tobytes(), where
                    if with_words:
                        assert words.tobytes() == want_words.tobytes(), where


@pytest.mark.parametrize("mode", MODES)
def test_refused_rows_are_unwritten_and_all_others_written(mode):
    n, d = 2 * BLOCK_ROWS + 4, PANEL + 6
    x = contents(n, d, 77)
    want, want_words = prepare_ref.prepare_rows(x, mode)
    for poison in (np.nan, np.inf, -np.inf):
        for col in (0, d - 1):
            for rows in ((0,), (n - 1,), (BLOCK_ROWS + 70, 70), (WAVE_ROWS - 1, WAVE_ROWS)):
                bad = x.copy()
                for r in rows:
                    bad[r, col] = poison
                where = (mode, poison, col, rows)
                for in_place in (False, True):
                    res, out, _, words = device_call(mode, bad, d + 1, in_place, True)
                    assert res == ("error", "vector contains a non-finite value", min(rows)), where
                    for r in range(n):
                        if r in rows:
                            kept = bad[r] if in_place else np.full(d, SENTINEL)
                            assert out[r, :d].tobytes() == kept.tobytes(), (where, r)
                            assert (words[r] == np.uint64(WORD_SENTINEL)).all(), (where, r)
                    ok_rows = [r for r in range(n) if r not in rows]
                    assert out[ok_rows, :d].tobytes() == want[ok_rows].tobytes(), where
                    assert words[ok_rows].tobytes() == want_words[ok_rows].tobytes(), where


@pytest.mark.parametrize("mode", MODES)
def test_long_rows_carry_their_chains_across_many_panels(mode):
    """d = 12 panels and a tail, more rows than one block, 64-word flushes not reached -- and one row of 70 words
    (d = 4 480 - 3) that does reach a flush."""
    from vettore_amd import nifs
    for n, d in ((BLOCK_ROWS + 9, 12 * PANEL + 7), (3, 70 * 64 - 3)):
        x = contents(n, d, 5)
        want, want_words = prepare_ref.prepare_rows(x, mode)
        res, out, _, words = device_call(mode, x, d, False, True)
        assert res == ("ok", ())
        assert out.tobytes() == want.tobytes() and words.tobytes() == want_words.tobytes()
        res = nifs.prepare_rows(x, mode)
        assert res[0] == "ok" and res[1][0].tobytes() == want.tobytes() and res[1][1].tobytes() == want_words.tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_host_form_equals_the_model(mode):
    from vettore_amd import nifs
    for d in (1, 3, PANEL, 2 * PANEL + 5):
        x, want, want_words = reference(d, mode)
        res = nifs.prepare_rows(x, mode)
        assert res[0] == "ok"
        assert res[1][0].tobytes() == want.tobytes() and res[1][1].tobytes() == want_words.tobytes()
        fn = {"l2": nifs.normalize_l2, "zscore": nifs.normalize_zscore, "minmax": nifs.normalize_minmax}.get(mode)
        if fn is not None:
            for i in range(7):
                one = fn(x[i])
                assert one[0] == "ok" and one[1].tobytes() == want[i].tobytes()
    bad = np.array(reference(3, mode)[0][:6])
    bad[4, 1] = np.inf
    assert nifs.prepare_rows(bad, mode) == ("error", "vector contains a non-finite value", 4)


def _raw_host_call(mode, m, out, words):
    from vettore_amd import _lib
    first = C.c_size_t(0)
    st = _lib.load().vt_prepare_rows(0, prepare_ref.MODES.index(mode), m.shape[0], m.shape[1],
                                     m.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)),
                                     words.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(first))
    return st, int(first.value)


def test_chunk_boundaries(request):
    """200 rows through chunks of 67 (three chunks, a ragged last), 199 (the last chunk is exactly one row) and 1 (every
    chunk is one row); a refused row in the middle chunk leaves the caller's buffers untouched.  The chunk size shrinks
    only in the hooks build."""
    if support.rerun_with_hooks_library(request):
        return
    from vettore_amd import nifs
    n, d = 200, 70
    x = contents(n, d, 31)
    try:
        for chunk in (67, 199, 1):
            nifs.debug_set("test_prepare_chunk_rows", chunk)
            for mode in MODES:
                want, want_words = prepare_ref.prepare_rows(x, mode)
                res = nifs.prepare_rows(x, mode)
                assert res[0] == "ok", (chunk, mode)
                assert res[1][0].tobytes() == want.tobytes() and res[1][1].tobytes() == want_words.tobytes(), (chunk, mode)
        nifs.debug_set("test_prepare_chunk_rows", 67)
        bad = x.copy()
        bad[100, 5] = np.nan   # (the middle chunk: rows 67 .. 133)
        out = np.full((n, d), SENTINEL, dtype=np.float32)
        words = np.full((n, 2), WORD_SENTINEL, dtype=np.uint64)
        for mode in MODES:
            assert _raw_host_call(mode, bad, out, words) == (3, 100)
            assert (out == SENTINEL).all() and (words == np.uint64(WORD_SENTINEL)).all()
    finally:
        nifs.debug_set("test_prepare_chunk_rows", 0)


def test_the_product_library_has_no_chunk_switch():
    from vettore_amd import nifs
    if "hooks" in os.path.basename(os.environ.get("VETTORE_HIP_LIB", "")):
        return   # (a session pointed at the hooks build: nothing to say)
    with pytest.raises(KeyError):
        nifs.debug_set("test_prepare_chunk_rows", 3)


def test_back_to_back_calls_of_other_sizes_share_the_pooled_buffers():
    """The session's buffers grow and stay: a smaller call after a larger one must not see its tail, nor a larger one
    after a smaller one a short buffer."""
    from vettore_amd import nifs
    for n, d, mode in ((300, 133, "l2"), (5, 7, "zscore"), (400, 200, "minmax"), (2, 133, "none"), (300, 133, "zscore")):
        x = contents(n, d, n + d)
        want, want_words = prepare_ref.prepare_rows(x, mode)
        res = nifs.prepare_rows(x, mode)
        assert res[0] == "ok", (n, d, mode)
        assert res[1][0].tobytes() == want.tobytes() and res[1][1].tobytes() == want_words.tobytes(), (n, d, mode)


def test_four_threads_get_the_answers_of_calls_made_alone():
    from vettore_amd import nifs
    jobs = [(contents(90 + 37 * t, 60 + 11 * t, 400 + t), MODES[t]) for t in range(4)]
    alone = [nifs.prepare_rows(x, mode) for x, mode in jobs]
    for (x, mode), res in zip(jobs, alone):
        want, want_words = prepare_ref.prepare_rows(x, mode)
        assert res[0] == "ok" and res[1][0].tobytes() == want.tobytes() and res[1][1].tobytes() == want_words.tobytes()
    wrong = []

    def worker(t):
        x, mode = jobs[t]
        for _ in range(8):
            res = nifs.prepare_rows(x, mode)
            if res[0] != "ok" or res[1][0].tobytes() != alone[t][1][0].tobytes() or \
                    res[1][1].tobytes() != alone[t][1][1].tobytes():
                wrong.append(t)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert wrong == []


def test_pipeline_prepare_in_hbm_then_load_then_search(oracle_mod):
    """Raw rows in HBM -> vt_prepare_device_rows(l2) in place -> vt_flat_load_device_matrix into a cosine index -> search:
    hits and scores of the oracle index fed with the oracle's normalize_l2 of the same rows, bit for bit."""
    import torch
    from vettore_amd import nifs
    oracle = oracle_mod
    rng = np.random.default_rng(96)
    n, d = 2000, 96
    raw = rng.uniform(-1, 1, size=(n, d)).astype(np.float32)
    raw[100] = raw[7]
    ids = [b"doc-%d" % (i + 1) for i in range(n)]
    t = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    assert nifs.prepare_device_rows("l2", n, d, t.data_ptr(), d, t.data_ptr(), d) == ("ok", ())
    ref = nifs.flat_new_cosine()
    assert nifs.flat_load_device_matrix(ref, nifs._pack_ids(ids), t.data_ptr(), n, d) == ("ok", ())
    want_rows = np.stack([oracle.normalize_l2(r) for r in raw])
    assert t.cpu().numpy().tobytes() == want_rows.tobytes()
    for q in (oracle.normalize_l2(rng.uniform(-1, 1, d).astype(np.float32)), want_rows[7]):
        status, hits = nifs.flat_search(ref, q, 10)
        assert status == "ok"
        want = oracle.matrix_search(2, want_rows, oracle.pack_ids(ids), q, 10)
        assert [(h[0], np.float32(h[1]).tobytes()) for h in hits] == [(w[0], np.float32(w[1]).tobytes()) for w in want]
