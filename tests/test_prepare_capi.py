"""vt_prepare_rows, vt_normalize_zscore and vt_normalize_minmax at the C ABI, the part that needs no device: the mode
and the finiteness of every row are checked on the host before any device is touched (the arithmetic itself:
tests/test_gpu_prepare.py)."""
import ctypes as C

import numpy as np
import pytest

from vettore_amd import _lib

VT_OK, VT_ERR_NON_FINITE, VT_ERR_ARGUMENT = 0, 3, 19
MODES = {"none": 0, "l2": 1, "zscore": 2, "minmax": 3}
F32P, U64P = C.POINTER(C.c_float), C.POINTER(C.c_uint64)


def _call(mode, matrix, with_words=True):
    L = _lib.load()
    m = np.ascontiguousarray(matrix, dtype=np.float32)
    count, d = m.shape
    out = np.full((count, d), 7.5, dtype=np.float32)
    words = np.full((count, (d + 63) // 64), 0xABCD, dtype=np.uint64)
    first = C.c_size_t(12345)
    st = L.vt_prepare_rows(0, mode, count, d, m.ctypes.data_as(F32P), out.ctypes.data_as(F32P),
                           words.ctypes.data_as(U64P) if with_words else None, C.byref(first))
    return st, int(first.value), out, words


def test_mode_codes_are_the_headers():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vettore_flat.h")).read()
    assert "enum { VT_NORM_NONE = 0, VT_NORM_L2 = 1, VT_NORM_ZSCORE = 2, VT_NORM_MINMAX = 3 };" in header
    from vettore_amd import nifs
    assert nifs.NORM_MODES == MODES


@pytest.mark.parametrize("mode", [-1, 4, 99])
def test_unknown_mode_is_a_bad_argument(mode):
    st, _, out, words = _call(mode, np.ones((4, 3)))
    assert st == VT_ERR_ARGUMENT
    assert (out == 7.5).all() and (words == 0xABCD).all()
    # ... before the rows are looked at
    bad = np.ones((4, 3), dtype=np.float32)
    bad[2, 1] = np.nan
    assert _call(mode, bad)[0] == VT_ERR_ARGUMENT
    L = _lib.load()
    assert L.vt_prepare_device_rows(0, mode, 4, 3, 3, None, 3, None, None, None) == VT_ERR_ARGUMENT


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_non_finite_row_is_refused_on_the_host_with_its_index(mode, poison):
    m = np.arange(20, dtype=np.float32).reshape(4, 5)
    m[2, 3] = poison
    m[3, 0] = poison   # (a later one: the smallest refused row is the answer)
    for with_words in (True, False):
        st, first, out, words = _call(MODES[mode], m, with_words)
        assert st == VT_ERR_NON_FINITE and first == 2
        assert (out == 7.5).all() and (words == 0xABCD).all()   # nothing written
    assert _lib.error_text(VT_ERR_NON_FINITE) == "vector contains a non-finite value"


@pytest.mark.parametrize("name", ["vt_normalize_zscore", "vt_normalize_minmax"])
@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_the_two_normalize_entry_points_refuse_before_any_device_is_touched(name, poison):
    fn = getattr(_lib.load(), name)
    m = np.ones((4, 6), dtype=np.float32)
    m[2, 5] = poison
    out = np.full((4, 6), 7.5, dtype=np.float32)
    assert fn(0, 4, 6, m.ctypes.data_as(F32P), out.ctypes.data_as(F32P)) == VT_ERR_NON_FINITE
    assert (out == 7.5).all()
    # device 10 000 does not exist: a call that reached for it would answer "device error", not status 3
    assert fn(10000, 4, 6, m.ctypes.data_as(F32P), out.ctypes.data_as(F32P)) == VT_ERR_NON_FINITE


@pytest.mark.parametrize("mode", sorted(MODES))
def test_empty_batches_and_empty_rows_are_ok_and_write_nothing(mode):
    L = _lib.load()
    for count, d in ((0, 5), (3, 0), (0, 0)):
        st, first, out, words = _call(MODES[mode], np.zeros((count, d), dtype=np.float32))
        assert st == VT_OK and first == count
    one = np.ones(4, dtype=np.float32)
    for fn in (L.vt_normalize_zscore, L.vt_normalize_minmax):
        assert fn(0, 0, 4, one.ctypes.data_as(F32P), one.ctypes.data_as(F32P)) == VT_OK
        assert fn(0, 1, 0, None, None) == VT_OK
    assert L.vt_prepare_device_rows(0, MODES[mode], 0, 4, 4, None, 4, None, None, None) == VT_OK
    assert L.vt_prepare_device_rows(0, MODES[mode], 5, 0, 0, None, 0, None, None, None) == VT_OK


def test_missing_buffers_are_bad_arguments():
    L = _lib.load()
    one = np.ones(4, dtype=np.float32)
    assert L.vt_prepare_rows(0, 1, 1, 4, None, one.ctypes.data_as(F32P), None, None) == VT_ERR_ARGUMENT
    assert L.vt_prepare_rows(0, 1, 1, 4, one.ctypes.data_as(F32P), None, None, None) == VT_ERR_ARGUMENT
    assert L.vt_abi_version() == 4
