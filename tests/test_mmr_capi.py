"""The MMR calls' C ABI (vt_mmr_rerank, vt_flat_mmr_*, include/vettore_flat.h) and their Python mirror without a GPU:
the names are declared, exported and bound, the new status carries its string, every call answers its arguments in the
documented order and only then looks for a device, count == 0 needs none."""
import ctypes as C
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vt_mmr_rerank", "vt_flat_mmr_rerank", "vt_flat_mmr_rerank_batch", "vt_flat_mmr_search", "vt_flat_mmr_search_batch"]
OK, EMPTY, NON_FINITE, UNKNOWN_METRIC, DEVICE, ARGUMENT, MMR_ARGS = 0, 1, 3, 5, 17, 19, 38


def lib():
    import vettore_amd._lib as L
    return L.load()


def test_every_new_name_is_declared_exported_and_bound():
    import vettore_amd._lib as L
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vettore_flat.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib(), name), name
        assert name in L.SYMBOLS, name
    assert lib().vt_abi_version() == 4
    assert re.search(r"\bVT_ERR_MMR_ARGS\s*=\s*38\b", header)


def test_the_new_status_carries_its_string():
    assert lib().vt_strerror(MMR_ARGS).decode() == "invalid mmr args"
    assert lib().vt_strerror(MMR_ARGS + 1).decode() == "unknown status"


def rerank(metric, rows, scores, alpha, final_k, device=0):
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n = len(scores)
    d = rows.shape[1] if rows.ndim == 2 else 0
    sc = np.ascontiguousarray(scores, dtype=np.float64)
    order = np.zeros(max(n, 1), dtype=np.uint32)
    count = C.c_size_t(77)
    st = lib().vt_mmr_rerank(device, metric, n, d, rows.ctypes.data_as(C.POINTER(C.c_float)),
                             sc.ctypes.data_as(C.POINTER(C.c_double)), alpha, final_k,
                             order.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(count))
    return st, count.value


def test_stateless_validation_order_up_to_the_device():
    good = np.ones((2, 3), np.float32)
    bad_rows = good.copy()
    bad_rows[1, 2] = np.inf
    # alpha, final_k and the scores come first, whatever else is wrong
    for alpha in (-0.1, 1.5, math.nan, math.inf):
        assert rerank(99, bad_rows, [1.0, 2.0], alpha, 1) == (MMR_ARGS, 0)
    assert rerank(99, bad_rows, [1.0, 2.0], 0.5, 0) == (MMR_ARGS, 0)
    for score in (math.nan, math.inf, -math.inf, 3.5e38, -3.5e38):
        assert rerank(99, bad_rows, [1.0, score], 0.5, 1) == (MMR_ARGS, 0)
    # then the metric, the dimension, the values
    assert rerank(99, bad_rows, [1.0, 2.0], 0.5, 1) == (UNKNOWN_METRIC, 0)
    assert rerank(-1, bad_rows, [1.0, 2.0], 0.5, 1) == (UNKNOWN_METRIC, 0)
    assert rerank(0, np.zeros((2, 0), np.float32), [1.0, 2.0], 0.5, 1) == (EMPTY, 0)
    assert rerank(0, bad_rows, [1.0, 2.0], 0.5, 1) == (NON_FINITE, 0)
    # only then the device: a score at the edge of the f32 range and both ends of alpha are fine
    for alpha in (0.0, 1.0):
        st, count = rerank(0, good, [3.4028234663852886e38, -3.4028234663852886e38], alpha, 5, device=10 ** 6)
        assert (st, count) == (DEVICE, 0)
        # (the detail is the context's: no device at all here, no such ordinal on a GPU machine)
        assert lib().vt_last_error() in (b"no HIP device visible: libvettore_hip has no CPU fallback", b"device ordinal out of range")


def test_count_zero_is_ok_without_a_device():
    assert rerank(0, np.zeros((0, 4), np.float32), [], 0.5, 3, device=10 ** 6) == (OK, 0)
    assert rerank(0, np.zeros((0, 4), np.float32), [], 1.5, 3, device=10 ** 6) == (MMR_ARGS, 0)
    assert rerank(99, np.zeros((0, 4), np.float32), [], 0.5, 3, device=10 ** 6) == (UNKNOWN_METRIC, 0)
    # NULL where a result must go
    assert lib().vt_mmr_rerank(0, 0, 0, 4, None, None, 0.5, 3, None, None) == ARGUMENT
    sc = (C.c_double * 1)(1.0)
    assert lib().vt_mmr_rerank(0, 0, 1, 4, None, sc, 0.5, 3, None, C.byref(C.c_size_t())) == ARGUMENT


def test_handle_calls_refuse_a_null_handle_before_anything_else():
    L = lib()
    n = C.c_size_t()
    order = (C.c_uint32 * 4)()
    sc = (C.c_double * 1)(math.nan)
    off = (C.c_size_t * 2)(0, 1)
    assert L.vt_flat_mmr_rerank(None, 1, b"a", off, sc, 2.0, 0, order, C.byref(n)) == ARGUMENT
    poff = (C.c_size_t * 2)(0, 1)
    alphas, ks, status = (C.c_double * 1)(2.0), (C.c_size_t * 1)(0), (C.c_int * 1)()
    assert L.vt_flat_mmr_rerank_batch(None, 1, poff, b"a", off, sc, alphas, ks, order, C.byref(n), status) == ARGUMENT
    assert L.vt_flat_mmr_rerank_batch(None, 0, None, None, None, None, None, None, None, None, None) == ARGUMENT
    q = (C.c_float * 2)(1.0, 2.0)
    h = C.c_void_p()
    assert L.vt_flat_mmr_search(None, q, 2, 4, 0, 2.0, 7, C.byref(h), order, C.byref(n)) == ARGUMENT
    outs = (C.c_void_p * 1)()
    lens = (C.c_size_t * 1)()
    assert L.vt_flat_mmr_search_batch(None, q, 1, 2, 4, 0, 2.0, 7, outs, order, lens, None) == ARGUMENT
    # and a handle cannot be had without a device
    assert L.vt_flat_new(0, 10 ** 6, C.byref(h)) == DEVICE


def test_python_mirror_validates_in_the_reference_order_before_any_device_call():
    from vettore_amd import nifs
    ok_i, ok_e = [("a", 1.0)], [("a", [1.0])]
    inv = ("error", "invalid_mmr_args")
    assert nifs.mmr_rerank(ok_i, ok_e, "nope", 1.5, 1) == inv
    assert nifs.mmr_rerank(ok_i, ok_e, "nope", 0.5, 0) == inv
    assert nifs.mmr_rerank(ok_i, ok_e, "nope", True, 1) == inv
    assert nifs.mmr_rerank(ok_i, [("a", [])], "nope", 0.5, 1) == ("error", ("unknown_metric", "nope"))
    assert nifs.mmr_rerank([("zz", 1.0)], [("a", [])], "l2", 0.5, 1) == inv
    for bad in ([("", [1.0])], [("a", [1.0]), ("b", [1.0, 2.0])], [("a", [math.inf])], [("a", [4e38])], [("a", [True])],
                [("a", [1.0]), ("a", [1.0])], ["bad"]):
        assert nifs.mmr_rerank(ok_i, bad, "l2", 0.5, 1) == inv, bad
    for bad in ([("", 1.0)], [("a", math.nan)], [("a", 4e38)], [("b", 1.0)], [("a", 1.0), ("a", 1.0)], ["bad"]):
        assert nifs.mmr_rerank(bad, ok_e, "l2", 0.5, 1) == inv, bad
    assert nifs.mmr_rerank([], [], "l2", 0.5, 10) == ("ok", [])
    assert nifs.mmr_rerank([], ok_e, "l2", 1, 10) == ("ok", [])


def test_python_mirror_agrees_with_the_restatement_on_every_error_of_the_fixture():
    import mmr_ref
    from support import load
    from vettore_amd import nifs
    seen = 0
    for case in load("mmr_ex.json")["cases"]:
        if case["expect"][0] != "error" or case["expect"][1] == "metric_overflow":
            continue
        entries = lambda xs: [tuple(x) if isinstance(x, list) else x for x in xs]
        args = (entries(case["initial"]), entries(case["embeddings"]), case["metric"], case["alpha"], case["final_k"])
        assert nifs.mmr_rerank(*args) == mmr_ref.mmr_rerank(*args), case["source"]
        seen += 1
    assert seen == 9
