"""The HNSW index's C ABI (vt_hnsw_*, include/vettore_flat.h) and its Python mirror without a GPU: the new statuses
carry HnswParams::validate's strings, vt_hnsw_new answers the metric first, then the parameters, and only then looks
for a device, NULL handles are refused, and HnswGpu.new rejects what hnsw.ex rejects."""
import ctypes as C
import re
import os

from support import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = load("hnsw_rs.json")
NAMES = ["vt_hnsw_new", "vt_hnsw_free", "vt_hnsw_insert", "vt_hnsw_insert_many", "vt_hnsw_delete", "vt_hnsw_search",
         "vt_hnsw_search_batch", "vt_hnsw_len", "vt_hnsw_dimension", "vt_hnsw_node", "vt_hnsw_neighbors", "vt_hnsw_counters",
         "vt_hnsw_memory"]
STRINGS = {29: "m must be positive", 30: "m0 must be positive", 31: "invalid hnsw degree", 32: "ef_construction must be >= m",
           33: "ef_construction exceeds safety limit", 34: "ef_search must be positive", 35: "max_level must be positive",
           36: "hnsw lock poisoned"}


def test_every_new_name_is_declared_exported_and_bound():
    import vettore_amd._lib as L
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vettore_flat.h")).read(), flags=re.S)
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in L.SYMBOLS, name
    assert lib.vt_abi_version() == 4


def test_new_statuses_carry_the_reference_strings():
    import vettore_amd._lib as L
    lib = L.load()
    for status, text in STRINGS.items():
        assert lib.vt_strerror(status).decode() == text
    assert lib.vt_strerror(37).decode() == "unknown status"


def test_new_answers_metric_then_parameters_then_device():
    import vettore_amd._lib as L
    lib = L.load()
    h = C.c_void_p()
    p = GOLD["params"]
    order = ("m", "m0", "ef_construction", "ef_search", "max_level")
    by_text = {v: k for k, v in STRINGS.items()}
    # the eleven invalid sets of hnsw.rs:527-563: the parameter's status, with or without a device
    for over, text in GOLD["invalid"]:
        args = [dict(p, **over)[k] for k in order]
        assert lib.vt_hnsw_new(0, 0, *args, C.byref(h)) == by_text[text], over
        assert not h.value
    args = [p[k] for k in order]
    # an unsupported metric comes before a bad parameter
    for metric in (1, 4, 5, 6, 7, 8, 9, -1):
        assert lib.vt_hnsw_new(metric, 0, 0, 0, 0, 0, 0, C.byref(h)) == 18  # VT_ERR_UNSUPPORTED
        assert b"l2, cosine and inner_product" in lib.vt_last_error()
    assert lib.vt_hnsw_new(0, 0, *args, None) == 19
    for metric in (0, 2, 3):
        st = lib.vt_hnsw_new(metric, 0, *args, C.byref(h))
        if lib.vt_device_count() == 0:
            assert st == 17 and not h.value                  # VT_ERR_DEVICE: no CPU fallback
            assert b"no CPU fallback" in lib.vt_last_error()
        else:
            assert st == 0 and h.value
            assert lib.vt_hnsw_len(h) == 0 and lib.vt_hnsw_dimension(h) == -1
            lib.vt_hnsw_free(h)
            h = C.c_void_p()


def test_null_handles_are_refused():
    import vettore_amd._lib as L
    lib = L.load()
    one = (C.c_float * 1)(1.0)
    off = (C.c_size_t * 2)(0, 1)
    out = C.c_void_p()
    n = C.c_size_t()
    assert lib.vt_hnsw_insert(None, b"a", 1, one, 1) == 19
    assert lib.vt_hnsw_insert_many(None, 1, b"a", off, one, off) == 19
    assert lib.vt_hnsw_delete(None, b"a", 1) == 19
    fake = C.c_void_p(1)   # (argument checks come before the handle is touched)
    assert lib.vt_hnsw_insert_many(fake, 1, None, off, one, off) == 19   # ids missing
    assert lib.vt_hnsw_insert_many(fake, 1, b"a", off, None, off) == 19  # values missing
    assert lib.vt_hnsw_search(None, one, 1, 1, C.byref(out)) == 19
    assert lib.vt_hnsw_search_batch(None, one, 1, 1, 1, C.byref(out), None) == 19
    assert lib.vt_hnsw_node(None, b"a", 1, None, None, None) == 19
    assert lib.vt_hnsw_neighbors(None, 0, 0, None, 0, C.byref(n)) == 19
    assert lib.vt_hnsw_counters(None, None, None, None) == 19
    assert lib.vt_hnsw_memory(None, None, None, None, None) == 19
    assert lib.vt_hnsw_len(None) == 0 and lib.vt_hnsw_dimension(None) == -1
    lib.vt_hnsw_free(None)


def test_hnswgpu_new_rejects_what_hnsw_ex_rejects():
    from vettore_amd.index_hnsw import DEFAULT_OPTIONS, HnswGpu
    from vettore_amd.collection import Collection
    assert DEFAULT_OPTIONS == {"m": 16, "m0": 32, "ef_construction": 100, "ef_search": 64, "max_level": 12}
    assert HnswGpu.defaults() == DEFAULT_OPTIONS
    bad = [{"m": 0}, {"m": 1025, "m0": 2048}, {"m0": 2049}, {"m": 16, "m0": 8}, {"ef_construction": 8}, {"ef_construction": 1000001},
           {"ef_search": 0}, {"ef_search": 1000001}, {"max_level": 0}, {"max_level": 65}, {"m": 1.5}, {"m": True}, {"unknown": 1},
           {"device": -1}, [("m", 8), ("m", 8)], "m", [1, 2], 7]
    for opts in bad:
        assert HnswGpu.new("l2", opts) == ("error", "invalid_hnsw_options"), opts
    for metric in ("l2_squared", "negative_inner_product", "manhattan", "chebyshev", "hamming", "jaccard", "nonsense"):
        assert HnswGpu.new(metric, []) == ("error", ("unsupported_hnsw_metric", metric))
    # options are looked at before the metric (hnsw.ex:31-35)
    assert HnswGpu.new("hamming", {"m": 0}) == ("error", "invalid_hnsw_options")
    assert Collection.new(dimensions=4, metric="hamming", index="hnsw") == ("error", ("unsupported_hnsw_metric", "hamming"))
    assert Collection.new(dimensions=4, metric="l2", index="hnsw_gpu", index_options={"m": 0}) == ("error", "invalid_hnsw_options")
