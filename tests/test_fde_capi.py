"""The MUVERA retrieval calls over a resident store (vt_mv_encode_documents, vt_mv_fde_sync, vt_mv_fde_top_k,
vt_mv_fde_top_k_batch) without a GPU: declared, exported and bound, additive (the ABI version stays 4), and a NULL
handle is VT_ERR_ARGUMENT before anything else is looked at.  What they compute is tests/test_gpu_fde.py."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vt_mv_encode_documents", "vt_mv_fde_sync", "vt_mv_fde_top_k", "vt_mv_fde_top_k_batch"]
CFG = (4, 1, 0, 1, 4, 0, 0)   # a valid configuration: dimension 4, identity
BAD = (0, 0, 31, 1, 0, 0, 1)  # every field refused


def test_every_new_name_is_declared_exported_and_bound():
    import vettore_amd._lib as L
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vettore_flat.h")).read(), flags=re.S)
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in L.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.vt_abi_version() == 4 and L.ABI_VERSION == 4
    assert len(L.SYMBOLS) == 108 and len(set(L.SYMBOLS)) == 108
    from vettore_amd import nifs
    from vettore_amd.collection import Collection
    from vettore_amd.mv_store import ResidentMultiVector
    for owner, names in ((nifs, ("mv_encode_documents", "mv_fde_sync", "mv_fde_top_k", "mv_fde_top_k_batch")),
                         (ResidentMultiVector, ("encode_documents", "fde_sync", "fde_top_k", "fde_top_k_batch")),
                         (Collection, ("muvera_search", "muvera_search_batch"))):
        for name in names:
            assert callable(getattr(owner, name)), name


def test_no_new_status_code():
    import vettore_amd._lib as L
    lib = L.load()
    lib.vt_strerror.restype = C.c_char_p
    assert lib.vt_strerror(37) == b"unknown status" and lib.vt_strerror(39) == b"unknown status"


def test_null_handles():
    """Without a device no store and no index can be made, so both are NULL here; a NULL index beside a real store, and
    the other way round, are refused in tests/test_gpu_fde.py."""
    import vettore_amd._lib as L
    lib = L.load()
    off = (C.c_size_t * 2)(0, 1)
    one = (C.c_float * 4)(1.0, 0.0, 0.0, 0.0)
    qoff = (C.c_size_t * 2)(0, 4)
    outs = (C.c_void_p * 1)()
    status = (C.c_int * 1)(7)
    row = (C.c_float * 4)()
    for cfg in (CFG, BAD):   # before the configuration is looked at
        assert lib.vt_mv_encode_documents(None, 1, b"a", off, *cfg, row, status) == 19
        assert lib.vt_mv_encode_documents(None, 0, None, None, *cfg, None, None) == 19
        assert lib.vt_mv_fde_sync(None, None, 1, b"a", off, *cfg, status) == 19
        assert lib.vt_mv_fde_sync(None, None, 0, None, None, *cfg, None) == 19
        for metric in (3, 99):   # ... and before the metric is decoded
            assert lib.vt_mv_fde_top_k(None, None, *cfg, one, qoff, 1, 10, metric, 1, outs) == 19
            assert lib.vt_mv_fde_top_k_batch(None, None, *cfg, 1, off, one, qoff, 10, metric, 1, outs, status) == 19
            assert lib.vt_mv_fde_top_k_batch(None, None, *cfg, 0, off, one, qoff, 10, metric, 1, outs, None) == 19
    assert status[0] == 7 and not outs[0]
