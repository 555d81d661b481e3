"""hnsw_quantized_search/4, hnsw_funnel_search/5 and hnsw_hybrid_search/4 of integration/c_src/vettore_gpu_nif.c on the fake
erl_nif runtime (tests/nif_runtime.py) -- `-m gpu`: one corpus through the shim and through the Python mirror of the
NIFs (vettore_amd/nifs.py), equal terms -- ids, order, the f32 bits of every raw value, the error binaries -- and badarg
for terms the NIFs cannot decode."""
import numpy as np
import pytest

import nif_runtime
from nif_runtime import ArgumentError, ERROR, FloatList, OK
from test_gpu_parity import nifs  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import vettore_amd._lib as L
    assert L.load().vt_device_count() >= 1, "no HIP device: GPU tests need the real hardware"
    return nif_runtime.Runtime()


def term(res):
    """a nifs.py answer as the shim's term"""
    if res[0] == "ok":
        return (OK, [(i, np.float32(r).tobytes()) for i, r in res[1]])
    return (ERROR, res[1].encode())


def shim(res):
    if res[0] == OK:
        return (OK, [(i, np.float32(r).tobytes()) for i, r in res[1]])
    return res


def test_the_three_nifs_answer_as_the_python_mirror(rt, nifs):
    funcs = rt.functions()
    assert ("hnsw_quantized_search", 4) in funcs and ("hnsw_funnel_search", 5) in funcs and ("hnsw_hybrid_search", 4) in funcs
    assert funcs[("hnsw_hybrid_search", 4)] == funcs[("hnsw_search", 3)] != 0   # dirty NIFs
    rng = np.random.default_rng(3)
    n, d = 200, 24
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    ids = [b"k%d" % ((i * 7919) % 1009) for i in range(n)]
    items = list(zip(ids, vecs))
    res = rt.call("hnsw_new_l2", 4, 8, 30, 16, 12, 0)
    assert res[0] == OK
    ref = res[1]
    assert rt.call("hnsw_insert_many", ref, [(i, FloatList(v)) for i, v in items]) == (OK, ())
    made = nifs.hnsw_new_l2(4, 8, 30, 16, 12)
    assert made[0] == "ok"
    idx = made[1]
    assert nifs.hnsw_insert_many(idx, items) == ("ok", ())
    for doomed in ids[:30]:
        assert rt.call("hnsw_delete", ref, doomed) == (OK, ())
        assert nifs.hnsw_delete(idx, doomed) == ("ok", ())
    gens = [(0, 40, [6, 12]), (1, 50, []), (2, 20, [])]
    for q in (vecs[50], rng.standard_normal(d).astype(np.float32)):
        ql = FloatList(q)
        for cand, limit in ((10, 5), (300, 10), (10, 0)):
            assert shim(rt.call("hnsw_quantized_search", ref, ql, cand, limit)) == term(nifs.hnsw_quantized_search(idx, q, cand, limit))
            for st in ([d], [6, 12], [d + 1], []):
                assert shim(rt.call("hnsw_funnel_search", ref, ql, st, cand, limit)) == term(nifs.hnsw_funnel_search(idx, q, st, cand, limit))
        for g in (gens, [(2, 20, [])], [(0, 10, [0])], [(0, 10, [])]):
            assert shim(rt.call("hnsw_hybrid_search", ref, ql, g, 7)) == term(nifs.hnsw_hybrid_search(idx, q, g, 7))
    assert rt.call("hnsw_quantized_search", ref, FloatList(vecs[0][:5]), 10, 5) == (ERROR, b"dimension mismatch")
    # terms the NIFs cannot decode
    flat = rt.call("flat_new", 0, [0])   # (a bare reference: a reference of the other resource type)
    q = FloatList(vecs[0])
    for name, args in (("hnsw_quantized_search", (ref, q, -1, 5)), ("hnsw_quantized_search", (ref, [b"x"], 10, 5)),
                       ("hnsw_quantized_search", (b"not a reference", q, 10, 5)), ("hnsw_funnel_search", (ref, q, [1.5], 10, 5)),
                       ("hnsw_funnel_search", (ref, q, 8, 10, 5)), ("hnsw_hybrid_search", (ref, q, [(0, 10)], 5)),
                       ("hnsw_hybrid_search", (ref, q, [(b"funnel", 10, [4])], 5)), ("hnsw_hybrid_search", (ref, q, 3, 5)),
                       ("hnsw_hybrid_search", (ref, q, [], 5)), ("hnsw_hybrid_search", (ref, q, [(3, 10, [])], 5))):   # (VT_ERR_ARGUMENT is badarg)
        with pytest.raises(ArgumentError):
            rt.call(name, *args)
    for name, args in (("hnsw_quantized_search", (flat, q, 10, 5)), ("hnsw_hybrid_search", (flat, q, gens, 5)),
                       ("flat_hybrid_search", (ref, q, gens, 5))):
        with pytest.raises(ArgumentError):
            rt.call(name, *args)
