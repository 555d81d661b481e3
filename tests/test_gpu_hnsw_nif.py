"""The seven hnsw_* NIFs of the erl_nif shim (integration/c_src/vettore_gpu_nif.c) EXECUTED against the real library on
the GPU through the fake runtime (tests/nif_runtime.py), in the manner of tests/test_gpu_nif_exec.py: what comes back --
{:ok, reference}, {:ok, {}}, hit lists, the reference's error strings, ArgumentError -- is compared with the restatement
of hnsw.rs (tests/hnsw_ref.py) bit for bit."""
import math

import numpy as np
import pytest

import nif_runtime
from hnsw_ref import COSINE, INNER_PRODUCT, L2, HnswError, HnswIndex
from nif_runtime import ArgumentError, ERROR, OK

pytestmark = pytest.mark.gpu

UNIT = (OK, ())


@pytest.fixture(scope="module")
def rt():
    import vettore_amd._lib as L
    assert L.load().vt_device_count() >= 1, "no HIP device: GPU tests need the real hardware"
    return nif_runtime.Runtime()


@pytest.fixture
def ref_order(oracle_mod):
    from vettore_amd import nifs
    oracle_mod.set_reduce_order(nifs.debug_get("reduce_order"))
    yield
    oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


def bits(hits):
    return [(h[0], np.float32(h[1]).tobytes()) for h in hits]


def test_the_table_holds_the_seven_nifs(rt):
    funcs = rt.functions()
    for name, arity in (("hnsw_new_l2", 6), ("hnsw_new_cosine", 6), ("hnsw_new_inner_product", 6), ("hnsw_insert", 3),
                        ("hnsw_insert_many", 2), ("hnsw_delete", 2), ("hnsw_search", 3)):
        assert (name, arity) in funcs, name
        assert funcs[(name, arity)] != 0   # a dirty scheduler: every call waits for the device


@pytest.mark.parametrize("metric,new", [(L2, "hnsw_new_l2"), (COSINE, "hnsw_new_cosine"), (INNER_PRODUCT, "hnsw_new_inner_product")])
def test_build_search_delete_through_the_shim(rt, ref_order, metric, new):
    made = rt.call(new, 4, 8, 30, 12, 12, 0)
    assert made[0] == OK and isinstance(made[1], nif_runtime.Resource)
    ref = made[1]
    want = HnswIndex(metric, m=4, m0=8, ef_construction=30, ef_search=12)
    rng = np.random.default_rng(41)
    vecs = rng.standard_normal((150, 6)).astype(np.float32)
    ids = [b"s%d" % ((i * 7919) % 1009) for i in range(150)]
    assert rt.call("hnsw_insert", ref, ids[0], [float(x) for x in vecs[0]]) == UNIT
    want.insert(ids[0], vecs[0])
    assert rt.call("hnsw_insert_many", ref, [(i, [float(x) for x in v]) for i, v in zip(ids[1:], vecs[1:])]) == UNIT
    want.insert_many(list(zip(ids[1:], vecs[1:])))
    assert rt.call("hnsw_insert", ref, ids[9], [float(x) for x in vecs[20]]) == UNIT   # an upsert
    want.insert(ids[9], vecs[20])
    assert rt.call("hnsw_delete", ref, ids[33]) == UNIT
    want.delete(ids[33])
    assert rt.call("hnsw_delete", ref, b"missing") == UNIT
    for q in (vecs[3], vecs[99], np.zeros(6, np.float32)):
        for limit in (1, 10, 200):
            got = rt.call("hnsw_search", ref, [float(x) for x in q], limit)
            assert got[0] == OK and bits(got[1]) == bits(want.search(q, limit))
    assert rt.call("hnsw_search", ref, [1.0], 0) == (OK, [])
    # the reference's strings, in its order
    assert rt.call("hnsw_search", ref, [], 3) == (ERROR, b"vector must not be empty")
    assert rt.call("hnsw_search", ref, [1.0], 3) == (ERROR, b"dimension mismatch")
    assert rt.call("hnsw_insert", ref, b"x", [1.0] * 5) == (ERROR, b"dimension mismatch")
    assert rt.call("hnsw_insert", ref, b"x", []) == (ERROR, b"vector must not be empty")
    with pytest.raises(ArgumentError):   # a BEAM float is finite: infinity does not decode
        rt.call("hnsw_insert", ref, b"x", [math.inf] + [0.0] * 5)
    assert rt.call("hnsw_insert_many", ref, [(b"y", [0.0] * 6), (b"z", [0.0])]) == (ERROR, b"dimension mismatch")
    with pytest.raises(HnswError):
        want.insert_many([(b"y", [0.0] * 6), (b"z", [0.0])])
    got = rt.call("hnsw_search", ref, [float(x) for x in vecs[3]], 10)
    assert bits(got[1]) == bits(want.search(vecs[3], 10))
    # terms that do not decode
    for call in (lambda: rt.call("hnsw_search", ref, [1.0] * 6, -1), lambda: rt.call("hnsw_insert", ref, 7, [1.0] * 6),
                 lambda: rt.call("hnsw_insert", b"not a reference", b"a", [1.0] * 6),
                 lambda: rt.call("hnsw_insert_many", ref, [(b"a", [1.0] * 6), b"b"]), lambda: rt.call(new, 4, 8, 30, 12, 12, -1)):
        with pytest.raises(ArgumentError):
            call()
    live, dtors = rt.live_resources(), rt.dtor_calls()
    ref.release()
    assert rt.live_resources() == live - 1 and rt.dtor_calls() == dtors + 1


def test_new_returns_validates_strings(rt):
    assert rt.call("hnsw_new_l2", 0, 8, 30, 12, 12, 0) == (ERROR, b"m must be positive")
    assert rt.call("hnsw_new_cosine", 8, 4, 30, 12, 12, 0) == (ERROR, b"invalid hnsw degree")
    assert rt.call("hnsw_new_inner_product", 8, 16, 4, 12, 12, 0) == (ERROR, b"ef_construction must be >= m")
    assert rt.call("hnsw_new_l2", 8, 16, 30, 0, 12, 0) == (ERROR, b"ef_search must be positive")
    assert rt.call("hnsw_new_l2", 8, 16, 30, 12, 65, 0) == (ERROR, b"max_level must be positive")
    got = rt.call("hnsw_new_l2", 8, 16, 30, 12, 12, 4096)
    assert got[0] == ERROR and b"device ordinal out of range" in got[1]
