"""MaxSim without a device: the test-side reference (tests/maxsim_ref.py) against the literals of the reference's own
tests (tests/golden/multi_vector_rs.json), and the C ABI / NIF shim refusing in the reference's order before any
device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import maxsim_ref
import nif_runtime
from maxsim_ref import MaxSimError
from nif_runtime import ArgumentError, Atom
from support import load, same_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = load("multi_vector_rs.json")


def fl(v):
    if isinstance(v, list):
        return [fl(x) for x in v]
    return float(v)  # (also "nan" / "inf")


def outcome(fn, *args):
    try:
        return ("ok", fn(*args))
    except MaxSimError as e:
        return ("error", str(e))


@pytest.fixture(autouse=True)
def default_order(oracle_mod):
    oracle_mod.set_reduce_order(oracle_mod.DEFAULT_ORDER)


@pytest.mark.parametrize("case", CASES["score"], ids=lambda c: c["line"])
def test_helper_reproduces_score_literals(case):
    got = outcome(maxsim_ref.score, fl(case["query"]), fl(case["document"]), case["metric"])
    if "ok" in case:
        assert got[0] == "ok" and same_f32(got[1], case["ok"]), got
    else:
        assert got == ("error", case["error"])


@pytest.mark.parametrize("case", CASES["top_k"], ids=lambda c: c["line"])
def test_helper_reproduces_top_k_literals(case):
    docs = [(i, fl(v)) for i, v in case["documents"]]
    got = outcome(maxsim_ref.top_k, docs, fl(case["query"]), case["metric"], case["limit"])
    if "ok" in case:
        assert got[0] == "ok"
        assert [(i.decode(), float(s)) for i, s in got[1]] == [tuple(h) for h in case["ok"]]
    else:
        assert got == ("error", case["error"])


def test_helper_matches_the_reference_oracle_for_every_metric():
    c = CASES["oracle_all_metrics"]
    for metric in range(9):
        got = maxsim_ref.score(c["query"], c["document"], metric)
        # score_oracle: per query vector max_by(total_cmp) of the similarities, summed
        exp = sum(max(maxsim_ref.pair(metric, q, t) for t in c["document"]) for q in c["query"])
        assert abs(float(got) - float(exp)) <= c["tolerance"], metric


def full_sort_documents():
    docs = []
    for i in range(CASES["full_sort"]["count"]):
        a = np.float32(np.float32(i - 12.0) / np.float32(5.0))
        b = np.float32(np.float32((i * 7 % 11) - 5.0) / np.float32(3.0))
        docs.append(("doc-%02d" % i, [[float(a), 1.0], [0.0, float(b)]]))
    return docs


@pytest.mark.parametrize("metric", range(9))
def test_helper_top_k_is_the_full_sort_truncated(metric):
    fs = CASES["full_sort"]
    docs = full_sort_documents()
    expected = [(i.encode(), maxsim_ref.score(fs["query"], v, metric)) for i, v in docs]
    expected.sort(key=lambda h: (-float(h[1]), h[0]))
    for limit in fs["limits"]:
        got = maxsim_ref.top_k(docs, fs["query"], metric, limit)
        assert [h[0] for h in got] == [h[0] for h in expected[:limit]]
        assert all(same_f32(a[1], b[1]) for a, b in zip(got, expected[:limit]))


# ---- the C ABI: validation in the reference's order, no device touched ------------------------------------------
def lib():
    from vettore_amd import _lib
    return _lib.load()


def abi_top_k(docs, query, metric, limit=5):
    from vettore_amd import nifs
    return nifs.multi_vector_top_k(docs, query, metric, limit)


def test_new_status_strings():
    L = lib()
    assert L.vt_strerror(9) == b"vectors must not be empty"
    assert L.vt_strerror(10) == b"score overflow"
    assert L.vt_abi_version() == 4


REFUSALS = [
    ("unknown metric", [("a", [[1.0]])], [[1.0]], 9),
    ("empty first query vector", [("a", [[1.0]])], [[]], 3),
    ("ragged query", [("a", [[1.0]])], [[1.0], [1.0, 2.0]], 3),
    ("NaN in the query", [("a", [[1.0]])], [[1.0], [float("nan")]], 3),
    ("document 0 with a wrong dimension", [("a", [[1.0, 2.0]]), ("b", [[1.0]])], [[1.0]], 3),
    ("empty query, document's first vector empty", [("a", [[]])], [], 0),
    ("metric beats a bad query", [("a", [[1.0]])], [[]], 11),
]


@pytest.mark.parametrize("name, docs, query, metric", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_abi_refuses_in_the_reference_order(name, docs, query, metric):
    want = outcome(maxsim_ref.top_k, docs, query, metric, 5)
    assert want[0] == "error", name
    assert abi_top_k(docs, query, metric) == want
    # the one-document form too
    from vettore_amd import nifs
    assert nifs.multi_vector_score(query, docs[0][1], metric) == outcome(maxsim_ref.score, query, docs[0][1], metric)


def test_valid_call_without_a_device_is_a_device_error():
    L = lib()
    if L.vt_device_count() > 0:
        pytest.skip("a GPU is present: tests/test_gpu_multi_vector.py scores on it")
    from vettore_amd import nifs
    tag, msg = abi_top_k([("a", [[1.0, 0.0]])], [[1.0, 0.0]], 3)
    assert tag == "error" and msg.startswith("device error")
    tag, msg = nifs.multi_vector_score([[1.0, 0.0]], [[1.0, 0.0]], 3)
    assert tag == "error" and msg.startswith("device error")
    assert L.vt_debug_set(b"maxsim_chunk_bytes", 4096) == 0
    v = C.c_long()
    assert L.vt_debug_get(b"maxsim_chunk_bytes", C.byref(v)) == 0 and v.value == 4096
    assert L.vt_debug_set(b"maxsim_chunk_bytes", 0) == 0


# ---- the NIF shim's decoding -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rt():
    return nif_runtime.Runtime()


def test_nif_table_has_the_maxsim_calls(rt):
    funcs = rt.functions()
    assert ("multi_vector_score", 3) in funcs and ("multi_vector_top_k", 4) in funcs


def test_nif_decode_failures_are_badarg(rt):
    for bad in (Atom("x"), [1.0], [[1]], [[Atom("nan")]], [[1e39]], (1.0,)):
        with pytest.raises(ArgumentError):
            rt.call("multi_vector_score", bad, [[1.0]], 3)
        with pytest.raises(ArgumentError):
            rt.call("multi_vector_score", [[1.0]], bad, 3)
        with pytest.raises(ArgumentError):
            rt.call("multi_vector_top_k", [(b"a", [[1.0]])], bad, 3, 1)
    for bad_code in (-1, 256, 1.0, Atom("l2")):
        with pytest.raises(ArgumentError):
            rt.call("multi_vector_score", [[1.0]], [[1.0]], bad_code)
    for bad_docs in (Atom("x"), [(b"a",)], [(b"a", [[1.0]], 3)], [(1, [[1.0]])], [(b"a", [1.0])], [(b"a", [[1]])],
                     [[b"a", [[1.0]]]]):
        with pytest.raises(ArgumentError):
            rt.call("multi_vector_top_k", bad_docs, [[1.0]], 3, 1)
    for bad_limit in (-1, 1.0):
        with pytest.raises(ArgumentError):
            rt.call("multi_vector_top_k", [(b"a", [[1.0]])], [[1.0]], 3, bad_limit)


def test_nif_refusals_before_the_device(rt):
    assert rt.call("multi_vector_top_k", [(b"a", [[1.0]])], [[1.0]], 9, 1) == (Atom("error"), b"unknown metric")
    assert rt.call("multi_vector_top_k", [(b"a", [[1.0, 2.0]])], [[1.0]], 3, 1) == (Atom("error"), b"dimension mismatch")
    assert rt.call("multi_vector_score", [[]], [[1.0]], 3) == (Atom("error"), b"vectors must not be empty")
    assert rt.call("multi_vector_top_k", [], [[1.0]], 3, 1) == (Atom("ok"), [])
