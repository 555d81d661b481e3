"""MUVERA without a GPU: the restatement of muvera.rs (tests/muvera_ref.py) against the answers the reference's own
tests state (tests/golden/muvera_rs.json), the C ABI's validation -- every status, string and their order are
decided on the host --, vettore_amd.muvera's error atoms, and the shim's two NIFs."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import muvera_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "muvera_rs.json")))
MODES = {"query": muvera_ref.QUERY, "document": muvera_ref.DOCUMENT}
U64_MAX = (1 << 64) - 1
MAX_OUT = 16_777_216

# include/vettore_flat.h
STRINGS = {
    2: "dimension mismatch", 3: "vector contains a non-finite value",
    20: "empty vectors", 21: "dimension must be positive", 22: "num_repetitions must be positive",
    23: "num_simhash_projections must be < 31", 24: "projection_dimension must be positive",
    25: "final_projection_dimension must be positive", 26: "fde dimension overflow",
    27: "fde dimension exceeds safety limit", 28: "encoding overflow",
}
CODE = {v: k for k, v in STRINGS.items()}


@pytest.fixture(scope="module")
def lib():
    import vettore_amd._lib as L
    return L.load()


def cfg_args(c):
    return (c["dimension"], c["num_repetitions"], c["num_simhash_projections"], c["seed"], c["projection_dimension"],
            c["final_projection_dimension"])


def as_vectors(rows):
    return [[float("nan") if x == "NaN" else x for x in v] for v in rows]


# ---------------------------------------------------------------- the restatement
def test_the_restatement_reproduces_the_references_answers():
    for c in GOLDEN["cases"]:
        got = muvera_ref.encode(as_vectors(c["vectors"]), *cfg_args(c["config"]), MODES[c["mode"]])
        e = c["expect"]
        if "ok" in e:
            assert got[0] == "ok" and got[1].tobytes() == np.asarray(e["ok"], dtype=np.float32).tobytes(), (c["name"], got)
        elif "len" in e:
            assert got[0] == "ok" and got[1].dtype == np.float32 and len(got[1]) == e["len"], c["name"]
        else:
            assert got == ("error", e.get("string", e["error"])), (c["name"], got)   # what muvera.rs returns on that path
            assert e["error"] in (None, got[1]), c["name"]                           # ... and what the test states, if it does


def test_the_restatement_keeps_the_references_invariants():
    """muvera.rs:359-378 and :391-402: order, seed, and the range of weights and signs."""
    p = GOLDEN["permutation"]
    vectors, args = p["vectors"], cfg_args(p["config"])
    query = muvera_ref.encode_query(vectors, *args)[1]
    assert query.tobytes() == muvera_ref.encode_query(vectors[::-1], *args)[1].tobytes()
    doc, rdoc = muvera_ref.encode_document(vectors, *args)[1], muvera_ref.encode_document(vectors[::-1], *args)[1]
    assert np.all(np.abs(doc - rdoc) <= p["document_tolerance"])
    other = list(args)
    other[3] += 1
    assert query.tobytes() != muvera_ref.encode_query(vectors, *other)[1].tobytes()
    for seed in (0, 1, 42, U64_MAX):
        j = np.arange(100, dtype=np.uint64)
        w = muvera_ref.random_weight(seed, 3, 7, j)
        assert w.dtype == np.float32 and np.all((w >= -1.0) & (w <= 1.0))
        assert set(muvera_ref.random_sign(seed, 3, 7, j).tolist()) <= {1.0, -1.0}
        # the vectorised hash and its spelling on Python integers agree
        assert [int(h) for h in muvera_ref.hash4(seed, 3, 7, j)] == [muvera_ref.hash4_int(seed, 3, 7, int(i)) for i in j]
    # count_sketch (muvera.rs:404-417): equal signs on two colliding maxima overflow; a zero dimension is refused
    fmax = np.finfo(np.float32).max
    results = [muvera_ref.count_sketch(np.array([fmax, fmax], np.float32), 1, s) for s in range(64)]
    assert ("error", "encoding overflow") in results and any(r[0] == "ok" for r in results)
    assert muvera_ref.count_sketch(np.array([1.0, 2.0], np.float32), 0, 0) == ("error", "final_projection_dimension must be positive")


# ---------------------------------------------------------------- the C ABI
def call(lib, sets, mode, d, R, k, seed, pd, final, statuses=False):
    """vt_muvera_encode over `sets`; returns (status, out rows, per-set statuses or None)."""
    per_set = [[np.asarray(v, dtype=np.float32) for v in s] for s in sets]
    set_off = np.cumsum([0] + [len(s) for s in per_set]).astype(np.uintp)
    flat = [v for s in per_set for v in s]
    val_off = np.cumsum([0] + [v.size for v in flat]).astype(np.uintp)
    values = np.concatenate(flat + [np.zeros(1, np.float32)])
    fde = lib.vt_muvera_fde_dimension(R, k, pd, final or 0, 0 if final is None else 1)
    out = np.full((len(sets), max(fde, 1)), 7.0, dtype=np.float32)
    st = np.full(max(len(sets), 1), -1, dtype=np.intc)
    sz, fp = C.POINTER(C.c_size_t), C.POINTER(C.c_float)
    rc = lib.vt_muvera_encode(0, mode, len(sets), set_off.ctypes.data_as(sz), values.ctypes.data_as(fp), val_off.ctypes.data_as(sz),
                              d, R, k, seed, pd, final or 0, 0 if final is None else 1, out.ctypes.data_as(fp),
                              st.ctypes.data_as(C.POINTER(C.c_int)) if statuses else None)
    return rc, out, (st[:len(sets)].tolist() if statuses else None)


def test_status_strings_are_the_references(lib):
    for code, text in STRINGS.items():
        assert lib.vt_strerror(code).decode() == text
    # every older status keeps its value and its string
    assert lib.vt_strerror(9).decode() == "vectors must not be empty" and lib.vt_strerror(10).decode() == "score overflow"
    assert lib.vt_strerror(19).decode() == "bad argument" and lib.vt_abi_version() == 4


def test_one_set_fails_like_the_nif_without_a_device(lib):
    """Every golden error case through the C ABI with count == 1: the reference's string, decided on the host."""
    for c in GOLDEN["cases"]:
        e = c["expect"]
        if "string" not in e:
            continue
        rc, _, _ = call(lib, [as_vectors(c["vectors"])], MODES[c["mode"]], *cfg_args(c["config"]))
        assert lib.vt_strerror(rc).decode() == e["string"], (c["name"], rc)


def test_validation_order_is_the_references(lib):
    one = [[1.0, 0.0]]
    order = [  # each row breaks one more rule, EARLIER in muvera.rs:76-106 / :29-42, than the row before
        (dict(sets=[[[1.0, float("inf")]]], R=MAX_OUT + 1, k=0, pd=1), "vector contains a non-finite value"),
        (dict(sets=[[[1.0, float("inf")], [1.0]]], R=MAX_OUT + 1, k=0, pd=1), "dimension mismatch"),
        (dict(sets=[[[1.0, float("inf")], [1.0]]], final=0), "final_projection_dimension must be positive"),
        (dict(sets=[[[1.0], [2.0, 3.0]]], pd=0, final=0), "projection_dimension must be positive"),
        (dict(sets=[one], k=31, pd=0, final=0), "num_simhash_projections must be < 31"),
        (dict(sets=[one], R=0, k=31, pd=0, final=0), "num_repetitions must be positive"),
        (dict(sets=[one], d=0, R=0, k=31, pd=0, final=0), "dimension must be positive"),
        (dict(sets=[[]], d=0, R=0, k=31, pd=0, final=0), "empty vectors"),
    ]
    for kw, text in order:
        a = dict(d=2, R=2, k=1, seed=42, pd=2, final=None)
        a.update(kw)
        rc, _, _ = call(lib, a["sets"], 0, a["d"], a["R"], a["k"], a["seed"], a["pd"], a["final"])
        assert lib.vt_strerror(rc).decode() == text, (kw, rc)
    # the sizes come last (muvera.rs:29-42), overflow before the limit
    assert call(lib, [one], 0, 2, MAX_OUT + 1, 0, 1, 1, None)[0] == CODE["fde dimension exceeds safety limit"]
    assert call(lib, [one], 0, 2, 1, 0, 1, 2, MAX_OUT + 1)[0] == CODE["fde dimension exceeds safety limit"]
    assert call(lib, [one], 0, 2, U64_MAX, 30, 1, 2, None)[0] == CODE["fde dimension overflow"]
    assert call(lib, [one], 0, 2, 2, 30, 1, U64_MAX, None)[0] == CODE["fde dimension overflow"]
    assert call(lib, [one], 0, 2, 1, 30, 1, 2, None)[0] == CODE["fde dimension exceeds safety limit"]
    # Some(0) is not None
    assert call(lib, [one], 0, 2, 1, 0, 1, 2, 0)[0] == 25 and call(lib, [one], 0, 2, 1, 0, 1, 2, None)[0] in (0, 17)
    # a mode that is none
    assert call(lib, [one], 2, 2, 1, 0, 1, 2, None)[0] == 19


def test_batches_report_per_set_without_a_device(lib):
    bad = [[], [[1.0]], [[float("nan"), 0.0]], [[1.0, 2.0, 3.0], [float("inf"), 0.0]]]
    rc, out, st = call(lib, bad, 1, 2, 1, 0, 1, 2, None, statuses=True)
    # no set is left for the device: the call succeeds, every row is zero
    assert rc == 0 and st == [20, 2, 3, 2] and not out.any()
    # without a place for statuses the first failing set's status is the call's
    assert call(lib, bad, 1, 2, 1, 0, 1, 2, None)[0] == 20
    assert call(lib, bad[1:], 1, 2, 1, 0, 1, 2, None)[0] == 2
    # an error of the configuration fails the whole call, whatever the sets are
    assert call(lib, bad, 1, 2, 0, 0, 1, 2, None, statuses=True)[0] == 22
    assert call(lib, bad, 1, 2, 1, 0, 1, 2, MAX_OUT + 1, statuses=True)[0] == 27
    assert call(lib, [], 1, 2, 0, 0, 1, 2, None)[0] == 22 and call(lib, [], 1, 2, 1, 0, 1, 2, None)[0] == 0
    if lib.vt_device_count() == 0:
        # no CPU fallback: a set that is valid needs the device
        rc, _, _ = call(lib, bad + [[[1.0, 0.0]]], 1, 2, 1, 0, 1, 2, None, statuses=True)
        assert rc == 17 and b"no CPU fallback" in lib.vt_last_error()


def test_fde_dimension_agrees_with_the_restatement(lib):
    rows = [(1, 0, 2, None), (2, 1, 2, None), (2, 1, 3, 5), (3, 4, 5, None), (20, 5, 16, None), (20, 5, 16, 2048),
            (MAX_OUT, 0, 1, None), (MAX_OUT + 1, 0, 1, None), (1, 24, 1, None), (1, 24, 2, None), (1, 30, 1, None),
            (2, 1, 2, MAX_OUT), (2, 1, 2, MAX_OUT + 1), (0, 1, 2, None), (1, 31, 2, None), (1, 1, 0, None), (1, 1, 2, 0),
            (U64_MAX, 30, 2, None)]
    for R, k, pd, final in rows:
        got = lib.vt_muvera_fde_dimension(R, k, pd, final or 0, 0 if final is None else 1)
        assert got == muvera_ref.fde_dimension(R, k, pd, final), (R, k, pd, final, got)
    from vettore_amd import nifs
    assert nifs.muvera_fde_dimension(20, 5, 16, None) == 10240 and nifs.muvera_fde_dimension(20, 5, 16, 2048) == 2048


# ---------------------------------------------------------------- the Python mirrors
def test_nifs_mirror_refuses_what_rustler_refuses():
    from vettore_amd import nifs
    assert nifs.muvera_encode_query([], 2, 1, 0, 42, 2, None) == ("error", "empty vectors")
    assert nifs.muvera_encode_document([[1.0]], 2, 1, 0, 42, 2, None) == ("error", "dimension mismatch")
    assert nifs.muvera_encode_query([[1.0, 0.0]], 2, 1, 0, U64_MAX, 2, 0) == ("error", "final_projection_dimension must be positive")
    for bad in ((2, 1, 0, -1, 2, None), (2, 1, 0, U64_MAX + 1, 2, None), (2, -1, 0, 1, 2, None), (2, 1, 0, 1, 2, -5),
                (2, 1.0, 0, 1, 2, None), (2, 1, 0, 1, 2, "nil")):
        with pytest.raises(TypeError):
            nifs.muvera_encode_query([[1.0, 0.0]], *bad)
    status, (matrix, reasons) = nifs.muvera_encode_batch([[], [[1.0]]], nifs.MUVERA_DOCUMENT, 2, 3, 1, 42, 2, None)
    assert status == "ok" and matrix.shape == (2, 12) and not matrix.any() and reasons == ["empty vectors", "dimension mismatch"]
    assert nifs.muvera_encode_batch([[]], nifs.MUVERA_QUERY, 2, 3, 1, 42, 2, None)[1][1] == ["empty vectors"]
    assert nifs.muvera_encode_batch([[[1.0, 0.0]], []], nifs.MUVERA_QUERY, 2, 0, 1, 42, 2, None) == ("error", "num_repetitions must be positive")


def test_muvera_module_returns_the_references_atoms():
    """test/vector_algorithms_hardening_test.exs:212-237, row by row."""
    from vettore_amd import muvera
    t = GOLDEN["elixir_atoms"]
    for config, atom in t["rows"]:
        config = [tuple(p) for p in config]
        assert muvera.encode_query(t["vectors"], config) == ("error", atom), (config, atom)
        assert muvera.encode_document(t["vectors"], config) == ("error", atom), (config, atom)
    for vectors, atom in t["vector_rows"]:
        assert muvera.encode_query(vectors) == ("error", atom), (vectors, atom)
    assert muvera.encode_document("bad") == ("error", t["not_a_list"])
    assert muvera.encode_query(t["vectors"], "bad") == ("error", "invalid_vectors")      # muvera.ex:51
    # keyword arguments spell the same configuration
    assert muvera.encode_query(t["vectors"], num_repetitions=0) == ("error", "invalid_repetitions")
    assert muvera.encode_query(t["vectors"], unknown=1) == ("error", "invalid_config")
    assert muvera.encode_query(t["vectors"], dimension=3) == ("error", "dimension_mismatch")
    # the batched extension: the configuration's errors fail the call, a set's own stay with the set
    assert muvera.encode_documents([t["vectors"]], num_repetitions=0) == ("error", "invalid_repetitions")
    assert muvera.encode_documents("bad") == ("error", "invalid_vectors")
    status, (matrix, atoms) = muvera.encode_documents([[], [1.0], [[1.0, "bad"]]], num_repetitions=2)
    assert status == "ok" and matrix.shape == (3, 2) and not matrix.any()
    assert atoms == ["empty_vectors", "invalid_vectors", "invalid_vectors"]
    assert muvera._native_error("encoding overflow") == "encoding_overflow" and muvera._native_error("x") == "x"


# ---------------------------------------------------------------- the shim
def test_the_shims_muvera_nifs_pass_the_shim_checks():
    import test_nif_shim as shim
    text = shim.strip_comments(open(shim.SHIM).read())
    table = {m.group(1): int(m.group(2)) for m in re.finditer(r'\{"([a-z0-9_]+)",\s*(\d+),\s*[a-z0-9_]+,', text)}
    assert table.get("muvera_encode_query") == 7 and table.get("muvera_encode_document") == 7
    shim.test_shim_compiles_against_the_header()
    shim.test_every_library_call_matches_its_declaration()
    shim.test_elixir_stubs_and_nif_table_agree()
    shim.test_no_nif_without_a_caller_in_the_adapter()
    assert len(shim.call_sites(text, "vt_muvera_encode")) == 1 and len(shim.call_sites(text, "vt_muvera_fde_dimension")) == 1
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "muvera_encode_query/7" in doc and "muvera_encode_document/7" in doc


def test_the_shims_muvera_nifs_decode_like_rustler():
    """nil | integer as the last argument, a full u64 seed, and the reference's strings as {:error, binary} --
    through the fake term runtime with interned atoms (tests/muvera_nif_runtime.py)."""
    import muvera_nif_runtime as R
    rt = R.Runtime()
    assert ("muvera_encode_query", 7) in rt.functions() and ("muvera_encode_document", 7) in rt.functions()
    err = R.Atom("error")
    for name in ("muvera_encode_query", "muvera_encode_document"):
        assert rt.call(name, [], 2, 1, 0, 42, 2, None) == (err, b"empty vectors")
        assert rt.call(name, [[1.0, 0.0]], 2, 1, 0, U64_MAX, 2, 0) == (err, b"final_projection_dimension must be positive")
        assert rt.call(name, [[1.0, 0.0]], 2, 0, 0, 0, 2, None) == (err, b"num_repetitions must be positive")
        assert rt.call(name, [[1.0, 0.0], [1.0]], 2, 1, 0, 1, 2, 5) == (err, b"dimension mismatch")
        assert rt.call(name, [[1.0, 0.0]], 2, MAX_OUT + 1, 0, 1, 1, None) == (err, b"fde dimension exceeds safety limit")
        for bad_final in (R.Atom("none"), R.Atom("undefined"), 1.5, -1, [], b"nil"):
            with pytest.raises(R.ArgumentError):
                rt.call(name, [[1.0, 0.0]], 2, 1, 0, 42, 2, bad_final)
        for bad in (([1.0, 0.0], 2, 1, 0, 42, 2, None), ([[1, 0]], 2, 1, 0, 42, 2, None), ([[1.0, 0.0]], -2, 1, 0, 42, 2, None),
                    ([[1.0, 0.0]], 2, 1, 0, -1, 2, None), ([[1.0, 0.0]], 2, 1, 0, 1.0, 2, None), ([[1.0, 0.0]], 2, None, 0, 1, 2, None)):
            with pytest.raises(R.ArgumentError):
                rt.call(name, *bad)
    lib = C.CDLL(os.path.join(ROOT, "vettore_amd", "lib", "libvettore_hip.so"))
    if lib.vt_device_count() == 0:
        tag, msg = rt.call("muvera_encode_query", [[1.0, 0.0], [0.0, 1.0]], 2, 1, 0, 42, 2, None)
        assert tag == err and b"no HIP device" in msg
    else:
        assert rt.call("muvera_encode_query", [[1.0, 0.0], [0.0, 1.0]], 2, 1, 0, 42, 2, None) == (R.Atom("ok"), [1.0, 1.0])
