"""The per-device session behind the calls without an index handle (host/vt_stateless.h) -- `-m gpu`: the upload ring
shared by MaxSim (K9) and MUVERA (K10) under alternating tenants, the lease under four threads, and the "first refused
row" walk of vector_top_k above its thread grain.  Every expected value comes from tests/maxsim_ref.py,
tests/muvera_ref.py or the oracle, bit for bit: the session only moves bytes and orders streams."""
import ctypes as C
import threading

import numpy as np
import pytest

import maxsim_ref
import muvera_ref
from test_gpu_multi_vector import assert_same_hits, vectors
from test_gpu_muvera import random_set
from test_gpu_parity import bits, nifs  # noqa: F401  (nifs: a fixture)

pytestmark = pytest.mark.gpu

DOT, COSINE, L2 = 3, 2, 0
MUVERA_ARGS = (8, 3, 3, 42, 4)   # d, repetitions, simhash projections, seed, projection dimension
MUVERA_CASES = [(mode, final) for mode in (muvera_ref.DOCUMENT, muvera_ref.QUERY) for final in (None, 37)]


def maxsim_chunks(sizes, chunk_rows):
    """vt_maxsim.h's cut: a chunk is as many documents as fit in `chunk_rows` vectors, at least one."""
    chunks, i = 0, 0
    while i < len(sizes):
        j = i + 1
        while j < len(sizes) and sum(sizes[i:j + 1]) <= chunk_rows:
            j += 1
        chunks, i = chunks + 1, j
    return chunks


@pytest.fixture(scope="module")
def workload(oracle_mod):
    """The two tenants' inputs and their references, computed once: MaxSim over 31 documents of 0-6 vectors (d = 9 and
    d = 17, inner product and cosine), MUVERA over 12 sets of 1-5 vectors with a refused set in the middle."""
    rng = np.random.default_rng(20261017)
    sizes = [int(s) for s in rng.integers(0, 7, size=31)]
    assert 0 in sizes and 6 in sizes, sizes
    w = {"sizes": sizes, "maxsim": {}, "muvera": {}}
    for d in (9, 17):
        docs = [("doc-%02d" % i, vectors(rng, t, d, DOT)) for i, t in enumerate(sizes)]
        query = vectors(rng, 4, d, DOT)
        for metric in (DOT, COSINE):
            w["maxsim"][d, metric] = (docs, query, maxsim_ref.top_k(docs, query, metric, len(docs)))
    sets = [random_set(rng, int(rng.integers(1, 6)), MUVERA_ARGS[0]) for _ in range(12)]
    sets[6] = [sets[6][0], sets[6][0][:-1]]   # "dimension mismatch": a chunk of its own without a vector
    w["sets"] = sets
    for mode, final in MUVERA_CASES:
        want = [muvera_ref.encode(s, *MUVERA_ARGS, final, mode) for s in sets]
        assert [x[0] for x in want] == ["ok"] * 6 + ["error"] + ["ok"] * 5
        fde = muvera_ref.fde_dimension(*MUVERA_ARGS[1:3], MUVERA_ARGS[4], final)
        matrix = np.stack([np.asarray(x[1], dtype=np.float32) if x[0] == "ok" else np.zeros(fde, np.float32) for x in want])
        w["muvera"][mode, final] = (matrix, [None if x[0] == "ok" else x[1] for x in want])
    return w


def one_vector_chunks(vt_debug):
    vt_debug.set("maxsim_chunk_bytes", 36)   # one vector at d = 9, less than one (so: one) at d = 17
    vt_debug.set("muvera_chunk_bytes", 1)    # one set


def check_maxsim(nifs, w, d, metric):
    docs, query, want = w["maxsim"][d, metric]
    assert_same_hits(nifs.multi_vector_top_k(docs, query, metric, len(docs)), want, ("maxsim", d, metric))


def check_muvera(nifs, w, mode, final):
    matrix, reasons = w["muvera"][mode, final]
    status, (got, got_reasons) = nifs.muvera_encode_batch(w["sets"], mode, *MUVERA_ARGS, final)
    assert status == "ok" and got_reasons == reasons, (mode, final, got_reasons)
    assert got.shape == matrix.shape and got.tobytes() == matrix.tobytes(), (mode, final)


def test_the_ring_survives_a_change_of_tenant(nifs, vt_debug, workload):
    w = workload
    # an odd number of MaxSim chunks and an even number of MUVERA chunks (one per set, the refused one included):
    # each tenant's last upload went through the slot the other one's last did not
    assert maxsim_chunks(w["sizes"], 1) % 2 == 1 and maxsim_chunks(w["sizes"], 1) > 3, maxsim_chunks(w["sizes"], 1)
    assert len(w["sets"]) % 2 == 0
    one_vector_chunks(vt_debug)

    def maxsim(d):
        for metric in (DOT, COSINE):
            check_maxsim(nifs, w, d, metric)

    def muvera():
        for mode, final in MUVERA_CASES:
            check_muvera(nifs, w, mode, final)

    maxsim(9)
    muvera()
    maxsim(9)
    maxsim(17)   # staging and device blocks regrow after MUVERA sized them
    muvera()


def test_the_lease_serialises_four_threads(nifs, oracle_mod, vt_debug, workload):
    from vettore_amd import _lib
    w, lib = workload, _lib.load()
    one_vector_chunks(vt_debug)
    rng = np.random.default_rng(4)
    plain = rng.uniform(-1, 1, size=(3, 5)).astype(np.float32)
    plain_want = np.stack([oracle_mod.normalize_l2(r) for r in plain])
    rows = [("row-%02d" % i, list(map(float, r))) for i, r in enumerate(rng.uniform(-1, 1, size=(40, 7)).astype(np.float32))]
    probe = list(map(float, rng.uniform(-1, 1, size=7).astype(np.float32)))
    rows_want = {m: bits(oracle_mod.vector_top_k(rows, probe, m, 7, 10)) for m in (COSINE, L2)}

    def normalize(i):
        out = np.empty_like(plain)
        fp = C.POINTER(C.c_float)
        st = lib.vt_normalize_l2(nifs.DEVICE, 3, 5, plain.ctypes.data_as(fp), out.ctypes.data_as(fp))
        assert st == 0 and out.tobytes() == plain_want.tobytes(), (i, st)

    def top_k(i):
        m = (COSINE, L2)[i % 2]
        got = nifs.vector_top_k(rows, probe, m, 7, 10)
        assert got[0] == "ok" and bits(got[1]) == rows_want[m], (i, m)

    kinds = [normalize, top_k, lambda i: check_maxsim(nifs, w, 9, (DOT, COSINE)[i % 2]),
             lambda i: check_muvera(nifs, w, *MUVERA_CASES[i % 4])]
    done, failures = [0] * len(kinds), []

    def worker(t):
        try:
            for i in range(20):
                kinds[t](i)
                done[t] += 1
        except BaseException as e:  # noqa: B036  (an assertion in a thread has to reach the test)
            failures.append((t, done[t], repr(e)))

    threads = [threading.Thread(target=worker, args=(t,), daemon=True) for t in range(len(kinds))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), ("a thread is still running", done)
    assert not failures and done == [20] * 4, (failures, done)


def test_the_first_refused_row_above_the_thread_grain(nifs, oracle_mod):
    """1 100 rows: two grains of 512 and a tail, so the walk runs on several threads.  The earliest refused row decides,
    whichever thread finds it, and a device error among the rows before it comes first."""
    rng = np.random.default_rng(1100)
    base = [("r%04d" % i, list(map(float, r))) for i, r in enumerate(rng.uniform(-1, 1, size=(1100, 4)).astype(np.float32))]
    query = list(map(float, rng.uniform(-1, 1, size=4).astype(np.float32)))
    short = lambda r: (r[0], r[1][:3])                          # noqa: E731
    nan = lambda r: (r[0], r[1][:2] + [float("nan")] + r[1][3:])  # noqa: E731

    def expect(rows, q, text):
        with pytest.raises(oracle_mod.OracleError) as e:
            oracle_mod.vector_top_k(rows, q, L2, 4, 5)
        assert str(e.value) == text
        assert nifs.vector_top_k(rows, q, L2, 4, 5) == ("error", text)

    rows = list(base)
    rows[700], rows[900] = short(rows[700]), nan(rows[900])
    expect(rows, query, "dimension mismatch")
    rows = list(base)
    rows[700], rows[900] = nan(rows[700]), short(rows[900])
    expect(rows, query, "vector contains a non-finite value")
    rows = list(base)
    rows[3], rows[700] = (rows[3][0], [3.0e38] * 4), short(rows[700])   # (3e38 - -3e38)^2 is not an f32
    expect(rows, [-3.0e38] * 4, "metric overflow")
    want = oracle_mod.vector_top_k(base, query, L2, 4, 5)               # ... and nothing refused: the plain answer
    got = nifs.vector_top_k(base, query, L2, 4, 5)
    assert got[0] == "ok" and bits(got[1]) == bits(want)
