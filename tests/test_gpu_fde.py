"""MUVERA retrieval over a resident multi-vector store (vt_mv_encode_documents, vt_mv_fde_sync, vt_mv_fde_top_k,
vt_mv_fde_top_k_batch; K10s in vt_muvera.hip) -- `-m gpu`.  Expected values come from the three reference models
(tests/muvera_ref.py, tests/maxsim_ref.py, the oracle's FlatIndex), never from the code under test; comparisons with the
existing public calls (vt_muvera_encode, vt_flat_search, vt_mv_top_k_ids, vt_mv_top_k) are a second, independent check.
Tolerance zero everywhere: ids, order and float32 bits.

The store of every case has been through upserts, deletes and one compaction before the calls under test, so dead rows
lie between live ones and first rows are not cumulative; d = 6 has a live pad (row stride 8)."""
import ctypes as C
import functools

import numpy as np
import pytest

import maxsim_ref
import muvera_ref
from test_gpu_parity import nifs  # noqa: F401  (a fixture)
from test_gpu_mv_store import ref_order  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

IP = 3
FMAX = float(np.finfo(np.float32).max)
# (dimension, repetitions, SimHash projections, seed, projection dimension, final) -- each reaches one path of K10s
CASES = {
    "identity": (6, 1, 0, 7, 6, None),            # C == 0: no table column at all
    "grouped": (6, 3, 3, 11, 4, None),            # several repetitions per wave
    "identity_simhash": (16, 20, 5, 42, 16, None),  # identity behind SimHash
    "wide": (100, 2, 4, 5, 70, None),             # C > 64: the wave walks the columns in passes
    "global_counts": (16, 1, 13, 9, 2, None),     # 8 192 partitions: counts in device memory
    "sketch": (16, 3, 3, 11, 4, 64),              # the count sketch behind the encode
}


def f32bits(x):
    return np.float32(x).tobytes()


def vecs(rng, n, d):
    return [list(map(float, r)) for r in rng.uniform(-1, 1, size=(n, d)).astype(np.float32)]


class Corpus:
    """The live documents of a store, in store order, as a Python dict beside the store that holds them."""

    def __init__(self, d, seed):
        from vettore_amd.mv_store import ResidentMultiVector
        self.d, self.rng = d, np.random.default_rng(seed)
        self.store = ResidentMultiVector()
        self.docs = {}   # id -> vectors, in the order of the last put

    def put(self, docs):
        assert self.store.put_many(docs) == "ok"
        for i, v in docs:   # (the last of equal ids is the one stored)
            self.docs.pop(i, None)
        for i, v in docs:
            self.docs.pop(i, None)
            self.docs[i] = v

    def delete(self, i):
        assert self.store.delete(i) == "ok"
        self.docs.pop(i, None)

    def ids(self):
        return list(self.docs)

    def live(self):
        return list(self.docs.items())


def build_corpus(d, seed=0):
    """About 300 documents of 0..12 vectors, a few with none; 200 long documents come and go in between so that one
    put compacts; upserts and deletes afterwards leave dead rows between live ones."""
    c = Corpus(d, 4000 + d + seed)
    rng = c.rng

    def doc(i):
        n = 0 if i % 50 == 7 else int(rng.integers(1, 13))
        return ("doc-%03d" % i, vecs(rng, n, d))
    c.put([doc(i) for i in range(150)])
    c.put([("tmp-%03d" % i, vecs(rng, 12, d)) for i in range(200)])
    c.put([doc(i) for i in range(150, 300)])
    for i in range(200):
        c.delete("tmp-%03d" % i)
    before = c.store.memory()
    assert before["dead_rows"] > before["vectors"]
    c.put([doc(i) for i in range(0, 300, 5)])          # this put compacts first; 60 upserts move to the end
    assert c.store.memory()["compactions"] == before["compactions"] + 1
    for i in range(3, 300, 15):
        c.delete("doc-%03d" % i)
    c.put([doc(i) for i in range(1, 300, 10)])         # (doc-007's successors among them: some lose, some gain vectors)
    c.put([("doc-002", [])])                           # a document that had vectors and has none now
    mem = c.store.memory()
    assert mem["dead_rows"] > 0 and len(c.store) == len(c.docs)
    firsts = sum(len(v) for v in c.docs.values())
    assert firsts == mem["vectors"]
    return c


def reference_rows(docs, cfg):
    """{id: ("ok", row) | ("error", reason)} from the model."""
    return {i: (muvera_ref.encode_document(v, *cfg) if v else ("error", "empty vectors")) for i, v in docs}


@functools.lru_cache(maxsize=None)
def base_reference(case):
    """The reference encodings of build_corpus's documents: computed once per case, shared, never changed."""
    cfg = CASES[case]
    c = build_corpus(cfg[0])
    return reference_rows(c.live(), cfg)


def doc_bytes(cfg):
    """What one document takes of a chunk's budget (host/vt_fde.h): intermediate row, final row, device counts, two words."""
    d, R, k, seed, pd, final = cfg
    out = R * (1 << k) * pd
    return (out + (final or 0) + (out // pd if (1 << k) > 4096 else 0)) * 4 + 8


def force_chunks(vt_debug, cfg, ndocs):
    """A budget under which `ndocs` documents span at least three chunks."""
    per = max(1, (ndocs - 1) // 3)
    vt_debug.set("muvera_chunk_bytes", doc_bytes(cfg) * per)
    assert -(-ndocs // per) >= 3


def oracle_index(oracle_mod, rows):
    ix = oracle_mod.FlatIndex(IP)
    good = [(i, r[1]) for i, r in rows.items() if r[0] == "ok"]
    ix.insert_matrix([i for i, _ in good], np.stack([r for _, r in good]))
    return ix


def same_hits(got, want, ctx):
    assert got[0] == "ok", (ctx, got)
    assert [h[0] for h in got[1]] == [h[0] for h in want], ctx
    assert [f32bits(h[1]) for h in got[1]] == [f32bits(h[1]) for h in want], ctx


def refused(res, reason):
    """("error", reason), or reason + ": " + the library's detail (statuses that carry one)."""
    return res[0] == "error" and (res[1] == reason or res[1].startswith(reason + ": "))


def fde_dim(cfg):
    return muvera_ref.fde_dimension(cfg[1], cfg[2], cfg[4], cfg[5])


def with_overflow(c, cfg, always=False):
    """The inputs the existing MUVERA tests overflow with, where the model says they overflow under `cfg` (an identity
    projection averages them to FLT_MAX instead: a row no inner-product search could be asked about) or where only the
    encoding is looked at (`always`)."""
    ovf = [[FMAX] * cfg[0]] * 3
    if always or muvera_ref.encode_document(ovf, *cfg)[0] == "error":
        c.put([("doc-ovf", ovf)])


# ------------------------------------------------------------------------------------------------ 1. the encodings
@pytest.mark.parametrize("case", list(CASES))
def test_encode_documents_bits(nifs, vt_debug, case):
    cfg = CASES[case]
    c = build_corpus(cfg[0])
    want = dict(base_reference(case))
    assert list(want) == c.ids()
    with_overflow(c, cfg, always=True)
    want["doc-ovf"] = muvera_ref.encode_document(c.docs["doc-ovf"], *cfg)
    if case in ("grouped", "sketch", "wide"):
        assert want["doc-ovf"] == ("error", "encoding overflow")
    ids = c.ids() + ["no-such-doc", "doc-003", "tmp-005", "doc-000", ""]   # unknown, deleted, deleted, a duplicate, the empty id
    assert "doc-003" not in c.docs and "doc-000" in c.docs
    encodable = sum(1 for i in ids if i in c.docs and c.docs[i])
    force_chunks(vt_debug, cfg, encodable)
    status, (matrix, reasons) = nifs.mv_encode_documents(c.store.ref, ids, cfg)
    assert status == "ok" and matrix.shape == (len(ids), fde_dim(cfg)) and matrix.dtype == np.float32
    kinds = set()
    for k, i in enumerate(ids):
        w = want.get(i, ("error", "empty vectors"))
        if w[0] == "ok":
            assert reasons[k] is None and matrix[k].tobytes() == np.asarray(w[1], np.float32).tobytes(), (case, i)
        else:
            assert reasons[k] == w[1] and not matrix[k].any(), (case, i, reasons[k])
        kinds.add(w[1] if w[0] == "error" else "ok")
    assert {"ok", "empty vectors"} <= kinds
    # the same vectors through vt_muvera_encode: the same bytes, the same statuses
    sets = [c.docs.get(i, []) for i in ids]
    status, (stateless, stateless_reasons) = nifs.muvera_encode_batch(sets, muvera_ref.DOCUMENT, *cfg)
    assert status == "ok" and stateless.tobytes() == matrix.tobytes() and stateless_reasons == reasons
    # one chunk for all of them: the same bytes
    vt_debug.reset("muvera_chunk_bytes")
    status, (whole, whole_reasons) = nifs.mv_encode_documents(c.store.ref, ids, cfg)
    assert status == "ok" and whole.tobytes() == matrix.tobytes() and whole_reasons == reasons


def test_encode_documents_statuses(nifs):
    import vettore_amd._lib as L
    lib = L.load()
    cfg = CASES["grouped"]
    c = build_corpus(cfg[0])
    with_overflow(c, cfg)
    # one document: its status is the call's
    status, (row, reasons) = nifs.mv_encode_documents(c.store.ref, ["no-such-doc"], cfg)
    assert status == "ok" and reasons == ["empty vectors"] and row.shape == (1, 96) and not row.any()
    assert nifs.mv_encode_documents(c.store.ref, ["doc-ovf"], cfg)[1][1] == ["encoding overflow"]
    # no place for statuses: the first failing document's, in list order
    ids = [c.ids()[0], "doc-ovf", "no-such-doc"]
    assert all(c.docs[i] for i in ids[:2])
    idb, off = nifs._pack_ids(ids)
    out = np.ones((3, 96), dtype=np.float32)
    args = (6, 3, 3, 11, 4, 0, 0)
    fp, sz = C.POINTER(C.c_float), C.POINTER(C.c_size_t)
    h = c.store.ref.handle
    assert lib.vt_mv_encode_documents(h, 3, idb, off.ctypes.data_as(sz), *args, out.ctypes.data_as(fp), None) == 28
    assert out[0].tobytes() == np.asarray(base_reference("grouped")[ids[0]][1]).tobytes() and not out[1:].any()
    # call-level checks, in order: NULLs, the configuration, the sizes, the store's dimension
    assert lib.vt_mv_encode_documents(h, 3, idb, None, 0, 3, 3, 11, 4, 0, 0, out.ctypes.data_as(fp), None) == 19
    assert lib.vt_mv_encode_documents(h, 3, idb, off.ctypes.data_as(sz), 0, 0, 3, 11, 4, 0, 0, out.ctypes.data_as(fp), None) == 21
    assert lib.vt_mv_encode_documents(h, 3, idb, off.ctypes.data_as(sz), 7, 0, 3, 11, 4, 0, 0, out.ctypes.data_as(fp), None) == 22
    assert lib.vt_mv_encode_documents(h, 3, idb, off.ctypes.data_as(sz), 7, 1 << 20, 30, 11, 4, 0, 0, out.ctypes.data_as(fp), None) == 27
    assert lib.vt_mv_encode_documents(h, 3, idb, off.ctypes.data_as(sz), 7, 3, 3, 11, 4, 0, 0, out.ctypes.data_as(fp), None) == 2
    assert lib.vt_mv_encode_documents(h, 0, None, None, 6, 3, 3, 11, 4, 0, 0, None, None) == 0


# ------------------------------------------------------------------------------------------------ 2. the whole store
def search_checks(nifs, oracle_mod, index, rows, cfg, rng, ctx):
    """`index` against the oracle's FlatIndex over the model's rows: one-hot queries read every column back where the
    encoding is short, eight query encodings otherwise."""
    want_ix = oracle_index(oracle_mod, rows)
    n, fde = len(want_ix), fde_dim(cfg)
    assert len(index) == n
    if fde <= 64:
        for j in range(fde):
            e = np.zeros(fde, dtype=np.float32)
            e[j] = 1.0
            got = nifs.flat_search(index, e, n)
            same_hits(got, want_ix.search(e, n), (ctx, j))
            assert len(got[1]) == n
            for i, raw in got[1]:   # the raw value IS column j (x * 1 + 0 * the rest; a zero's sign is the oracle's to say)
                v = rows[i.decode()][1][j]
                assert raw == float(v) and (v == 0 or f32bits(raw) == f32bits(v)), (ctx, j, i)
    else:
        for t in range(8):
            q = muvera_ref.encode_query(vecs(rng, 1 + t, cfg[0]), *cfg)
            assert q[0] == "ok"
            same_hits(nifs.flat_search(index, q[1], 17), want_ix.search(q[1], 17), (ctx, t))


@pytest.mark.parametrize("case", list(CASES))
def test_sync_of_the_whole_store(nifs, oracle_mod, ref_order, vt_debug, case):
    cfg = CASES[case]
    c = build_corpus(cfg[0])
    with_overflow(c, cfg)
    rows = dict(base_reference(case))
    if "doc-ovf" in c.docs:
        rows["doc-ovf"] = muvera_ref.encode_document(c.docs["doc-ovf"], *cfg)
    assert ("doc-ovf" in c.docs) == (case in ("grouped", "sketch", "wide", "global_counts"))
    index = nifs.flat_new_inner_product()
    force_chunks(vt_debug, cfg, sum(1 for v in c.docs.values() if v))
    assert c.store.fde_sync(index, None, cfg) == ("ok", [])
    encodable = sum(1 for r in rows.values() if r[0] == "ok")
    assert len(index) == encodable and index.dimension == fde_dim(cfg)
    assert encodable < len(c.docs)   # (documents without vectors, and the overflow where the model says so)
    search_checks(nifs, oracle_mod, index, rows, cfg, c.rng, case)
    # listing every id says which ones stayed out
    status, reasons = c.store.fde_sync(index, c.ids(), cfg)
    assert status == "ok" and reasons == [None if rows[i][0] == "ok" else rows[i][1] for i in c.ids()]
    assert len(index) == encodable


# ------------------------------------------------------------------------------------------------ 3. a subset
def dump(nifs, index, fde):
    """{id: row bytes} of an index of short rows, read back column by column."""
    n = len(index)
    cols = {}
    for j in range(fde):
        e = np.zeros(fde, dtype=np.float32)
        e[j] = 1.0
        status, hits = nifs.flat_search(index, e, n)
        assert status == "ok" and len(hits) == n
        for i, raw in hits:
            cols.setdefault(i.decode(), [0.0] * fde)[j] = raw
    return {i: np.asarray(r, np.float32) for i, r in cols.items()}


@pytest.mark.parametrize("case", ["sketch", "identity"])
def test_sync_of_a_subset(nifs, vt_debug, case):
    cfg = CASES[case]
    fde = fde_dim(cfg)
    c = build_corpus(cfg[0])
    index = nifs.flat_new_inner_product()
    assert c.store.fde_sync(index, None, cfg) == ("ok", [])
    before = dump(nifs, index, fde)
    base = base_reference(case)
    assert set(before) == {i for i, r in base.items() if r[0] == "ok"}
    with_vectors = [i for i in c.ids() if c.docs[i]]
    gone, emptied, overflowing, changed, untouched = with_vectors[3], with_vectors[40], with_vectors[77], with_vectors[120], with_vectors[200]
    c.delete(gone)
    c.put([(emptied, []), (overflowing, [[FMAX] * cfg[0]] * 3), (changed, vecs(c.rng, 5, cfg[0])), ("doc-new", vecs(c.rng, 12, cfg[0]))])
    c.put([(untouched, vecs(c.rng, 2, cfg[0]))])   # changed in the store, NOT listed: the index keeps its old row
    listed = [gone, emptied, overflowing, changed, changed, "doc-new", "never-there", changed]
    model = {i: muvera_ref.encode_document(c.docs[i], *cfg) for i in (overflowing, changed, "doc-new")}
    if case == "sketch":
        assert model[overflowing] == ("error", "encoding overflow")
    want_reasons = [None, "empty vectors", None if model[overflowing][0] == "ok" else model[overflowing][1], None, None, None, None, None]
    want = dict(before)
    for i in (gone, emptied, overflowing):
        del want[i]
    for i, r in model.items():
        if r[0] == "ok":
            want[i] = np.asarray(r[1], np.float32) + np.float32(0.0)   # (read back through a dot product: -0.0 comes back +0.0)
    vt_debug.set("muvera_chunk_bytes", doc_bytes(cfg))   # one document a chunk
    for again in range(2):
        status, reasons = c.store.fde_sync(index, listed, cfg)
        assert status == "ok" and reasons == want_reasons, (again, reasons)
        after = dump(nifs, index, fde)
        assert set(after) == set(want), again
        for i in want:
            assert after[i].tobytes() == want[i].tobytes(), (again, i)


# ------------------------------------------------------------------------------------------------ 4. the search
def composition(oracle_mod, c, rows, cfg, query, candidates, metric, limit):
    """The four steps from the three models."""
    q = muvera_ref.encode_query(query, *cfg)
    assert q[0] == "ok"
    found = {i for i, _ in oracle_index(oracle_mod, rows).search(q[1], candidates)} if candidates else set()
    docs = [(i, v) for i, v in c.live() if i.encode() in found]
    return maxsim_ref.top_k(docs, query, metric, limit)


@pytest.mark.parametrize("case", ["grouped", "wide"])
def test_top_k_is_the_composition(nifs, oracle_mod, ref_order, case):
    cfg = CASES[case]
    c = build_corpus(cfg[0])
    rows = base_reference(case)
    index = nifs.flat_new_inner_product()
    assert c.store.fde_sync(index, None, cfg) == ("ok", [])
    for metric in (maxsim_ref.COSINE, maxsim_ref.INNER_PRODUCT, maxsim_ref.NEGATIVE_INNER_PRODUCT):
        for nq, candidates, limit in ((4, 25, 10), (1, 7, 7), (3, 12, 40)):
            query = vecs(c.rng, nq, cfg[0])
            got = nifs.mv_fde_top_k(c.store.ref, index, cfg, query, candidates, metric, limit, with_keys=True)
            want = composition(oracle_mod, c, rows, cfg, query, candidates, metric, limit)
            same_hits(got, want, (case, metric, nq))
            assert len(got[1]) == min(limit, candidates)
            # ... and of the public calls it joins
            status, qf = nifs.muvera_encode_query(query, *cfg)
            assert status == "ok"
            status, found = nifs.flat_search(index, qf, candidates)
            assert status == "ok" and len(found) == candidates
            assert nifs.mv_top_k_ids(c.store.ref, [i for i, _ in found], query, metric, limit, with_keys=True) == got
    # every document of the index a candidate: MaxSim over the documents that have vectors
    query = vecs(c.rng, 5, cfg[0])
    n = len(index)
    for candidates in (n, n + 5):
        got = c.store.fde_top_k(index, cfg, query, candidates, IP, n + 5)
        status, everything = c.store.top_k(query, IP, len(c.store))
        assert status == "ok" and got == ("ok", [h for h in everything if c.docs[h[0].decode()]])
        assert len(got[1]) == n


def test_top_k_statuses_in_order(nifs):
    cfg = CASES["grouped"]
    bad_cfg = (6, 0, 3, 11, 4, None)
    c = build_corpus(cfg[0])
    store = c.store
    index, empty = nifs.flat_new_inner_product(), nifs.flat_new_inner_product()
    assert store.fde_sync(index, None, cfg) == ("ok", [])
    query = vecs(c.rng, 3, 6)
    assert store.fde_top_k(index, cfg, query, 20, IP, 0) == ("ok", [])         # limit 0: all the work, an empty list
    assert store.fde_top_k(index, cfg, query, 0, IP, 5) == ("ok", [])          # no candidate
    assert store.fde_top_k(empty, cfg, query, 20, IP, 5) == ("ok", [])         # an empty index
    assert store.fde_top_k(index, cfg, [], 20, IP, 5) == ("error", "empty vectors")
    assert store.fde_top_k(index, cfg, vecs(c.rng, 2, 7), 20, IP, 5) == ("error", "dimension mismatch")
    # the order: the index, the metric, the query on its own, its length against the store, the encoding's own checks
    cosine = nifs.flat_new_cosine()
    assert refused(store.fde_top_k(cosine, cfg, query, 20, 99, 5), "bad argument")
    assert store.fde_top_k(index, cfg, [[1.0, float("nan")]], 20, 99, 5) == ("error", "unknown metric")
    assert store.fde_top_k(index, bad_cfg, [[1.0] * 6, [1.0] * 5], 20, IP, 5) == ("error", "dimension mismatch")
    assert store.fde_top_k(index, bad_cfg, vecs(c.rng, 2, 7), 20, IP, 5) == ("error", "dimension mismatch")
    assert store.fde_top_k(index, bad_cfg, [], 20, IP, 5) == ("error", "empty vectors")
    assert store.fde_top_k(index, bad_cfg, query, 20, IP, 5) == ("error", "num_repetitions must be positive")
    assert store.fde_top_k(empty, bad_cfg, query, 20, IP, 5) == ("error", "num_repetitions must be positive")
    # an overflowing query: vt_muvera_encode's status
    assert muvera_ref.encode_query([[FMAX] * 6] * 3, *cfg) == ("error", "encoding overflow")
    assert store.fde_top_k(index, cfg, [[FMAX] * 6] * 3, 20, maxsim_ref.COSINE, 5) == ("error", "encoding overflow")
    assert len(index) == sum(1 for v in c.docs.values() if v)


# ------------------------------------------------------------------------------------------------ 5. many query sets
def test_batch_equals_the_lone_calls(nifs):
    import vettore_amd._lib as L
    cfg = CASES["grouped"]
    c, twin = build_corpus(cfg[0]), build_corpus(cfg[0])
    assert c.live() == twin.live()
    index = nifs.flat_new_inner_product()
    assert c.store.fde_sync(index, None, cfg) == ("ok", [])
    rng = np.random.default_rng(77)
    sets = [vecs(rng, n, 6) for n in (4, 9, 1, 3, 12, 2, 5, 8, 6)]   # (one with a single vector)
    sets[3][1][2] = float("nan")                                      # one invalid
    candidates, limit = 30, 10
    for metric in (IP, maxsim_ref.COSINE):
        lone = [nifs.mv_fde_top_k(c.store.ref, index, cfg, s, candidates, metric, limit, with_keys=True) for s in sets]
        assert lone[3] == ("error", "vector contains a non-finite value") and sum(r[0] == "ok" for r in lone) == 8
        assert all(len(r[1]) == limit for r in lone if r[0] == "ok")
        before = c.store.counters()["batched_sets"]
        got = nifs.mv_fde_top_k_batch(c.store.ref, index, cfg, sets, candidates, metric, limit, with_keys=True)
        grown = c.store.counters()["batched_sets"] - before
        assert got == lone
        # the rerank is the batched one: the same candidate lists through vt_mv_top_k_ids_batch on an identical store
        valid = [s for k, s in enumerate(sets) if k != 3]
        lists = []
        for s in valid:
            status, qf = nifs.muvera_encode_query(s, *cfg)
            assert status == "ok"
            lists.append([i for i, _ in nifs.flat_search(index, qf, candidates)[1]])
        before = twin.store.counters()["batched_sets"]
        direct = nifs.mv_top_k_ids_batch(twin.store.ref, lists, valid, metric, limit, with_keys=True)
        assert direct == [r for k, r in enumerate(lone) if k != 3]
        assert grown == twin.store.counters()["batched_sets"] - before
    # nothing to do, and the conventions of vt_mv_top_k_ids_batch
    assert nifs.mv_fde_top_k_batch(c.store.ref, index, cfg, [], candidates, IP, limit) == []
    assert nifs.mv_fde_top_k_batch(c.store.ref, index, cfg, sets, candidates, 99, limit) == ("error", "unknown metric")
    assert nifs.mv_fde_top_k_batch(c.store.ref, index, cfg, sets[:1], candidates, IP, limit, with_keys=True) == [lone_ip(nifs, c, index, cfg, sets[0], candidates, limit)]
    qv, qoff, set_off = nifs._pack_sets(sets)
    outs = (C.c_void_p * 9)()
    fp, sz = C.POINTER(C.c_float), C.POINTER(C.c_size_t)
    st = L.load().vt_mv_fde_top_k_batch(c.store.ref.handle, index.handle, 6, 3, 3, 11, 4, 0, 0, 9, set_off.ctypes.data_as(sz),
                                        qv.ctypes.data_as(fp), qoff.ctypes.data_as(sz), candidates, IP, limit, outs, None)
    assert st == 3 and not any(outs)   # no place for statuses: the first failing set's, every list dropped


def lone_ip(nifs, c, index, cfg, s, candidates, limit):
    return nifs.mv_fde_top_k(c.store.ref, index, cfg, s, candidates, IP, limit, with_keys=True)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_index_alone(nifs):
    import vettore_amd._lib as L
    lib = L.load()
    cfg = CASES["grouped"]
    c = build_corpus(cfg[0])
    query = vecs(c.rng, 2, 6)
    cosine = nifs.flat_new_cosine()
    assert nifs.flat_insert(cosine, "x", [1.0] * 96) == ("ok", ())
    other = nifs.flat_new_inner_product()
    assert nifs.flat_insert(other, "x", [1.0, 2.0, 3.0]) == ("ok", ())
    for index, reason in ((cosine, "bad argument"), (other, "dimension mismatch")):
        assert refused(c.store.fde_sync(index, None, cfg), reason)
        assert refused(c.store.fde_sync(index, c.ids()[:4], cfg), reason)
        assert refused(c.store.fde_top_k(index, cfg, query, 10, IP, 5), reason)
        assert refused(nifs.mv_fde_top_k_batch(c.store.ref, index, cfg, [query, query], 10, IP, 5), reason)
        assert len(index) == 1 and nifs.flat_search(index, [1.0] * index.dimension, 3)[1][0][0] == b"x"
    # a NULL index beside a real store, a NULL store beside a real index
    h, good = c.store.ref.handle, nifs.flat_new_inner_product()
    assert lib.vt_mv_fde_sync(h, None, 0, None, None, 6, 3, 3, 11, 4, 0, 0, None) == 19
    assert lib.vt_mv_fde_sync(None, good.handle, 0, None, None, 6, 3, 3, 11, 4, 0, 0, None) == 19
    assert len(good) == 0
    # the configuration's own errors come before the index is looked at or touched
    assert c.store.fde_sync(good, None, (6, 3, 31, 11, 4, None)) == ("error", "num_simhash_projections must be < 31")
    assert c.store.fde_sync(good, None, (7, 3, 3, 11, 4, None)) == ("error", "dimension mismatch")
    assert len(good) == 0


def test_refusals_that_need_two_devices(nifs):
    import vettore_amd._lib as L
    if L.load().vt_device_count() < 2:
        pytest.skip("a sharded index and an index on another device need two devices")
    cfg = CASES["grouped"]
    c = build_corpus(cfg[0])
    sharded = nifs.flat_new_sharded(IP, [0, 1])
    elsewhere = nifs.flat_new_sharded(IP, [1 - nifs.DEVICE])
    for index, reason in ((sharded, "unsupported on device"), (elsewhere, "bad argument")):
        assert refused(c.store.fde_sync(index, None, cfg), reason)
        assert refused(c.store.fde_top_k(index, cfg, vecs(c.rng, 2, 6), 10, IP, 5), reason)
        assert len(index) == 0
    c.store.fde_sync(sharded, None, cfg)
    assert b"single-shard" in L.load().vt_last_error()
