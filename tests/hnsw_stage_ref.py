"""A numpy model of K15's two key columns (vettore_amd/csrc/vt_hnsw_stage.hip): what hnsw_stage_bits_kernel and
hnsw_stage_score_kernel write for every scanned position of an HNSW slab -- key = orderable(rank) << 32 | id_rank[row],
payload (row, raw), EMPTY_KEY for a position that does not take part.

tests/test_hnsw_stage_model.py holds it to the oracle (packed_hamming of compress_sign_bits, vector_top_k) on the CPU;
tests/test_gpu_hnsw_stage_kernels.py holds the kernels to it, key by key and payload by payload.

The arithmetic restated: the sign bits are `v >= 0.0` over the first d floats of a row; the f32 families (l2, inner product)
fold eight separately rounded element operations per chunk in one of the four lane orders, add chunk after chunk, then
the tail element by element, finish (sqrt for l2) and recover a non-finite value in f64 (distances.rs:42-98); cosine is
the f64 dot over the two f64 norms, all three sequential over the prefix (distances.rs:160-185).  The query is the left
operand."""
import numpy as np

NO_ROW = 0xFFFFFFFF
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
L2, COSINE, INNER_PRODUCT = 0, 2, 3            # VT_L2, VT_COSINE, VT_INNER_PRODUCT
PAIR, AVX, SEQ, SSE2 = 0, 1, 2, 3              # VT_ORDER_*
ERR_OVERFLOW = 4
PAYLOAD = np.dtype([("row", "<u4"), ("raw", "<f4")])
FLT_MAX = float(np.finfo(np.float32).max)


def orderable(values):
    """f32::total_cmp as an order-preserving u32."""
    u = np.asarray(values, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def id_ranks(ids):
    """ids[row]: the row's external id (bytes), None for a dead row -> the rank column."""
    live = sorted((bytes(b), r) for r, b in enumerate(ids) if b is not None)
    out = np.full(len(ids), NO_ROW, np.uint32)
    for rank, (_, r) in enumerate(live):
        out[r] = rank
    return out


def _columns(n):
    return np.full(n, EMPTY_KEY, np.uint64), np.zeros(n, PAYLOAD)


def bits_column(X, d, id_rank, q):
    """K15b over X[rows][stride]: (keys, payloads), one per row."""
    X = np.asarray(X, np.float32)
    rows = X.shape[0]
    keys, pay = _columns(rows)
    pay["row"] = np.arange(rows, dtype=np.uint32)
    qbits = np.asarray(q, np.float32)[:d] >= 0
    count = ((X[:, :d] >= 0) != qbits[None, :]).sum(axis=1).astype(np.float32)
    live = np.asarray(id_rank, np.uint32) != NO_ROW
    pay["raw"] = np.where(live, count, np.float32(0))
    keys[live] = (orderable(count[live]).astype(np.uint64) << np.uint64(32)) | np.asarray(id_rank, np.uint64)[live]
    return keys, pay


def _chunk_sum(l, order):
    a = lambda x, y: (x + y).astype(np.float32)
    if order == AVX:
        return a(a(a(l[0], l[4]), a(l[2], l[6])), a(a(l[1], l[5]), a(l[3], l[7])))
    if order == SEQ:
        return a(a(a(a(l[0], l[1]), l[2]), l[3]), a(a(a(l[4], l[5]), l[6]), l[7]))
    if order == SSE2:
        return a(a(a(l[0], l[2]), a(l[1], l[3])), a(a(l[4], l[6]), a(l[5], l[7])))
    return a(a(a(l[0], l[1]), a(l[2], l[3])), a(a(l[4], l[5]), a(l[6], l[7])))


def _f32_raws(metric, order, q, Xp):
    """compute(metric, q, row) for every row of Xp[n][p] (distances.rs:42-98); NaN: "metric overflow"."""
    n, p = Xp.shape
    with np.errstate(all="ignore"):
        def elem(e):
            if metric == L2:
                t = (q[e] - Xp[:, e]).astype(np.float32)
                return (t * t).astype(np.float32)
            return (q[e] * Xp[:, e]).astype(np.float32)
        acc = np.zeros(n, np.float32)
        for c in range(p // 8):
            acc = (acc + _chunk_sum([elem(c * 8 + e) for e in range(8)], order)).astype(np.float32)
        for e in range(p // 8 * 8, p):
            acc = (acc + elem(e)).astype(np.float32)
        raw = acc.copy()
        if metric == L2:
            raw = np.where(np.isfinite(acc), np.sqrt(np.where(np.isfinite(acc), acc, 0)).astype(np.float32), acc)
        for i in np.flatnonzero(~np.isfinite(raw)):
            x64, q64 = Xp[i].astype(np.float64), q[:p].astype(np.float64)
            s = 0.0
            for e in range(p):  # sequentially, as the reference's iterator sum
                s += (q64[e] - x64[e]) ** 2 if metric == L2 else q64[e] * x64[e]
            if metric == L2:
                v = np.float32(np.sqrt(s))
                raw[i] = v if np.isfinite(v) else np.float32(np.nan)
            else:
                raw[i] = np.float32(s) if np.isfinite(s) and abs(s) <= FLT_MAX else np.float32(np.nan)
    return raw


def _cosine_raws(q, Xp):
    """cosine(q, row) (distances.rs:160-177) for every row of Xp[n][p]; NaN: "metric overflow"."""
    n, p = Xp.shape
    X64, q64 = Xp.astype(np.float64), q[:p].astype(np.float64)
    qq, xx, qx = 0.0, np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        for e in range(p):
            qq = qq + q64[e] * q64[e]
            xx = xx + X64[:, e] * X64[:, e]
            qx = qx + q64[e] * X64[:, e]
        ln, rn = np.sqrt(qq), np.sqrt(xx)
        sim = qx / (ln * rn)
        raw = np.where(np.isfinite(sim), np.clip(sim, -1.0, 1.0), np.nan).astype(np.float32)
        raw = np.where((ln == 0.0) | (rn == 0.0), np.float32(0), raw)
    return raw


def rank_values(metric, raw):
    """distances.rs:113-119."""
    raw = np.asarray(raw, np.float32)
    if metric == COSINE:
        return (np.float32(1.0) - raw).astype(np.float32)
    if metric == INNER_PRODUCT:
        return (-raw).astype(np.float32)
    return raw


def score_column(X, d, p, id_rank, q, metric, order, rows=None):
    """K15p over X[slab rows][stride] on the prefix p: position i is row rows[i], or row i when rows is None.
    -> (keys, payloads, status word)."""
    X = np.asarray(X, np.float32)
    q = np.asarray(q, np.float32)
    id_rank = np.asarray(id_rank, np.uint32)
    assert 1 <= p <= d <= X.shape[1]
    rows = np.arange(X.shape[0], dtype=np.uint32) if rows is None else np.asarray(rows, np.uint32)
    n = len(rows)
    keys, pay = _columns(n)
    pay["row"] = rows
    if n == 0:
        return keys, pay, 0
    live = id_rank[rows] != NO_ROW
    Xp = np.ascontiguousarray(X[rows][:, :p])
    raw = _cosine_raws(q, Xp) if metric == COSINE else _f32_raws(metric, order, q, Xp)
    pay["raw"] = np.where(live, raw, np.float32(0))
    ok = live & ~np.isnan(raw)
    keys[ok] = (orderable(rank_values(metric, raw[ok])).astype(np.uint64) << np.uint64(32)) | id_rank[rows][ok].astype(np.uint64)
    return keys, pay, (ERR_OVERFLOW if (live & np.isnan(raw)).any() else 0)


def top(keys, pay, k):
    """The k smallest keys' payloads, ascending: what K3 selects."""
    order = np.argsort(keys, kind="stable")
    order = order[keys[order] != EMPTY_KEY][:k]
    return pay[order]


# ---- the shapes both test files use -----------------------------------------------------------------------------------
ROWS = (1, 63, 64, 65, 257)
DIMS = (1, 3, 63, 64, 65, 100, 130, 768)   # strides 4 .. 768; 130 leaves two pad floats


def stride_of(d):
    return (d + 3) // 4 * 4


def make_slab(rng, rows, d, kind="normal"):
    """X[rows][stride]: the pad behind d is NaN (nothing may look at it).  kind: "normal"; "zeros" -- values from
    {+0.0, -0.0, 1.0, -1.0}; "two" -- every row one of two sign patterns."""
    X = np.full((rows, stride_of(d)), np.nan, np.float32)
    if kind == "zeros":
        X[:, :d] = rng.choice(np.asarray([0.0, -0.0, 1.0, -1.0], np.float32), size=(rows, d))
    elif kind == "two":
        pat = np.where(rng.random((2, d)) < 0.5, -1.0, 1.0).astype(np.float32)
        X[:, :d] = pat[rng.integers(0, 2, rows)] * rng.uniform(0.5, 2.0, (rows, d)).astype(np.float32)
    else:
        X[:, :d] = rng.standard_normal((rows, d)).astype(np.float32)
    return X


def make_ids(rows):
    """ids whose byte order is not the row order, some of them prefixes of others"""
    return [b"k" + (b"%d" % ((r * 7919) % 1009)) + (b"" if r % 3 else b"x" * (r % 5)) + b"/%d" % r for r in range(rows)]


def dead_sets(rows):
    """name -> the dead rows"""
    sets = {"none": [], "every third": list(range(0, rows, 3)), "first and last": sorted({0, rows - 1}), "all": list(range(rows))}
    return sets


def ranks_with_dead(rows, dead):
    ids = make_ids(rows)
    for r in dead:
        ids[r] = None
    return ids, id_ranks(ids)
