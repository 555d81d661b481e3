"""The int8 sketch's L2 family without a GPU (tests/sketch8_l2_ref.py; DESIGN.md 4.10, DESIGN_APPENDIX A.5b): the column with
xx survives the tile layout and leaves the fourth dword zero when it is not asked for; for every row of the adversarial
corpora, both metrics and every lane order the oracle knows, the oracle's f32 K1 value lies between the two words the pass
would store, under f32's total order; the guard declines where a square could overflow; and the model's own certificate
serves the end-to-end GPU test's searches (same corpora, same seeds)."""
import numpy as np
import pytest

import sketch6_ref as ref6
import sketch8_l2_ref as ref
import sketch8_ref as ref8

DIMS = (1, 7, 100, 192, 768)
METRICS = (ref.M_L2, ref.M_L2SQ)


def model_queries(d, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, d).astype(np.float32), (ref.unit(rng.uniform(-1, 1, d)) * np.float32(7.5)).astype(np.float32),
            (rng.uniform(-1, 1, d) * 1e-3).astype(np.float32)]


@pytest.mark.parametrize("d", DIMS)
def test_the_column_round_trips_with_and_without_xx(d):
    q = model_queries(d, 3 + d)[0]
    x = np.vstack(list(ref.adversarial(d, q, 40 + d).values()))[:130]
    n = len(x)
    X, s, rho, nu, xx = ref.quantise_rows(x)
    exact = (x.astype(np.float64) ** 2).sum(axis=1)
    assert np.all(xx.astype(np.float64) >= exact)
    assert np.all(xx.astype(np.float64) * (1.0 - 2.0 ** -22) <= exact + 2.0 ** -149)  # (subnormal xx: one step of 2^-149)
    plain = ref.pack_tiles(X, s, rho, nu)
    assert np.array_equal(plain, ref8.pack_tiles(X, s, rho, nu))
    assert not ref.unpack_tiles(plain, n, d)[4].view(np.uint32).any()   # not asked for: the fourth dword is zero
    img = ref.pack_tiles(X, s, rho, nu, xx)
    assert img.shape == plain.shape
    nch = ref8.chunks_of(d)
    assert np.array_equal(img[:, :nch], plain[:, :nch])                 # the chunks are the dot family's
    X2, s2, rho2, nu2, xx2 = ref.unpack_tiles(img, n, d)
    assert np.array_equal(X2, X) and np.array_equal(s2, s) and np.array_equal(rho2, rho) and np.array_equal(nu2, nu)
    assert np.array_equal(xx2.view(np.uint32), xx.view(np.uint32))
    # sketch_offset: row r's metadata at ((r / 64) (nch + 1) + nch) 1024 + (r % 64) 16; xx in its last four bytes
    flat = img.reshape(-1)
    for r in (0, 63, 64, n - 1):
        off = ((r // 64) * (nch + 1) + nch) * 1024 + (r % 64) * 16
        assert flat[off + 12:off + 16].view(np.uint32)[0] == xx[r:r + 1].view(np.uint32)[0], r
    tiles = img.shape[0]
    meta = np.ascontiguousarray(img[:, nch]).reshape(tiles * 64, 16)
    assert not meta[n:].any()                                           # rows past n: zero metadata


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_the_oracles_distance_lies_between_the_two_words(oracle_mod, d, metric):
    saved = oracle_mod.get_reduce_order()
    try:
        for qi, q in enumerate(model_queries(d, 177 + d)):
            for name, x in ref.adversarial(d, q, 900 + 10 * d + qi).items():
                X, s, rho, nu, xx = ref.quantise_rows(x)
                qy = ref.Query(q)
                assert not ref.declines(qy.qn, ref.max_norm_of(rho, nu))
                first, second = ref.pass_words(metric, X, s, rho, nu, xx, qy)
                assert np.all(first <= second), (name, qi)
                for order in oracle_mod.ORDERS:
                    oracle_mod.set_reduce_order(order)
                    raw = np.array([oracle_mod.compute(metric, q, row) for row in x], np.float32)
                    word = ref6.orderable(raw)  # (the rank of both metrics is the raw value)
                    bad = np.nonzero((word < first) | (word > second))[0]
                    assert bad.size == 0, (name, qi, order, bad[:5], raw[bad[:5]], first[bad[:5]], second[bad[:5]])
                if name == "query":  # c = 0 exactly, in every order
                    assert raw[0] == 0.0 and first[0] == ref6.orderable(np.float32(0.0))[()]
    finally:
        oracle_mod.set_reduce_order(saved)


def test_the_words_are_tight_where_the_distance_is_large():
    """Not a bound's proof but its use: for uniform rows the two words lie within a few units of the sketch's own error of
    each other, relative to the distance -- far inside the spread of the distances themselves."""
    d = 192
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (400, d)).astype(np.float32)
    q = rng.uniform(-1, 1, d).astype(np.float32)
    first, second = ref.words_for(ref.M_L2SQ, x, q)
    lo = (first ^ np.uint32(0x80000000)).view(np.float32).astype(np.float64)   # (non-negative floats)
    hi = (second ^ np.uint32(0x80000000)).view(np.float32).astype(np.float64)
    exact = ((x.astype(np.float64) - q.astype(np.float64)) ** 2).sum(axis=1)
    assert np.all((lo <= exact) & (exact <= hi))
    assert np.all(hi - lo < 0.02 * exact)


def test_the_guard_declines_where_a_square_can_overflow():
    """(qn + max norm) up >= 2^62: there the f32 square of a difference can overflow and the plain scan decides."""
    d = 64
    rng = np.random.default_rng(9)
    x = rng.uniform(-1, 1, (70, d)).astype(np.float32)
    q = np.full(d, 2.0, np.float32)
    _, _, rho, nu, _ = ref.quantise_rows(x)
    assert not ref.declines(ref.Query(q).qn, ref.max_norm_of(rho, nu))
    x[10] = np.float32(2.0 ** 60)  # ||x|| = 2^63
    _, _, rho, nu, xx = ref.quantise_rows(x)
    assert np.all(np.isfinite(xx))
    assert ref.declines(ref.Query(q).qn, ref.max_norm_of(rho, nu))
    x[10] = np.float32(2.0 ** 57)  # ||x|| = 2^60: every square stays below 2^122
    _, _, rho, nu, _ = ref.quantise_rows(x)
    assert not ref.declines(ref.Query(q).qn, ref.max_norm_of(rho, nu))
    assert ref.declines(ref.Query(np.full(d, np.float32(2.0 ** 60))).qn, ref.max_norm_of(rho, nu))


def test_the_certificate_on_hand_made_lists():
    E = ref.EMPTY
    B = 0x80000000
    # two lists of four, k = 2: Kt is the second smallest kmax word; a slot is a candidate iff kmin <= Kt
    hi = np.array([B + 1, B + 5, B + 9, E, B + 2, B + 30, E, E], np.uint32)
    lo = np.array([B + 4, B + 8, B + 12, E, B + 6, B + 40, E, E], np.uint32)
    rows = np.arange(8, dtype=np.uint32) + 100
    c = ref.certify(lo, hi, rows, 2, 4, 2)
    assert c["kt"] == B + 6 and c["cnt"] == 3 and c["ok"] and list(c["rows"]) == [100, 101, 104]
    assert ref.tail_outcome(c, 2, 4, 192) == 1
    # a full list of candidates alone refuses: it may have dropped a row that matters
    hi2 = np.array([B + 1, B + 2, B + 3, B + 4, B + 50, E, E, E], np.uint32)
    lo2 = np.array([B + 9, B + 9, B + 9, B + 9, B + 60, E, E, E], np.uint32)
    assert not ref.certify(lo2, hi2, rows, 2, 4, 2)["ok"]
    # k or fewer live: every live slot is a candidate
    c3 = ref.certify(lo[:4], hi[:4], rows[:4], 1, 4, 3)
    assert c3["kt"] == 0xFFFFFFFF and c3["cnt"] == 3 and c3["ok"]
    # over the cap
    assert not ref.certify(lo, hi, rows, 2, 4, 2, cap=2)["ok"]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [1, 10, 100])
def test_the_model_certifies_the_end_to_end_searches(metric, k):
    """The exact corpora and queries of tests/test_gpu_sketch_l2.py: at least 11 of 12 searches per case certify in the model
    (the one that may not sits on the block of 48 identical rows, which fills a block's list with candidates)."""
    for d, n in ref.E2E_SHAPES:
        x, ids, qs = ref.e2e_case(metric, k, d, n)
        rank = np.arange(n)  # (ids in ascending byte order: the id rank is the row)
        X, s, rho, nu, xx = ref.quantise_rows(x)
        kp = ref.list_k(k)
        blocks = 256 * (4 if kp <= 64 else 2)
        ok = 0
        for q in qs:
            first, second = ref.pass_words(metric, X, s, rho, nu, xx, ref.Query(q))
            lo, hi, rows = ref.block_lists(first, second, rank, blocks, kp)
            cert = ref.certify(lo, hi, rows, blocks, kp, k)
            ok += bool(cert["ok"])
            if cert["ok"]:
                assert cert["cnt"] >= min(k, n)
        assert ok >= ref.E2E_QUERIES - 1, (metric, k, d, ok)
