"""The int8 sketch's arithmetic without a GPU (tests/sketch8_ref.py): X survives the chunked tile layout; the query's two
levels leave exactly the residual the bound is told about; and for every row the oracle's f32 K1 dot -- cosine (unit rows)
and dot (rows of any scale) -- lies inside the interval the pass would give it."""
import numpy as np
import pytest

import sketch6_ref as ref6
import sketch8_ref as ref
from test_sketch5_model import DIMS, DOT, corpora, unit


@pytest.mark.parametrize("d", DIMS)
def test_rows_round_trip_through_the_tile_layout(d):
    for name, x in corpora(d, n=130).items():
        X, s, rho, nu = ref.quantise_rows(x)
        assert np.abs(X).max() <= 127
        img = ref.pack_tiles(X, s, rho, nu)
        ld8 = ref6.ld8_of(d)
        assert img.shape[1] == ref.chunks_of(d) + 1 == ld8 // 16 + 1
        assert img.nbytes == (130 + 63) // 64 * (ld8 // 16 + 1) * 1024
        # sketch_offset: row r's chunk c at ((r / 64) (nch + 1) + c) 1024 + (r % 64) 16
        flat = img.reshape(-1)
        for r, c in ((0, 0), (63, 1), (64, ld8 // 16 - 1), (129, 3)):
            off = ((r // 64) * (ld8 // 16 + 1) + c) * 1024 + (r % 64) * 16
            want = np.zeros(16, np.int8)
            got = X[r, 16 * c:16 * c + 16]
            want[:len(got)] = got
            assert np.array_equal(flat[off:off + 16].view(np.int8), want), (name, r, c)
        X2, s2, rho2, nu2 = ref.unpack_tiles(img, *X.shape)
        assert np.array_equal(X2, X), name
        assert np.array_equal(s2, s) and np.array_equal(rho2, rho) and np.array_equal(nu2, nu), name
        assert not img[2, :, 130 - 128:].any(), name  # rows past n: zero chunks, zero metadata


@pytest.mark.parametrize("d", DIMS)
def test_the_query_levels_leave_the_residual_they_report(d):
    rng = np.random.default_rng(80 + d)
    for q in (unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0], np.eye(1, d, d // 3)[0].astype(np.float32),
              np.zeros(d, np.float32), (rng.uniform(-1, 1, d) * 1e-30).astype(np.float32)):
        Q, t, eta = ref.query_levels(q)
        assert np.abs(Q).max() <= 127
        back = np.float64(t[0]) * Q[0] + np.float64(t[1]) * Q[1] + eta
        assert np.allclose(back, q.astype(np.float64), rtol=0, atol=2.0 ** -50 * max(1e-300, np.abs(q).max()))
        if np.abs(q).max() > 0:  # two levels of seven bits: the residual is under 2^-13 of the largest element
            assert np.abs(eta).max() <= np.abs(q).max() * 2.0 ** -13


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("d", DIMS)
def test_the_oracles_dot_lies_inside_the_interval(oracle_mod, d, metric):
    rng = np.random.default_rng(177 + d)
    qs = [unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0], np.eye(1, d, d // 3)[0].astype(np.float32)]
    if metric == "dot":
        qs = [(q * np.float32(7.5)).astype(np.float32) for q in qs]
    for name, x in corpora(d).items():
        if metric == "dot":  # rows of any length
            x = (x * rng.uniform(0.05, 24, (len(x), 1)).astype(np.float32)).astype(np.float32)
        X, s, rho, nu = ref.quantise_rows(x)
        for qi, q in enumerate(qs):
            a, e = ref.intervals(X, s, rho, nu, q)
            assert np.all(np.isfinite(a)) and np.all(np.isfinite(e))
            dots = np.array([oracle_mod.compute(DOT, q, row) for row in x], np.float64)
            bad = np.nonzero((dots < a - e) | (dots > a + e))[0]
            assert bad.size == 0, (name, qi, bad[:5], dots[bad[:5]], a[bad[:5]], e[bad[:5]])
            # and the words the pass would store hold the rank value's word, in f32's total order
            Q, t, eta_v = ref.query_levels(q)
            qn = np.sqrt((q.astype(np.float64) ** 2).sum()) * ref6.UP
            eta = np.sqrt((eta_v ** 2).sum()) * ref6.UP
            code = ref6.M_COS if metric == "cosine" else ref6.M_IP
            first, second = ref.pass_words(code, X, s, rho, nu, Q, t, qn, eta, 8.0 * d * 2.0 ** -24)
            rank = np.array([oracle_mod.rank_value(code, v) for v in dots.astype(np.float32)], np.float32)
            word = ref6.orderable(rank)
            assert np.all((first <= word) & (word <= second)), (name, qi)
