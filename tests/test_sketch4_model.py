"""The 4-bit sketch's model on the CPU (tests/sketch4_ref.py): every interval holds the oracle's f32 dot,
the intervals are about twice the 5-bit sketch's, and the exact-threshold rule behind the pass keeps the oracle's top k."""
import numpy as np
import pytest

import sketch4_ref as ref4
import sketch5_ref as ref5
import sketch6_ref as ref6
from test_sketch5_model import corpora, unit

COS, IP = ref6.M_COS, ref6.M_IP


def dots(oracle_mod, q, x):
    return np.array([oracle_mod.compute(IP, q, row) for row in x], np.float32)


def test_every_interval_holds_the_oracles_dot(oracle_mod):
    """4 000 uniform unit rows and the spiky, tiny-norm and zero rows of the other models' corpora: zero violations."""
    d = 768
    rng = np.random.default_rng(44)
    x = unit(rng.uniform(-1, 1, (4000, d)).astype(np.float32))
    sets = {"uniform": x}
    sets.update(corpora(d, n=200, seed=4))
    for name, rows in sets.items():
        X, s, rho, nu = ref4.quantise_rows(rows)
        assert np.abs(X).max() <= 7
        for q in (unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0], rows[3].copy()):
            a, e = ref4.intervals(X, s, rho, nu, q)
            got = dots(oracle_mod, q, rows).astype(np.float64)
            bad = np.nonzero(~((a - e <= got) & (got <= a + e)))[0]
            assert bad.size == 0, (name, bad[:5])


def test_the_intervals_are_about_twice_the_5bit_sketchs():
    """Mean e under 2.25 x the 5-bit model's on uniform unit rows (rho itself: 2.14 x)."""
    d = 768
    rng = np.random.default_rng(45)
    x = unit(rng.uniform(-1, 1, (4000, d)).astype(np.float32))
    q = unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0]
    X4, s4, rho4, nu4 = ref4.quantise_rows(x)
    X5, s5, rho5, nu5 = ref5.quantise_rows(x)
    _, e4 = ref4.intervals(X4, s4, rho4, nu4, q)
    _, e5 = ref5.intervals(X5, s5, rho5, nu5, q)
    ratio_e, ratio_rho = e4.mean() / e5.mean(), rho4.astype(np.float64).mean() / rho5.astype(np.float64).mean()
    print("mean e: 4-bit / 5-bit = %.3f; mean rho: %.3f" % (ratio_e, ratio_rho))
    assert ratio_e < 2.25, ratio_e
    assert 1.9 < ratio_rho < 2.25, ratio_rho


def test_pack_and_unpack_are_inverse():
    for d in (200, 256, 768):
        rng = np.random.default_rng(d)
        x = (rng.uniform(-1, 1, (130, d)) * rng.uniform(0.01, 30, (130, 1))).astype(np.float32)
        X, s, rho, nu = ref4.quantise_rows(x)
        img = ref4.pack_tiles(X, s, rho, nu)
        assert img.shape == (3, ref4.runs_of(d), 64, 4)
        Xb, sb, rhob, nub = ref4.unpack_tiles(img, 130, d)
        assert np.array_equal(Xb, X) and sb.tobytes() == s.tobytes() and rhob.tobytes() == rho.tobytes() and nub.tobytes() == nu.tobytes()


@pytest.mark.parametrize("metric", [COS, IP])
@pytest.mark.parametrize("k", [1, 10])
def test_the_exact_threshold_keeps_the_oracles_top_k(oracle_mod, metric, k):
    """Fixed corpora, every row retained (one list of everything): the candidate set h <= Kt' contains the oracle's top k
    and every tie of the k-th, and Kt' <= Kt -- whichever copies of Kt the refine step picks."""
    d = 256
    rng = np.random.default_rng(46 + k)
    base = unit(rng.uniform(-1, 1, (3000, d)).astype(np.float32))
    tied = base.copy()
    tied[100:140] = tied[100]           # a block of identical rows around the top
    for name, x, q in (("uniform", base, unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0]), ("ties", tied, tied[100].copy())):
        if metric != COS:
            x = (x * np.float32(3.5)).astype(np.float32)
        X, s, rho, nu = ref4.quantise_rows(x)
        Q, t, eta_v = ref6.query_levels(q)
        qn = np.sqrt((q.astype(np.float64) ** 2).sum()) * ref6.UP
        eta = np.sqrt((eta_v ** 2).sum()) * ref6.UP
        hi_w, lo_w = ref4.pass_words(metric, X, s, rho, nu, Q, t, qn, eta, 8.0 * d * 2.0 ** -24)
        dot = dots(oracle_mod, q, x)
        rank = np.array([oracle_mod.rank_value(COS if metric == COS else IP, v) for v in dot], np.float32)
        exact = ref6.orderable(rank)
        assert np.all(hi_w <= exact) and np.all(exact <= lo_w), name
        kt, kt_low, kt_high = ref4.exact_threshold(lo_w, None, exact, k)
        assert kt_low <= kt_high <= kt, name
        kth = np.sort(exact)[k - 1]
        needed = np.nonzero(exact <= kth)[0]          # the top k and every tie of the k-th
        for ktp in (kt_low, kt_high):
            cand = hi_w <= np.uint32(ktp)
            assert cand[needed].all(), (name, ktp)
            assert cand.sum() <= (hi_w <= np.uint32(kt)).sum()
        print("%s metric %d k %d: candidates %d under Kt, %d under Kt'" % (name, metric, k, (hi_w <= np.uint32(kt)).sum(),
                                                                          (hi_w <= np.uint32(kt_high)).sum()))
