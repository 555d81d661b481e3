"""The 6-bit sketch's arithmetic without a GPU (tests/sketch6_ref.py): X = 4 H + L survives the two-plane tile layout, and
for every row the oracle's f32 dot -- in each of the four reduce orders -- lies inside the interval the pass would give it."""
import numpy as np
import pytest

import sketch6_ref as ref

DIMS = (129, 192, 257, 768)


def corpora(d, n=96, seed=0):
    rng = np.random.default_rng(1000 + d + seed)
    uni = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    gau = rng.standard_normal((n, d)).astype(np.float32)
    spiky = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    for r in range(n):
        spiky[r, rng.choice(d, 8, replace=False)] *= 6.0
    out = {}
    for name, x in (("uniform", uni), ("gaussian", gau), ("spiky", spiky)):
        out[name] = x / np.sqrt((x.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)
    out["tiny"] = (out["uniform"] * np.float32(1e-30)).astype(np.float32)
    out["huge"] = (out["uniform"] * np.float32(1e30)).astype(np.float32)
    zeros = out["gaussian"].copy()
    zeros[::3] = 0.0
    out["zero_rows"] = zeros
    return out


@pytest.mark.parametrize("d", DIMS)
def test_planes_round_trip_through_the_tile_layout(d):
    for name, x in corpora(d, n=130).items():
        X, s, rho, nu = ref.quantise_rows(x)
        assert np.abs(X).max() <= 31
        H, L = ref.split_planes(X)
        assert H.min() >= -8 and H.max() <= 7 and L.min() >= 0 and L.max() <= 3
        assert np.array_equal(4 * H + L, X), name
        img = ref.pack_tiles(X, s, rho, nu)
        assert img.shape[1] == ref.runs_of(d) and img.nbytes == (130 + 63) // 64 * ref.runs_of(d) * 1024
        X2, s2, rho2, nu2 = ref.unpack_tiles(img, *X.shape)
        assert np.array_equal(X2, X), name
        assert np.array_equal(s2, s) and np.array_equal(rho2, rho) and np.array_equal(nu2, nu), name


def test_query_levels_are_signed_nibbles_and_leave_eta():
    rng = np.random.default_rng(5)
    for d in DIMS:
        for q in (rng.uniform(-1, 1, d), rng.standard_normal(d) * 1e-20, np.eye(1, d, 7)[0], np.zeros(d)):
            q = q.astype(np.float32)
            Q, t, eta = ref.query_levels(q)
            assert np.abs(Q).max() <= 7
            back = sum(np.float64(t[j]) * Q[j] for j in range(ref.LEVELS)) + eta
            assert np.allclose(back, q.astype(np.float64), rtol=0, atol=np.abs(q).max() * 2.0 ** -48)
            if np.abs(q).max() > 0:  # a level leaves at most t_j / 2 = (its input's maximum) / 14 per coordinate
                assert np.abs(eta).max() <= np.abs(q).max() / 14 ** 3 * (1 + 1e-6)


@pytest.mark.parametrize("d", DIMS)
def test_every_reduce_order_of_the_oracle_lies_inside_the_interval(oracle_mod, d):
    rng = np.random.default_rng(77 + d)
    qs = [rng.uniform(-1, 1, d).astype(np.float32), np.eye(1, d, d // 3)[0].astype(np.float32)]
    qs[0] /= np.float32(np.sqrt((qs[0].astype(np.float64) ** 2).sum()))
    before = oracle_mod.get_reduce_order()
    try:
        for name, x in corpora(d).items():
            X, s, rho, nu = ref.quantise_rows(x)
            for qi, q in enumerate(qs):
                a, e = ref.intervals(X, s, rho, nu, q)
                assert np.all(np.isfinite(a)) and np.all(np.isfinite(e))
                for order in range(4):
                    oracle_mod.set_reduce_order(order)
                    dots = np.array([oracle_mod.compute(3, q, row) for row in x], np.float64)
                    bad = np.nonzero((dots < a - e) | (dots > a + e))[0]
                    assert bad.size == 0, (name, qi, order, bad[:5], dots[bad[:5]], a[bad[:5]], e[bad[:5]])
    finally:
        oracle_mod.set_reduce_order(before)
