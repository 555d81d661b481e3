"""The 5-bit sketch's arithmetic without a GPU (tests/sketch5_ref.py): X = 2 H + L survives the tile layout with its one-bit
L plane; for every row the oracle's f32 K1 dot -- cosine (unit rows) and dot (rows of any scale) -- lies inside the
interval the pass would give it; and the interval is about twice the 6-bit sketch's, hardly wider for the level kept off
the L plane."""
import numpy as np
import pytest

import sketch5_ref as ref
import sketch6_ref as ref6

DIMS = (129, 200, 768)
DOT = 3  # the oracle's inner product: K1's f32 dot, which a cosine index takes over its normalised rows too


def unit(x):
    return x / np.sqrt((x.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)


def corpora(d, n=96, seed=0):
    rng = np.random.default_rng(5000 + d + seed)
    uni = unit(rng.uniform(-1, 1, (n, d)).astype(np.float32))
    out = {"uniform": uni}
    huge = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    huge[np.arange(n), rng.integers(0, d, n)] *= np.float32(1e3)  # one huge coordinate: every other one quantises to 0
    out["one_huge"] = unit(huge)
    zeros = uni.copy()
    zeros[::3] = 0.0
    out["zero_rows"] = zeros
    out["pm_max"] = unit(rng.choice(np.array([-1.0, 1.0], np.float32), (n, d)))  # rows of +-max only: X = +-15 everywhere
    return out


@pytest.mark.parametrize("d", DIMS)
def test_planes_round_trip_through_the_tile_layout(d):
    for name, x in corpora(d, n=130).items():
        X, s, rho, nu = ref.quantise_rows(x)
        assert np.abs(X).max() <= 15
        H, L = ref.split_planes(X)
        assert H.min() >= -8 and H.max() <= 7 and L.min() >= 0 and L.max() <= 1
        assert np.array_equal(2 * H + L, X), name
        img = ref.pack_tiles(X, s, rho, nu)
        ld8 = ref6.ld8_of(d)
        assert img.shape[1] == ref.runs_of(d) == 5 * ld8 // 128 + 1
        assert img.nbytes == (130 + 63) // 64 * (5 * ld8 // 128 + 1) * 1024
        X2, s2, rho2, nu2 = ref.unpack_tiles(img, *X.shape)
        assert np.array_equal(X2, X), name
        assert np.array_equal(s2, s) and np.array_equal(rho2, rho) and np.array_equal(nu2, nu), name


def test_the_h_runs_are_the_6bit_sketchs_layout():
    """The same signed nibbles in the same places: one nibble image of the query per level serves both columns."""
    rng = np.random.default_rng(3)
    d = 200
    H = rng.integers(-8, 8, (70, d))
    img5 = ref.pack_tiles(2 * H, *(np.zeros(70, np.float32),) * 3)
    img6 = ref6.pack_tiles(4 * H, *(np.zeros(70, np.float32),) * 3)
    nh = ref6.ld8_of(d) // 32
    assert np.array_equal(img5[:, :nh], img6[:, :nh])


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


def test_interval_widths_on_uniform_unit_rows():
    """4 000 uniform unit rows of d = 768.  Half the steps double the rounding error rho, the term that carries e: mean e is
    2.02 times the 6-bit column's in the model, and must stay under 2.15.  Level 3 off the L plane adds s_r w3 =
    s_r 0.5 t3 ||Q3||_1, about 0.7 % of e (1.007 by the arithmetic), and must stay under 1.02."""
    rng = np.random.default_rng(9)
    d = 768
    x = unit(rng.uniform(-1, 1, (4000, d)).astype(np.float32))
    q = unit(rng.uniform(-1, 1, (1, d)).astype(np.float32))[0]
    X5, s5, rho5, nu5 = ref.quantise_rows(x)
    X6, s6, rho6, nu6 = ref6.quantise_rows(x)
    e5 = ref.intervals(X5, s5, rho5, nu5, q)[1].mean()
    e5_full = ref.intervals(X5, s5, rho5, nu5, q, split=False)[1].mean()
    e6 = ref6.intervals(X6, s6, rho6, nu6, q)[1].mean()
    print("mean e: 5-bit %.6f (level 3 on the L plane: %.6f), 6-bit %.6f; ratios %.4f, %.4f" % (e5, e5_full, e6, e5 / e6, e5 / e5_full))
    assert e5 / e6 < 2.15, (e5, e6)
    assert e5 / e5_full < 1.02, (e5, e5_full)
