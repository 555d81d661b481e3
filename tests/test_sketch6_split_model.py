"""The 6-bit pass with its third query level kept off the L plane, without a GPU (tests/sketch6_split_ref.py): for every row
the oracle's f32 dot -- in each of the four reduce orders -- lies inside the interval the pass gives it, on the corpora of
test_sketch6_model.py and on rows built so that the dropped term Q3.L sits at either end of its range; and the interval is
hardly wider than the one with all three levels on both planes."""
import numpy as np
import pytest

import sketch6_ref as ref
import sketch6_split_ref as split
from test_sketch6_model import DIMS, corpora


def the_queries(d):
    rng = np.random.default_rng(77 + d)
    qs = [rng.uniform(-1, 1, d).astype(np.float32), np.eye(1, d, d // 3)[0].astype(np.float32)]
    qs[0] /= np.float32(np.sqrt((qs[0].astype(np.float64) ** 2).sum()))
    return qs


def assert_inside(oracle_mod, x, X, s, rho, nu, q, note):
    a, e = split.intervals(X, s, rho, nu, q)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(e))
    for order in range(4):
        oracle_mod.set_reduce_order(order)
        dots = np.array([oracle_mod.compute(3, q, row) for row in x], np.float64)
        bad = np.nonzero((dots < a - e) | (dots > a + e))[0]
        assert bad.size == 0, (note, order, bad[:5], dots[bad[:5]], a[bad[:5]], e[bad[:5]])


@pytest.mark.parametrize("d", DIMS)
def test_every_reduce_order_of_the_oracle_lies_inside_the_split_interval(oracle_mod, d):
    before = oracle_mod.get_reduce_order()
    try:
        for name, x in corpora(d).items():
            X, s, rho, nu = ref.quantise_rows(x)
            for qi, q in enumerate(the_queries(d)):
                assert_inside(oracle_mod, x, X, s, rho, nu, q, (name, qi))
    finally:
        oracle_mod.set_reduce_order(before)


@pytest.mark.parametrize("d", DIMS)
def test_the_dropped_term_at_either_end_of_its_range(oracle_mod, d):
    before = oracle_mod.get_reduce_order()
    try:
        q = the_queries(d)[0]
        Q, t, _ = ref.query_levels(q)
        pos, neg, _ = split.level_sums(Q[2])
        assert pos > 0 and neg < 0
        for mirror in (False, True):
            x, Xwant = split.adversarial_rows(q, 64, 9 + d, mirror)
            X, s, rho, nu = ref.quantise_rows(x)
            assert np.array_equal(X, Xwant)
            L = ref.split_planes(X)[1]
            assert np.all(L @ Q[2] == 3 * (neg if mirror else pos))  # the end of [3 N3, 3 P3]
            assert_inside(oracle_mod, x, X, s, rho, nu, q, ("adversarial", mirror))
            # the interval's end is met to within the other terms of e: the widening is no wider than it must be
            a, e = split.intervals(X, s, rho, nu, q)
            a_full, e_full = ref.intervals(X, s, rho, nu, q)
            w = s.astype(np.float64) * 1.5 * np.float64(t[2]) * (pos - neg)
            assert np.allclose(np.abs(a_full - a), w, rtol=1e-9, atol=0)
            assert np.all(e <= (e_full + w) * (1 + 1e-9))
    finally:
        oracle_mod.set_reduce_order(before)


def test_the_interval_widens_by_a_few_percent_on_uniform_rows():
    d = 768
    rng = np.random.default_rng(4000)
    x = rng.uniform(-1, 1, (4000, d)).astype(np.float32)
    x /= np.sqrt((x.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)
    q = rng.uniform(-1, 1, d).astype(np.float32)
    q /= np.float32(np.sqrt((q.astype(np.float64) ** 2).sum()))
    X, s, rho, nu = ref.quantise_rows(x)
    _, e_old = ref.intervals(X, s, rho, nu, q)
    _, e_new = split.intervals(X, s, rho, nu, q)
    ratio = float((e_new / e_old).mean())
    print("mean e_new / e_old = %.4f (mean e_old %.6f, e_new %.6f)" % (ratio, e_old.mean(), e_new.mean()))
    assert 1.0 <= ratio <= 1.05
