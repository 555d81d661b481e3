"""The numpy model of K15's key columns (tests/hnsw_stage_ref.py) held to the oracle on the CPU, on the shapes the GPU
test uses: the sign-bit column against packed_hamming(compress_sign_bits(row), compress_sign_bits(query)), the prefix
scores against vector_top_k -- ids, order and the f32 bits of every raw value, in every lane order.  So the yardstick of
tests/test_gpu_hnsw_stage_kernels.py is itself checked here."""
import numpy as np
import pytest

import oracle
import hnsw_stage_ref as ref
from hnsw_stage_ref import COSINE, DIMS, INNER_PRODUCT, L2, NO_ROW, ROWS

METRICS = (L2, COSINE, INNER_PRODUCT)


def bits_of(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.fixture(autouse=True)
def lane_order():
    before = oracle.get_reduce_order()
    yield
    oracle.set_reduce_order(before)


def prefixes(d):
    return sorted({p for p in (1, 7, 8, 9, d - 1, d) if 1 <= p <= d})


@pytest.mark.parametrize("kind", ["normal", "zeros", "two"])
@pytest.mark.parametrize("d", DIMS)
def test_bits_column_is_packed_hamming_of_the_sign_bits(d, kind):
    rng = np.random.default_rng(d * 3 + len(kind))
    for rows in (ROWS if d in (65, 130) else (65,)):
        X = ref.make_slab(rng, rows, d, kind)
        q = ref.make_slab(rng, 1, d, "zeros" if kind == "zeros" else "normal")[0, :d]
        for name, dead in ref.dead_sets(rows).items():
            ids, rk = ref.ranks_with_dead(rows, dead)
            keys, pay = ref.bits_column(X, d, rk, q)
            qw = oracle.compress_sign_bits(q)
            for r in range(rows):
                assert pay["row"][r] == r
                if rk[r] == NO_ROW:
                    assert keys[r] == ref.EMPTY_KEY, (name, r)
                    continue
                want = oracle.packed_hamming(qw, oracle.compress_sign_bits(X[r, :d]), d)
                assert bits_of(pay["raw"][r]) == bits_of(want), (name, r)
                assert int(keys[r]) == (int(ref.orderable(want)) << 32) | int(rk[r])
            # ... and the column's order is binary_top_k's
            live = [(ids[r], oracle.compress_sign_bits(X[r, :d])) for r in range(rows) if ids[r] is not None]
            want = oracle.binary_top_k(live, qw, d, rows) if live else []
            got = ref.top(keys, pay, rows)
            assert [(ids[r], bits_of(v)) for r, v in zip(got["row"], got["raw"])] == [(i, bits_of(v)) for i, v in want], name


def test_minus_zero_sets_the_bit():
    X = np.asarray([[-0.0, 0.0, -1.0, 1.0]], np.float32)
    keys, pay = ref.bits_column(X, 4, np.asarray([0], np.uint32), np.asarray([1.0, -1.0, 1.0, -1.0], np.float32))
    assert pay["raw"][0] == 3.0  # the row's bits are 1 1 0 1, the query's 1 0 1 0


# (cosine has no lane order: once)
@pytest.mark.parametrize("metric,order", [(m, o) for m in METRICS for o in oracle.ORDERS if m != COSINE or o == oracle.ORDERS[0]])
@pytest.mark.parametrize("d", DIMS)
def test_score_column_is_vector_top_k(d, metric, order):
    oracle.set_reduce_order(order)
    rng = np.random.default_rng(d * 11 + metric)
    rows = 65 if d != 100 else 257
    X = ref.make_slab(rng, rows, d)
    q = rng.standard_normal(d).astype(np.float32)
    for name, dead in ref.dead_sets(rows).items():
        ids, rk = ref.ranks_with_dead(rows, dead)
        live = [(ids[r], X[r, :d]) for r in range(rows) if ids[r] is not None]
        for p in prefixes(d):
            keys, pay, status = ref.score_column(X, d, p, rk, q, metric, order)
            assert status == 0 and (keys[rk == NO_ROW] == ref.EMPTY_KEY).all() and (keys[rk != NO_ROW] != ref.EMPTY_KEY).all()
            want = oracle.vector_top_k(live, q, metric, p, rows) if live else []
            got = ref.top(keys, pay, rows)
            assert [(ids[r], bits_of(v)) for r, v in zip(got["row"], got["raw"])] == [(i, bits_of(v)) for i, v in want], (name, p)


def test_list_mode_places_position_i_at_list_i():
    rng = np.random.default_rng(5)
    X = ref.make_slab(rng, 20, 9)
    q = rng.standard_normal(9).astype(np.float32)
    ids, rk = ref.ranks_with_dead(20, [4])
    full = ref.score_column(X, 9, 7, rk, q, L2, 0)
    rows = [19, 3, 3, 4, 0]
    keys, pay, _ = ref.score_column(X, 9, 7, rk, q, L2, 0, rows)
    assert list(pay["row"]) == rows and list(keys) == [full[0][r] for r in rows] and keys[3] == ref.EMPTY_KEY
    keys, pay, status = ref.score_column(X, 9, 7, rk, q, L2, 0, [])
    assert len(keys) == 0 and len(pay) == 0 and status == 0


def test_a_zero_prefix_and_an_overflow():
    X = np.zeros((3, 8), np.float32)
    X[1] = 1.0
    X[2, 0] = 3e38
    rk = np.arange(3, dtype=np.uint32)
    q = np.asarray([0, 0, 1, 1, 1, 1, 1, 1], np.float32)
    # cosine with a zero norm on either side is 0.0 (distances.rs:168), not an error
    keys, pay, status = ref.score_column(X, 8, 2, rk, q, COSINE, 0)
    assert status == 0 and list(pay["raw"]) == [0.0, 0.0, 0.0]
    keys, pay, status = ref.score_column(X, 8, 8, rk, q, COSINE, 0)
    assert status == 0 and pay["raw"][0] == 0.0 and bits_of(pay["raw"][1]) == bits_of(oracle.cosine(q, X[1]))
    # an f32 chain that overflows and an f64 recovery that is finite; one whose recovery is not
    big = np.asarray([3e38, 0, 0, 0, 0, 0, 0, 0], np.float32)
    keys, pay, status = ref.score_column(X, 8, 8, rk, 0 * big, L2, 0)
    assert status == 0 and bits_of(pay["raw"][2]) == bits_of(oracle.compute(L2, 0 * big, X[2]))
    keys, pay, status = ref.score_column(X, 8, 8, rk, big, INNER_PRODUCT, 0)
    assert status == ref.ERR_OVERFLOW and keys[2] == ref.EMPTY_KEY and np.isnan(pay["raw"][2]) and keys[1] != ref.EMPTY_KEY
    with pytest.raises(oracle.OracleError):
        oracle.compute(INNER_PRODUCT, big, X[2])
