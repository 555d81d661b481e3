"""tests/prepare_ref.py, the model the K14 tests compare against, checked on its own: against the reference's test
literals (tests/golden/normalize_rs.json) and, where the CPU oracle has the operation (l2, sign bits), against the oracle
bit for bit."""
import numpy as np
import pytest

import oracle
import prepare_ref
import support

GOLDEN = support.load("normalize_rs.json")["cases"]
_SPELLED = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf}


def _input(case):
    return np.array([_SPELLED.get(v, v) if isinstance(v, str) else v for v in case["input"]], dtype=np.float32)


@pytest.mark.parametrize("case", GOLDEN, ids=["%s %s %d" % (c["mode"], c["source"].split("/")[-1], i) for i, c in enumerate(GOLDEN)])
def test_model_reproduces_the_references_own_tests(case):
    x = _input(case)
    if case["check"] == "error":
        with pytest.raises(ValueError, match=prepare_ref.NON_FINITE):
            prepare_ref.normalize(x, case["mode"])
        return
    got = prepare_ref.normalize(x, case["mode"])
    assert got.dtype == np.float32 and got.shape == x.shape
    if case["check"] == "eq":
        assert len(case["values"]) == got.size
        for g, want in zip(got, case["values"]):
            assert want is None or float(g) == want
    elif case["check"] == "delta":
        for g, want in zip(got, case["values"]):
            assert want is None or abs(float(g) - want) <= case["delta"]
    else:  # moments: distances.rs:655-662, in f32 like the reference's test
        mean = np.float32(sum(got, np.float32(0))) / np.float32(got.size)
        var = np.float32(sum(((g - mean) ** 2 for g in got), np.float32(0))) / np.float32(got.size)
        assert support.close(float(mean), 0.0, case["delta"]) and support.close(float(var), 1.0, case["delta"])


def test_cumsum_is_the_sequential_sum_and_np_sum_is_not():
    rng = np.random.default_rng(14)
    differs = 0
    for n in (1, 2, 63, 64, 65, 130, 1000):
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(np.float32).astype(np.float64)
        assert prepare_ref.sequential_sum(v).tobytes() == prepare_ref.sequential_sum_loop(v).tobytes()
        differs += prepare_ref.sequential_sum(v).tobytes() != np.float64(np.sum(v)).tobytes()
    assert differs > 0   # (pairwise summation is another order: the model must not use it)
    assert prepare_ref.sequential_sum(np.array([-0.0, -0.0])).tobytes() == np.float64(0.0).tobytes()


def _rows():
    rng = np.random.default_rng(2014)
    rows = []
    for d in (1, 2, 63, 64, 65, 130):
        rows.append(rng.standard_normal(d).astype(np.float32))
        rows.append((rng.standard_normal(d) * 10.0 ** rng.integers(-20, 20, d)).astype(np.float32))
        rows.append(np.zeros(d, dtype=np.float32))
        rows.append(np.where(rng.random(d) < 0.5, np.float32(3e38), np.float32(-3e38)).astype(np.float32))
        rows.append((rng.integers(-(2 ** 22), 2 ** 22, d) * np.float64(2.0 ** -149)).astype(np.float32))   # subnormals
        # small negatives beside one huge value: their quotients underflow to -0.0
        under = np.full(d, np.float32(-1e-30), dtype=np.float32)
        under[0] = np.float32(3e38)
        rows.append(under)
    return rows


@pytest.mark.parametrize("row", _rows(), ids=lambda r: "d%d" % r.size)
def test_l2_and_sign_bits_equal_the_oracle_bit_for_bit(row):
    got = prepare_ref.normalize(row, "l2")
    assert got.tobytes() == oracle.normalize_l2(row).tobytes()
    for v in (row, got):
        assert prepare_ref.sign_bits(v).tobytes() == np.asarray(oracle.compress_sign_bits(v), dtype=np.uint64).tobytes()


def test_underflowed_negatives_set_their_bits():
    """The bits are taken from the rounded f32 output: a negative input whose quotient underflows is -0.0 there, and
    -0.0 >= 0.0 holds (distances.rs:417)."""
    row = np.array([3e38, -1e-30, -1e-30, 1.0], dtype=np.float32)
    out = prepare_ref.normalize(row, "l2")
    assert out[1].tobytes() == np.float32(-0.0).tobytes() and out[2].tobytes() == np.float32(-0.0).tobytes()
    assert int(prepare_ref.sign_bits(out)[0]) == 0b1111
    assert int(prepare_ref.sign_bits(row)[0]) == 0b1001
    assert prepare_ref.sign_bits(out).tobytes() == np.asarray(oracle.compress_sign_bits(out), dtype=np.uint64).tobytes()


def test_degenerate_rows_and_the_unpinned_ones():
    one = np.array([5.0], dtype=np.float32)
    for mode in ("zscore", "minmax"):
        assert prepare_ref.normalize(one, mode).tobytes() == np.zeros(1, dtype=np.float32).tobytes()
        assert prepare_ref.normalize(np.zeros(0, dtype=np.float32), mode).size == 0
    assert prepare_ref.normalize(one, "none").tobytes() == one.tobytes()
    assert prepare_ref.minmax_is_pinned(np.array([0.0, -0.0, 1.0], dtype=np.float32)) is False
    assert prepare_ref.minmax_is_pinned(np.array([-1.0, -0.0, 0.0, 1.0], dtype=np.float32)) is True
    assert prepare_ref.minmax_is_pinned(np.array([0.0, 0.0, 1.0], dtype=np.float32)) is True
    out, words = prepare_ref.prepare_rows(np.array([[1.0, -2.0, 3.0], [4.0, 4.0, 4.0]], dtype=np.float32), "minmax")
    assert out.tolist() == [[0.6000000238418579, 0.0, 1.0], [0.0, 0.0, 0.0]] and words.tolist() == [[7], [7]]
    with pytest.raises(ValueError) as e:
        prepare_ref.prepare_rows(np.array([[1.0], [np.inf]], dtype=np.float32), "none")
    assert e.value.row == 1
