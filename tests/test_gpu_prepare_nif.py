"""normalize_zscore/1, normalize_minmax/1 and prepare_rows/2 of the erl_nif shim against the real library, on small
inputs: the terms that come back are tests/prepare_ref.py's numbers, bit for bit (a float term is the f32 widened)."""
import numpy as np
import pytest

import muvera_nif_runtime
import prepare_ref
import support
from nif_runtime import Atom

pytestmark = pytest.mark.gpu

OK, ERROR = Atom("ok"), Atom("error")


@pytest.fixture(scope="module")
def rt():
    return muvera_nif_runtime.Runtime()   # (interned atoms: the shim knows its mode atoms by identity)


def _rows(n, d, seed):
    rng = np.random.default_rng(seed)
    m = (rng.standard_normal((n, d)) * 10.0 ** rng.integers(-3, 4, (n, d))).astype(np.float32)
    m[1] = 4.0       # a constant row
    m[2] = 0.0       # an all-zero row
    return m


def _terms(matrix):
    return [[float(v) for v in row] for row in matrix]


def test_the_references_literals_through_the_shim(rt):
    for case in support.load("normalize_rs.json")["cases"]:
        if case["check"] != "eq" or None in case["values"]:
            continue
        name = {"zscore": "normalize_zscore", "minmax": "normalize_minmax"}[case["mode"]]
        assert rt.call(name, [float(v) for v in case["input"]]) == (OK, [float(v) for v in case["values"]]), case["source"]
    tag, z = rt.call("normalize_zscore", [1.0, 2.0, 3.0])           # vector_distance_test.exs:88-91
    assert tag == OK and abs(z[0] + 1.224744871391589) <= 1e-6 and z[1] == 0.0 and abs(z[2] - 1.224744871391589) <= 1e-6


@pytest.mark.parametrize("d", [1, 5, 64, 130])
def test_the_three_nifs_equal_the_model(rt, d):
    m = _rows(9, d, 50 + d)
    for mode in prepare_ref.MODES:
        want, want_words = prepare_ref.prepare_rows(m, mode)
        tag, pairs = rt.call("prepare_rows", Atom(mode), _terms(m))
        assert tag == OK and len(pairs) == len(m)
        for i, (vector, words) in enumerate(pairs):
            assert np.array(vector, dtype=np.float64).tobytes() == want[i].astype(np.float64).tobytes(), (mode, i)
            assert words == [int(w) for w in want_words[i]], (mode, i)
    for name, mode in (("normalize_zscore", "zscore"), ("normalize_minmax", "minmax")):
        for i in range(4):
            tag, vector = rt.call(name, _terms(m[i:i + 1])[0])
            want = prepare_ref.normalize(m[i], mode)
            assert tag == OK and np.array(vector, dtype=np.float64).tobytes() == want.astype(np.float64).tobytes()
    assert rt.live_resources() == 0
