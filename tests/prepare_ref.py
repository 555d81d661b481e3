"""A numpy / Python model of the reference's normalizations and sign bits (native/vettore/src/distances.rs:350-423),
operation by operation in the reference's order -- what the K14 tests compare against, byte for byte.

  validate    every value finite, else ValueError("vector contains a non-finite value")
  l2          norm = sqrt(sum f64(x) * f64(x)), a sequential f64 sum from 0.0 (f64_dot, :179-184); norm == 0 -> zeros,
              else f32(f64(x) / norm)
  zscore      mean = (sequential sum f64(x)) / d; var = (sequential sum (f64(x) - mean)^2) / d; sd = sqrt(var);
              sd == 0 -> zeros, else f32((f64(x) - mean) / sd)
  minmax      min / max: an in-order f32 fold from +-inf; min == max -> zeros,
              else f32((f64(x) - f64(min)) / (f64(max) - f64(min)))
  none        the values themselves
  sign bits   bit j % 64 of word j // 64 is out[j] >= 0.0, on the ROUNDED f32 output (:413-423)

The sequential sums are np.cumsum(...)[-1]: cumsum adds in index order (np.sum is pairwise and gives other last bits);
`sequential_sum_loop` is the plain loop, and tests/test_prepare_model.py holds the two equal.  Products, differences and
quotients are single IEEE f64 operations, which numpy performs one by one (no fused multiply-add).

Unpinned by the reference: Rust's f32::min / max do not say which zero wins between +0.0 and -0.0.  `fold_min` /
`fold_max` below behave like C's fminf / fmaxf as the compilers here lower them (a later zero of the other sign does not
replace the running one); tests keep rows whose minimum or maximum is a zero and that hold zeros of both signs out of
the bit-exact comparisons (`minmax_is_pinned`).
"""
import numpy as np

MODES = ("none", "l2", "zscore", "minmax")
NON_FINITE = "vector contains a non-finite value"


def sequential_sum(values64: np.ndarray) -> np.float64:
    """f64 sum in index order, starting from 0.0."""
    if values64.size == 0:
        return np.float64(0.0)
    return np.float64(0.0) + np.cumsum(values64, dtype=np.float64)[-1]


def sequential_sum_loop(values64: np.ndarray) -> np.float64:
    acc = np.float64(0.0)
    for v in values64:
        acc = acc + np.float64(v)
    return acc


def fold_min(x: np.ndarray) -> np.float32:
    m = np.float32(np.inf)
    for v in x:
        if v < m:
            m = v
    return np.float32(m)


def fold_max(x: np.ndarray) -> np.float32:
    m = np.float32(-np.inf)
    for v in x:
        if v > m:
            m = v
    return np.float32(m)


def minmax_is_pinned(x: np.ndarray) -> bool:
    """False for the rows whose result depends on which zero f32::min / max return."""
    x = np.asarray(x, dtype=np.float32)
    if x.size == 0:
        return True
    zeros = x[x == 0]
    both_signs = zeros.size > 0 and np.signbit(zeros).any() and not np.signbit(zeros).all()
    return not (both_signs and (x.min() == 0 or x.max() == 0))


def _f32(values64: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore", under="ignore"):
        return values64.astype(np.float32)


def normalize(vector, mode: str) -> np.ndarray:
    x = np.ascontiguousarray(vector, dtype=np.float32).reshape(-1)
    if mode not in MODES:
        raise KeyError(mode)
    if not np.isfinite(x).all():
        raise ValueError(NON_FINITE)
    if mode == "none" or x.size == 0:
        return x.copy()
    x64 = x.astype(np.float64)
    zeros = np.zeros(x.size, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if mode == "l2":
            norm = np.sqrt(sequential_sum(x64 * x64))
            return zeros if norm == 0.0 else _f32(x64 / norm)
        if mode == "zscore":
            n = np.float64(x.size)
            mean = sequential_sum(x64) / n
            diff = x64 - mean
            sd = np.sqrt(sequential_sum(diff * diff) / n)
            return zeros if sd == 0.0 else _f32((x64 - mean) / sd)
        lo, hi = fold_min(x), fold_max(x)
        if lo == hi:
            return zeros
        return _f32((x64 - np.float64(lo)) / (np.float64(hi) - np.float64(lo)))


def sign_bits(vector) -> np.ndarray:
    x = np.ascontiguousarray(vector, dtype=np.float32).reshape(-1)
    words = np.zeros((x.size + 63) // 64, dtype=np.uint64)
    for j in np.nonzero(x >= np.float32(0.0))[0]:
        words[j // 64] |= np.uint64(1) << np.uint64(j % 64)
    return words


def prepare_rows(matrix, mode: str):
    """Row by row: (normalized [n][d] float32, words [n][(d + 63) // 64] uint64); ValueError with .row on a refusal."""
    m = np.ascontiguousarray(matrix, dtype=np.float32)
    n, d = m.shape
    out = np.empty_like(m)
    words = np.zeros((n, (d + 63) // 64), dtype=np.uint64)
    for i in range(n):
        try:
            out[i] = normalize(m[i], mode)
        except ValueError as e:
            e.row = i
            raise
        words[i] = sign_bits(out[i])
    return out, words
