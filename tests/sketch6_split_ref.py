"""numpy restatement of the 6-bit pass with its last query level kept off the L plane (K1s: vettore_amd/csrc/vt_sketch_nibble.hip,
host/vt_sketch6.h sketch6_level_sums), beside sketch6_ref.py: levels 1-3 meet the H plane, levels 1-2 the L
plane, and level 3's share there, Q3.L with 0 <= L_i <= 3, is replaced by its centre c3 and half-width w3.
Test infrastructure for tests/test_sketch6_split_model.py and tests/test_gpu_sketch6_split.py; nothing of the library is loaded."""
import numpy as np

import sketch6_ref as ref


def level_sums(Qj):
    """P = the sum of the positive entries, N = the sum of the negative ones (<= 0), ||Q||_1 = P - N."""
    Qj = np.asarray(Qj, np.int64)
    pos, neg = int(Qj[Qj > 0].sum()), int(Qj[Qj < 0].sum())
    return pos, neg, pos - neg


def intervals(X, s, rho, nu, q):
    """[a - e, a + e] per row as the pass forms it: c3 = 1.5 t3 (P3 + N3) joins the sum s_r multiplies, s_r w3 with
    w3 = 1.5 t3 ||Q3||_1 joins e_r."""
    assert ref.LEVELS == 3
    d = X.shape[1]
    Q, t, eta_v = ref.query_levels(q)
    H, L = ref.split_planes(X)
    qn = np.sqrt((np.asarray(q, np.float64) ** 2).sum()) * ref.UP
    eta = np.sqrt((eta_v ** 2).sum()) * ref.UP
    pos, neg, l1 = level_sums(Q[2])
    t3 = 1.5 * np.float64(t[2])
    c3, w3 = t3 * float(pos + neg), t3 * float(l1)
    total = np.zeros(X.shape[0], np.float64)
    for j in range(2):
        total += np.float64(t[j]) * (4 * (H @ Q[j]) + (L @ Q[j])).astype(np.float64)
    total += np.float64(t[2]) * (4 * (H @ Q[2])).astype(np.float64)
    total += c3
    s64 = s.astype(np.float64)
    a = s64 * total
    rho, nu = rho.astype(np.float64), nu.astype(np.float64)
    kerr = 8.0 * d * 2.0 ** -24
    tiny = (d + 16.0) * 2.0 ** -125
    e = (qn * rho + eta * nu + kerr * qn * (nu + rho) + 2.0 ** -40 * nu * (qn + eta) + s64 * w3) * ref.SLACK + tiny
    return a, e


def level_bound(Q3, t3):
    """c3, w3 as host/vt_sketch6.h (sketch6_level_bound) forms them for the 6-bit pass: 1.5 t3 (P3 + N3) and 1.5 t3 ||Q3||_1."""
    pos, neg, l1 = level_sums(Q3)
    t15 = 1.5 * np.float64(np.float32(t3))
    return t15 * float(pos + neg), t15 * float(l1)


def pass_words(metric, X, s, rho, nu, Q, t, qn, eta, kerr, c3, w3):
    """sketch6_scan_kernel's two words per row, bit for bit (sketch6_ref.split_pass_words says how); `intervals` above adds
    c3 in another association and stays the model of the bound, not of the bits."""
    return ref.split_pass_words(metric, X, s, rho, nu, Q, t, qn, eta, kerr, c3, w3, 2)


def adversarial_rows(q, n, seed, mirror=False, scale=2.0 ** -9):
    """n rows x = scale * X with X in [-31, 31] chosen so that, for the query q, the term the pass drops sits at an end of
    its range: L = X mod 4 is 3 exactly where Q3 > 0 and 0 where Q3 < 0 (Q3.L = 3 P3, the upper end), or the mirror image
    (3 where Q3 < 0, 0 where Q3 > 0: Q3.L = 3 N3).  H is random; one element is 31 so that the row's scale is `scale`
    and x / s is X itself (scale a power of two: every step of the quantiser is exact)."""
    q = np.asarray(q, np.float32)
    d = len(q)
    Q3 = ref.query_levels(q)[0][2]
    rng = np.random.default_rng(seed)
    up, down = (Q3 < 0, Q3 > 0) if mirror else (Q3 > 0, Q3 < 0)
    L = rng.integers(0, 4, (n, d))
    L[:, up] = 3
    L[:, down] = 0
    H = rng.integers(-7, 8, (n, d))  # (-7: X = 4 H + L >= -28 stays inside [-31, 31])
    X = 4 * H + L
    pin = np.nonzero(~down)[0]  # an element that may be 31 = 4 * 7 + 3
    assert pin.size
    X[np.arange(n), pin[rng.integers(0, pin.size, n)]] = 31
    assert np.abs(X).max() == 31
    x = (X * scale).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), X * scale)
    return x, X
