"""The numpy model of K1n's 4-bit sketch (vt_sketch_nibble.hip): the column, the interval and the exact-threshold
rule behind the pass.  The query's levels are the 6-bit sketch's (sketch6_ref.query_levels), unchanged."""
import numpy as np

import sketch6_ref as ref6

TILE_ROWS = ref6.TILE_ROWS
EMPTY = np.uint32(0xFFFFFFFF)


def runs_of(d):
    return ref6.ld8_of(d) // 32 + 1


def quantise_rows(x):
    """X in [-7, 7] (int32), s, rho, nu (float32) per row, with the kernel's f32 scale and reciprocal."""
    x = np.ascontiguousarray(x, np.float32)
    n, d = x.shape
    m = np.abs(x).max(axis=1) if d else np.zeros(n, np.float32)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        s = (m / np.float32(7.0)).astype(np.float32)
        inv = (np.float32(7.0) / m).astype(np.float32)
    ok = (m > 0) & np.isfinite(inv) & (s > 0)
    s = np.where(ok, s, np.float32(0)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        X = np.where(ok[:, None], np.clip(np.rint((x * inv[:, None]).astype(np.float32)), -7, 7), 0).astype(np.int32)
    r = x.astype(np.float64) - s.astype(np.float64)[:, None] * X
    rho = np.sqrt((r * r).sum(axis=1)) * ref6.UP
    nu = s.astype(np.float64) * np.sqrt((X.astype(np.float64) ** 2).sum(axis=1)) * ref6.UP
    return X, s, np.array([ref6.f32_up(v) for v in rho], np.float32), np.array([ref6.f32_up(v) for v in nu], np.float32)


def pack_tiles(X, s, rho, nu):
    """The image as the build kernel writes it: dwords [tiles][runs][64 lanes][4]."""
    n, d = X.shape
    ld8 = ref6.ld8_of(d)
    nh, runs = ld8 // 32, runs_of(d)
    tiles = (n + TILE_ROWS - 1) // TILE_ROWS
    Xp = np.zeros((tiles * TILE_ROWS, ld8), np.int64)
    Xp[:n, :d] = X
    img = np.zeros((tiles, runs, TILE_ROWS, 4), np.uint32)
    Ht = (Xp & 0xF).reshape(tiles, TILE_ROWS, nh, 4, 8)        # [t][lane][run c][dword j][nibble i]
    for i in range(8):
        img[:, :nh] |= (Ht[..., i].transpose(0, 2, 1, 3) << (4 * i)).astype(np.uint32)
    meta = np.zeros((tiles * TILE_ROWS, 4), np.uint32)
    meta[:n, 0] = s.view(np.uint32)
    meta[:n, 1] = rho.view(np.uint32)
    meta[:n, 2] = nu.view(np.uint32)
    img[:, nh] = meta.reshape(tiles, TILE_ROWS, 4)
    return img


def unpack_tiles(img, n, d):
    """X, s, rho, nu back out of the image, the way the pass reads it: signed nibbles."""
    tiles = img.shape[0]
    ld8 = ref6.ld8_of(d)
    nh = ld8 // 32
    H = np.zeros((tiles, TILE_ROWS, nh, 4, 8), np.int64)
    for i in range(8):
        nib = ((img[:, :nh] >> (4 * i)) & 0xF).astype(np.int64)
        H[..., i] = np.where(nib >= 8, nib - 16, nib).transpose(0, 2, 1, 3)
    X = H.reshape(tiles * TILE_ROWS, ld8)
    meta = img[:, nh].reshape(tiles * TILE_ROWS, 4)
    return (X[:n, :d], meta[:n, 0].copy().view(np.float32), meta[:n, 1].copy().view(np.float32),
            meta[:n, 2].copy().view(np.float32))


def intervals(X, s, rho, nu, q):
    """[a - e, a + e] per row: DESIGN 4.10's formula with this column's s, rho, nu, every level on the one plane."""
    d = X.shape[1]
    Q, t, eta_v = ref6.query_levels(q)
    qn = np.sqrt((np.asarray(q, np.float64) ** 2).sum()) * ref6.UP
    eta = np.sqrt((eta_v ** 2).sum()) * ref6.UP
    total = np.zeros(X.shape[0], np.float64)
    for j in range(ref6.LEVELS):
        total += np.float64(t[j]) * (np.asarray(X, np.int64) @ Q[j]).astype(np.float64)
    a = s.astype(np.float64) * total
    return a, ref6.pass_error(d, s, rho, nu, qn, eta, 8.0 * d * 2.0 ** -24)


def pass_words(metric, X, s, rho, nu, Q, t, qn, eta, kerr, c3=0.0, w3=0.0):
    """sketch4_scan_kernel's two words per row, bit for bit: sum = t1 X.Q1 + t2 X.Q2 + t3 X.Q3 left to right (each product
    exact in f64), a_r = s_r sum, e_r without a level term (c3 and w3 are not read)."""
    X, Q = np.asarray(X, np.int64), np.asarray(Q, np.int64)
    t = np.asarray(t, np.float32).astype(np.float64)
    acc = X @ Q.T
    total = t[0] * acc[:, 0].astype(np.float64) + t[1] * acc[:, 1].astype(np.float64) + t[2] * acc[:, 2].astype(np.float64)
    av = np.asarray(s, np.float32).astype(np.float64) * total
    return ref6.interval_words(metric, av, ref6.pass_error(X.shape[1], s, rho, nu, qn, eta, kerr))


def exact_threshold(lo, slots_rank, exact_words, k):
    """The refine step on flat arrays of live slots: lo = the key(lo) words, exact_words = K1's key word per slot.  Kt = the
    k-th smallest key(lo) word; Kt' = min(Kt, the largest exact word among k slots with the smallest key(lo) words) -- any
    choice among the copies of Kt is allowed, so the answer is the pair (lowest, highest) Kt' a choice can give.  With k or
    fewer live words both are 0xffffffff."""
    lo = np.asarray(lo, np.uint32)
    if len(lo) <= k:
        return 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF
    order = np.argsort(lo, kind="stable")
    kt = int(lo[order[k - 1]])
    below = order[lo[order] < kt]
    ties = np.nonzero(lo == kt)[0]
    need = k - len(below)
    base = int(exact_words[below].max()) if len(below) else 0
    tw = np.sort(exact_words[ties])
    low = max(base, int(tw[need - 1]))
    high = max(base, int(tw[-1]))
    return kt, min(kt, low), min(kt, high)
