"""numpy restatement of the int8 sketch (K1q: vettore_amd/csrc/vt_sketch.hip sketch_row / sketch_scan_kernel, vt_device.h
sketch_offset, host/vt_sketchsearch.h sketch_query_image): the row quantiser, the chunked tile layout, the query's
two int8 levels and the interval every row's K1 dot must lie in.
Test infrastructure for tests/test_sketch8_model.py and tests/test_gpu_sketch_kernels.py; nothing of the library is loaded."""
import numpy as np

import sketch6_ref as ref6

TILE_ROWS = ref6.TILE_ROWS
HALF = 127


def chunks_of(d):
    return ref6.ld8_of(d) // 16


def quantise_rows(x):
    """X in [-127, 127] (int32), s, rho, nu (float32) per row, with the kernel's f32 scale and reciprocal."""
    x = np.ascontiguousarray(x, np.float32)
    n, d = x.shape
    m = np.abs(x).max(axis=1) if d else np.zeros(n, np.float32)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        s = (m / np.float32(127.0)).astype(np.float32)
        inv = (np.float32(127.0) / m).astype(np.float32)
    ok = (m > 0) & np.isfinite(inv) & (s > 0)
    s = np.where(ok, s, np.float32(0)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        X = np.where(ok[:, None], np.clip(np.rint((x * inv[:, None]).astype(np.float32)), -127, 127), 0).astype(np.int32)
    r = x.astype(np.float64) - s.astype(np.float64)[:, None] * X
    rho = np.sqrt((r * r).sum(axis=1)) * ref6.UP
    nu = s.astype(np.float64) * np.sqrt((X.astype(np.float64) ** 2).sum(axis=1)) * ref6.UP
    return X, s, np.array([ref6.f32_up(v) for v in rho], np.float32), np.array([ref6.f32_up(v) for v in nu], np.float32)


def pack_tiles(X, s, rho, nu):
    """The image as the build kernel writes it: bytes [tiles][nch + 1][64 lanes][16] -- byte b of a row's chunk c is element
    16 c + b, and the tile's last run holds {s, rho, nu, 0} per row (sketch_offset)."""
    n, d = X.shape
    ld8, nch = ref6.ld8_of(d), chunks_of(d)
    tiles = (n + TILE_ROWS - 1) // TILE_ROWS
    Xp = np.zeros((tiles * TILE_ROWS, ld8), np.int8)
    Xp[:n, :d] = X
    img = np.zeros((tiles, nch + 1, TILE_ROWS, 16), np.uint8)
    img[:, :nch] = Xp.view(np.uint8).reshape(tiles, TILE_ROWS, nch, 16).transpose(0, 2, 1, 3)
    meta = np.zeros((tiles * TILE_ROWS, 4), np.uint32)
    meta[:n, 0] = s.view(np.uint32)
    meta[:n, 1] = rho.view(np.uint32)
    meta[:n, 2] = nu.view(np.uint32)
    img[:, nch] = meta.view(np.uint8).reshape(tiles, TILE_ROWS, 16)
    return img


def unpack_tiles(img, n, d):
    """X, s, rho, nu back out of the image, the way the pass reads it: a lane's 16 bytes of run c are its row's chunk c."""
    tiles = img.shape[0]
    nch = chunks_of(d)
    X = img[:, :nch].transpose(0, 2, 1, 3).reshape(tiles * TILE_ROWS, nch * 16).view(np.int8).astype(np.int32)
    meta = np.ascontiguousarray(img[:, nch]).view(np.uint32).reshape(tiles * TILE_ROWS, 4)
    return (X[:n, :d], meta[:n, 0].copy().view(np.float32), meta[:n, 1].copy().view(np.float32),
            meta[:n, 2].copy().view(np.float32))


def query_levels(q):
    """Q [2][d] in [-127, 127], t [2] float32, eta = q - t1 Q1 - t2 Q2 (float64), as sketch_query_image forms them: t1 from the
    f32 maximum divided in f32, t2 from the first residual's f64 maximum divided in f64; the integers from a reciprocal."""
    q32 = np.asarray(q, np.float32)
    r = q32.astype(np.float64)
    Q = np.zeros((2, len(r)), np.int64)
    t = np.zeros(2, np.float32)
    m1 = np.abs(q32).max() if len(r) else np.float32(0)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        t1 = np.float32(m1) / np.float32(127.0)
        if not (t1 > 0 and np.isfinite(np.float32(127.0) / np.float32(m1))):
            t1 = np.float32(0)
    t[0] = t1
    inv = 1.0 / np.float64(t1) if t1 > 0 else 0.0
    Q[0] = np.clip(np.rint(r * inv), -127, 127).astype(np.int64)
    r = r - np.float64(t1) * Q[0]
    m2 = np.abs(r).max() if len(r) else 0.0
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        t2 = np.float32(m2 / 127.0)
        if not (t2 > 0 and np.isfinite(127.0 / np.float64(t2))):
            t2 = np.float32(0)
    t[1] = t2
    inv = 1.0 / np.float64(t2) if t2 > 0 else 0.0
    Q[1] = np.clip(np.rint(r * inv), -127, 127).astype(np.int64)
    return Q, t, r - np.float64(t2) * Q[1]


def query_image(Q, d):
    """The two levels as the pass reads them: [2][ld8] int8, zero past d."""
    img = np.zeros((2, ref6.ld8_of(d)), np.int8)
    img[:, :d] = Q
    return img


def intervals(X, s, rho, nu, q):
    """[a - e, a + e] per row: a_r = s_r (t1 Q1.X_r + t2 Q2.X_r), e_r = DESIGN 4.10's with this column's s, rho, nu."""
    d = X.shape[1]
    Q, t, eta_v = query_levels(q)
    qn = np.sqrt((np.asarray(q, np.float64) ** 2).sum()) * ref6.UP
    eta = np.sqrt((eta_v ** 2).sum()) * ref6.UP
    f = np.asarray(X, np.int64) @ Q.T
    a = s.astype(np.float64) * (np.float64(t[0]) * f[:, 0].astype(np.float64) + np.float64(t[1]) * f[:, 1].astype(np.float64))
    return a, ref6.pass_error(d, s, rho, nu, qn, eta, 8.0 * d * 2.0 ** -24)


def pass_words(metric, X, s, rho, nu, Q, t, qn, eta, kerr):
    """sketch_scan_kernel's two words per row, bit for bit, for any integer levels Q [2][d] with scales t: a_r =
    s_r (t1 f1 + t2 f2) in f64, e_r as written in the kernel, then sketch6_ref.interval_words."""
    f = np.asarray(X, np.int64) @ np.asarray(Q, np.int64).T
    t = np.asarray(t, np.float32).astype(np.float64)
    av = np.asarray(s, np.float32).astype(np.float64) * (t[0] * f[:, 0].astype(np.float64) + t[1] * f[:, 1].astype(np.float64))
    return ref6.interval_words(metric, av, ref6.pass_error(X.shape[1], s, rho, nu, qn, eta, kerr))
