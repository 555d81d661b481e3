"""numpy restatement of the 6-bit sketch (K1s: vettore_amd/csrc/vt_sketch.hip, host/vt_sketch6.h): the row
quantiser, the two-plane tile layout, the query's signed-nibble levels and the interval every row's K1 dot must lie in.
Test infrastructure for tests/test_sketch6_model.py; no GPU, nothing of the library is loaded."""
import numpy as np

LEVELS = 3
TILE_ROWS = 64
UP = 1.0 + 2.0 ** -30
SLACK = 1.0 + 2.0 ** -40


def ld8_of(d):
    return (d + 127) // 128 * 128


def runs_of(d):
    return 3 * (ld8_of(d) // 64) + 1


def f32_up(v):
    f = np.float32(v)
    return np.nextafter(f, np.float32(np.inf)) if float(f) < v else f


def quantise_rows(x):
    """X in [-31, 31] (int32), s, rho, nu (float32) per row, with the kernel's f32 scale and reciprocal."""
    x = np.ascontiguousarray(x, np.float32)
    n, d = x.shape
    m = np.abs(x).max(axis=1) if d else np.zeros(n, np.float32)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        s = (m / np.float32(31.0)).astype(np.float32)
        inv = (np.float32(31.0) / m).astype(np.float32)
    ok = (m > 0) & np.isfinite(inv) & (s > 0)
    s = np.where(ok, s, np.float32(0)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        X = np.where(ok[:, None], np.clip(np.rint((x * inv[:, None]).astype(np.float32)), -31, 31), 0).astype(np.int32)
    r = x.astype(np.float64) - s.astype(np.float64)[:, None] * X
    rho = np.sqrt((r * r).sum(axis=1)) * UP
    nu = s.astype(np.float64) * np.sqrt((X.astype(np.float64) ** 2).sum(axis=1)) * UP
    return X, s, np.array([f32_up(v) for v in rho], np.float32), np.array([f32_up(v) for v in nu], np.float32)


def split_planes(X):
    H = X >> 2            # arithmetic: [-8, 7]
    L = X & 3             # [0, 3]
    return H, L


def pack_tiles(X, s, rho, nu):
    """The image as the build kernel writes it: bytes [tiles][runs][64 lanes][16]."""
    n, d = X.shape
    ld8 = ld8_of(d)
    nh, nl, runs = ld8 // 32, ld8 // 64, runs_of(d)
    tiles = (n + TILE_ROWS - 1) // TILE_ROWS
    Xp = np.zeros((tiles * TILE_ROWS, ld8), np.int64)
    Xp[:n, :d] = X
    H, L = split_planes(Xp)
    img = np.zeros((tiles, runs, TILE_ROWS, 4), np.uint32)
    Ht = (H & 0xF).reshape(tiles, TILE_ROWS, nh, 4, 8)        # [t][lane][run c][dword j][nibble i]
    for i in range(8):
        img[:, :nh] |= (Ht[..., i].transpose(0, 2, 1, 3) << (4 * i)).astype(np.uint32)
    Lt = L.reshape(tiles, TILE_ROWS, nl, 2, 4, 8)             # [t][lane][run c'][half h][dword j][i]
    for h in range(2):
        for i in range(8):
            img[:, nh:nh + nl] |= (Lt[:, :, :, h, :, i].transpose(0, 2, 1, 3) << (4 * i + 2 * h)).astype(np.uint32)
    meta = np.zeros((tiles * TILE_ROWS, 4), np.uint32)
    meta[:n, 0] = s.view(np.uint32)
    meta[:n, 1] = rho.view(np.uint32)
    meta[:n, 2] = nu.view(np.uint32)
    img[:, nh + nl] = meta.reshape(tiles, TILE_ROWS, 4)
    return img


def unpack_tiles(img, n, d):
    """X, s, rho, nu back out of the image, the way the pass reads it (masks and shifts on whole dwords)."""
    tiles, runs = img.shape[:2]
    ld8 = ld8_of(d)
    nh, nl = ld8 // 32, ld8 // 64
    H = np.zeros((tiles, TILE_ROWS, nh, 4, 8), np.int64)
    for i in range(8):
        nib = ((img[:, :nh] >> (4 * i)) & 0xF).astype(np.int64)
        H[..., i] = np.where(nib >= 8, nib - 16, nib).transpose(0, 2, 1, 3)
    L = np.zeros((tiles, TILE_ROWS, nl, 2, 4, 8), np.int64)
    lo = img[:, nh:nh + nl] & 0x33333333
    hi = (img[:, nh:nh + nl] >> 2) & 0x33333333
    for h, w in enumerate((lo, hi)):
        for i in range(8):
            L[:, :, :, h, :, i] = ((w >> (4 * i)) & 0xF).astype(np.int64).transpose(0, 2, 1, 3)
    X = 4 * H.reshape(tiles * TILE_ROWS, ld8) + L.reshape(tiles * TILE_ROWS, ld8)
    meta = img[:, nh + nl].reshape(tiles * TILE_ROWS, 4)
    return (X[:n, :d], meta[:n, 0].copy().view(np.float32), meta[:n, 1].copy().view(np.float32),
            meta[:n, 2].copy().view(np.float32))


def query_levels(q, levels=LEVELS):
    """Q [levels][d] in [-7, 7], t [levels] float32, eta = q - sum_j t_j Q_j (float64), as host/vt_sketch6.h forms them."""
    r = np.asarray(q, np.float32).astype(np.float64)
    Q = np.zeros((levels, len(r)), np.int64)
    t = np.zeros(levels, np.float32)
    for j in range(levels):
        m = np.abs(r).max() if len(r) else 0.0
        with np.errstate(over="ignore", divide="ignore"):
            tj = np.float32(m / 7.0)
            if not (tj > 0 and np.isfinite(tj) and np.isfinite(7.0 / np.float64(tj))):
                tj = np.float32(0)
        t[j] = tj
        inv = 1.0 / np.float64(tj) if tj > 0 else 0.0
        Q[j] = np.clip(np.rint(r * inv), -7, 7).astype(np.int64)
        r = r - np.float64(tj) * Q[j]
    return Q, t, r


def intervals(X, s, rho, nu, q, levels=LEVELS):
    """[a - e, a + e] per row: DESIGN 4.10's formula with this column's s, rho, nu and this query's eta."""
    d = X.shape[1]
    Q, t, eta_v = query_levels(q, levels)
    H, L = split_planes(X)
    qn = np.sqrt((np.asarray(q, np.float64) ** 2).sum()) * UP
    eta = np.sqrt((eta_v ** 2).sum()) * UP
    total = np.zeros(X.shape[0], np.float64)
    for j in range(levels):
        total += np.float64(t[j]) * (4 * (H @ Q[j]) + (L @ Q[j])).astype(np.float64)
    a = s.astype(np.float64) * total
    rho, nu = rho.astype(np.float64), nu.astype(np.float64)
    kerr = 8.0 * d * 2.0 ** -24
    tiny = (d + 16.0) * 2.0 ** -125
    e = (qn * rho + eta * nu + kerr * qn * (nu + rho) + 2.0 ** -40 * nu * (qn + eta)) * SLACK + tiny
    return a, e


# ---- the pass's own arithmetic, operation by operation ------------------------------------------------------------------
# What sketch6_scan_kernel, sketch5_scan_kernel and sketch_scan_kernel do once a row's integer dots are complete, in the
# kernels' order of operations.  numpy's float64 and float32 are the IEEE formats the device uses and the units are built
# without contraction, so the words below are the pass's words bit for bit (tests/test_gpu_sketch_kernels.py).
M_COS, M_IP, M_NIP = 2, 3, 4


def f32_up_v(v):
    """f64 -> f32 towards +inf, element-wise (f32_up of vt_sketch.cuh)."""
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        f = v.astype(np.float32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def f32_down_v(v):
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        f = v.astype(np.float32)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def orderable(f):
    """f32::total_cmp as an order-preserving u32 (vt_common.cuh)."""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def pass_error(d, s, rho, nu, qn, eta, kerr, w3=None):
    """e_r as the kernels write it: the four terms left to right, s_r w3 behind them where the pass has one, the slack, tiny."""
    s, rho, nu = (np.asarray(v, np.float32).astype(np.float64) for v in (s, rho, nu))
    qn, eta, kerr = np.float64(qn), np.float64(eta), np.float64(kerr)
    tiny = (np.float64(d) + 16.0) * 2.0 ** -125
    e = qn * rho + eta * nu + kerr * qn * (nu + rho) + 2.0 ** -40 * nu * (qn + eta)
    if w3 is not None:
        e = e + s * np.float64(w3)
    return e * SLACK + tiny


def interval_words(metric, av, e):
    """(orderable key(hi_r) word -- the high half of the list's key --, orderable key(lo_r) word -- the payload's --) from
    a_r and e_r: f32_up / f32_down, then 1.0f - x or -x in f32."""
    hi, lo = f32_up_v(av + e), f32_down_v(av - e)
    if metric == M_COS:
        first, second = np.float32(1.0) - hi, np.float32(1.0) - lo
    else:
        first, second = -hi, -lo
    return orderable(first), orderable(second)


def split_pass_words(metric, X, s, rho, nu, Q, t, qn, eta, kerr, c3, w3, shift):
    """The 6-bit (shift = 2) and 5-bit (shift = 1) passes for any integer levels Q [3][d] with scales t:
    sum = t1 (2^shift H.Q1 + L.Q1) + t2 (2^shift H.Q2 + L.Q2) + t3 (2^shift H.Q3) + c3, left to right; a_r = s_r sum."""
    X, Q = np.asarray(X, np.int64), np.asarray(Q, np.int64)
    H = X >> shift
    t = np.asarray(t, np.float32).astype(np.float64)
    full = X @ Q[:2].T                                     # 2^shift accH_j + accL_j: the whole of X . Q_j
    top = (H @ Q[2]) << shift
    total = t[0] * full[:, 0].astype(np.float64) + t[1] * full[:, 1].astype(np.float64) + t[2] * top.astype(np.float64) + np.float64(c3)
    av = np.asarray(s, np.float32).astype(np.float64) * total
    return interval_words(metric, av, pass_error(X.shape[1], s, rho, nu, qn, eta, kerr, w3))
