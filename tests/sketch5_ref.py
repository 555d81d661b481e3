"""numpy restatement of the 5-bit sketch (K1f: vettore_amd/csrc/vt_sketch_nibble.hip, host/vt_sketch5.h): the row
quantiser, the tile layout with its one-bit L plane, and the interval every row's K1 dot must lie in -- levels 1-3 of the
query (sketch6_ref.query_levels, the 6-bit sketch's own) meet the H plane, levels 1-2 the L plane, and level 3's share
there, Q3.L with 0 <= L_i <= 1, is replaced by its centre c3 and half-width w3.
Test infrastructure for tests/test_sketch5_model.py; no GPU, nothing of the library is loaded."""
import numpy as np

import sketch6_ref as ref6

TILE_ROWS = ref6.TILE_ROWS


def runs_of(d):
    return 5 * (ref6.ld8_of(d) // 128) + 1


def quantise_rows(x):
    """X in [-15, 15] (int32), s, rho, nu (float32) per row, with the kernel's f32 scale and reciprocal."""
    x = np.ascontiguousarray(x, np.float32)
    n, d = x.shape
    m = np.abs(x).max(axis=1) if d else np.zeros(n, np.float32)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        s = (m / np.float32(15.0)).astype(np.float32)
        inv = (np.float32(15.0) / m).astype(np.float32)
    ok = (m > 0) & np.isfinite(inv) & (s > 0)
    s = np.where(ok, s, np.float32(0)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        X = np.where(ok[:, None], np.clip(np.rint((x * inv[:, None]).astype(np.float32)), -15, 15), 0).astype(np.int32)
    r = x.astype(np.float64) - s.astype(np.float64)[:, None] * X
    rho = np.sqrt((r * r).sum(axis=1)) * ref6.UP
    nu = s.astype(np.float64) * np.sqrt((X.astype(np.float64) ** 2).sum(axis=1)) * ref6.UP
    return X, s, np.array([ref6.f32_up(v) for v in rho], np.float32), np.array([ref6.f32_up(v) for v in nu], np.float32)


def split_planes(X):
    H = X >> 1            # arithmetic: [-8, 7]
    L = X & 1             # [0, 1]
    return H, L


def pack_tiles(X, s, rho, nu):
    """The image as the build kernel writes it: bytes [tiles][runs][64 lanes][16]."""
    n, d = X.shape
    ld8 = ref6.ld8_of(d)
    nh, nl, runs = ld8 // 32, ld8 // 128, runs_of(d)
    tiles = (n + TILE_ROWS - 1) // TILE_ROWS
    Xp = np.zeros((tiles * TILE_ROWS, ld8), np.int64)
    Xp[:n, :d] = X
    H, L = split_planes(Xp)
    img = np.zeros((tiles, runs, TILE_ROWS, 4), np.uint32)
    Ht = (H & 0xF).reshape(tiles, TILE_ROWS, nh, 4, 8)        # [t][lane][run c][dword j][nibble i]
    for i in range(8):
        img[:, :nh] |= (Ht[..., i].transpose(0, 2, 1, 3) << (4 * i)).astype(np.uint32)
    Lt = L.reshape(tiles, TILE_ROWS, nl, 4, 4, 8)             # [t][lane][run c'][b][dword j][i]: element 128 c' + 32 b + 8 j + i
    for b in range(4):
        for i in range(8):
            img[:, nh:nh + nl] |= (Lt[:, :, :, b, :, i].transpose(0, 2, 1, 3) << (4 * i + b)).astype(np.uint32)
    meta = np.zeros((tiles * TILE_ROWS, 4), np.uint32)
    meta[:n, 0] = s.view(np.uint32)
    meta[:n, 1] = rho.view(np.uint32)
    meta[:n, 2] = nu.view(np.uint32)
    img[:, nh + nl] = meta.reshape(tiles, TILE_ROWS, 4)
    return img


def unpack_tiles(img, n, d):
    """X, s, rho, nu back out of the image, the way the pass reads it: (w >> b) & 0x11111111 is the nibble vector that
    lines up with dword j of the H-run 4 c' + b."""
    tiles = img.shape[0]
    ld8 = ref6.ld8_of(d)
    nh, nl = ld8 // 32, ld8 // 128
    H = np.zeros((tiles, TILE_ROWS, nh, 4, 8), np.int64)
    for i in range(8):
        nib = ((img[:, :nh] >> (4 * i)) & 0xF).astype(np.int64)
        H[..., i] = np.where(nib >= 8, nib - 16, nib).transpose(0, 2, 1, 3)
    L = np.zeros((tiles, TILE_ROWS, nl, 4, 4, 8), np.int64)
    for b in range(4):
        w = (img[:, nh:nh + nl] >> b) & 0x11111111
        for i in range(8):
            L[:, :, :, b, :, i] = ((w >> (4 * i)) & 0xF).astype(np.int64).transpose(0, 2, 1, 3)
    X = 2 * H.reshape(tiles * TILE_ROWS, ld8) + L.reshape(tiles * TILE_ROWS, ld8)
    meta = img[:, nh + nl].reshape(tiles * TILE_ROWS, 4)
    return (X[:n, :d], meta[:n, 0].copy().view(np.float32), meta[:n, 1].copy().view(np.float32),
            meta[:n, 2].copy().view(np.float32))


def level_sums(Qj):
    """P = the sum of the positive entries, N = the sum of the negative ones (<= 0), ||Q||_1 = P - N."""
    Qj = np.asarray(Qj, np.int64)
    pos, neg = int(Qj[Qj > 0].sum()), int(Qj[Qj < 0].sum())
    return pos, neg, pos - neg


def intervals(X, s, rho, nu, q, split=True):
    """[a - e, a + e] per row as the pass forms it: a_r = s_r (sum_{j <= 2} t_j (2 H.Q_j + L.Q_j) + 2 t_3 H.Q_3 + c3) with
    c3 = 0.5 t3 (P3 + N3), and s_r w3 with w3 = 0.5 t3 ||Q3||_1 joins e_r.  split=False: level 3 on the L plane too (what the
    pass would give if it spent the dots), for the price of keeping it off."""
    d = X.shape[1]
    Q, t, eta_v = ref6.query_levels(q)
    H, L = split_planes(X)
    qn = np.sqrt((np.asarray(q, np.float64) ** 2).sum()) * ref6.UP
    eta = np.sqrt((eta_v ** 2).sum()) * ref6.UP
    total = np.zeros(X.shape[0], np.float64)
    for j in range(2):
        total += np.float64(t[j]) * (2 * (H @ Q[j]) + (L @ Q[j])).astype(np.float64)
    c3 = w3 = 0.0
    if split:
        pos, neg, l1 = level_sums(Q[2])
        c3, w3 = 0.5 * np.float64(t[2]) * float(pos + neg), 0.5 * np.float64(t[2]) * float(l1)
        total += np.float64(t[2]) * (2 * (H @ Q[2])).astype(np.float64) + c3
    else:
        total += np.float64(t[2]) * (2 * (H @ Q[2]) + (L @ Q[2])).astype(np.float64)
    s64 = s.astype(np.float64)
    a = s64 * total
    rho, nu = rho.astype(np.float64), nu.astype(np.float64)
    kerr = 8.0 * d * 2.0 ** -24
    tiny = (d + 16.0) * 2.0 ** -125
    e = (qn * rho + eta * nu + kerr * qn * (nu + rho) + 2.0 ** -40 * nu * (qn + eta) + s64 * w3) * ref6.SLACK + tiny
    return a, e


def level_bound(Q3, t3):
    """c3, w3 as host/vt_sketch5.h sketch5_level_bound forms them: 0.5 t3 (P3 + N3) and 0.5 t3 ||Q3||_1."""
    pos, neg, l1 = level_sums(Q3)
    half = 0.5 * np.float64(np.float32(t3))
    return half * float(pos + neg), half * float(l1)


def pass_words(metric, X, s, rho, nu, Q, t, qn, eta, kerr, c3, w3):
    """sketch5_scan_kernel's two words per row, bit for bit (sketch6_ref.split_pass_words says how); `intervals` above adds
    c3 in another association and stays the model of the bound, not of the bits."""
    return ref6.split_pass_words(metric, X, s, rho, nu, Q, t, qn, eta, kerr, c3, w3, 1)
