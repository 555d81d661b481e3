"""numpy model of the matrix-core nomination family (K2 / K2b / K2s): what the kernels of vt_batch.hip,
vt_batch_bf16.hip and vt_batch_shadow.hip are documented to compute, written without looking at how they compute it.

  * bf16 rounding: round to nearest even on the f32 bit pattern (v_cvt_pk_bf16_f32);
  * the three images: q_image (K2b's queries), q_image16 (K2s's queries), shadow_image (K2s's rows; vt_device.h shadow_index);
  * scores: f64 dots of the exact operands and of the bf16-rounded ones, the L2 family as 2 q.x - |x|^2; a sequential f32
    accumulation of the rounded products (what test_batch_model.py holds against the margin on the CPU);
  * thresholds: the rank-th largest by f32::total_cmp, with the kernels' documented answers for short samples;
  * the certificate's margin, derived here from its statement (host/vt_batchbound.h is the library's own);
  * the input classes the model test and the kernel tests share.
"""
import math

import numpy as np

U = 2.0 ** -24    # f32 unit roundoff
UB = 2.0 ** -8    # bf16 unit roundoff
SENTINEL16 = np.uint16(0xA5A5)


# ---- bf16 ---------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """f32 -> the 16 bits of its bf16 rounding (nearest, ties to even); inf stays inf, a finite value may round to inf."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    return (r & 0xFFFF).astype(np.uint16)


def bf16_round(x):
    """f32 -> the f32 value of its bf16 rounding."""
    x = np.ascontiguousarray(x, np.float32)
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32).reshape(x.shape)


# ---- images -------------------------------------------------------------------------------------------------------------
def q_image(Q, ld, nq_pad):
    """K2b's query image as u16: image[c][t][s][lane = 32 h + r][e] = bf16(Q[32 t + r][32 c + 16 h + 8 s + e]); the image is
    sized for 256 columns (ld / 32 x 16 KiB), what a narrower batch does not write keeps the sentinel."""
    nchunk, qt = ld // 32, nq_pad // 32
    img = np.full(nchunk * 8 * 2 * 64 * 8, SENTINEL16, np.uint16)
    qb = bf16_bits(Q).reshape(nq_pad, ld)
    c, t, s, h, r, e = np.meshgrid(np.arange(nchunk), np.arange(qt), np.arange(2), np.arange(2), np.arange(32), np.arange(8), indexing="ij")
    slot = ((c * qt + t) * 2 + s) * 64 + 32 * h + r
    img[(slot * 8 + e).ravel()] = qb[(32 * t + r).ravel(), (32 * c + 16 * h + 8 * s + e).ravel()]
    return img


def q_image16(Q, ld, nq_pad):
    """K2s's query image as u16: image[c][query / 16][g][query % 16][e] = bf16(Q[query][32 c + 8 g + e])."""
    nchunk, nqt = ld // 32, nq_pad // 16
    img = np.full(nchunk * 16 * 64 * 8, SENTINEL16, np.uint16)
    qb = bf16_bits(Q).reshape(nq_pad, ld)
    c, t, g, r, e = np.meshgrid(np.arange(nchunk), np.arange(nqt), np.arange(4), np.arange(16), np.arange(8), indexing="ij")
    slot = (c * nqt + t) * 64 + 16 * g + r
    img[(slot * 8 + e).ravel()] = qb[(16 * t + r).ravel(), (32 * c + 8 * g + e).ravel()]
    return img


def shadow_index(row, col, ld):
    """[row / 16][col / 32][(col / 8) % 4][row % 16][col % 8], 1 KiB per (16 rows, 32 columns)."""
    return ((row >> 4) * (ld >> 5) + (col >> 5)) * 512 + ((col >> 3) & 3) * 128 + (row & 15) * 8 + (col & 7)


def shadow_image(X, rows_src, rows_img, ld):
    """K2s's row image as u16: rows >= rows_src are zero."""
    img = np.zeros(rows_img * ld, np.uint16)
    if rows_src:
        xb = bf16_bits(np.ascontiguousarray(X[:rows_src, :ld]))
        row, col = np.meshgrid(np.arange(rows_src), np.arange(ld), indexing="ij")
        img[shadow_index(row, col, ld).ravel()] = xb.ravel()
    return img


# ---- scores -------------------------------------------------------------------------------------------------------------
def scores64(Q, X, l2):
    """[query][row] in f64 from the operands as given: q.x, or 2 q.x - |x|^2."""
    Qd, Xd = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    s = Qd @ Xd.T
    return 2.0 * s - (Xd * Xd).sum(axis=1)[None, :] if l2 else s


def scores64_rounded(Q, X, l2):
    """the same from the bf16-rounded operands; the L2 family's norm stays the exact row's (the kernels subtract the stored
    norm of the f32 row)."""
    s = np.asarray(bf16_round(Q), np.float64) @ np.asarray(bf16_round(X), np.float64).T
    Xd = np.asarray(X, np.float64)
    return 2.0 * s - (Xd * Xd).sum(axis=1)[None, :] if l2 else s


def xnorm2_f32(X):
    """what launch_row_sqnorms stores: float32 of the f64 sum of squares."""
    Xd = np.asarray(X, np.float64)
    return (Xd * Xd).sum(axis=1).astype(np.float32)


def scores_f32_sequential(Q, X, l2, round_operands):
    """[query][row] as a plain f32 machine forms it: products (exact in f32 when the operands are bf16) added one by one in
    f32 in column order; the L2 family as 2 s - xnorm2 in f32."""
    Qf = bf16_round(Q) if round_operands else np.asarray(Q, np.float32)
    Xf = bf16_round(X) if round_operands else np.asarray(X, np.float32)
    acc = np.zeros((Qf.shape[0], Xf.shape[0]), np.float32)
    for j in range(Qf.shape[1]):
        acc = (acc + (Qf[:, j][:, None] * Xf[:, j][None, :]).astype(np.float32)).astype(np.float32)
    if l2:
        acc = (np.float32(2.0) * acc - xnorm2_f32(X)[None, :]).astype(np.float32)
    return acc


def norms(A):
    return np.sqrt((np.asarray(A, np.float64) ** 2).sum(axis=1))


# ---- thresholds ---------------------------------------------------------------------------------------------------------
def total_key(v):
    """f32::total_cmp as an unsigned key (-0 below +0, the kernels' `orderable`)."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def rank_largest(values, rank, short="smallest"):
    """The rank-th largest of `values` by total order, as f32.  Fewer values than the rank: the smallest of them
    (sample_tau_kernel's small-rank path, rank <= 16, and sample_tau_groups_kernel) or, short = "nan", a NaN
    (sample_tau_kernel's histogram path, rank > 16: nothing is nominated)."""
    v = np.ascontiguousarray(values, np.float32)
    order = np.argsort(total_key(v), kind="stable")[::-1]
    if rank > v.size:
        return np.float32(np.nan) if short == "nan" else v[order[-1]]
    return v[order[rank - 1]]


# ---- the margin ---------------------------------------------------------------------------------------------------------
def bf16_terms(l2, d, qn, xn):
    """(rounding, accumulation, flush) of the K2b / K2s margin.  Each operand carries a relative error <= UB, a product
    (1 + UB)^2 - 1 = 2 UB + UB^2, the sum by Cauchy-Schwarz that times |q| X (the L2 score holds 2 q.x: twice); the f32
    accumulation is priced at 8 d U times |q| X (dot) or (|q| + X)^2 (L2); flushed subnormals at 2^-120 sqrt(d) (|q| + X)."""
    rel = (1.0 + UB) ** 2 - 1.0
    flush = 2.0 ** -120 * math.sqrt(d) * (qn + xn)
    if l2:
        return 2.0 * rel * qn * xn, 8.0 * d * U * (qn + xn) ** 2, flush
    return rel * qn * xn, 8.0 * d * U * qn * xn, flush


def eps(l2, bf16, d, qn, xn):
    if bf16:
        return sum(bf16_terms(l2, d, qn, xn))
    return 3.5 * d * U * (qn + xn) ** 2 if l2 else 2.5 * d * U * qn * xn


# ---- input classes ------------------------------------------------------------------------------------------------------
CLASSES = ("gaussian", "positive", "large", "small", "subnormal", "equal")


def make_class(name, seed, n, nq, ld, d=None):
    """X [n][ld] and Q [nq][ld] of a class, columns >= d zero (d defaults to ld)."""
    d = ld if d is None else d
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    if name == "positive":      # no cancellation: the sums grow to their full length
        X, Q = np.abs(X), np.abs(Q)
    elif name == "large":       # inside the 1e18 guard: products of 1e30, squared norms of 1e30 d
        X, Q = X * np.float32(1e15), Q * np.float32(1e15)
    elif name == "small":       # products of 1e-40: below f32's normal range
        X, Q = X * np.float32(1e-20), Q * np.float32(1e-20)
    elif name == "subnormal":   # a fifth of the elements subnormal (1e-45 .. 1e-38), in rows and queries
        for A in (X, Q):
            m = rng.random(A.shape) < 0.2
            A[m] = (rng.uniform(-1.0, 1.0, A.shape) * 1e-38).astype(np.float32)[m]
    elif name == "equal":       # every third row is one of the queries
        for r in range(0, n, 3):
            X[r] = Q[(r // 3) % nq]
    else:
        assert name == "gaussian", name
    Xp, Qp = np.zeros((n, ld), np.float32), np.zeros((nq, ld), np.float32)
    Xp[:, :d], Qp[:, :d] = X, Q
    return Xp, Qp
