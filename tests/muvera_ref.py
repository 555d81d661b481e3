"""A restatement of the reference's MUVERA encoder (native/vettore/src/muvera.rs:26-225) in numpy, for the tests.

Every rule that decides a bit is spelled out:
  * hash4 is uint64 arithmetic that wraps (numpy arrays of uint64 wrap silently);
  * random_weight goes u64 -> f64 (round to nearest even), / 2^64 (u64::MAX as f64 is 2^64), -> f32, then
    `* 2 - 1` in f32 -- two f32 roundings;
  * every f64 dot product is summed sequentially over the dimension index from 0.0 (np.cumsum over float64,
    never np.sum, whose pairwise order differs), each term the exact f64 product of two f32 values;
  * accumulate rounds to f32 (np.float32) after every vector, in input order;
  * the count sketch walks the input indices in order and rounds to f32 at every step.

encode() returns ("ok", float32 array) or ("error", the reference's string).
"""
import functools

import numpy as np

MAX_OUTPUT_DIMENSIONS = 16_777_216
USIZE_MAX = (1 << 64) - 1
F32_MAX = np.float64(np.finfo(np.float32).max)
QUERY, DOCUMENT = 0, 1
_M64 = (1 << 64) - 1


def _u64(v):
    return np.atleast_1d(np.asarray(v, dtype=np.uint64))


def _rotl(x, s):
    return (x << np.uint64(s)) | (x >> np.uint64(64 - s))


def hash4(a, b, c, d):
    """muvera.rs:219-225 on broadcastable uint64 arrays."""
    a, b, c, d = _u64(a), _u64(b), _u64(c), _u64(d)
    x = a ^ _rotl(b, 17) ^ _rotl(c, 31) ^ _rotl(d, 47)
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def hash4_int(a, b, c, d):
    """The same on Python integers (an independent spelling: the two must agree)."""
    rot = lambda v, s: ((v << s) | (v >> (64 - s))) & _M64
    x = a ^ rot(b, 17) ^ rot(c, 31) ^ rot(d, 47)
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def random_weight(seed, repetition, projection, dimension):
    """muvera.rs:203-207."""
    h = hash4(seed, repetition, projection, dimension)
    unit = (h.astype(np.float64) / np.float64(2.0 ** 64)).astype(np.float32)
    return unit * np.float32(2.0) - np.float32(1.0)


def random_sign(seed, repetition, projection, dimension):
    """muvera.rs:210-216."""
    h = hash4(seed, repetition, projection, dimension)
    return np.where((h & np.uint64(1)) == 0, np.float32(1.0), np.float32(-1.0)).astype(np.float32)


@functools.lru_cache(maxsize=64)
def _tables(seed, d, R, k, pd):
    """weights [R][k][d] and signs [R][pd][d] (None when the projection is the identity)."""
    r = np.arange(R, dtype=np.uint64)[:, None, None]
    j = np.arange(d, dtype=np.uint64)[None, None, :]
    w = random_weight(seed, r, np.arange(k, dtype=np.uint64)[None, :, None], j) if k else np.zeros((R, 0, d), np.float32)
    s = None
    if pd != d:
        s = random_sign((seed + 17) & _M64, r, np.arange(pd, dtype=np.uint64)[None, :, None], j)
    return w, s


def _seq_dot(x, t):
    """x [n][d] f32, t [R][c][d] f32 -> [n][R][c] f64: 0.0 + x0*t0 + x1*t1 + ... in that order."""
    prod = x.astype(np.float64)[:, None, None, :] * t.astype(np.float64)[None, :, :, :]   # exact
    zero = np.zeros(prod.shape[:-1] + (1,), np.float64)
    return np.cumsum(np.concatenate([zero, prod], axis=-1), axis=-1)[..., -1]


def validate(vectors, dimension, num_repetitions, num_simhash_projections, projection_dimension, final):
    """muvera.rs:76-106 -> the error string or None."""
    if len(vectors) == 0:
        return "empty vectors"
    if dimension == 0:
        return "dimension must be positive"
    if num_repetitions == 0:
        return "num_repetitions must be positive"
    if num_simhash_projections >= 31:
        return "num_simhash_projections must be < 31"
    if projection_dimension == 0:
        return "projection_dimension must be positive"
    if final == 0:
        return "final_projection_dimension must be positive"
    if any(len(v) != dimension for v in vectors):
        return "dimension mismatch"
    for v in vectors:
        if not np.all(np.isfinite(np.asarray(v, dtype=np.float32))):
            return "vector contains a non-finite value"
    return None


def sizes(num_repetitions, num_simhash_projections, projection_dimension, final):
    """muvera.rs:29-42 -> (output_size, final_size) or the error string."""
    partitions = 1 << num_simhash_projections
    repetition_size = partitions * projection_dimension
    if repetition_size > USIZE_MAX:
        return "fde dimension overflow"
    output_size = num_repetitions * repetition_size
    if output_size > USIZE_MAX:
        return "fde dimension overflow"
    final_size = output_size if final is None else final
    if output_size > MAX_OUTPUT_DIMENSIONS or final_size > MAX_OUTPUT_DIMENSIONS:
        return "fde dimension exceeds safety limit"
    return output_size, final_size


def fde_dimension(num_repetitions, num_simhash_projections, projection_dimension, final):
    """The length of an encoding, 0 when the configuration is refused."""
    if num_repetitions == 0 or num_simhash_projections >= 31 or projection_dimension == 0 or final == 0:
        return 0
    s = sizes(num_repetitions, num_simhash_projections, projection_dimension, final)
    return 0 if isinstance(s, str) else s[1]


def _in_f32_range(next64):
    return np.isfinite(next64) & (next64 >= -F32_MAX) & (next64 <= F32_MAX)


def count_sketch(full, final, seed):
    """muvera.rs:180-200."""
    if final == 0:
        return ("error", "final_projection_dimension must be positive")
    n = full.size
    idx = np.arange(n, dtype=np.uint64)
    slot = (hash4(seed, 0x9E3779B97F4A7C15, idx, 0) % np.uint64(final)).astype(np.int64)
    neg = (hash4(seed, 0xD1B54A32D192ED03, idx, slot.astype(np.uint64)) & np.uint64(1)) != 0
    signed = np.where(neg, -full, full).astype(np.float32)      # sign * value in f32: exact
    out = np.zeros(final, dtype=np.float32)
    for i in range(n):                                           # sequential over the input index
        nxt = np.float64(out[slot[i]]) + np.float64(signed[i])
        if not _in_f32_range(nxt):
            return ("error", "encoding overflow")
        out[slot[i]] = np.float32(nxt)
    return ("ok", out)


def encode(vectors, dimension, num_repetitions, num_simhash_projections, seed, projection_dimension, final, mode):
    """muvera.rs:26-74.  `final` is None or an integer; mode QUERY or DOCUMENT."""
    err = validate(vectors, dimension, num_repetitions, num_simhash_projections, projection_dimension, final)
    if err:
        return ("error", err)
    s = sizes(num_repetitions, num_simhash_projections, projection_dimension, final)
    if isinstance(s, str):
        return ("error", s)
    output_size, _ = s
    d, R, k, pd = dimension, num_repetitions, num_simhash_projections, projection_dimension
    partitions = 1 << k
    x = np.asarray(vectors, dtype=np.float32).reshape(len(vectors), d)
    w, sg = _tables(seed, d, R, k, pd)
    # partition_index (muvera.rs:109-129): the earlier projection is the more significant bit
    part = np.zeros((len(x), R), dtype=np.int64)
    if k:
        bits = _seq_dot(x, w) >= 0.0                                       # [n][R][k]
        for p in range(k):
            part = (part << 1) + bits[:, :, p]
    # add_projected (muvera.rs:132-162)
    proj = np.broadcast_to(x.astype(np.float64)[:, None, :], (len(x), R, d)) if pd == d else _seq_dot(x, sg)
    out = np.zeros((R, partitions, pd), dtype=np.float32)
    counts = np.zeros((R, partitions), dtype=np.int64)
    for r in range(R):
        for v in range(len(x)):                                            # sequential over the set's vectors
            p = part[v, r]
            counts[r, p] += 1
            current = out[r, p].astype(np.float64)
            if mode == QUERY:
                nxt = current + proj[v, r]
            else:
                nxt = current + (proj[v, r] - current) / np.float64(counts[r, p])
            if not np.all(_in_f32_range(nxt)):
                return ("error", "encoding overflow")
            out[r, p] = nxt.astype(np.float32)
    full = out.reshape(output_size)
    return ("ok", full) if final is None else count_sketch(full, final, seed)


def encode_query(vectors, dimension, num_repetitions, num_simhash_projections, seed, projection_dimension, final):
    return encode(vectors, dimension, num_repetitions, num_simhash_projections, seed, projection_dimension, final, QUERY)


def encode_document(vectors, dimension, num_repetitions, num_simhash_projections, seed, projection_dimension, final):
    return encode(vectors, dimension, num_repetitions, num_simhash_projections, seed, projection_dimension, final, DOCUMENT)
