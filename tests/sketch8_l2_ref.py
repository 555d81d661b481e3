"""numpy restatement of the int8 sketch's L2 family (K1q over an L2 / squared-L2 handle: vettore_amd/csrc/vt_sketch.hip
sketch_row<true>, the L2 epilogue of sketch_scan_kernel, sketch_tail_kernel's certification; host/vt_sketchsearch.h sketch_search;
DESIGN.md 4.10, DESIGN_APPENDIX A.5b): the column with xx_r in the metadata run's fourth dword, the two words every row gets,
the tail's certificate over the block lists, and the corpora the CPU model test and the GPU tests share.
Everything the dot family has already is sketch8_ref's / sketch6_ref's.
Test infrastructure for tests/test_sketch8_l2_model.py, tests/test_gpu_sketch_l2_kernels.py and tests/test_gpu_sketch_l2.py;
nothing of the library is loaded."""
import numpy as np

import sketch6_ref as ref6
import sketch8_ref as ref8

M_L2, M_L2SQ = 0, 1
TILE_ROWS = ref8.TILE_ROWS
EMPTY = np.uint32(0xFFFFFFFF)
KAPPA_BITS = -23   # kappa = (d + 16) 2^-23
CAND_CAP = 4096    # host/vt_sketchtiers.h, the int8 tier's cand_cap
FUSE_MAX = 256     # vt_sketch.hip kTailFuseMax


# ---- the column ------------------------------------------------------------------------------------------------------------
def row_xx(x):
    """xx_r: f32, rounded up, of (sum of x_ri^2 in f64) (1 + 2^-30)."""
    x = np.ascontiguousarray(x, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return ref6.f32_up_v((x * x).sum(axis=1) * ref6.UP)


def quantise_rows(x):
    """sketch8_ref.quantise_rows and xx beside it."""
    X, s, rho, nu = ref8.quantise_rows(x)
    return X, s, rho, nu, row_xx(x)


def pack_tiles(X, s, rho, nu, xx=None):
    """sketch8_ref.pack_tiles; with xx the metadata run holds {s, rho, nu, xx} per row, without it the fourth dword is zero."""
    img = ref8.pack_tiles(X, s, rho, nu)
    if xx is not None:
        n, d = X.shape
        nch = ref8.chunks_of(d)
        tiles = img.shape[0]
        meta = np.ascontiguousarray(img[:, nch]).view(np.uint32).reshape(tiles * TILE_ROWS, 4)
        meta[:n, 3] = np.ascontiguousarray(xx, np.float32).view(np.uint32)
        img[:, nch] = meta.view(np.uint8).reshape(tiles, TILE_ROWS, 16)
    return img


def unpack_tiles(img, n, d):
    """X, s, rho, nu and the fourth dword (as float32) back out of the image."""
    X, s, rho, nu = ref8.unpack_tiles(img, n, d)
    nch = ref8.chunks_of(d)
    meta = np.ascontiguousarray(img[:, nch]).view(np.uint32).reshape(img.shape[0] * TILE_ROWS, 4)
    return X, s, rho, nu, meta[:n, 3].copy().view(np.float32)


# ---- the query side, as sketch_search forms it -----------------------------------------------------------------------------
class Query:
    """The query as the pass takes it: two int8 levels and their scales (sketch8_ref.query_levels), qn and eta rounded up,
    ||q||^2 summed in f64 element by element as the host does and widened by `up` both ways; kerr = 0 for this family."""

    def __init__(self, q):
        self.q = np.ascontiguousarray(q, np.float32)
        self.Q, self.t, eta_v = ref8.query_levels(self.q)
        qq = 0.0
        for v in self.q.astype(np.float64):
            qq += float(v) * float(v)
        self.qq = qq
        self.qq_lo, self.qq_hi = qq / ref6.UP, qq * ref6.UP
        self.qn = float(np.sqrt(np.float64(qq))) * ref6.UP
        self.eta = float(np.sqrt((eta_v ** 2).sum())) * ref6.UP
        self.kerr = 0.0
        self.image = ref8.query_image(self.Q, len(self.q))


def declines(qn, max_norm):
    """sketch_search's guard: a squared difference of K1's could overflow f32 -- the plain scan decides."""
    return not ((qn + max_norm) * ref6.UP < 2.0 ** 62)


def max_norm_of(rho, nu):
    return float(((rho.astype(np.float64) + nu.astype(np.float64)) * ref6.SLACK).max())


# ---- the pass's epilogue, operation by operation ---------------------------------------------------------------------------
def l2_words(metric, d, av, e, xx, qq_lo, qq_hi):
    """(orderable kmin_r word -- the high half of the list's key --, orderable kmax_r word -- the payload's --) from a_r, e_r
    and xx_r, in the kernel's order of operations."""
    av, e = np.asarray(av, np.float64), np.asarray(e, np.float64)
    xxu = np.asarray(xx, np.float32).astype(np.float64)
    xxl = xxu * (1.0 - 2.0 ** -22)
    kappa = (np.float64(d) + 16.0) * 2.0 ** KAPPA_BITS
    tiny = (np.float64(d) + 16.0) * 2.0 ** -125
    delta = 2.0 ** -40 * (np.float64(qq_hi) + xxu + 2.0 * e)
    v_lo = np.maximum(0.0, np.float64(qq_lo) + xxl - 2.0 * (av + e) - delta)
    v_hi = np.float64(qq_hi) + xxu - 2.0 * (av - e) + delta
    kmin = ref6.f32_down_v(v_lo * (1.0 - kappa) - tiny)
    kmin = np.where(kmin > 0, kmin, np.float32(0.0)).astype(np.float32)
    kmax = ref6.f32_up_v(v_hi * (1.0 + kappa) + tiny)
    if metric == M_L2:
        kmin, kmax = np.sqrt(kmin), np.sqrt(kmax)  # (float32 in, float32 out: correctly rounded, as K1's root is)
    return ref6.orderable(kmin), ref6.orderable(kmax)


def pass_words(metric, X, s, rho, nu, xx, qy):
    """sketch_scan_kernel<., true>'s two words per row, bit for bit: a_r and e_r as the dot family's pass has them with
    kerr = 0 (sketch8_ref.pass_words' first half), then l2_words."""
    f = np.asarray(X, np.int64) @ np.asarray(qy.Q, np.int64).T
    t = np.asarray(qy.t, np.float32).astype(np.float64)
    av = np.asarray(s, np.float32).astype(np.float64) * (t[0] * f[:, 0].astype(np.float64) + t[1] * f[:, 1].astype(np.float64))
    e = ref6.pass_error(X.shape[1], s, rho, nu, qy.qn, qy.eta, qy.kerr)
    return l2_words(metric, X.shape[1], av, e, xx, qy.qq_lo, qy.qq_hi)


def words_for(metric, x, q):
    """Both words of every row of x for the query q, through the whole model: quantiser, column, levels, epilogue."""
    X, s, rho, nu, xx = quantise_rows(x)
    return pass_words(metric, X, s, rho, nu, xx, Query(q))


# ---- the block lists and the tail's certificate ----------------------------------------------------------------------------
def owner_blocks(n, blocks):
    """The block whose list a row goes to: 4 waves a block numbered block by block, tile t to wave t mod waves."""
    tile = np.arange(n) // TILE_ROWS
    return (tile % (4 * blocks)) // 4


def block_lists(first, second, rank, blocks, kp):
    """What launch_sketch_scan leaves: per block the kp smallest (first word << 32 | id rank) keys of the rows it owns.
    Returns lo [blocks * kp] (the kmax / key(lo) words, EMPTY where a slot is empty), hi (the kmin / key(hi) words) and rows."""
    n = len(first)
    key = (first.astype(np.uint64) << np.uint64(32)) | np.asarray(rank, np.uint64)
    owner = owner_blocks(n, blocks)
    lo = np.full((blocks, kp), EMPTY, np.uint32)
    hi = np.full((blocks, kp), EMPTY, np.uint32)
    rows = np.zeros((blocks, kp), np.uint32)
    order = np.lexsort((key, owner))
    start = np.searchsorted(owner[order], np.arange(blocks))
    end = np.searchsorted(owner[order], np.arange(blocks), side="right")
    for b in range(blocks):
        keep = order[start[b]:min(end[b], start[b] + kp)]
        lo[b, :len(keep)] = second[keep]
        hi[b, :len(keep)] = first[keep]
        rows[b, :len(keep)] = keep
    return lo.reshape(-1), hi.reshape(-1), rows.reshape(-1)


def certify(lo, hi, rows, lists, kp, k, cap=CAND_CAP):
    """sketch_tail_kernel's certificate: Kt = the k-th smallest live kmax word (0xffffffff when at most k are
    live); a live slot is a candidate iff its kmin word is <= Kt; a list of candidates alone, or more than `cap`, refuses."""
    live = hi != EMPTY
    kt = int(np.sort(lo[live])[k - 1]) if live.sum() > k else 0xFFFFFFFF
    cand = live & (hi <= np.uint32(kt))
    fail = bool(cand.reshape(lists, kp).all(axis=1).any())
    cnt = int(cand.sum())
    return dict(kt=kt, cnt=cnt, ok=not fail and cnt <= cap, rows=np.sort(rows[cand]))


def padded_dim(d):
    return (d + 63) // 64 * 64


def tail_lds_words(lists, kp, d):
    """sketch_tail_lds_bytes / 4."""
    want = max(lists * kp, (lists + 4) + 64 * (padded_dim(d) // 8 + 12)) * 4
    return max(min(want, 128 * 1024), (lists + 4) * 4) // 4


def tail_outcome(cert, lists, kp, d):
    """info[0]: 0 not certified, 1 rescored by the tail's own block, 2 the candidates are left for the gathered K1."""
    if not cert["ok"]:
        return 0
    ss = padded_dim(d) // 8 + 12
    lists4 = (lists + 3) & ~3
    return 1 if cert["cnt"] <= FUSE_MAX and lists4 + cert["cnt"] * ss <= tail_lds_words(lists, kp, d) else 2


def list_k(limit):
    """host/vt_sketchtiers.h sketch_list_k."""
    return max(2 * limit, limit + 16)


def search_certifies(metric, x, rank, q, k, cus=256):
    """A whole lone search through the model on a card of `cus` compute units: the pass's lists, then the certificate."""
    kp = list_k(k)
    blocks = cus * (4 if kp <= 64 else 2)
    first, second = words_for(metric, x, q)
    lo, hi, rows = block_lists(first, second, rank, blocks, kp)
    return certify(lo, hi, rows, blocks, kp, k)


# ---- corpora the model test and the GPU tests share --------------------------------------------------------------------------
def unit(x):
    x = np.asarray(x, np.float32)
    nrm = np.sqrt((x.astype(np.float64) ** 2).sum(axis=-1, keepdims=True))
    return (x / np.where(nrm > 0, nrm, 1.0)).astype(np.float32)


def adversarial(d, q, seed, n_each=24):
    """The rows the bound must survive, by name: uniform, unit, norms over 10^-3 .. 10^3, a zero row, the query itself,
    near-copies of the query at relative distance 10^-7 .. 10^-3 (where q.q + x.x - 2 q.x cancels), 48 identical rows, rows
    with one spike (a large rho)."""
    rng = np.random.default_rng(seed)
    q = np.asarray(q, np.float32)
    uni = rng.uniform(-1, 1, (n_each, d)).astype(np.float32)
    out = {"uniform": uni, "unit": unit(rng.uniform(-1, 1, (n_each, d)))}
    out["norms"] = (rng.uniform(-1, 1, (n_each, d)) * 10.0 ** rng.uniform(-3, 3, (n_each, 1))).astype(np.float32)
    out["zero"] = np.zeros((1, d), np.float32)
    out["query"] = q[None].copy()
    rel = 10.0 ** rng.uniform(-7, -3, (n_each, 1))
    qs = np.abs(q).max() if np.abs(q).max() > 0 else 1.0
    out["near"] = (q.astype(np.float64) + rel * qs * rng.uniform(-1, 1, (n_each, d))).astype(np.float32)
    out["ties"] = np.repeat(rng.uniform(-1, 1, (1, d)).astype(np.float32), 48, axis=0)
    spike = rng.uniform(-1, 1, (n_each, d)).astype(np.float32)
    spike[np.arange(n_each), rng.integers(0, d, n_each)] *= np.float32(1e3)
    out["spike"] = spike
    return out


def corpus(n, d, seed, tie_block=0, dup_frac=0.01):
    """iid uniform(-1, 1) rows, 1 % verbatim duplicates, a block of identical rows in the middle; ids in ascending byte order
    (the rank column stays strictly current: the pass never serves a lazily ranked shard)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=(n, d)).astype(np.float32)
    ndup = int(n * dup_frac)
    if ndup:
        src, dst = rng.integers(0, n, ndup), rng.integers(0, n, ndup)
        x[dst] = x[src]
    if tie_block:
        x[n // 2:n // 2 + tie_block] = x[n // 2]
    return x, [b"doc-%08d" % i for i in range(n)]


def queries(seed, x, nq):
    """nq uniform queries; the first sits on the block of identical rows, the second is a stored row too."""
    rng = np.random.default_rng(seed)
    qs = rng.uniform(-1, 1, size=(nq, x.shape[1])).astype(np.float32)
    qs[0] = x[len(x) // 2]
    qs[1] = x[3]
    return qs


E2E_SHAPES = ((192, 30000), (100, 9000))
E2E_QUERIES = 12


def e2e_case(metric, k, d, n):
    """The end-to-end GPU test's corpus and queries for one (metric, k, shape): the model test certifies the same ones."""
    x, ids = corpus(n, d, 7300 + metric + d, tie_block=48)
    return x, ids, queries(k + d, x, E2E_QUERIES)


def spread_corpus(n, d, seed):
    """Norms spread over 10^-2 .. 10^2, 200 spiky rows, 50 zero rows, and near-copies of what will be the queries."""
    rng = np.random.default_rng(seed)
    x, ids = corpus(n, d, seed + 1, tie_block=30)
    x = (x * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)
    spiky = rng.integers(0, n, 200)
    x[spiky, rng.integers(0, d, 200)] = (rng.choice([-1, 1], 200) * rng.uniform(50, 400, 200)).astype(np.float32)
    x[rng.integers(0, n, 50)] = 0.0
    qs = queries(seed + 2, x, 8)
    qs[2] = x[spiky[0]]
    qs[3] = 0.0
    qs[3, 5] = 1.0
    for j, qi in enumerate((4, 5, 6)):  # near-copies of three queries at relative distance 10^-7 .. 10^-3
        at = rng.integers(0, n, 6)
        rel = 10.0 ** rng.uniform(-7, -3, (6, 1))
        x[at] = (qs[qi].astype(np.float64) * (1.0 + rel * rng.uniform(-1, 1, (6, d)))).astype(np.float32)
    return x, ids, qs
