"""What the CPU model test and the GPU tests of K1qm share: the end-to-end corpora and queries, the host's
planner and grid restated, and a batch's outcome per query through the numpy model of the int8 sketch (sketch8_ref.py for
the dot family, sketch8_l2_ref.py for the L2 family)."""
import numpy as np

import sketch6_ref as ref6
import sketch8_l2_ref as refl
import sketch8_ref as ref8

L2, L2SQ, COS, IP, NIP = 0, 1, 2, 3, 4
METRICS = (COS, IP, NIP, L2, L2SQ)
DOT = (COS, IP, NIP)
NQS = (2, 3, 8, 9, 17)
LIMITS = (1, 10, 32)
CORPORA = ("uniform", "ties")   # 8 000 x 96; 20 000 x 128 with a block of 16 identical rows
MAX_GROUP, WAVE_BUF, WAVES, LDS_HALF, LDS_STATIC = 8, 2048, 4, 80 * 1024, 1024


def case(which, metric):
    """(rows, ids, 17 queries): unit rows and queries for the cosine metric, uniform ones otherwise; the first query sits on
    the block of identical rows, the second is a stored row."""
    n, d, tie = {"uniform": (8000, 96, 0), "ties": (20000, 128, 16)}[which]
    x, ids = refl.corpus(n, d, 8100 + 7 * metric + d, tie_block=tie)
    if metric == COS:
        x = refl.unit(x)
    qs = refl.queries(8200 + metric + d, x, max(NQS))
    if metric == COS:
        qs = refl.unit(qs)
    return x, ids, qs


def spiky_case(metric):
    """Every row carries +-400 in coordinate 7 and the queries nothing there: the int8 step is set by the spike, every
    other coordinate rounds to zero, so every row gets the same wide interval around a sum of zero, every slot of every
    list is a candidate, and no tail block certifies."""
    n, d = 8000, 96
    rng = np.random.default_rng(8300 + metric)
    x, ids = refl.corpus(n, d, 8301 + metric)
    x[:, 7] = rng.choice([-400.0, 400.0], n).astype(np.float32)
    qs = rng.uniform(-1, 1, (8, d)).astype(np.float32)
    qs[:, 7] = 0.0
    return x, ids, qs


# ---- the host side restated (host/vt_sketchbatch.h, host/vt_sketchsearch.h) --------------------------------------------------
def list_k(limit):
    return max(2 * limit, limit + 16)


def ld8_of(d):
    return (d + 127) // 128 * 128


def lds_bytes(d, kp, group):
    b = group * 2 * ld8_of(d) + group * WAVES * WAVE_BUF
    return b if kp <= 64 and b + LDS_STATIC <= LDS_HALF else 0


def max_group(d, kp):
    for g in (8, 4, 2):
        if lds_bytes(d, kp, g):
            return g
    return 0


def compiled_group(ng):
    return 2 if ng <= 2 else 4 if ng <= 4 else 8


def plan(nq, gmax):
    if gmax < 2:
        return []
    while nq >= 2:
        groups = (nq + gmax - 1) // gmax
        if nq // groups >= 2:
            return [nq // groups + (1 if g < nq % groups else 0) for g in range(groups)]
        nq -= 1
    return []


def group_blocks(d, kp, ng, cus=256):
    """The grid sketch_group_search launches a group of ng on: as many blocks a CU as its LDS holds, four at the most."""
    per_cu = min(4, (160 * 1024) // (lds_bytes(d, kp, compiled_group(ng)) + LDS_STATIC))
    return cus * max(1, per_cu)


# ---- the model -------------------------------------------------------------------------------------------------------------
class Column:
    """The int8 column of a corpus as the builders write it (with xx for the L2 family)."""

    def __init__(self, metric, x):
        self.metric = metric
        self.d = x.shape[1]
        if metric in DOT:
            self.X, self.s, self.rho, self.nu = ref8.quantise_rows(x)[:4]
            self.xx = None
        else:
            self.X, self.s, self.rho, self.nu, self.xx = refl.quantise_rows(x)

    def words(self, q):
        """(key(hi) word, key(lo) word) per row for one query, as the pass -- lone or group -- leaves them."""
        qy = refl.Query(q)
        if self.metric in DOT:
            kerr = 8.0 * self.d * 2.0 ** -24
            return ref8.pass_words(self.metric, self.X, self.s, self.rho, self.nu, qy.Q, qy.t, qy.qn, qy.eta, kerr)
        return refl.pass_words(self.metric, self.X, self.s, self.rho, self.nu, self.xx, qy)


def outcome(col, q, k, blocks, rank=None):
    """The tail block's outcome for one query of a group whose pass ran on `blocks` blocks: 1 rescored, 2 a candidate list
    too long for the block, 0 not certified."""
    first, second = col.words(q)
    kp = list_k(k)
    rank = np.arange(len(first)) if rank is None else rank
    lo, hi, rows = refl.block_lists(first, second, rank, blocks, kp)
    return refl.tail_outcome(refl.certify(lo, hi, rows, blocks, kp, k), blocks, kp, col.d)
