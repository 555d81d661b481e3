"""The inputs of tests/test_gpu_select_kernels.py, built without a GPU so that tests/test_select_model.py can show on the CPU
that they enter every branch of select_topk_kernel (csrc/vt_select.hip) they are meant to enter.

A Case is one launch: `form` names the launcher, `keys` is the list (1-D) or the lists (2-D, one per query), `k` the limit,
`lo` the has_lo key or None, `m_dev` the device-side length(s) or None.  block_inputs(case) yields what each block of
select_topk_kernel sees of it.  Every family is seed-fixed.

Key families:
  random      64-bit keys, distinct in practice
  dups        keys from a range a third of the list's length: equal keys everywhere, some straddle every threshold
  product     what a search makes: orderable f32 of a normal score << 32 | a permutation rank below 2^24
  crowded     three high words over distinct low ranks, 70 % of the keys under the smallest word: above 4096 keys share
              the first digit, and the walk goes on over the global keys
  bits        keys that differ in bit 63 and bit 0 only: the second digit is cut 56 bits below the first
  ladder      four two-bit steps 16 bits apart over ten low bits: every digit starts at a far varying bit and leaves a
              quarter of the keys, so the LDS list is walked three times and more
  equal       one value
  straggler   the suspected defect: many equal keys E and one smaller key at the END of the list (past position 1024, so that
              its thread reaches it after every thread has filed a first key), in three places of the walk --
                first    S = 0x100, E = 0x200: the first digit exhausts the varying bits
                cand     Z = 0x000200 once, F = 0x100100 last, E = 0x100200: exhausted on the LDS list
                crowded  the same with more than 4096 E: exhausted on the global keys
              each with the constant low bits not all ones (as written) and all ones (| 0xFF), where the bin's top IS the key
  whole_bin   exactly k keys under the smallest top byte: the first bin's count is what remains to select
  bin_top     winners equal to the top of their bin (low bits all ones) on the LDS path
  holes       kEmptyKey in a share of the places, up to all of them
"""
import functools

import numpy as np

from select_ref import EMPTY, expected_topk

MAX_FUSED_K = 256        # vt_device.h kMaxFusedK
SEL_LIST_MAX = 4096      # kSelListMax
TWO_LEVEL_MIN = 16384    # kSelTwoLevelMin
SEL_GROUPS = 16          # kSelGroups
SPREAD_KEYS = 2048       # vt_select.hip kSpreadKeys (file-local there)
U64 = np.uint64


def _rng(seed):
    return np.random.default_rng(seed)


def random_keys(m, seed):
    return _rng(seed).integers(0, 2 ** 64 - 1, size=m, dtype=np.uint64)


def dups(m, seed):
    return _rng(seed).integers(0, max(2, m // 3), size=m, dtype=np.uint64) + U64(0x3F80000000000000)


def orderable(f):
    u = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & U64(0x80000000), ~u & U64(0xFFFFFFFF), u | U64(0x80000000)).astype(np.uint64)


def product(m, seed):
    r = _rng(seed)
    return (orderable(r.standard_normal(m)) << U64(32)) | r.permutation(m).astype(np.uint64)


def crowded(m, seed):
    r = _rng(seed)
    words = np.array([0x40000100, 0x40000200, 0x40000300], np.uint64)
    pick = r.choice(3, size=m, p=[0.7, 0.15, 0.15])
    return (words[pick] << U64(32)) | r.permutation(m).astype(np.uint64)


def bits(m, seed):
    vals = np.array([0, 1, 1 << 63, (1 << 63) | 1], np.uint64) | U64(0x00F0F0F0F0F0F0F0)
    return vals[_rng(seed).integers(0, 4, size=m)]


def ladder(m, seed):
    r = _rng(seed)
    steps = [r.integers(0, 4, size=m, dtype=np.uint64) << U64(sh) for sh in (48, 32, 16)]
    return steps[0] | steps[1] | steps[2] | r.integers(0, 1024, size=m, dtype=np.uint64) | U64(0x1100110011000000)


def equal(m):
    return np.full(m, 0x0123456789ABCDEF, np.uint64)


def straggler(m, where, ones):
    low = 0xFF if ones else 0
    if where == "first":
        keys = np.full(m, 0x200 | low, np.uint64)
        keys[m - 1] = 0x100 | low
    else:
        keys = np.full(m, 0x100200 | low, np.uint64)
        keys[5] = 0x000200 | low
        keys[m - 1] = 0x100100 | low
    return keys


def whole_bin(m, k, seed):
    r = _rng(seed)
    keys = r.integers(0, 2 ** 56, size=m, dtype=np.uint64) | (r.integers(1, 255, size=m, dtype=np.uint64) << U64(56))
    keys[r.permutation(m)[:k]] &= U64(2 ** 56 - 1)
    if m > k:
        keys[np.flatnonzero(keys >> U64(56))[0]] |= U64(0xF0 << 56)  # (bit 63 varies whatever was drawn)
    return keys


def bin_top(m, seed):
    r = _rng(seed)
    keys = r.integers(0x100, 0x10000, size=m, dtype=np.uint64)
    keys[r.permutation(m)[:7]] = np.array([0x10, 0x20, 0x30, 0xFF, 0xFF, 0xFF, 0xFF], np.uint64)
    return keys | U64(0x7700000000000000)


def holes(keys, share, seed):
    keys = keys.copy()
    keys[_rng(seed).random(keys.size) < share] = U64(EMPTY)
    return keys


def kth_key(keys, k):
    return expected_topk(keys, k)[-1][0]


class Case:
    def __init__(self, name, form, keys, k, lo=None, m_dev=None):
        self.name, self.form, self.k, self.lo, self.m_dev = name, form, k, lo, m_dev
        self.keys = np.ascontiguousarray(keys, np.uint64)

    def __repr__(self):
        return self.name

    def lengths(self):
        """The length the kernel takes for each list: min(m_dev, stride) where the device decides."""
        if self.keys.ndim == 1:
            return [self.keys.size if self.m_dev is None else min(int(self.m_dev), self.keys.size)]
        nq, m = self.keys.shape
        return [m] * nq if self.m_dev is None else [min(int(x), m) for x in self.m_dev]


def block_inputs(case):
    """(keys, k, lo, one_key_per_thread) for every block of select_topk_kernel the case's launch (without `spread`) runs.
    The second level of the two-level form sees what expected_topk leaves of each slice, padded with kEmptyKey."""
    if case.form == "two-level":
        m = case.keys.size
        slice_ = (m + SEL_GROUPS - 1) // SEL_GROUPS
        second = []
        for g in range(SEL_GROUPS):
            part = case.keys[g * slice_:(g + 1) * slice_]
            yield part, case.k, case.lo, False
            won = [key for key, _ in expected_topk(part, case.k, case.lo)]
            second += won + [EMPTY] * (case.k - len(won))
        yield np.array(second, np.uint64), case.k, None, True
        return
    lists = case.keys[None, :] if case.keys.ndim == 1 else case.keys
    for row, n in zip(lists, case.lengths()):
        yield row[:n], case.k, case.lo, case.form != "list"


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(*a, **kw):
        out.append(Case(*a, **kw))

    # ---- launch_select, one level: the one-key-per-thread path
    for m in (1, 63, 64, 65, 1023, 1024):
        for k in (1, 5, 70, 256):
            add("short-dups-m%d-k%d" % (m, k), "lone", holes(dups(m, 10 + m), 0.2 if m > 1 else 0.0, 20 + m), k)
    add("short-random-m1024-k70", "lone", random_keys(1024, 30), 70)
    add("short-product-m1023-k256", "lone", product(1023, 31), 256)
    add("short-all-empty-m65-k5", "lone", np.full(65, EMPTY, np.uint64), 5)
    # ---- one level: the radix path
    for m in (1025, 4097, 9001):
        for k in (1, 5, 70, 256) if m == 9001 else (5, 256):
            add("random-m%d-k%d" % (m, k), "lone", random_keys(m, 40 + m), k)
        add("product-m%d-k70" % m, "lone", product(m, 41 + m), 70)
        add("dups-m%d-k70" % m, "lone", dups(m, 42 + m), 70)
        for k in (5, 70):
            add("bits-m%d-k%d" % (m, k), "lone", bits(m, 43 + m), k)
            add("whole-bin-m%d-k%d" % (m, k), "lone", whole_bin(m, k, 44 + m), k)
        add("equal-m%d-k5" % m, "lone", equal(m), 5)
        add("ladder-m%d-k70" % m, "lone", ladder(m, 48 + m), 70)
        add("bin-top-m%d-k5" % m, "lone", bin_top(m, 45 + m), 5)
        add("holes-m%d-k70" % m, "lone", holes(random_keys(m, 46 + m), 0.3, 47 + m), 70)
        few = np.full(m, EMPTY, np.uint64)
        few[[3, m // 2, m - 1]] = [9, 7, 8]
        add("three-live-m%d-k5" % m, "lone", few, 5)
        add("all-empty-m%d-k5" % m, "lone", np.full(m, EMPTY, np.uint64), 5)
        for ones in (False, True):
            tag = "-ones" if ones else ""
            add("straggler-first%s-m%d-k3" % (tag, m), "lone", straggler(m, "first", ones), 3)
            add("straggler-%s%s-m%d-k3" % ("crowded" if m > 4097 else "cand", tag, m), "lone", straggler(m, "rest", ones), 3)
    add("crowded-m9001-k5", "lone", crowded(9001, 50), 5)
    add("crowded-m9001-k256", "lone", crowded(9001, 50), 256)
    keys = random_keys(4097, 51)
    add("lo-at-kth-m4097-k70", "lone", keys, 70, lo=kth_key(keys, 70))
    add("lo-above-all-m4097-k5", "lone", keys, 5, lo=int(keys.max()))
    add("lo-dups-m4097-k70", "lone", dups(4097, 52), 70, lo=kth_key(dups(4097, 52), 70))
    add("lo-short-m700-k5", "lone", dups(700, 53), 5, lo=kth_key(dups(700, 53), 5))
    for m_dev in (2000, 700, 0, 5000):
        add("m-dev-%d-m4097-k70" % m_dev, "lone", keys, 70, m_dev=m_dev)

    # ---- launch_select, two levels
    for m in (TWO_LEVEL_MIN, TWO_LEVEL_MIN + 37):
        slice_ = (m + SEL_GROUPS - 1) // SEL_GROUPS
        for k in (5, 256):
            tag = "-m%d-k%d" % (m, k)
            high = random_keys(m, 60 + k) | U64(1 << 63)
            one = high.copy()
            one[3 * slice_ + 7:3 * slice_ + 7 + k + 10] = random_keys(k + 10, 61) >> U64(1)
            add("winners-in-one-slice" + tag, "two-level", one, k)
            each = high.copy()
            each[np.arange(SEL_GROUPS) * slice_ + 11] = random_keys(SEL_GROUPS, 62) >> U64(1)
            add("a-winner-in-each-slice" + tag, "two-level", each, k)
            gaps = random_keys(m, 63 + k)
            gaps[4 * slice_:10 * slice_] = U64(EMPTY)
            gaps[15 * slice_:] = U64(EMPTY)
            add("empty-slices" + tag, "two-level", gaps, k)
            add("lo" + tag, "two-level", gaps, k, lo=kth_key(gaps, 20))
            add("dups" + tag, "two-level", holes(dups(m, 64 + k), 0.1, 65), k)
            add("whole-bin" + tag, "two-level", np.concatenate([whole_bin(slice_, k, 66), high[slice_:]]), k)
    m = TWO_LEVEL_MIN + 37  # (slices of 1027 keys: a slice's last keys lie past its position 1024)
    for ones in (False, True):
        for where in ("first", "rest"):
            keys = straggler(m, where, ones)
            part = straggler((m + SEL_GROUPS - 1) // SEL_GROUPS, where, ones)
            keys[:part.size] = part
            keys[m - 1] = keys[m - 2]  # (the last slice is shorter than 1024 keys: no late key there)
            add("straggler-%s%s-m%d-k3" % (where, "-ones" if ones else "", m), "two-level", keys, 3)

    # ---- launch_select_list
    for name, keys, k, m_dev in (("random", random_keys(6000, 70), 300, 6000), ("random-cut", random_keys(6000, 70), 300, 5000),
                                 ("crowded", crowded(6000, 71), 300, 6000), ("dups", holes(dups(6000, 72), 0.2, 73), 300, 6000),
                                 ("whole-bin", whole_bin(6000, 300, 74), 300, 6000), ("random", random_keys(6000, 75), 4096, 6000),
                                 ("dups", dups(6000, 76), 4096, 7000), ("random", random_keys(3000, 77), 4096, 3000),
                                 ("holes", holes(random_keys(3000, 78), 0.5, 79), 4096, 3000),
                                 ("straggler-first", straggler(6000, "first", False), 300, 6000),
                                 ("straggler-first-ones", straggler(6000, "first", True), 300, 6000),
                                 ("straggler-cand", straggler(6000, "rest", False), 300, 4000),
                                 ("straggler-cand-ones", straggler(6000, "rest", True), 300, 4000),
                                 ("straggler-crowded", straggler(6000, "rest", False), 300, 6000),
                                 ("straggler-crowded-ones", straggler(6000, "rest", True), 300, 6000)):
        if name.startswith("straggler-cand"):
            keys[3999] = keys[5999]  # (the smaller key at the end of what m_dev leaves)
        add("%s-m%d-k%d-mdev%d" % (name, keys.size, k, m_dev), "list", keys, k, m_dev=m_dev)

    # ---- launch_select_queries
    for k in (5, 70):
        add("queries-m700-k%d" % k, "queries", np.stack([holes(dups(700, 80), 0.2, 81), random_keys(700, 82), np.full(700, EMPTY, np.uint64)]), k)
        add("queries-m1500-k%d" % k, "queries", np.stack([random_keys(1500, 83), holes(dups(1500, 84), 0.2, 85), whole_bin(1500, k, 86)]), k)
    few = np.full(1500, EMPTY, np.uint64)
    few[[0, 1, 1499]] = [5, 5, 4]
    add("queries-m1500-k3-stragglers", "queries", np.stack([straggler(1500, "first", False), straggler(1500, "rest", False), few]), 3)
    add("queries-m1500-k3-stragglers-ones", "queries", np.stack([straggler(1500, "first", True), straggler(1500, "rest", True), bits(1500, 87)]), 3)

    # ---- launch_select_lists
    def lists(rows, stride):
        keys = np.full((len(rows), stride), 0x1111, np.uint64)  # (what lies past a list's length is live and small: it must not be read)
        for y, row in enumerate(rows):
            keys[y, :row.size] = row
        return keys

    lens = (0, 700, 2048, 2049, 5000)
    for k in (5, 70):
        rows = [holes(dups(min(n, 3000), 90 + n % 97), 0.2, 91) for n in lens]
        add("lists-stride3000-k%d" % k, "lists", lists(rows, 3000), k, m_dev=lens)
    lens = (3000, 2500, 2048, 1500, 1025, 2600)
    rows = [straggler(3000, "first", False), straggler(2500, "rest", False), dups(2048, 93) >> U64(4),
            np.full(1500, EMPTY, np.uint64), straggler(1025, "first", True), straggler(2600, "rest", True)]
    add("lists-stride3000-k3-stragglers", "lists", lists(rows, 3000), 3, m_dev=lens)
    lens = (1000, 300, 0, 1024)
    add("lists-stride1000-k5", "lists", lists([holes(dups(min(n, 1000), 94 + n), 0.2, 95) for n in lens], 1000), 5, m_dev=lens)
    return tuple(out)


def of_form(form):
    return [c for c in cases() if c.form == form]
