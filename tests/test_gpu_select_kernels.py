"""The selection kernels against a plain sort, launch by launch (csrc/vt_select.hip, K3).

Every search ends in K3, and the searches' own tests reach it only with keys a search makes: distinct, spread over many
digits.  Here its seven kernels are launched one at a time through tests/select_probe.cpp (libvt_select_probe.so: vt_select.o
and nothing else of the library) on hand-made keys (tests/select_cases.py; tests/test_select_model.py shows on the CPU which
branch each enters), and everything is read back and compared with select_ref.expected_topk, a sort:

  payloads    row is the key's position in the caller's array, raw a float made from it: a payload gathered from the wrong
              index shows;
  exact rule  where a kernel orders equal keys by position -- the one-key-per-thread path, the spread kernel, sort_list,
              merge_blocks -- entries are compared one by one, in order;
  radix rule  the radix path files equal keys in the atomics' order: the key sequence is exact, every (key, row, raw) is an
              input triple used once, every key strictly below the k-th is present, the count is exact;
  fill        entries at and past the count, the header's padding and all bytes outside the contract keep the probe's 0xA5.

test_suspected_defect_* name the case the kernel failed before its threshold for exhausted digits was the key itself: with
keys 0x200 (many) and 0x100 (once, last), k = 3, it returned three 0x200.
"""
import ctypes as C
import os

import numpy as np
import pytest

import select_cases as sc
from select_ref import EMPTY, expected_topk, kth_threshold

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
ENTRY = np.dtype([("key", "<u8"), ("row", "<u4"), ("raw", "<u4")])
HEADER = 16
FILL = 0xA5
FILL32 = 0xA5A5A5A5
FILL64 = 0xA5A5A5A5A5A5A5A5
NPOS = 1 << 15
ROWS = np.arange(NPOS, dtype=np.uint32)
RAW = (np.arange(NPOS) * 0.5 + 0.25).astype(np.float32).view(np.uint32)  # (exact in f32, distinct)


def ptr(a):
    return None if a is None else a.ctypes.data


class Probe:
    def __init__(self):
        # VT_SELECT_PROBE_LIB: another build of the same probe (a deliberately broken kernel, to see these tests fail)
        path = os.environ.get("VT_SELECT_PROBE_LIB") or os.path.join(ROOT, "vettore_amd", "lib", "libvt_select_probe.so")
        assert os.path.exists(path), "build it with `make` (%s)" % os.path.basename(path)
        L = self.lib = C.CDLL(path)
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        for name in ("max_fused_k", "sel_list_max", "sel_two_level_min", "sel_groups", "radix_bins", "result_block_bytes"):
            getattr(L, "vsp_" + name).restype = u32
            setattr(self, name, getattr(L, "vsp_" + name)())
        self.status_retry = L.vsp_status_retry()
        L.vsp_select.argtypes = [vp, vp, vp, u64, u32, u32, u64, i32, vp, i32, vp, vp, u64]
        L.vsp_select_list.argtypes = [vp, vp, vp, u64, u32, vp, u32, vp, vp, vp, u64]
        L.vsp_select_many.argtypes = [vp, vp, vp, u64, u32, u32, vp, i32, u32, vp, u64, u32]
        L.vsp_sort_list.argtypes = [vp, vp, vp, u64, u32, vp, vp, vp, u64]
        L.vsp_merge_blocks.argtypes = [vp, u64, u32, u32, u32, vp, u64, vp, u64]
        L.vsp_radix.argtypes = [vp, u32, u32, u32, i32, u32, u32, vp, i32, vp, vp, vp, u64, vp, vp, vp]

    @staticmethod
    def _list(keys, length=None):
        keys = np.ascontiguousarray(keys, np.uint64).reshape(-1)
        n = keys.size if length is None else length
        return keys, ROWS[:max(n, 1)].copy(), RAW[:max(n, 1)].copy(), n

    def select(self, keys, m, k, lo=None, m_dev=None, two_level=False, status=None, out_bytes=None, length=None, expect=0):
        """launch_select -> (the result block's bytes, the device's status word afterwards or None)."""
        keys, rows, raw, n = self._list(keys, length)
        out = np.zeros(self.result_block_bytes if out_bytes is None else out_bytes, np.uint8)
        md = None if m_dev is None else np.array([m_dev], np.uint32)
        st = None if status is None else np.array([status], np.int32)
        rc = self.lib.vsp_select(ptr(keys), ptr(rows), ptr(raw), n, m, k, int(lo or 0), int(lo is not None), ptr(md), int(two_level), ptr(st),
                                 ptr(out), out.size)
        assert rc == expect, "vsp_select: hipError_t %d" % rc
        return out, None if st is None else int(st[0])

    def select_list(self, keys, m, m_dev, k, out_len=None, length=None, expect=0):
        keys, rows, raw, n = self._list(keys, length)
        out_len = k + 16 if out_len is None else out_len
        ok, orow, oraw = np.zeros(out_len, np.uint64), np.zeros(out_len, np.uint32), np.zeros(out_len, np.uint32)
        md = None if m_dev is None else np.array([m_dev], np.uint32)
        rc = self.lib.vsp_select_list(ptr(keys), ptr(rows), ptr(raw), n, m, ptr(md), k, ptr(ok), ptr(orow), ptr(oraw), out_len)
        assert rc == expect, "vsp_select_list: hipError_t %d" % rc
        return ok, orow, oraw

    def select_many(self, keys, nq, m, k, out_stride, m_dev=None, spread=False, out_bytes=None, length=None, expect=0):
        keys, rows, raw, n = self._list(keys, length)
        out = np.zeros(nq * out_stride if out_bytes is None else out_bytes, np.uint8)
        md = None if m_dev is None else np.ascontiguousarray(m_dev, np.uint32)
        rc = self.lib.vsp_select_many(ptr(keys), ptr(rows), ptr(raw), n, nq, m, ptr(md), int(spread), k, ptr(out), out.size, out_stride)
        assert rc == expect, "vsp_select_many: hipError_t %d" % rc
        return out

    def sort_list(self, keys, m, status=0, out_entries=None, length=None, expect=0):
        keys, rows, raw, n = self._list(keys, length)
        st, head = np.array([status], np.int32), np.zeros(2, np.uint32)
        out = np.zeros((m if out_entries is None else out_entries) * 16 or 16, np.uint8)
        rc = self.lib.vsp_sort_list(ptr(keys), ptr(rows), ptr(raw), n, m, ptr(st), ptr(head), ptr(out), out.size // 16 if m else 0)
        assert rc == expect, "vsp_sort_list: hipError_t %d" % rc
        return head, out, int(st[0])

    def merge(self, blocks, world, k, block_bytes, shard_len=None, blocks_len=None):
        out = np.zeros(self.result_block_bytes, np.uint8)
        shard = np.zeros(k + 4 if shard_len is None else shard_len, np.uint32)
        rc = self.lib.vsp_merge_blocks(ptr(blocks), blocks.size if blocks_len is None else blocks_len, world, k, block_bytes, ptr(out), out.size,
                                       ptr(shard), shard.size)
        return rc, out, shard

    def radix(self, keys, k, passes, blocks, cap, pay=True, key_offset=0, only_pass=-1, list_len=None, expect=0):
        keys = np.ascontiguousarray(keys, np.uint64)
        list_len = cap + 5 if list_len is None else list_len
        lk, lrow, lraw = np.zeros(list_len, np.uint64), np.zeros(list_len, np.uint32), np.zeros(list_len, np.uint32)
        count, status = np.zeros(1, np.uint32), np.full(1, -1, np.int32)
        raw = RAW[:keys.size].copy() if pay else None
        rc = self.lib.vsp_radix(ptr(keys), keys.size, key_offset, k, passes, blocks, cap, ptr(raw), only_pass, ptr(lk), ptr(lrow), ptr(lraw),
                                list_len, ptr(count), ptr(status), None)
        assert rc == expect, "vsp_radix: hipError_t %d" % rc
        return lk, lrow, lraw, int(count[0]), int(status[0])


@pytest.fixture(scope="module")
def probe():
    return Probe()


def parse(block):
    """(status, count, every entry slot the bytes hold) of a result block."""
    raw = block.tobytes()
    head = np.frombuffer(raw[:8], np.int32)
    slots = (len(raw) - HEADER) // 16
    return int(head[0]), int(head[1].view(np.uint32)), np.frombuffer(raw[HEADER:HEADER + slots * 16], ENTRY)


def check_winners(got, keys, base, k, lo, exact):
    """got: the winners' (key, row, raw); keys: the list; base: its first key's position in the caller's array."""
    want = expected_topk(keys, k, lo)
    assert len(got) == len(want)
    assert got["key"].tolist() == [key for key, _ in want]
    rows = got["row"].astype(np.int64) - base
    if exact:
        assert rows.tolist() == [pos for _, pos in want]
    else:
        assert ((rows >= 0) & (rows < keys.size)).all()
        assert len(set(rows.tolist())) == len(want)
        assert (keys[rows] == got["key"]).all()
        if want:
            missing = {pos for key, pos in want if key < want[-1][0]} - set(rows.tolist())
            assert not missing, "keys strictly below the k-th left out, at positions %s" % sorted(missing)
    assert (got["raw"] == RAW[got["row"]]).all()


def check_block(block, keys, base, k, lo, exact, status=0):
    got_status, count, slots = parse(block)
    assert count == len(expected_topk(keys, k, lo))
    check_winners(slots[:count], keys, base, k, lo, exact)
    assert got_status == status
    assert (block[8:HEADER] == FILL).all() and (block[HEADER + 16 * count:] == FILL).all()


def test_constants_are_what_the_case_table_assumes(probe):
    assert probe.max_fused_k == sc.MAX_FUSED_K and probe.sel_list_max == sc.SEL_LIST_MAX
    assert probe.sel_two_level_min == sc.TWO_LEVEL_MIN and probe.sel_groups == sc.SEL_GROUPS
    assert probe.result_block_bytes == HEADER + 16 * probe.max_fused_k
    assert probe.radix_bins == 2048 and probe.status_retry == 100


# ---------------------------------------------------------------------------------------------------------------- launch_select
@pytest.mark.parametrize("case", sc.of_form("lone"), ids=repr)
def test_select_one_level(probe, case):
    n = case.lengths()[0]
    block, after = probe.select(case.keys, case.keys.size, case.k, lo=case.lo, m_dev=case.m_dev, status=7)
    check_block(block, case.keys[:n], 0, case.k, case.lo, exact=n <= 1024, status=7)
    assert after == 0


@pytest.mark.parametrize("m", (1500, 9001))
@pytest.mark.parametrize("ones", (False, True), ids=("low-bits-mixed", "low-bits-ones"))
def test_suspected_defect_a_smaller_key_after_many_equals_is_selected(probe, m, ones):
    """The issue's hand trace: 0x200 many times, 0x100 once at the end, k = 3.  The digits are exhausted with more equals than
    remain; the threshold must be the key, not the top of its bin, or 0x100 races the equals for a place and loses."""
    keys = sc.straggler(m, "first", ones)
    block, _ = probe.select(keys, m, 3)
    _, count, slots = parse(block)
    assert count == 3
    assert slots["key"][:3].tolist() == [int(keys[m - 1]), int(keys[0]), int(keys[0])] and slots["row"][0] == m - 1
    check_block(block, keys, 0, 3, None, exact=False)


def test_select_without_a_status_word_reports_zero(probe):
    for m in (700, 1500):
        keys = sc.dups(m, 1)
        block, after = probe.select(keys, m, 5, status=None)
        check_block(block, keys, 0, 5, None, exact=m <= 1024, status=0)
        assert after is None


@pytest.mark.parametrize("m,k", ((1500, 256), (4097, 256), (700, 70)))
def test_paging_with_has_lo_returns_the_sorted_list_once(probe, m, k):
    keys = sc.random_keys(m, 5)
    assert np.unique(keys).size == m
    pages, lo = [], None
    for _ in range(m // k + 2):
        block, _ = probe.select(keys, m, k, lo=lo)
        check_block(block, keys, 0, k, lo, exact=True)  # (distinct keys: the order is the sort's on either path)
        _, count, slots = parse(block)
        if count == 0:
            break
        pages.append(slots[:count].copy())
        lo = int(slots["key"][count - 1])
    got = np.concatenate(pages)
    assert got["key"].tolist() == sorted(keys.tolist()) and got["row"].tolist() == np.argsort(keys, kind="stable").tolist()


@pytest.mark.parametrize("case", sc.of_form("two-level"), ids=repr)
def test_select_two_levels_and_one_level_agree(probe, case):
    m = case.keys.size
    assert m >= probe.sel_two_level_min
    two, after = probe.select(case.keys, m, case.k, lo=case.lo, two_level=True, status=7)
    check_block(two, case.keys, 0, case.k, case.lo, exact=False, status=7)
    assert after == 0  # (the first level leaves the word alone, the second moves it)
    one, after = probe.select(case.keys, m, case.k, lo=case.lo, two_level=False, status=7)
    check_block(one, case.keys, 0, case.k, case.lo, exact=False, status=7)
    assert after == 0
    assert parse(one)[2]["key"].tolist() == parse(two)[2]["key"].tolist()


# ----------------------------------------------------------------------------------------------------------- launch_select_list
@pytest.mark.parametrize("case", sc.of_form("list"), ids=repr)
def test_select_list(probe, case):
    n, k = case.lengths()[0], case.k
    ok, orow, oraw = probe.select_list(case.keys, case.keys.size, case.m_dev, k)
    want = expected_topk(case.keys[:n], k)
    got = np.zeros(len(want), ENTRY)
    got["key"], got["row"], got["raw"] = ok[:len(want)], orow[:len(want)], oraw[:len(want)]
    check_winners(np.sort(got, order=["key", "row"]), case.keys[:n], 0, k, None, exact=False)   # (unsorted: compared as a set)
    pad = slice(len(want), k)
    assert (ok[pad] == EMPTY).all() and (orow[pad] == 0).all() and (oraw[pad] == 0).all()       # padding: (kEmptyKey, row 0, 0.0f)
    assert (ok[k:] == FILL64).all() and (orow[k:] == FILL32).all() and (oraw[k:] == FILL32).all()


# -------------------------------------------------------------------------------- launch_select_queries, launch_select_lists
@pytest.mark.parametrize("wide", (False, True), ids=("tight", "wide"))
@pytest.mark.parametrize("case", sc.of_form("queries"), ids=repr)
def test_select_queries(probe, case, wide):
    nq, m = case.keys.shape
    stride = probe.result_block_bytes if wide else HEADER + 16 * case.k
    out = probe.select_many(case.keys, nq, m, case.k, stride)
    for y in range(nq):
        check_block(out[y * stride:(y + 1) * stride], case.keys[y], y * m, case.k, None, exact=m <= 1024)


@pytest.mark.parametrize("spread", (False, True), ids=("one-block", "spread"))
@pytest.mark.parametrize("case", sc.of_form("lists"), ids=repr)
def test_select_lists(probe, case, spread):
    """Lists of up to 2048 keys go to the spread kernel when `spread` is set and the stride is above 1024, the longer ones to
    the one-block kernel beside it; each block is written by one of the two, and what the spread kernel writes is in
    position order among equals -- a block the other kernel wrote over it would not be."""
    nq, stride_keys = case.keys.shape
    stride = HEADER + 16 * case.k + 32
    out = probe.select_many(case.keys, nq, stride_keys, case.k, stride, m_dev=case.m_dev, spread=spread)
    for y, n in enumerate(case.lengths()):
        by_position = n <= 1024 or (spread and stride_keys > 1024 and n <= sc.SPREAD_KEYS)
        check_block(out[y * stride:(y + 1) * stride], case.keys[y, :n], y * stride_keys, case.k, None, exact=by_position)


# ------------------------------------------------------------------------------------------------------------- launch_sort_list
@pytest.mark.parametrize("m", (1, 1024, 1025, 4096))
def test_sort_list(probe, m):
    for keys in (sc.holes(sc.dups(m, 3), 0.25 if m > 1 else 0.0, 4), sc.random_keys(m, 5), np.full(m, EMPTY, np.uint64)):
        head, out, after = probe.sort_list(keys, m, status=7)
        want = expected_topk(keys, m)
        assert int(head[1]) == len(want) and int(head[0]) == 7 and after == 0
        check_winners(np.frombuffer(out.tobytes(), ENTRY)[:len(want)], keys, 0, m, None, exact=True)
        assert (out[16 * len(want):] == FILL).all()


def test_sort_list_refuses_no_list_and_a_list_too_long(probe):
    keys = sc.random_keys(probe.sel_list_max + 1, 6)
    probe.sort_list(keys, 0, expect=HIP_INVALID_VALUE)
    head, out, after = probe.sort_list(keys, probe.sel_list_max + 1, status=7, expect=HIP_INVALID_VALUE)
    assert after == 7 and not out.any() and not head.any()  # (nothing ran, nothing was copied back)


# ---------------------------------------------------------------------------------------------------------- launch_merge_blocks
def shard_blocks(world, k, block_bytes, seed):
    """`world` result blocks: sorted keys from a small range (equal keys across shards), counts of 0, below k, k and above k,
    slots at and past a block's count holding a key that would win if it were read."""
    r = np.random.default_rng(seed)
    counts = ([k + 7, 0, k - 1, k, 1] + r.integers(0, k + 1, size=world).tolist())[:world] if world > 1 else [max(k - 2, 1)]
    statuses = r.integers(0, 50, size=world).tolist()
    statuses[world // 2] = 99
    buf = np.full(world * block_bytes, 0x77, np.uint8)
    merged = []
    for w in range(world):
        ents = np.zeros(k, ENTRY)
        ents["row"] = 0xBAD00000
        live = min(counts[w], k)
        ents["key"][:live] = np.sort(r.integers(0, 4 * k, size=live, dtype=np.uint64)) + np.uint64(1 << 40)
        ents["row"][:live] = w * 1000 + np.arange(live)
        ents["raw"][:live] = RAW[w * 1000 + np.arange(live)]
        merged += [(int(e["key"]), w, j) for j, e in enumerate(ents[:live])]
        head = np.array([statuses[w], counts[w], 0, 0], np.uint32).view(np.uint8)
        at = w * block_bytes
        buf[at:at + HEADER] = head
        buf[at + HEADER:at + HEADER + 16 * k] = ents.view(np.uint8)
    merged.sort()
    return buf, merged[:k], max(statuses)


@pytest.mark.parametrize("world,k", ((1, 5), (2, 70), (8, 256), (32, 256)))
def test_merge_blocks(probe, world, k):
    """(32, 256) asks for exactly the 64 KiB of dynamic LDS the launcher's check allows, beside the kernel's few static bytes:
    the device takes it, and the block comes back written."""
    block_bytes = HEADER + 16 * k + 48
    buf, want, status = shard_blocks(world, k, block_bytes, 7 + world)
    rc, out, shard = probe.merge(buf, world, k, block_bytes)
    assert rc == 0
    got_status, count, slots = parse(out)
    assert count == len(want) and got_status == status
    assert slots["key"][:count].tolist() == [key for key, _, _ in want]
    assert shard[:count].tolist() == [w for _, w, _ in want]                    # equal keys: the lowest shard first
    assert slots["row"][:count].tolist() == [w * 1000 + j for _, w, j in want]
    assert (slots["raw"][:count] == RAW[slots["row"][:count]]).all()
    assert (out[8:HEADER] == FILL).all() and (out[HEADER + 16 * count:] == FILL).all() and (shard[count:] == FILL32).all()


# ------------------------------------------------------------------------------------------- launch_radix_pass, launch_radix_collect
def tied_scores(n, seed):
    r = np.random.default_rng(seed)
    scores = r.choice(np.linspace(-1, 1, 16).astype(np.float32), size=n)
    return (sc.orderable(scores) << np.uint64(32)) | r.permutation(n).astype(np.uint64)


RADIX_FAMILIES = {"random": sc.random_keys, "tied-scores": tied_scores, "crowded": sc.crowded,
                  "holes": lambda n, seed: sc.holes(sc.random_keys(n, seed), 0.3, seed + 1),
                  "tied-holes": lambda n, seed: sc.holes(tied_scores(n, seed), 0.3, seed + 1)}


def listed_rows(keys, k, passes):
    bits = 64 if passes == 6 else 33
    mask = ((1 << bits) - 1) << (64 - bits)
    thr = kth_threshold(keys, k, bits)
    return {i for i, x in enumerate(keys.tolist()) if x != EMPTY and (x & mask) <= thr}


@pytest.mark.parametrize("family", sorted(RADIX_FAMILIES))
@pytest.mark.parametrize("n", (1, 2, 4097, 20001))
def test_radix_kth_and_collect(probe, n, family):
    """The listed positions are exactly the live keys at or below the k-th key of the column (empties counted, as the
    histograms count them) on the digits the passes resolve -- all 64 bits, or the top 33 --, whatever the number of blocks;
    equals of the k-th key are all listed; k past the column's end lists every live key."""
    keys = RADIX_FAMILIES[family](n, 11 + n)
    for passes in (6, 3):
        for k in sorted({1, 300, n, n + 5}):
            want = listed_rows(keys, k, passes)
            for blocks in (1, 3, 64):
                pay = blocks != 3
                lk, lrow, lraw, count, status = probe.radix(keys, k, passes, blocks, cap=n + 3, pay=pay)
                assert count == len(want) and status == 0, (passes, k, blocks)
                assert set(lrow[:count].tolist()) == want and (lk[:count] == keys[lrow[:count]]).all(), (passes, k, blocks)
                assert (lraw[:count] == (RAW[lrow[:count]] if pay else 0)).all()          # no payload column: raw = 0.0f
                assert (lk[count:] == FILL64).all() and (lrow[count:] == FILL32).all() and (lraw[count:] == FILL32).all()


def test_radix_kth_inside_the_crowded_value(probe):
    keys = sc.crowded(20001, 12)
    low_word = int(keys.min() >> np.uint64(32))
    for k in (300, 9000):
        assert kth_threshold(keys, k, 64) >> 32 == low_word
        want = listed_rows(keys, k, 6)
        assert len(want) == k  # (distinct keys: six passes leave exactly the k smallest)
        _, lrow, _, count, _ = probe.radix(keys, k, 6, 64, cap=20001)
        assert count == k and set(lrow[:count].tolist()) == want
        _, lrow, _, count, _ = probe.radix(keys, k, 3, 64, cap=20001)
        assert set(lrow[:count].tolist()) == listed_rows(keys, k, 3) and count > 9000  # (33 bits: the whole crowded value)


def test_radix_collect_overflow_raises_retry_and_stays_inside_the_cap(probe):
    keys = sc.random_keys(4097, 13)
    want = listed_rows(keys, 300, 6)
    lk, lrow, lraw, count, status = probe.radix(keys, 300, 6, 3, cap=100, list_len=140)
    assert status == probe.status_retry and count == len(want) == 300  # (the count runs on: the host sees by how much)
    assert len(set(lrow[:100].tolist())) == 100 and set(lrow[:100].tolist()) <= want
    assert (lk[:100] == keys[lrow[:100]]).all() and (lraw[:100] == RAW[lrow[:100]]).all()
    assert (lk[100:] == FILL64).all() and (lrow[100:] == FILL32).all() and (lraw[100:] == FILL32).all()


def test_radix_refuses_a_misaligned_column_and_a_pass_out_of_range(probe):
    keys = sc.random_keys(4097, 14)
    for kw in (dict(key_offset=1), dict(passes=3, only_pass=3), dict(passes=6, only_pass=6), dict(k=0)):
        args = dict(k=5, passes=3, blocks=3, cap=4100)
        args.update(kw)
        lk, _, _, count, status = probe.radix(keys, expect=HIP_INVALID_VALUE, **args)
        assert not lk.any() and count == 0 and status == -1  # (nothing ran, nothing was copied back)
    _, lrow, _, count, _ = probe.radix(keys, 5, 6, 3, cap=4100, only_pass=5, expect=0)  # (in range: one pass alone lists nothing)
    assert (lrow == FILL32).all()


# ----------------------------------------------------------------------------------------------------------- the probe's own checks
def test_probe_refuses_what_the_kernels_would_overrun(probe):
    bad = HIP_INVALID_VALUE
    keys = sc.random_keys(3000, 15)
    size = probe.result_block_bytes
    # a list shorter than the launch is told, a block too small for its header and kMaxFusedK entries
    probe.select(keys, 3001, 5, expect=bad)
    probe.select(keys, 1500, 5, length=1499, expect=bad)
    probe.select(keys, 3000, 5, out_bytes=size - 16, expect=bad)
    probe.select_list(keys, 3001, None, 5, expect=bad)
    probe.select_list(keys, 3000, 3000, 300, out_len=299, expect=bad)
    # nq lists of m keys, nq blocks of out_stride bytes, a stride that holds k entries
    probe.select_many(keys, 3, 1001, 5, 96, expect=bad)
    probe.select_many(keys, 3, 1000, 5, 96, out_bytes=3 * 96 - 16, expect=bad)
    probe.select_many(keys, 3, 1000, 5, 80, expect=bad)
    probe.select_many(keys, 0, 1000, 5, 96, out_bytes=96, expect=bad)
    probe.select_many(keys, 3, 1000, 5, 96, m_dev=[1000, 1000, 1000], spread=True, out_bytes=3 * 96 - 16, expect=bad)
    # what the launchers refuse comes back as they give it: k = 0, k above the form's limit, a stride off its alignment
    probe.select(keys, 3000, 0, expect=bad)
    probe.select(keys, 3000, probe.max_fused_k + 1, expect=bad)
    probe.select_list(keys, 3000, 3000, probe.sel_list_max + 1, expect=bad)
    probe.select_many(keys, 3, 1000, 5, 104, expect=bad)
    probe.select_many(keys, 3, 1000, probe.max_fused_k + 1, HEADER + 16 * (probe.max_fused_k + 1), expect=bad)
    # a sorted list longer than its output
    probe.sort_list(keys, 3000, out_entries=2999, expect=bad)
    probe.sort_list(keys, 3001, expect=bad)
    # blocks shorter than world * block_bytes, a block narrower than k entries, a shard list shorter than k
    block_bytes = HEADER + 16 * 70
    buf, _, _ = shard_blocks(4, 70, block_bytes, 16)
    assert probe.merge(buf, 4, 70, block_bytes, blocks_len=buf.size - 16)[0] == bad
    assert probe.merge(buf, 4, 70, block_bytes - 16)[0] == bad
    assert probe.merge(buf, 4, 70, block_bytes, shard_len=69)[0] == bad
    assert probe.merge(buf, 0, 70, block_bytes)[0] == bad
    assert probe.merge(buf, 4, 70, block_bytes)[0] == 0
    # a list shorter than its cap, a pass count that is neither, no blocks
    probe.radix(keys, 5, 3, 3, cap=100, list_len=99, expect=bad)
    probe.radix(keys, 5, 4, 3, cap=100, expect=bad)
    probe.radix(keys, 5, 3, 0, cap=100, expect=bad)
    probe.radix(keys, 5, 3, 3, cap=0, expect=bad)
