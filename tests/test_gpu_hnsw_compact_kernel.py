"""K11c, the compaction of an HNSW slab and its device mirror (vt_hnsw.hip: launch_hnsw_compact), launched through
tests/hnsw_compact_probe.cpp (libvt_hnsw_compact_probe.so: vt_hnsw.hip and nothing else of the library) on hand-made
mirrors, against the numpy restatement in tests/hnsw_compact_model.py (which tests/test_hnsw_plan.py checks on the CPU).

Every output buffer -- rows, level, offsets, both list arrays with their zero fill, the remap table, the guards' status
words -- is compared word for word; the buffers start as 0xA5 bytes, so a word the launch left alone shows.  Two guards
are driven: an entry that names a dead row inside the table, and a count of m0 + 1.  The third, an entry beyond the
table, exists to keep a read inside a buffer: it is checked on the CPU model and by reading the kernel, and the probe
refuses such a mirror before anything is launched."""
import ctypes as C
import os

import numpy as np
import pytest

import hnsw_compact_model as model
from hnsw_compact_model import COUNT, DEAD, NO_ROW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, M0 = 4, 8
OUTPUTS = ("outX", "out_adj0", "out_level", "out_upoff", "out_upper", "remap", "status")


class CompactProbe:
    def __init__(self):
        path = os.environ.get("VT_HNSW_COMPACT_PROBE_LIB") or os.path.join(ROOT, "vettore_amd", "lib", "libvt_hnsw_compact_probe.so")
        assert os.path.exists(path), "build it with `make` (%s)" % os.path.basename(path)
        F = self.lib = C.CDLL(path)
        f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        F.vthc_guards.restype = F.vthc_no_row.restype = C.c_uint32
        F.vthc_compact.argtypes = [f32p, u32p, u32p, u32p, u32p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p,
                                   C.c_uint32, C.c_uint64, f32p, u32p, u32p, u32p, u32p, u32p, u32p]
        assert F.vthc_guards() == 4 and F.vthc_no_row() == NO_ROW

    def compact(self, mir, m, m0, src, new_upoff, new_upper):
        """(hipError_t, outputs): the launch on a copy of the mirror."""
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float if a.dtype == np.float32 else C.c_uint32))
        old = {k: np.ascontiguousarray(v) for k, v in mir.items()}
        old_rows, stride = old["X"].shape
        src, new_upoff = np.ascontiguousarray(src, np.uint32), np.ascontiguousarray(new_upoff, np.uint32)
        rows = len(src)
        out = dict(outX=np.zeros((rows, stride), np.float32), out_adj0=np.zeros((rows, m0 + 1), np.uint32),
                   out_level=np.zeros(rows, np.uint32), out_upoff=np.zeros(rows, np.uint32),
                   out_upper=np.zeros(max(new_upper, 1), np.uint32), remap=np.zeros(old_rows, np.uint32), status=np.zeros(4, np.uint32))
        rc = self.lib.vthc_compact(p(old["X"]), p(old["adj0"]), p(old["level"]), p(old["upoff"]), p(old["upper"]), old_rows,
                                   len(old["upper"]), stride, m, m0, p(src), p(new_upoff), rows, new_upper, p(out["outX"]),
                                   p(out["out_adj0"]), p(out["out_level"]), p(out["out_upoff"]), p(out["out_upper"]), p(out["remap"]),
                                   p(out["status"]))
        out["out_upper"] = out["out_upper"][:new_upper]
        return rc, out


@pytest.fixture(scope="module")
def probe():
    import vettore_amd._lib as L
    assert L.load().vt_device_count() >= 1, "no HIP device: GPU tests need the real hardware"
    return CompactProbe()


def live_sets(rows):
    sets = {"first row dead": range(1, rows), "last row dead": range(0, rows - 1), "every other row dead": range(0, rows, 2),
            "the other rows dead": range(1, rows, 2), "nothing dead": range(rows)}
    return {k: list(v) for k, v in sets.items() if len(v)}


def assert_same(got, want):
    for name in OUTPUTS:
        g, w = got[name], want[name]
        assert g.shape == w.shape, name
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        assert bad.size == 0, (name, int(bad[0]), int(g.reshape(-1)[bad[0]]), int(w.reshape(-1)[bad[0]]))


@pytest.mark.parametrize("stride", [4, 8, 772])
@pytest.mark.parametrize("rows", [1, 65, 300])
def test_every_word_is_the_models(probe, rows, stride):
    rng = np.random.default_rng(1000 * rows + stride)
    sets = live_sets(rows)
    assert rows == 1 or {"first row dead", "last row dead", "every other row dead"} <= set(sets)
    for name, live in sets.items():
        mir = model.make_mirror(rng, rows, stride, M, M0, live)
        src, new_upoff, new_upper = model.plan_for(mir["level"], live, M)
        want = model.compact(mir["X"], mir["adj0"], mir["level"], mir["upoff"], mir["upper"], M, M0, src, new_upoff, new_upper)
        rc, got = probe.compact(mir, M, M0, src, new_upoff, new_upper)
        assert rc == 0, (name, rc)
        assert list(want["status"]) == [0, 0, 0, 0]
        assert_same(got, want)
        if rows == 300:
            assert set(mir["level"][src].tolist()) == {0, 1, 2, 3} and new_upper > 256   # more than one block of list words


def guarded_case(rows=300, stride=8):
    rng = np.random.default_rng(77)
    live = list(range(0, rows, 2))
    mir = model.make_mirror(rng, rows, stride, M, M0, live)
    src, new_upoff, new_upper = model.plan_for(mir["level"], live, M)
    return mir, live, src, new_upoff, new_upper


def test_an_entry_that_names_a_dead_row_is_flagged_and_replaced(probe):
    mir, live, src, new_upoff, new_upper = guarded_case()
    clean = model.compact(mir["X"], mir["adj0"], mir["level"], mir["upoff"], mir["upper"], M, M0, src, new_upoff, new_upper)
    # one entry on layer 0 and one on an upper layer, each inside its count, now name dead rows inside the table
    r0 = next(r for r in live if mir["adj0"][r][0] >= 2)
    mir["adj0"][r0][2] = 1
    r1 = next(r for r in live if mir["level"][r] >= 2 and mir["upper"][mir["upoff"][r] + M + 1] >= 1)
    mir["upper"][mir["upoff"][r1] + M + 2] = len(mir["level"]) - 1   # (the last row: odd, dead)
    want = model.compact(mir["X"], mir["adj0"], mir["level"], mir["upoff"], mir["upper"], M, M0, src, new_upoff, new_upper)
    i0, i1 = live.index(r0), live.index(r1)
    assert list(want["status"]) == [0, 1, 0, 0] and want["out_adj0"][i0][2] == NO_ROW and want["out_upper"][new_upoff[i1] + M + 2] == NO_ROW
    differ = sum(int((want[k] != clean[k]).sum()) for k in ("out_adj0", "out_upper", "outX", "out_level", "out_upoff", "remap"))
    assert differ == 2 and want["status"][DEAD] == 1
    rc, got = probe.compact(mir, M, M0, src, new_upoff, new_upper)
    assert rc == 0
    assert_same(got, want)


def test_a_count_above_the_degree_is_clamped_and_flagged(probe):
    mir, live, src, new_upoff, new_upper = guarded_case()
    r0 = live[5]
    mir["adj0"][r0][0] = M0 + 1
    mir["adj0"][r0][1:] = live[:M0]
    want = model.compact(mir["X"], mir["adj0"], mir["level"], mir["upoff"], mir["upper"], M, M0, src, new_upoff, new_upper)
    assert list(want["status"]) == [0, 0, 1, 0] and want["status"][COUNT] == 1
    assert want["out_adj0"][5].tolist() == [M0] + list(range(M0))
    rc, got = probe.compact(mir, M, M0, src, new_upoff, new_upper)
    assert rc == 0
    assert_same(got, want)


def test_the_probe_launches_nothing_on_a_mirror_it_cannot_vouch_for(probe):
    mir, live, src, new_upoff, new_upper = guarded_case(rows=65)
    bad = dict(mir, adj0=mir["adj0"].copy())
    r0 = next(r for r in live if bad["adj0"][r][0] >= 1)
    bad["adj0"][r0][1] = 65                       # an entry beyond the table
    assert probe.compact(bad, M, M0, src, new_upoff, new_upper)[0] == 1   # hipErrorInvalidValue
    assert probe.compact(mir, M, M0, src[::-1], new_upoff, new_upper)[0] == 1
    assert probe.compact(mir, M, M0, src, new_upoff, new_upper + 1)[0] == 1
