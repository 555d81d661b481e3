"""The bookkeeping of the HNSW index's compaction on the CPU: vettore_amd/csrc/host/vt_hnswplan.h (the rule, the capacities,
the plan, its 32-bit refusal) and HnswGraph::close_rows() (vt_hnswgraph.h), built into a stand-alone program with
AddressSanitizer and UBSan (tests/hnswplan_check.cpp) and run as a child process; and the numpy restatement of the kernel
(tests/hnsw_compact_model.py) against examples written out by hand, the three guards among them -- the one for an entry
beyond the table is checked here and by reading the kernel, never on a GPU."""
import os
import subprocess
import tempfile

import numpy as np

import hnsw_compact_model as model
from hnsw_compact_model import BEYOND, COUNT, DEAD, NO_ROW, SHAPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_header_and_close_rows_under_the_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(), "hnswplan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "hnswplan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout[-2000:] + out.stderr[-2000:]


def test_the_plan_header_stands_alone():
    text = open(os.path.join(ROOT, "vettore_amd", "csrc", "host", "vt_hnswplan.h")).read()
    assert "hip" not in text.split("#pragma once")[1].lower() and '#include "' not in text


# m = 2, m0 = 3: five rows, rows 1 and 3 dead.  G marks words behind a count: garbage the compaction must not carry over.
G = 0xDEADBEEF
M, M0 = 2, 3


def tiny():
    X = np.arange(20, dtype=np.float32).reshape(5, 4)
    adj0 = np.asarray([[2, 2, 4, G], [0, G, G, G], [3, 0, 4, 2], [1, 0, G, G], [0, G, G, G]], np.uint32)
    level = np.asarray([1, 0, 2, 1, 0], np.uint32)
    upoff = np.asarray([0, 3, 5, 11, 14], np.uint32)          # (two unused words in front of row 2's lists)
    upper = np.asarray([1, 2, G, G, G, 2, 0, 2, 0, G, G, 0, G, G], np.uint32)
    return dict(X=X, adj0=adj0, level=level, upoff=upoff, upper=upper)


def test_the_model_on_an_example_written_out_by_hand():
    t = tiny()
    src, new_upoff, new_upper = model.plan_for(t["level"], [4, 0, 2], M)
    assert list(src) == [0, 2, 4] and list(new_upoff) == [0, 3, 9] and new_upper == 9
    out = model.compact(t["X"], t["adj0"], t["level"], t["upoff"], t["upper"], M, M0, src, new_upoff, new_upper)
    assert list(out["remap"]) == [0, NO_ROW, 1, NO_ROW, 2]
    assert out["outX"].tolist() == t["X"][[0, 2, 4]].tolist()
    assert out["out_adj0"].tolist() == [[2, 1, 2, 0], [3, 0, 2, 1], [0, 0, 0, 0]]
    assert list(out["out_level"]) == [1, 2, 0] and list(out["out_upoff"]) == [0, 3, 9]
    assert list(out["out_upper"]) == [1, 1, 0, 2, 0, 1, 0, 0, 0]
    assert list(out["status"]) == [0, 0, 0, 0]


def test_the_models_guards():
    # an entry that names a dead row inside the table: the sentinel in its place, every other word as before
    t = tiny()
    src, new_upoff, new_upper = model.plan_for(t["level"], [0, 2, 4], M)
    clean = model.compact(t["X"], t["adj0"], t["level"], t["upoff"], t["upper"], M, M0, src, new_upoff, new_upper)
    t["upper"][6] = 3
    out = model.compact(t["X"], t["adj0"], t["level"], t["upoff"], t["upper"], M, M0, src, new_upoff, new_upper)
    assert list(out["status"]) == [0, 1, 0, 0] and out["out_upper"][4] == NO_ROW
    assert np.array_equal(np.delete(out["out_upper"], 4), np.delete(clean["out_upper"], 4))
    assert np.array_equal(out["out_adj0"], clean["out_adj0"])
    # an entry beyond the table: flagged without a look at the table (an index error here would be the kernel's stray read)
    t = tiny()
    t["adj0"][2][3] = 5
    out = model.compact(t["X"], t["adj0"], t["level"], t["upoff"], t["upper"], M, M0, src, new_upoff, new_upper)
    assert list(out["status"]) == [1, 0, 0, 0] and out["out_adj0"].tolist() == [[2, 1, 2, 0], [3, 0, 2, NO_ROW], [0, 0, 0, 0]]
    t["adj0"][2][3] = NO_ROW
    out = model.compact(t["X"], t["adj0"], t["level"], t["upoff"], t["upper"], M, M0, src, new_upoff, new_upper)
    assert list(out["status"]) == [1, 0, 0, 0] and out["out_adj0"][1][3] == NO_ROW
    # a count above the degree: clamped, flagged, the list otherwise renumbered
    t = tiny()
    t["adj0"][0] = [M0 + 1, 2, 4, 0]
    out = model.compact(t["X"], t["adj0"], t["level"], t["upoff"], t["upper"], M, M0, src, new_upoff, new_upper)
    assert list(out["status"]) == [0, 0, 1, 0] and out["out_adj0"][0].tolist() == [3, 1, 2, 0]
    t["upper"][0] = 7
    t["upper"][1:3] = [4, 4]
    out = model.compact(t["X"], t["adj0"], t["level"], t["upoff"], t["upper"], M, M0, src, new_upoff, new_upper)
    assert list(out["status"]) == [0, 0, 1, 0] and list(out["out_upper"][:3]) == [2, 2, 2]
    # a level of the mirror that is not the plan's: that row's upper-layer lists stay empty, nothing outside is read
    t = tiny()
    t["level"][2] = 3
    out = model.compact(t["X"], t["adj0"], t["level"], t["upoff"], t["upper"], M, M0, src, new_upoff, new_upper)
    assert list(out["status"]) == [0, 0, 0, 1] and list(out["out_upper"]) == [1, 1, 0, 0, 0, 0, 0, 0, 0]


def test_hand_made_mirrors_name_live_rows_only():
    rng = np.random.default_rng(3)
    live = list(range(1, 65, 2))
    mir = model.make_mirror(rng, 65, 8, 4, 8, live)
    assert set(mir["level"].tolist()) == {0, 1, 2, 3}
    src, new_upoff, new_upper = model.plan_for(mir["level"], live, 4)
    out = model.compact(mir["X"], mir["adj0"], mir["level"], mir["upoff"], mir["upper"], 4, 8, src, new_upoff, new_upper)
    assert list(out["status"]) == [0, 0, 0, 0] and new_upper > 0
    for lists, lim in ((out["out_adj0"], 8), (out["out_upper"].reshape(-1, 5), 4)):
        counts = lists[:, 0]
        assert counts.max() == lim and counts.min() == 0
        for row in lists:
            assert row[1:1 + row[0]].max(initial=0) < len(live) and not row[1 + row[0]:].any()
