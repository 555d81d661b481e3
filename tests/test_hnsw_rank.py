"""The id-rank column of an HNSW slab on the CPU: vettore_amd/csrc/host/vt_hnswrank.h (ids and rows in, ranks out), built
into a stand-alone program with AddressSanitizer and UBSan (tests/hnswrank_check.cpp) and run as a child process -- against
a plain sort: ids whose byte order is not the row order, ids that are prefixes of one another, dead rows first, last, in
between and everywhere, zero rows, and the inputs it refuses.  The numpy restatement the kernel tests use
(hnsw_stage_ref.id_ranks) is held to the same examples."""
import os
import subprocess
import tempfile

import hnsw_stage_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rank_header_under_the_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(), "hnswrank_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "hnswrank_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout[-2000:] + out.stderr[-2000:]


def test_the_rank_header_stands_alone():
    text = open(os.path.join(ROOT, "vettore_amd", "csrc", "host", "vt_hnswrank.h")).read()
    assert "hip" not in text.split("#pragma once")[1].lower() and '#include "' not in text


def test_the_numpy_restatement_on_the_same_examples():
    assert list(ref.id_ranks([b"b", b"a", None])) == [1, 0, ref.NO_ROW]
    assert list(ref.id_ranks([b"k1", b"k", b"", b"k10", b"k\xff", b"k\x00z", b"k\x7f"])) == [3, 1, 0, 4, 6, 2, 5]
    assert list(ref.id_ranks([None, None])) == [ref.NO_ROW, ref.NO_ROW] and len(ref.id_ranks([])) == 0
