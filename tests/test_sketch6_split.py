"""host/vt_sketch6.h's sketch6_level_sums -- the sums of a query level's positive and negative entries and its 1-norm, which
bound the level the 6-bit pass keeps off the L plane -- is plain C++: built here with g++ and checked against a naive
recount with AddressSanitizer and UBSan on."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_level_sums_under_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(), "sketch6_split_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "sketch6_split_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-2000:], out.stderr[-2000:])
