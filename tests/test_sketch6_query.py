"""The host side of the 6-bit sketch (vettore_amd/csrc/host/vt_sketch6.h: the query's signed-nibble levels and the
restatement of the row quantiser) is plain C++: built here with g++ and checked with AddressSanitizer and UBSan on."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_levels_and_row_quantiser_under_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(), "sketch6_query_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "sketch6_query_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-2000:], out.stderr[-2000:])
