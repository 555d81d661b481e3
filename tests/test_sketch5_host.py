"""host/vt_sketch5.h -- the 5-bit sketch's row quantiser restated and the bound of the query level its pass keeps off the
one-bit L plane -- is plain C++: built here with g++ and checked against naive recounts with AddressSanitizer and UBSan on."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quantiser_and_level_bound_under_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(), "sketch5_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "sketch5_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-2000:], out.stderr[-2000:])
