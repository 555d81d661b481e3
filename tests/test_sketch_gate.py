"""host/vt_sketchtiers.h -- the sketch tiers' table and the one gate that says which of them a lone search wants (DESIGN.md
4.10) -- is plain C++: built here with g++ and checked by tests/sketch_gate_check.cpp, against the four predicates stated one
by one, with AddressSanitizer and UBSan on."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gate_agrees_with_the_four_predicates_under_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(), "sketch_gate_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "sketch_gate_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-2000:], out.stderr[-2000:])
