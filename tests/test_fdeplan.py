"""The planning behind vt_mv_fde_sync (vettore_amd/csrc/host/vt_fdeplan.h: deduplication of the listed ids, which are
encoded and which leave the index, chunk cuts under a byte budget, runs of good documents in a chunk) is plain C++ with no
HIP call in it: tests/fdeplan_check.cpp drives it against a brute-force model, built as a stand-alone program with
AddressSanitizer and UBSan."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_against_a_model():
    exe = os.path.join(tempfile.mkdtemp(), "fdeplan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "fdeplan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-2000:])
    assert out.stdout.strip() == "ok"
