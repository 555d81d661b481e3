"""host/vt_sketchbatch.h -- K1qm's gate, planner, LDS formula and per-query decline -- is plain C++: built
here with g++ and checked by tests/sketch_batch_plan_check.cpp with AddressSanitizer and UBSan on."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_lds_decline_and_gate_under_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(), "sketch_batch_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "sketch_batch_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-2000:], out.stderr[-2000:])
