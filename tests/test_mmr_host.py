"""The host code of MMR reranking that needs no device (vettore_amd/csrc/host/vt_mmrplan.h: argument checks, score
conversion, id validation for the handle call, order bookkeeping), compiled into a stand-alone program with
AddressSanitizer and UBSan (tests/mmr_check.cpp) and compared line by line with the restatement.  CPU only."""
import math
import os
import struct
import subprocess
import tempfile

import numpy as np

import mmr_ref
import oracle
from vettore_amd.index_flat import result_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def d64(x):
    return struct.pack(">d", float(x)).hex()


def f32(x):
    return struct.pack(">f", float(x)).hex()


def hx(b):
    return b.hex() or "-"


def test_host_code_under_the_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(), "mmr_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "mmr_check.cpp"), "-o", exe])
    script, expected = [], []
    # the guards and finite_number?/1, as the restatement has them
    ok_i, ok_e = [("a", 1.0)], [("a", [1.0])]
    for alpha in (0.0, 1.0, 0.5, -0.0, -1e-300, 1.0000000000000002, math.nan, math.inf, -math.inf):
        for k in (0, 1, 2 ** 63):
            script.append("G %s %d" % (d64(alpha), k))
            expected.append("1" if mmr_ref.mmr_rerank(ok_i, ok_e, "l2", alpha, k)[0] == "ok" else "0")
    edge = mmr_ref.F32_MAX
    for scores in ([], [0.0], [edge, -edge], [math.nextafter(edge, math.inf)], [1.0, math.nan], [-math.inf], [1.0, 2.0, 3.5e38]):
        script.append("S %d %s" % (len(scores), " ".join(d64(s) for s in scores)))
        expected.append("1" if all(mmr_ref.finite_number(s) for s in scores) else "0")
    # result_values/3's score for every metric and both modes, bit for bit
    for name in oracle.METRICS:
        for raw in (0.0, -0.0, 0.25, -1.0, 1.0, 3.0e38, 1e-45, 5.0):
            raw = float(np.float32(raw))
            if raw == -1.0 and name in mmr_ref.DISTANCE_METRICS and name != "negative_inner_product":
                continue  # (a distance is never negative: 1.0 / (1.0 + raw) has no value there)
            for mode, mode_name in ((0, "raw"), (1, "similarity")):
                script.append("H %d %s %d" % (oracle.METRIC_CODE[name], f32(raw), mode))
                expected.append(d64(result_values(name, raw, mode_name)[0]))
    # ids through the table, after swap-deletes have moved rows
    ids = [b"id%03d" % i for i in range(200)] + [b"", b"\x00", b"\x00\x00"]
    script.append("T %d %s" % (len(ids), " ".join(hx(i) for i in ids)))
    rows = list(ids)
    for gone in (b"id007", b"id199", b"", b"id100", b"\x00\x00"):
        script.append("E " + hx(gone))
        r = rows.index(gone)
        rows[r] = rows[-1]
        rows.pop()
    place = {i: r for r, i in enumerate(rows)}
    for ask in ([b"id001", b"\x00", b"id150"], [], [rows[-1], rows[0], rows[6]], [b"id007"], [b"id001", b"id002", b"id001"],
                [b""], [b"id0010"], rows):
        script.append("R %d %s" % (len(ask), " ".join(hx(i) for i in ask)))
        good = all(i in place for i in ask) and len(set(ask)) == len(ask)
        expected.append("".join("%d " % place[i] for i in ask) if good else "bad")
    # a call's problems, and what comes back
    jobs = [(5, 3), (0, 4), (7, 99), (1, 1)]
    script.append("L %d %s" % (len(jobs), " ".join("%d:%d" % j for j in jobs)))
    expected.append("0:5:3 5:0:0 5:7:7 12:1:1 13 7 7")
    order = list(range(100, 113))
    for p, status, count, want in ((0, 0, 3, "0: 100 101 102"), (1, 0, 0, "0:"), (2, 0, 7, "0: 105 106 107 108 109 110 111"),
                                   (2, 4, 2, "4:"), (0, 0, 2, "-1:"), (3, 0, 1, "0: 112")):
        script.append("C %d %d %d %s" % (p, status, count, " ".join(map(str, order))))
        expected.append(want)
    script.append("L 2 %d:1 %d:1" % (2 ** 31, 5))
    expected.append("bad")
    script.append("L 3 %d:1 %d:1 %d:9" % (2 ** 31 - 1, 2 ** 31 - 1, 100))
    expected.append("bad")
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    got = [line.rstrip() for line in out.stdout.splitlines()]
    assert len(got) == len(expected)
    for line, (g, e) in enumerate(zip(got, expected)):
        assert g == e.rstrip(), (line, g, e)
