#!/usr/bin/env python3
"""tools/hnsw_compact_probe.py -- the two figures DESIGN.md 4.14 quotes for the HNSW index's compaction (K11c).  Needs an
MI355X; there is no fallback.

  speed [--rows N --dim D --m M --m0 M0 --reps R] [--out FILE]
      the compaction launch (tests/hnsw_compact_probe.cpp: vthc_time, HIP events) on a slab of N rows of D floats, every
      other row live, beside device-to-device copies of the same number of live bytes in the same process -- what the
      slab's growth path does.  One JSON object: both times (the fastest of R), the bytes, the ratio.
  inserts [--count N --dim D --m M] [--out FILE]
      the wall time of N vt_hnsw_insert calls with no deletes (the compaction adds one comparison to each), through the
      library VETTORE_HIP_LIB names or the tree's own.  One JSON object; run it in fresh processes, alternating builds,
      and compare medians.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def speed(a):
    path = os.path.join(ROOT, "vettore_amd", "lib", "libvt_hnsw_compact_probe.so")
    F = C.CDLL(path)
    F.vthc_time.argtypes = [C.c_uint32] * 5 + [C.POINTER(C.c_float)] * 2 + [C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    compact, copy, nbytes, status = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint32()
    stride = (a.dim + 3) // 4 * 4
    rc = F.vthc_time(a.rows, stride, a.m, a.m0, a.reps, C.byref(compact), C.byref(copy), C.byref(nbytes), C.byref(status))
    if rc != 0:
        raise SystemExit("vthc_time: hipError_t %d" % rc)
    return {"what": "K11c compaction beside device-to-device copies of the same live bytes, fastest of %d, HIP events" % a.reps,
            "command": "python tools/hnsw_compact_probe.py speed --rows %d --dim %d --m %d --m0 %d --reps %d" % (a.rows, a.dim, a.m, a.m0, a.reps),
            "old_rows": a.rows, "live_rows": (a.rows + 1) // 2, "dim": a.dim, "m": a.m, "m0": a.m0, "live_bytes": nbytes.value,
            "compact_ms": round(compact.value, 4), "copy_ms": round(copy.value, 4),
            "compact_gb_per_s_read_plus_write": round(2 * nbytes.value / compact.value / 1e6, 1),
            "copy_gb_per_s_read_plus_write": round(2 * nbytes.value / copy.value / 1e6, 1),
            "ratio_compact_over_copy": round(compact.value / copy.value, 3), "guards_fired": status.value}


def inserts(a):
    import numpy as np
    from vettore_amd import nifs
    rng = np.random.default_rng(7)
    vecs = rng.standard_normal((a.count, a.dim)).astype(np.float32)
    ids = [b"doc-%d" % i for i in range(a.count)]
    made = nifs.hnsw_new_cosine(a.m, 2 * a.m, 100, 64, 12)
    assert made[0] == "ok", made
    idx = made[1]
    for i in range(64):    # (code objects, the first allocations)
        assert nifs.hnsw_insert(idx, b"warm-%d" % i, vecs[i]) == ("ok", ())
    t0 = time.perf_counter()
    for i in range(a.count):
        nifs.hnsw_insert(idx, ids[i], vecs[i])
    wall = time.perf_counter() - t0     # (every insert ends in a stream synchronise)
    mem = nifs.hnsw_memory(idx)
    assert mem["rows"] == a.count + 64 and mem["dead_rows"] == 0, mem
    return {"what": "wall time of %d vt_hnsw_insert calls, no deletes" % a.count,
            "command": "python tools/hnsw_compact_probe.py inserts --count %d --dim %d --m %d" % (a.count, a.dim, a.m),
            "build": a.label, "count": a.count, "dim": a.dim, "m": a.m, "m0": 2 * a.m,
            "wall_s": round(wall, 3), "inserts_per_s": round(a.count / wall, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["speed", "inserts"])
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=None)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--m0", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count", type=int, default=20000)
    ap.add_argument("--label", default="this tree", help="inserts: which build VETTORE_HIP_LIB names, for the record")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.dim is None:
        a.dim = 768 if a.mode == "speed" else 128
    line = json.dumps(speed(a) if a.mode == "speed" else inserts(a))
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
