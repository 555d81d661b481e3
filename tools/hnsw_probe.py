#!/usr/bin/env python3
"""tools/hnsw_probe.py [--rows N] [--dims 128,768] [--build-seconds S] [--out profiles/hnsw_probe.json]

What the HNSW index (vt_hnsw_*, K11) does on one MI355X, measured once: build rows/s, lone-search latency,
search_batch queries/s at 64 and 1 024 queries per call, and recall@10 against the flat index on the same rows, with
the default parameters (m 16, m0 32, ef_construction 100, ef_search 64) under cosine on normalised random rows.

Every shape runs in a child process of its own under a time limit, and inside it the build stops at --build-seconds
with the rows it has (the figures then describe that many rows: the JSON says how many).  Nothing is asserted."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_shape(rows, d, build_seconds):
    import numpy as np
    from vettore_amd import nifs
    from vettore_amd.index_hnsw import DEFAULT_OPTIONS as P
    rng = np.random.default_rng(20261018)
    x = rng.standard_normal((rows, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    ids = [b"r%07d" % i for i in range(rows)]
    made = nifs.hnsw_new_cosine(P["m"], P["m0"], P["ef_construction"], P["ef_search"], P["max_level"])
    assert made[0] == "ok", made
    idx = made[1]
    out = {"d": d, "rows_asked": rows, "parameters": dict(P), "metric": "cosine"}
    t0 = time.perf_counter()
    built = 0
    while built < rows and time.perf_counter() - t0 < build_seconds:
        hi = min(rows, built + 500)
        assert nifs.hnsw_insert_many(idx, list(zip(ids[built:hi], x[built:hi]))) == ("ok", ())
        built = hi
    dt = time.perf_counter() - t0
    out.update(rows=built, build_s=round(dt, 3), build_rows_per_s=round(built / dt, 1), counters_after_build=nifs.hnsw_counters(idx))
    q = rng.standard_normal((1024, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    for v in q[:8]:
        nifs.hnsw_search(idx, v, 10)
    lat = []
    for v in q[:200]:
        t = time.perf_counter()
        nifs.hnsw_search(idx, v, 10)
        lat.append(time.perf_counter() - t)
    lat.sort()
    out["lone_search_us"] = {"median": round(lat[len(lat) // 2] * 1e6, 1), "p90": round(lat[int(len(lat) * 0.9)] * 1e6, 1)}
    for nq in (64, 1024):
        nifs.hnsw_search_batch(idx, q[:nq], 10)
        best = min(_timed(lambda: nifs.hnsw_search_batch(idx, q[:nq], 10)) for _ in range(3))
        out["search_batch_%d_queries_per_s" % nq] = round(nq / best, 1)
    flat = nifs.flat_new_cosine()
    assert nifs.flat_load_matrix(flat, ids[:built], x[:built]) == ("ok", ())
    st, exact = nifs.flat_search_batch(flat, q[:200], 10)
    assert st == "ok"
    approx = nifs.hnsw_search_batch(idx, q[:200], 10)
    hit = sum(len({i for i, _ in e} & {i for i, _ in a[1]}) for e, a in zip(exact, approx))
    out["recall_at_10"] = round(hit / (10.0 * 200), 4)
    out["counters"] = nifs.hnsw_counters(idx)
    return out


def _timed(f):
    t = time.perf_counter()
    f()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--dims", default="128,768")
    ap.add_argument("--build-seconds", type=float, default=240.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_probe.json"))
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(one_shape(a.rows, a.child, a.build_seconds)))
        return
    shapes = []
    for d in [int(v) for v in a.dims.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--build-seconds", str(a.build_seconds), "--child", str(d)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.build_seconds + 240)
        except subprocess.TimeoutExpired:
            shapes.append({"d": d, "error": "time limit"})
            break  # (a shape that ran out of time: nothing more is started on the device)
        line = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
        if res.returncode != 0 or not line:
            shapes.append({"d": d, "error": "exit %d" % res.returncode, "stderr": res.stderr[-600:]})
            break
        shapes.append(json.loads(line[0][7:]))
        print(json.dumps(shapes[-1]), flush=True)
    doc = {"what": "tools/hnsw_probe.py: one run on one MI355X, nothing averaged over boxes", "shapes": shapes,
           "unmeasured": ["per-hop cost", "10 M-row build time"]}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
