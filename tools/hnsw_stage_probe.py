#!/usr/bin/env python3
"""tools/hnsw_stage_probe.py [--rows N] [--dims 128,768] [--build-seconds S] [--out profiles/hnsw_stage/probe.json]

What quantized_search, funnel_search and hybrid_search cost on the HNSW handle (vt_hnsw_*_search, K15) on one MI355X,
measured once: the median time per call of each, and beside it the same call on a flat handle loaded with the same rows
(the existing path, not the code under test).  Default parameters (m 16, m0 32, ef_construction 100, ef_search 64),
cosine, normalised random rows; limit 10, candidates 100; the funnel's stage is min(d, 128); hybrid runs the HNSW
collection's default generators (the traversal and quantized) on the HNSW handle and search + quantized on the flat one.

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


def median_us(call, queries):
    for v in queries[:8]:
        call(v)
    lat = []
    for v in queries:
        t = time.perf_counter()
        res = call(v)
        lat.append(time.perf_counter() - t)
        assert res[0] == "ok", res
    lat.sort()
    return {"median": round(lat[len(lat) // 2] * 1e6, 1), "p90": round(lat[int(len(lat) * 0.9)] * 1e6, 1)}


def one_shape(rows, d, build_seconds):
    import numpy as np
    from vettore_amd import nifs
    from vettore_amd.index_hnsw import DEFAULT_OPTIONS as P
    rng = np.random.default_rng(20261021)
    x = rng.standard_normal((rows, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    ids = [b"r%07d" % i for i in range(rows)]
    made = nifs.hnsw_new_cosine(P["m"], P["m0"], P["ef_construction"], P["ef_search"], P["max_level"])
    assert made[0] == "ok", made
    idx = made[1]
    t0 = time.perf_counter()
    built = 0
    while built < rows and time.perf_counter() - t0 < build_seconds:
        hi = min(rows, built + 500)
        assert nifs.hnsw_insert_many(idx, list(zip(ids[built:hi], x[built:hi]))) == ("ok", ())
        built = hi
    flat = nifs.flat_new_cosine()
    assert nifs.flat_load_matrix(flat, ids[:built], x[:built]) == ("ok", ())
    q = rng.standard_normal((200, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    limit, cand, stage = 10, 100, [min(d, 128)]
    t = time.perf_counter()
    nifs.hnsw_quantized_search(idx, q[0], cand, limit)   # (the id ranks are sorted and uploaded here)
    first = time.perf_counter() - t
    out = {"d": d, "rows_asked": rows, "rows": built, "metric": "cosine", "parameters": dict(P), "limit": limit, "candidates": cand,
           "funnel_stages": stage, "first_staged_call_us": round(first * 1e6, 1), "us_per_call": {}}
    gh = [(nifs.GEN_SEARCH, cand, []), (nifs.GEN_QUANTIZED, cand, [])]
    for name, on_hnsw, on_flat in (
            ("quantized_search", lambda v: nifs.hnsw_quantized_search(idx, v, cand, limit), lambda v: nifs.flat_quantized_search(flat, v, cand, limit)),
            ("funnel_search", lambda v: nifs.hnsw_funnel_search(idx, v, stage, cand, limit), lambda v: nifs.flat_funnel_search(flat, v, stage, cand, limit)),
            ("hybrid_search", lambda v: nifs.hnsw_hybrid_search(idx, v, gh, limit), lambda v: nifs.flat_hybrid_search(flat, v, gh, limit))):
        out["us_per_call"][name] = {"hnsw_handle": median_us(on_hnsw, q), "flat_handle": median_us(on_flat, q)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000)
    ap.add_argument("--dims", default="128,768")
    ap.add_argument("--build-seconds", type=float, default=120.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_stage", "probe.json"))
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(one_shape(a.rows, a.child, a.build_seconds)))
        return
    shapes = []
    for d in [int(v) for v in a.dims.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--build-seconds", str(a.build_seconds), "--child", str(d)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.build_seconds + 120)
        except subprocess.TimeoutExpired:
            shapes.append({"d": d, "error": "time limit"})
            break  # (a shape that ran out of time: nothing more is started on the device)
        line = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
        if res.returncode != 0 or not line:
            shapes.append({"d": d, "error": "exit %d" % res.returncode, "stderr": res.stderr[-600:]})
            break
        shapes.append(json.loads(line[0][7:]))
        print(json.dumps(shapes[-1]), flush=True)
    doc = {"what": "tools/hnsw_stage_probe.py: one run on one MI355X, nothing averaged over boxes; wall time per call in "
                   "microseconds through the Python mirror of the NIFs", "shapes": shapes,
           "unmeasured": ["the kernels' own times", "slabs with dead rows", "the rank column's rebuild beyond the first call"]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
