#!/usr/bin/env python3
"""tools/maxsim_resident_probe.py [--out FILE] [--skip-stateless] [--stats KERNEL_STATS_CSV] -- the resident
multi-vector store (vt_mv_*, K9r) beside the stateless call it replaces, at tools/maxsim_probe.py's shape (20 000
documents of 0..256 vectors, d = 128, 32 query vectors, limit 100), inner product and cosine, in one process.  The legs
alternate -- the stateless call, the resident call, the resident call with K9 forced over the same slab --, REPS times
after a warm-up round, so that whatever else the box does meets all of them alike; per leg the best, the median and the
worst call, and the spread (worst - best) / best that a difference between two legs has to exceed to count.
The stateless call is what the parent commit does: it is unchanged.

The K9 leg needs the test hook `test_mv_k9`, so run against the hooks build:

    VETTORE_HIP_LIB=vettore_amd/lib/libvettore_hip_hooks.so python3 tools/maxsim_resident_probe.py --out X.json

Kernel times come from a run of its own under the profiler, without the stateless leg (its launches of maxsim_kernel
could not be told from the forced ones):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o probe -- \\
        python3 tools/maxsim_resident_probe.py --skip-stateless --out Y.json
    python3 tools/maxsim_resident_probe.py --out X.json --stats DIR/.../probe_kernel_stats.csv    (no GPU needed)
"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, NQ, LIMIT, REPS = 20000, 128, 32, 100, 5
PUT_DOCS = 2000  # documents per vt_mv_put_many


def kernel_stats(path, calls):
    """maxsim_resident_kernel<0, order> / maxsim_kernel<0, order> serve inner product, <6, 0> cosine; per metric every
    kernel saw `calls` calls (warm-up included)."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for kernel in ("maxsim_resident_kernel", "maxsim_kernel"):
                if kernel + "<" in name:
                    metric = "cosine" if kernel + "<6" in name else "inner_product"
                    total_ms = float(row.get("TotalDurationNs", 0)) / 1e6
                    out.setdefault(metric, {})[kernel] = {"launches": int(row.get("Calls", 0)), "total_ms": total_ms,
                                                          "ms_per_call": total_ms / calls}
    return out


def summary(times):
    best, worst = min(times), max(times)
    return {"call_s": times, "best_ms": best * 1e3, "median_ms": statistics.median(times) * 1e3, "worst_ms": worst * 1e3,
            "spread": (worst - best) / best}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--stats")
    ap.add_argument("--skip-stateless", action="store_true")
    args = ap.parse_args()
    if args.stats:  # merge the profiler's kernel statistics into an earlier run's JSON
        res = json.load(open(args.out))
        res["kernels"] = kernel_stats(args.stats, REPS + 1)
        json.dump(res, open(args.out, "w"), indent=1)
        print(json.dumps(res))
        return
    from vettore_amd import _lib, nifs
    L = _lib.load()
    rng = np.random.default_rng(2026)
    counts = rng.integers(0, 257, size=N)
    doc_vec_off = np.zeros(N + 1, dtype=np.uintp)
    doc_vec_off[1:] = np.cumsum(counts)
    nvec = int(doc_vec_off[-1])
    values = rng.standard_normal(size=(nvec, D), dtype=np.float32)
    query = rng.standard_normal(size=(NQ, D), dtype=np.float32)
    idb, ioff = nifs._pack_ids("doc%06d" % i for i in range(N))
    voff = (np.arange(nvec + 1, dtype=np.uintp) * D).astype(np.uintp)
    qoff = (np.arange(NQ + 1, dtype=np.uintp) * D).astype(np.uintp)
    q = query.reshape(-1)

    store = C.c_void_p()
    assert L.vt_mv_new(nifs.DEVICE, C.byref(store)) == 0, L.vt_last_error()
    t0 = time.perf_counter()
    for i0 in range(0, N, PUT_DOCS):
        i1 = min(N, i0 + PUT_DOCS)
        st = L.vt_mv_put_many(store, i1 - i0, idb, nifs._szp(ioff[i0:i1 + 1]), nifs._szp(doc_vec_off[i0:i1 + 1]),
                              nifs._fp(values), nifs._szp(voff))
        assert st == 0, _lib.error_text(st)
    put_s = time.perf_counter() - t0
    try:
        nifs.debug_get("test_mv_k9")
        have_hook = True
    except Exception:
        have_hook = False

    def stateless(code):
        h = C.c_void_p()
        st = L.vt_multi_vector_top_k(nifs.DEVICE, N, idb, nifs._szp(ioff), nifs._szp(doc_vec_off), nifs._fp(values),
                                     nifs._szp(voff), nifs._fp(q), nifs._szp(qoff), NQ, code, LIMIT, C.byref(h))
        assert st == 0, _lib.error_text(st)
        return nifs._take_hits(h)

    def resident(code):
        h = C.c_void_p()
        st = L.vt_mv_top_k(store, nifs._fp(q), nifs._szp(qoff), NQ, code, LIMIT, C.byref(h))
        assert st == 0, _lib.error_text(st)
        return nifs._take_hits(h)

    def resident_k9(code):
        nifs.debug_set("test_mv_k9", 1)
        try:
            return resident(code)
        finally:
            nifs.debug_set("test_mv_k9", 0)

    legs = ([] if args.skip_stateless else [("stateless", stateless)]) + [("resident", resident)] + \
        ([("resident_k9", resident_k9)] if have_hook else [])
    res = {"shape": {"documents": N, "d": D, "query_vectors": NQ, "vectors": nvec, "limit": LIMIT, "token_bytes": values.nbytes},
           "put_s": put_s, "reps": REPS, "metrics": {}}
    for name, code in (("inner_product", 3), ("cosine", 2)):
        times = {leg: [] for leg, _ in legs}
        hits = {}
        for r in range(REPS + 1):  # round 0 warms up (allocations, code objects)
            for leg, fn in legs:
                t0 = time.perf_counter()
                got = fn(code)
                dt = time.perf_counter() - t0
                if r:
                    times[leg].append(dt)
                hits.setdefault(leg, got)
                assert got == hits[leg], leg
        first = hits[legs[0][0]]
        assert all(h == first for h in hits.values()), "the legs disagree"   # ids, order and score bits
        m = {leg: summary(t) for leg, t in times.items()}
        m["gflop"] = 2.0 * NQ * nvec * D / 1e9
        if "stateless" in m:
            m["resident_over_stateless"] = m["resident"]["best_ms"] / m["stateless"]["best_ms"]
        if "resident_k9" in m:
            m["k9r_over_k9_call"] = m["resident"]["best_ms"] / m["resident_k9"]["best_ms"]
        res["metrics"][name] = m
    L.vt_mv_free(store)
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
