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

--batch: the batched calls (vt_mv_top_k_ids_batch / vt_mv_top_k_batch, K9rb) on the same store against a loop of single
calls -- the loop is the parent commit's path, unchanged --, inner product, limit 10: B in {1, 8, 64} query sets of 32
vectors with their own 100 and 1 000 random candidate ids each, and B in {1, 8} sets over the whole store.  Batch call and
loop alternate in one process, REPS times after a warm-up round; per shape both legs' best / median / worst, the ratio of
the medians, and the launches and batched sets the handle counted for one batch call:

    python3 tools/maxsim_resident_probe.py --batch --out profiles/maxsim_resident_batch.json
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


BATCH_LIMIT, BATCH_CODE = 10, 3


def batch_probe(L, _lib, nifs, store, rng, nvec, put_s):
    """--batch: see the module's docstring."""
    def counters():
        a, b = C.c_uint64(), C.c_uint64()
        assert L.vt_mv_counters(store, C.byref(a), C.byref(b)) == 0
        return a.value, b.value

    shapes = [("ids", B, cands) for cands in (100, 1000) for B in (1, 8, 64)] + [("whole", B, None) for B in (1, 8)]
    res = {"shape": {"documents": N, "d": D, "query_vectors": NQ, "vectors": nvec, "limit": BATCH_LIMIT, "metric": "inner_product"},
           "put_s": put_s, "reps": REPS, "shapes": []}
    for mode, B, cands in shapes:
        query = rng.standard_normal(size=(B * NQ, D), dtype=np.float32).reshape(-1)
        qoff = (np.arange(B * NQ + 1, dtype=np.uintp) * D).astype(np.uintp)
        set_off = (np.arange(B + 1, dtype=np.uintp) * NQ).astype(np.uintp)
        lists = [["doc%06d" % i for i in rng.choice(N, size=cands, replace=False)] for _ in range(B)] if cands else []
        packed = [nifs._pack_ids(ids) for ids in lists]
        idb, ioff = nifs._pack_ids(i for ids in lists for i in ids)
        set_id_off = (np.arange(B + 1, dtype=np.uintp) * (cands or 0)).astype(np.uintp)

        def batch():
            outs, status = (C.c_void_p * B)(), (C.c_int * B)()
            if cands:
                st = L.vt_mv_top_k_ids_batch(store, B, nifs._szp(set_id_off), idb, nifs._szp(ioff), nifs._szp(set_off),
                                             nifs._fp(query), nifs._szp(qoff), BATCH_CODE, BATCH_LIMIT, outs, status)
            else:
                st = L.vt_mv_top_k_batch(store, B, nifs._szp(set_off), nifs._fp(query), nifs._szp(qoff), BATCH_CODE, BATCH_LIMIT,
                                         outs, status)
            assert st == 0 and not any(status), _lib.error_text(st)
            return outs

        def loop():
            outs = (C.c_void_p * B)()
            for b in range(B):
                h = C.c_void_p()
                qb, ob = query[b * NQ * D:], qoff[:NQ + 1]
                if cands:
                    st = L.vt_mv_top_k_ids(store, cands, packed[b][0], nifs._szp(packed[b][1]), nifs._fp(qb), nifs._szp(ob), NQ,
                                           BATCH_CODE, BATCH_LIMIT, C.byref(h))
                else:
                    st = L.vt_mv_top_k(store, nifs._fp(qb), nifs._szp(ob), NQ, BATCH_CODE, BATCH_LIMIT, C.byref(h))
                assert st == 0, _lib.error_text(st)
                outs[b] = h.value
            return outs

        times = {"batch": [], "loop": []}
        counted = None
        for r in range(REPS + 1):  # round 0 warms up (allocations, code objects)
            hits = {}
            for leg, fn in (("batch", batch), ("loop", loop)):
                c0 = counters()
                t0 = time.perf_counter()
                outs = fn()
                dt = time.perf_counter() - t0
                c1 = counters()
                if r:
                    times[leg].append(dt)
                if leg == "batch":
                    counted = {"scoring_launches": c1[0] - c0[0], "batched_sets": c1[1] - c0[1]}
                hits[leg] = [nifs._take_hits(C.c_void_p(outs[b])) for b in range(B)]   # (outside the timed part, for both legs)
            assert hits["batch"] == hits["loop"], "the batch call and the loop disagree"   # ids, order and score bits
        m = {"mode": mode, "sets": B, "candidates": cands, "batch": summary(times["batch"]), "loop": summary(times["loop"]),
             "one_batch_call": counted}
        m["batch_over_loop_median"] = m["batch"]["median_ms"] / m["loop"]["median_ms"]
        res["shapes"].append(m)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--stats")
    ap.add_argument("--skip-stateless", action="store_true")
    ap.add_argument("--batch", action="store_true")
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
    if args.batch:
        res = batch_probe(L, _lib, nifs, store, rng, nvec, put_s)
        L.vt_mv_free(store)
        if args.out:
            json.dump(res, open(args.out, "w"), indent=1)
        print(json.dumps(res))
        return
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
