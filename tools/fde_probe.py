#!/usr/bin/env python3
"""tools/fde_probe.py [--documents N] [--out FILE] -- the MUVERA retrieval flow over a resident multi-vector store
(vt_mv_fde_sync, vt_mv_fde_top_k; K10s) beside the same work through the public calls that were there before it, in one
process.  Shape: N documents (default 100 000) of 32 vectors, d = 128; R = 20, k = 5, pd = 16, final projection 2 048.

(a) indexing: vt_mv_fde_sync of every document into a fresh inner-product handle, against vt_muvera_encode(mode 1) of the
    same vectors from host rows followed by vt_flat_load_matrix of the rows it returned, into a fresh handle as well.
(b) search: vt_mv_fde_top_k at limit 10 and 100 candidates, against vt_muvera_encode(mode 0), vt_flat_search and
    vt_mv_top_k_ids made one after the other (the ids taken across with vt_hits_export); and, for the design note only,
    vt_mv_top_k over the whole store -- a different answer, so no condition.

The legs of a pair alternate, REPS times after a warm-up round, so that whatever else the box does meets both alike; per
leg the best, the median and the worst call and the spread (worst - best).  A pair's condition: the new leg's median is
no worse than the comparison's median plus the larger of the two spreads.  The answers of a pair are compared too.

    python3 tools/fde_probe.py --out profiles/fde_resident.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VECS, D, REPS = 32, 128, 5
CFG = (D, 20, 5, 42, 16, 2048, 1)   # vt_muvera_encode's seven trailing arguments
LIMIT, CANDIDATES, IP = 10, 100, 3
PUT_DOCS = 2000  # documents per vt_mv_put_many


def summary(times):
    best, worst = min(times), max(times)
    return {"call_s": times, "best_ms": best * 1e3, "median_ms": statistics.median(times) * 1e3, "worst_ms": worst * 1e3,
            "spread_ms": (worst - best) * 1e3, "spread": (worst - best) / best}


def pair(new, old):
    allowance = max(new["spread_ms"], old["spread_ms"])
    return {"new_over_comparison_median": new["median_ms"] / old["median_ms"], "allowance_ms": allowance,
            "condition_met": new["median_ms"] <= old["median_ms"] + allowance}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--documents", type=int, default=100000)
    ap.add_argument("--out")
    args = ap.parse_args()
    from vettore_amd import _lib, nifs
    L = _lib.load()
    N = args.documents
    rng = np.random.default_rng(2026)
    nvec = N * VECS
    values = rng.standard_normal(size=(nvec, D), dtype=np.float32)
    doc_vec_off = (np.arange(N + 1, dtype=np.uintp) * VECS).astype(np.uintp)
    voff = (np.arange(nvec + 1, dtype=np.uintp) * D).astype(np.uintp)
    ids = ["doc%06d" % i for i in range(N)]
    idb, ioff = nifs._pack_ids(ids)
    query = rng.standard_normal(size=(VECS, D), dtype=np.float32).reshape(-1)
    qoff = (np.arange(VECS + 1, dtype=np.uintp) * D).astype(np.uintp)
    one_set = np.array([0, VECS], dtype=np.uintp)
    fde = int(L.vt_muvera_fde_dimension(CFG[1], CFG[2], CFG[4], CFG[5], CFG[6]))
    ip, fp, sz = C.POINTER(C.c_int), nifs._fp, nifs._szp

    store = C.c_void_p()
    assert L.vt_mv_new(nifs.DEVICE, C.byref(store)) == 0, L.vt_last_error()
    t0 = time.perf_counter()
    for i0 in range(0, N, PUT_DOCS):
        i1 = min(N, i0 + PUT_DOCS)
        st = L.vt_mv_put_many(store, i1 - i0, idb, sz(ioff[i0:i1 + 1]), sz(doc_vec_off[i0:i1 + 1]), fp(values), sz(voff))
        assert st == 0, _lib.error_text(st)
    put_s = time.perf_counter() - t0

    def fresh():
        return nifs.flat_new_inner_product()

    # ---- (a) indexing
    host_rows = np.zeros((N, fde), dtype=np.float32)
    status = np.zeros(N, dtype=np.intc)

    def sync(index):
        st = L.vt_mv_fde_sync(store, index.handle, 0, None, None, *CFG, None)
        assert st == 0, _lib.error_text(st)

    def through_host(index):
        st = L.vt_muvera_encode(nifs.DEVICE, 1, N, sz(doc_vec_off), fp(values.reshape(-1)), sz(voff), *CFG, fp(host_rows.reshape(-1)),
                                status.ctypes.data_as(ip))
        assert st == 0 and not status.any(), _lib.error_text(st)
        st = L.vt_flat_load_matrix(index.handle, N, fde, idb, sz(ioff), fp(host_rows.reshape(-1)))
        assert st == 0, _lib.error_text(st)

    times = {"sync": [], "through_host": []}
    kept = {}
    for r in range(REPS + 1):  # round 0 warms up (allocations, code objects)
        for leg, fn in (("sync", sync), ("through_host", through_host)):
            index = fresh()
            t0 = time.perf_counter()
            fn(index)
            dt = time.perf_counter() - t0
            if r:
                times[leg].append(dt)
            assert len(index) == N
            kept[leg] = index   # (the last round's handles serve the search legs; the earlier ones are freed here)
    indexing = {leg: summary(t) for leg, t in times.items()}
    indexing.update(pair(indexing["sync"], indexing["through_host"]))
    index = kept["sync"]
    probe = np.zeros(fde, dtype=np.float32)
    probe[::7] = 1.0
    assert nifs.flat_search(index, probe, 50) == nifs.flat_search(kept["through_host"], probe, 50), "the two indexes disagree"
    del kept["through_host"]

    # ---- (b) search
    qfde = np.zeros(fde, dtype=np.float32)
    blob = C.create_string_buffer(CANDIDATES * 16)
    hoff = (C.c_size_t * (CANDIDATES + 1))()
    raw = (C.c_float * CANDIDATES)()

    def flow():
        h = C.c_void_p()
        st = L.vt_mv_fde_top_k(store, index.handle, *CFG, fp(query), sz(qoff), VECS, CANDIDATES, IP, LIMIT, C.byref(h))
        assert st == 0, _lib.error_text(st)
        return h

    def three_calls():
        st = L.vt_muvera_encode(nifs.DEVICE, 0, 1, sz(one_set), fp(query), sz(qoff), *CFG, fp(qfde), None)
        assert st == 0, _lib.error_text(st)
        found = C.c_void_p()
        st = L.vt_flat_search(index.handle, fp(qfde), fde, CANDIDATES, C.byref(found))
        assert st == 0, _lib.error_text(st)
        n = L.vt_hits_len(found)
        assert n <= CANDIDATES and L.vt_hits_id_bytes(found) <= len(blob)
        L.vt_hits_export(found, blob, hoff, raw, None)
        L.vt_hits_free(found)
        h = C.c_void_p()
        st = L.vt_mv_top_k_ids(store, n, blob, hoff, fp(query), sz(qoff), VECS, IP, LIMIT, C.byref(h))
        assert st == 0, _lib.error_text(st)
        return h

    def brute_force():
        h = C.c_void_p()
        st = L.vt_mv_top_k(store, fp(query), sz(qoff), VECS, IP, LIMIT, C.byref(h))
        assert st == 0, _lib.error_text(st)
        return h

    times = {"flow": [], "three_calls": [], "brute_force": []}
    for r in range(REPS + 1):
        hits = {}
        for leg, fn in (("flow", flow), ("three_calls", three_calls), ("brute_force", brute_force)):
            t0 = time.perf_counter()
            h = fn()
            dt = time.perf_counter() - t0
            if r:
                times[leg].append(dt)
            hits[leg] = nifs._take_hits(h)   # (outside the timed part, for every leg)
        assert hits["flow"] == hits["three_calls"] and len(hits["flow"]) == LIMIT, "the flow and the three calls disagree"
        recall = len({i for i, _ in hits["flow"]} & {i for i, _ in hits["brute_force"]}) / LIMIT
    search = {leg: summary(t) for leg, t in times.items()}
    search.update(pair(search["flow"], search["three_calls"]))
    search["overlap_with_brute_force_top_10"] = recall

    L.vt_mv_free(store)
    res = {"shape": {"documents": N, "vectors_per_document": VECS, "d": D, "num_repetitions": CFG[1], "num_simhash_projections": CFG[2],
                     "seed": CFG[3], "projection_dimension": CFG[4], "final_projection_dimension": CFG[5], "fde_dimension": fde,
                     "limit": LIMIT, "candidates": CANDIDATES, "metric": "inner_product", "token_bytes": values.nbytes,
                     "fde_bytes": host_rows.nbytes},
           "put_s": put_s, "reps": REPS, "indexing": indexing, "search": search}
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
