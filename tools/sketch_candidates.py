#!/usr/bin/env python3
"""tools/sketch_candidates.py OUT.json [--queries 300] [--limit 10] [--seed S] -- candidates per lone search of the
bench's 10 M x 768 cosine corpus: bench.py's generator for rows and queries (the queries from another seed), profiling
on, one search at a time.  Per query the growth of the path's `_candidates` counter (the limit's path: K1n up to 10 --
K1f where `VT_SKETCH6=3` switches K1n off --, else `sketch6_candidates`) and whether the pass certified; OUT.json holds
min / max / mean / median, the passes that did not certify, the queries' seed and the per-query list, so two builds can be
compared query by query (`profiles/sketch_tail_spread/`, `profiles/sketch4/`)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=300)
    ap.add_argument("--limit", type=int, default=10)
    ap.add_argument("--seed", type=int, default=bench.SEED_QUERY + 1)
    a = ap.parse_args()
    import torch
    from vettore_amd import nifs, _lib
    L = _lib.load()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    nifs.set_device(0)
    x = bench.build_shard(torch, device, a.rows, a.dim, bench.SEED_CORPUS, normalize=True)
    # (build_shard's `x[dst] = x[src]` meets repeated dst rows and src rows that are dst rows too: which copy wins is not
    # fixed from process to process, so two runs compare query by query only where this sum of the rows' bits agrees)
    checksum = 0
    for s in range(0, a.rows, 1 << 20):
        checksum += int(x[s:s + (1 << 20)].view(torch.int32).sum(dtype=torch.int64).item())
    ref = nifs._flat_new(nifs.METRIC_CODE["cosine"])
    nifs.flat_set_reduce_order(ref, bench.ORDER_CODE["sse2"])
    assert nifs.flat_load_device_matrix(ref, bench.doc_ids(0, a.rows), x.data_ptr(), a.rows, a.dim) == ("ok", ())
    del x
    torch.cuda.empty_cache()
    qs = bench.normalized_queries(a.queries, a.dim, a.seed)
    hp = C.c_void_p()

    def search(q):
        st = L.vt_flat_search(ref.handle, q.ctypes.data_as(C.POINTER(C.c_float)), a.dim, a.limit, C.byref(hp))
        assert st == 0, (L.vt_last_error() or b"").decode()
        L.vt_hits_free(hp)

    search(qs[0])  # (builds the columns)
    nifs.flat_set_profiling(ref, True)
    name = "sketch6" if a.limit > 10 else "sketch5" if os.environ.get("VT_SKETCH6") == "3" else "sketch4"
    per, missed, delivered = [], 0, 0  # (delivered: K1n searches whose result the filtered K1 wrote itself)
    prev = nifs.flat_get_profile(ref)
    for q in qs:
        search(q)
        cur = nifs.flat_get_profile(ref)
        assert cur[name + "_launches"] == prev[name + "_launches"] + 1, "the search did not take the %s path" % name
        if cur[name + "_fallbacks"] != prev[name + "_fallbacks"]:
            missed += 1
            per.append(None)
        else:
            per.append(int(cur[name + "_candidates"] - prev[name + "_candidates"]))
            delivered += int(cur.get("sketch4_finished", 0) - prev.get("sketch4_finished", 0))
        prev = cur
    ok = [c for c in per if c is not None]
    out = {"rows": a.rows, "dim": a.dim, "queries": a.queries, "limit": a.limit, "seed": a.seed, "path": name, "corpus_checksum": checksum,
           "fallbacks": missed, "candidates_min": min(ok), "candidates_max": max(ok), "candidates_mean": float(np.mean(ok)),
           "candidates_median": float(np.median(ok)), "per_query": per}
    if name == "sketch4":  # (certified searches the filtered K1 did not deliver took the lists and the select behind a second wait)
        out["delivered"], out["second_wait"] = delivered, len(ok) - delivered
    json.dump(out, open(a.out, "w"))
    print(json.dumps({k: v for k, v in out.items() if k != "per_query"}))


if __name__ == "__main__":
    main()
