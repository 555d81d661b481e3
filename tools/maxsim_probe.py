#!/usr/bin/env python3
"""tools/maxsim_probe.py [--out FILE] [--stats KERNEL_STATS_CSV] -- one large stateless MaxSim call
(vt_multi_vector_top_k: 20 000 documents of 0..256 vectors, d = 128, 32 query vectors, limit 100) with inner product
and with cosine: the call's wall time, its rate in document-vector bytes per second, and beside it a plain pinned
host-to-device copy of the same bytes timed in the same process.  Run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o probe -- python3 tools/maxsim_probe.py --out X.json

and pass the kernel-stats CSV rocprofv3 wrote with --stats (a second run of this script, no GPU needed) to add the
kernel times (maxsim_kernel, maxsim_norms_kernel) to the JSON."""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, NQ, LIMIT, REPS = 20000, 128, 32, 100, 3


def kernel_stats(path):
    """Per kernel instance: maxsim_kernel<0, order> serves inner product, maxsim_kernel<6, 0> and maxsim_norms_kernel
    cosine -- each instance belongs to one metric's REPS + 1 calls."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            if "maxsim" not in name:
                continue
            metric = "cosine" if ("maxsim_kernel<6" in name or "norms" in name) else "inner_product"
            short = re.search(r"maxsim_\w+(?:<[^>]*>)?", name).group(0)
            out[short] = {"metric": metric, "launches": int(row.get("Calls", 0)),
                          "total_ms": float(row.get("TotalDurationNs", 0)) / 1e6}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--stats")
    args = ap.parse_args()
    if args.stats:  # merge rocprofv3's kernel statistics into an earlier run's JSON
        res = json.load(open(args.out))
        res["kernels"] = kernel_stats(args.stats)
        for name, m in res["metrics"].items():  # device time of one call: every launch of its kernels / its calls
            calls = len(m["call_s"]) + 1  # (+1: the warm-up call)
            m["kernel_ms_per_call"] = sum(v["total_ms"] for v in res["kernels"].values() if v["metric"] == name) / calls
            m["kernel_fraction_of_call"] = m["kernel_ms_per_call"] / m["best_call_ms"]
        res.pop("kernel_ms_per_call", None)
        json.dump(res, open(args.out, "w"), indent=1)
        print(json.dumps(res))
        return
    import torch
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
    token_bytes = values.nbytes
    res = {"shape": {"documents": N, "d": D, "query_vectors": NQ, "vectors": nvec, "limit": LIMIT,
                     "token_bytes": token_bytes}, "metrics": {}}
    for name, code in (("inner_product", 3), ("cosine", 2)):
        times = []
        for r in range(REPS + 1):  # call 0 warms up (allocations, code objects)
            h = C.c_void_p()
            t0 = time.perf_counter()
            st = L.vt_multi_vector_top_k(0, N, idb, nifs._szp(ioff), nifs._szp(doc_vec_off), nifs._fp(values),
                                         nifs._szp(voff), nifs._fp(query.reshape(-1)), nifs._szp(qoff), NQ, code, LIMIT,
                                         C.byref(h))
            dt = time.perf_counter() - t0
            assert st == 0, _lib.error_text(st)
            L.vt_hits_free(h)
            if r:
                times.append(dt)
        best = min(times)
        res["metrics"][name] = {"call_s": times, "best_call_ms": best * 1e3, "token_GBps": token_bytes / best / 1e9,
                                "gflop": 2.0 * NQ * nvec * D / 1e9}
    # a plain pinned host-to-device copy of the same bytes (one transfer; best of REPS)
    src = torch.from_numpy(values.reshape(-1)).pin_memory()
    dst = torch.empty(src.numel(), dtype=torch.float32, device="cuda")
    copy = []
    for r in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        if r:
            copy.append(time.perf_counter() - t0)
    res["pinned_copy"] = {"s": copy, "GBps": token_bytes / min(copy) / 1e9}
    for m in res["metrics"].values():
        m["fraction_of_pinned_copy_rate"] = m["token_GBps"] / res["pinned_copy"]["GBps"]
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
