#!/usr/bin/env python3
"""tools/muvera_probe.py [--out FILE] [--stats KERNEL_STATS_CSV] [--docs N] [--reps N] -- the batched MUVERA encoder
(vt_muvera_encode) on a seeded corpus: N documents (default 100 000) of 32 vectors, d = 128, 20 repetitions, 5 SimHash
projections, projection dimension 16 -- 10 240 floats per document, kept whole (final None) or folded to 2 048 -- and
one 32-vector query under the same configurations.  It reports the wall time per call (median of --reps calls after a
warm-up call, a host clock around a call that ends in a device synchronise), the bytes that cross the host link, and,
for scale, the time tests/muvera_ref.py (a Python restatement of the reference, NOT its Rust) takes for 100 of those
documents on the host.  It fails without a GPU.  Run it once plainly for the wall times, and once more under

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o probe -- python3 tools/muvera_probe.py --reps 3 --out Y.json

then pass the kernel-stats CSV of that run (no GPU needed) with --stats to add the kernel times and the achieved f64
multiply-add rate -- vectors * R * (k_sim + d_proj) * d over the encode kernel's time -- beside the device's f64 vector
peak to the first run's JSON."""
import argparse
import csv
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VECS, D, R, K, PD, SEED = 32, 128, 20, 5, 16, 2026
FINALS = {"final_none": None, "final_2048": 2048}
# MI355X f64 vector peak: 78.6 TFLOPS (AMD's data sheet; half the FP32 vector rate) = 39.3e12 multiply-adds per second
PEAK_F64_FMA = 39.3e12


def kernel_stats(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            if "muvera" not in name:
                continue
            short = re.search(r"muvera_\w+", name).group(0)
            out[short] = {"launches": int(row.get("Calls", 0)), "total_ms": float(row.get("TotalDurationNs", 0)) / 1e6}
    return out


def encode(L, mode, count, set_off, values, val_off, final, out):
    sz, fp = C.POINTER(C.c_size_t), C.POINTER(C.c_float)
    t0 = time.perf_counter()
    st = L.vt_muvera_encode(0, mode, count, set_off.ctypes.data_as(sz), values.ctypes.data_as(fp), val_off.ctypes.data_as(sz),
                            D, R, K, SEED, PD, final or 0, 0 if final is None else 1, out.ctypes.data_as(fp), None)
    dt = time.perf_counter() - t0
    assert st == 0, st
    return dt


def timed(L, reps, *args):
    encode(L, *args)  # the warm-up call: allocations, code objects
    times = [encode(L, *args) for _ in range(reps)]
    return {"call_s": times, "median_ms": statistics.median(times) * 1e3, "min_ms": min(times) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--stats")
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-docs", type=int, default=100)
    args = ap.parse_args()
    if args.stats:  # merge the profiled run's kernel statistics into the plain run's JSON
        res = json.load(open(args.out))
        ks = kernel_stats(args.stats)
        p = res["profiled_run"] = {"kernels": ks, "docs": args.docs, "calls_per_configuration": args.reps + 1}
        # the profiled run made (reps + 1) document calls and as many query calls per configuration, in both configurations
        fma_docs = float(args.docs) * VECS * R * (K + PD) * D
        fma_total = 2 * (args.reps + 1) * (fma_docs + VECS * R * (K + PD) * D)
        enc = ks.get("muvera_encode_kernel")
        if enc:
            p["encode_kernel_s_total"] = enc["total_ms"] / 1e3
            p["f64_fma_total"] = fma_total
            p["f64_fma_per_s"] = fma_total / (enc["total_ms"] / 1e3)
            p["f64_vector_peak_fma_per_s"] = PEAK_F64_FMA
            p["share_of_f64_vector_peak"] = p["f64_fma_per_s"] / PEAK_F64_FMA
            p["encode_kernel_ms_per_document_call"] = enc["total_ms"] / (2 * (args.reps + 1))  # (the query calls' share is 1 / docs)
        json.dump(res, open(args.out, "w"), indent=1)
        print(json.dumps(res))
        return

    from vettore_amd import _lib
    L = _lib.load()
    assert L.vt_device_count() >= 1, "no HIP device: this probe measures the GPU and has no fallback"
    rng = np.random.default_rng(SEED)
    n = args.docs
    values = rng.standard_normal(size=(n * VECS, D), dtype=np.float32)
    set_off = (np.arange(n + 1, dtype=np.uintp) * VECS).astype(np.uintp)
    val_off = (np.arange(n * VECS + 1, dtype=np.uintp) * D).astype(np.uintp)
    query = rng.standard_normal(size=(VECS, D), dtype=np.float32)
    q_set_off = np.array([0, VECS], dtype=np.uintp)
    q_val_off = (np.arange(VECS + 1, dtype=np.uintp) * D).astype(np.uintp)
    fma = float(n) * VECS * R * (K + PD) * D
    res = {"shape": {"documents": n, "vectors_per_document": VECS, "d": D, "num_repetitions": R, "num_simhash_projections": K,
                     "projection_dimension": PD, "seed": SEED, "full_dimension": R * (1 << K) * PD,
                     "upload_bytes": values.nbytes, "f64_fma_per_document_call": fma, "reps": args.reps},
           "configurations": {}}
    for name, final in FINALS.items():
        fde = L.vt_muvera_fde_dimension(R, K, PD, final or 0, 0 if final is None else 1)
        out = np.empty((n, fde), dtype=np.float32)
        qout = np.empty((1, fde), dtype=np.float32)
        docs = timed(L, args.reps, 1, n, set_off, values, val_off, final, out)
        docs["download_bytes"] = out.nbytes
        docs["documents_per_s"] = n / (docs["median_ms"] / 1e3)
        docs["upload_GBps_at_median"] = values.nbytes / (docs["median_ms"] / 1e3) / 1e9
        docs["f64_fma_per_s_of_the_whole_call"] = fma / (docs["median_ms"] / 1e3)
        one = timed(L, args.reps, 0, 1, q_set_off, query, q_val_off, final, qout)
        res["configurations"][name] = {"fde_dimension": fde, "documents": docs, "query": one}
        del out
    # for scale: the Python restatement on the host (numpy; NOT the Rust reference)
    import muvera_ref
    h = min(args.host_docs, n)
    sets = values[:h * VECS].reshape(h, VECS, D)
    host = {}
    for name, final in FINALS.items():
        t0 = time.perf_counter()
        for s in sets:
            assert muvera_ref.encode_document(list(s), D, R, K, SEED, PD, final)[0] == "ok"
        per_doc = (time.perf_counter() - t0) / h
        gpu_per_doc = res["configurations"][name]["documents"]["median_ms"] / 1e3 / n
        host[name] = {"documents": h, "s_per_document": per_doc, "gpu_s_per_document": gpu_per_doc, "ratio": per_doc / gpu_per_doc}
    res["python_restatement_on_host"] = host
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "configurations"}))
    for name, c in res["configurations"].items():
        print(name, "documents median %.1f ms (min %.1f)" % (c["documents"]["median_ms"], c["documents"]["min_ms"]),
              "query median %.3f ms" % c["query"]["median_ms"])


if __name__ == "__main__":
    main()
