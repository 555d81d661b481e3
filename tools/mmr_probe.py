#!/usr/bin/env python3
"""tools/mmr_probe.py [--rows N] [--dim D] [--out profiles/mmr_probe.json] [--trace-only]

What MMR costs on top of the search it follows (K12), on one handle of --rows normalised random rows under
cosine: a lone flat_search(limit = candidates) against flat_mmr_search with the same candidates, alternated in one
process, for candidates in {100, 1 000} and limit in {10, 100}; the same as one batch call of 256 queries; and the time
tests/mmr_ref.py takes for the 1 000-candidate case, for context.  The search itself is the same in both calls, so the
difference is MMR's, reported per round (limit + 1 step launches).  Nothing is asserted.

--trace-only runs a few diversified searches and nothing else: the run to put behind
`rocprofv3 --kernel-trace --stats -- python tools/mmr_probe.py --trace-only` (no counters in that run); tools/step_chain.py
reads the chain's kernel times and gaps from its trace."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    from vettore_amd import nifs
    rng = np.random.default_rng(20261018)
    ref = nifs.flat_new_cosine()
    ids = [b"r%07d" % i for i in range(a.rows)]
    x = rng.standard_normal((a.rows, a.dim), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    assert nifs.flat_load_matrix(ref, ids, x) == ("ok", ())
    x_keep = x[:1000].copy()
    del x
    q = rng.standard_normal((256, a.dim)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    if a.trace_only:
        for v in q[:4]:
            assert nifs.flat_mmr_search(ref, v, 1000, 100, 0.5)[0] == "ok"
        return
    out = {"rows": a.rows, "d": a.dim, "metric": "cosine", "alpha": 0.5, "reps": a.reps, "lone": [], "batch_256": []}
    for candidates in (100, 1000):
        for limit in (10, 100):
            for v in q[:3]:
                nifs.flat_search(ref, v, candidates)
                nifs.flat_mmr_search(ref, v, candidates, limit, 0.5)
            plain, mmr = [], []
            for r in range(a.reps):
                v = q[r % 256]
                t = time.perf_counter()
                nifs.flat_search(ref, v, candidates)
                plain.append(time.perf_counter() - t)
                t = time.perf_counter()
                nifs.flat_mmr_search(ref, v, candidates, limit, 0.5)
                mmr.append(time.perf_counter() - t)
            diff = median(mmr) - median(plain)
            out["lone"].append({"candidates": candidates, "limit": limit, "search_ms": round(median(plain) * 1e3, 4),
                                "mmr_search_ms": round(median(mmr) * 1e3, 4), "mmr_ms": round(diff * 1e3, 4),
                                "mmr_us_per_round": round(diff * 1e6 / (limit + 1), 3)})
            plain, mmr = [], []
            for r in range(3):
                t = time.perf_counter()
                nifs.flat_search_batch(ref, q, candidates)
                plain.append(time.perf_counter() - t)
                t = time.perf_counter()
                nifs.flat_mmr_search_batch(ref, q, candidates, limit, 0.5)
                mmr.append(time.perf_counter() - t)
            diff = min(mmr) - min(plain)
            out["batch_256"].append({"candidates": candidates, "limit": limit, "search_batch_ms": round(min(plain) * 1e3, 3),
                                     "mmr_search_batch_ms": round(min(mmr) * 1e3, 3), "mmr_ms": round(diff * 1e3, 3),
                                     "mmr_us_per_round": round(diff * 1e6 / (limit + 1), 3)})
    # for context only: the restatement on a 1 000-candidate problem over the handle's first rows
    import mmr_ref
    m = min(1000, len(x_keep))
    initial = [(ids[i], float(s)) for i, s in enumerate(rng.uniform(0, 1, size=m))]
    t = time.perf_counter()
    mmr_ref.mmr_rerank(initial, [(ids[i], [float(c) for c in x_keep[i]]) for i in range(m)], "cosine", 0.5, 100)
    out["mmr_ref_seconds"] = {"candidates": m, "limit": 100, "seconds": round(time.perf_counter() - t, 3)}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
