#!/usr/bin/env python3
"""tools/sketch_batch_bench.py -- small batches on a large corpus, K1qm's group passes against the route a batch takes
without them (profiles/README.md has the commands).

    python tools/sketch_batch_bench.py --rows 10000000 --metric cosine --label this --out profiles/sketch_batch/runs.jsonl
    VETTORE_HIP_LIB=<an older build> python tools/sketch_batch_bench.py ... --label parent --routes today

(`bench.py --mode batch` takes no --dump-outputs and prices config 3's corpus only, so the sweep has a tool of its own; the
corpus is bench.py's -- build_shard, the same seed -- and the queries are its normalized_queries.)

One process, one corpus, every batch size of --batches under each route of --routes:

    today    `sketch = 2`: lone searches read the sketches, batches never do -- what every batch took before K1qm, and all
             an older library knows (the setting is then a no-op);
    groups   `force_sketch = 2`: every batch of two or more with a limit up to 32 shares passes over the int8 sketch,
             whatever the two measured bounds of host/vt_sketchbatch.h say;
    default  no setting: the library's own routing.

--callers N[,N]: bench.py's callers leg (native_callers) on the same corpus with N threads looping on the one handle, the
library routing on its own; one line per N with queries/s and the batches the coalescer formed.

Per (route, batch size): --reps runs of --iters batches, a run's figure the mean wall time of a batch; the routes
alternate inside a repetition.  The hits of the first batch of every size are hashed (ids and raw bits, sha256): equal
digests across routes and builds are byte-for-byte equal dumps.  One JSON line per (route, batch size) to --out."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--metric", choices=["cosine", "l2", "inner_product"], default="cosine")
    ap.add_argument("--limit", type=int, default=10)
    ap.add_argument("--batches", default="2,3,4,8,9,16,24,32")
    ap.add_argument("--routes", default="today,groups")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--label", default="this")
    ap.add_argument("--counters", type=int, default=0, help="with profiling on: this many groups of eight, their counters")
    ap.add_argument("--callers", default="", help="comma-separated caller counts: native threads searching the one handle "
                    "(bench.py's callers leg) for --caller-seconds each, under the library's own routing")
    ap.add_argument("--caller-seconds", type=float, default=2.0)
    ap.add_argument("--sweep", type=int, default=1, help="a tag copied into every line")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import bench
    from vettore_amd import nifs
    device = torch.device("cuda", 0)
    x = bench.build_shard(torch, device, a.rows, a.dim, bench.SEED_CORPUS, normalize=a.metric == "cosine")
    ref = {"cosine": nifs.flat_new_cosine, "l2": nifs.flat_new_l2, "inner_product": nifs.flat_new_inner_product}[a.metric]()
    assert nifs.flat_load_device_matrix(ref, bench.doc_ids(0, a.rows), x.data_ptr(), a.rows, a.dim) == ("ok", ())
    del x
    sizes = [int(v) for v in a.batches.split(",")]
    pool = bench.normalized_queries(4 * max(sizes + [8]), a.dim, 5)
    if a.metric != "cosine":
        pool = (pool * np.float32(3.0)).astype(np.float32)
    routes = [r for r in a.routes.split(",") if r]
    # (which build: the one VETTORE_HIP_LIB names is the older one of a comparison; its path stays out of the record)
    library = "parent commit" if os.environ.get("VETTORE_HIP_LIB") else "this build"

    def take(route):
        nifs.debug_set("sketch", 2 if route == "today" else 1)
        nifs.debug_set("force_sketch", 2 if route == "groups" else 0)

    def batch(b, i):
        s = (i * b) % (len(pool) - b + 1)
        st, lists = nifs.flat_search_batch(ref, pool[s:s + b], a.limit)
        assert st == "ok", lists
        return lists

    def digest(lists):
        h = hashlib.sha256()
        for hits in lists:
            for hit in hits:
                h.update(bytes(hit[0]))
                h.update(np.float32(hit[1]).tobytes())
        return h.hexdigest()

    assert nifs.flat_search(ref, pool[0], a.limit)[0] == "ok"   # (a lone search first: it brings the sketches up to date)
    runs, digests = {}, {}
    for route in routes:
        take(route)
        for b in sizes:   # (untimed: the columns each route reads are built here, and the dumps are taken)
            digests[(route, b)] = digest(batch(b, 0))
            batch(b, 1)
    for rep in range(a.reps):
        for b in sizes:
            for route in routes:
                take(route)
                batch(b, 0)
                t0 = time.perf_counter()
                for i in range(a.iters):
                    batch(b, i)
                runs.setdefault((route, b), []).append((time.perf_counter() - t0) / a.iters * 1e3)
    lines = []
    for (route, b), ms in sorted(runs.items()):
        lines.append({"label": a.label, "library": library, "sweep": a.sweep, "route": route, "rows": a.rows,
                      "dim": a.dim, "metric": a.metric, "limit": a.limit, "batch": b, "iters": a.iters,
                      "ms_per_batch": [round(v, 4) for v in ms], "queries_per_s": [round(b / v * 1e3, 1) for v in ms],
                      "sha256": digests[(route, b)]})
    if a.counters:
        take("groups")
        nifs.flat_set_profiling(ref, True)
        nifs.flat_get_profile(ref, True)
        t0 = time.perf_counter()
        for i in range(a.counters):
            batch(8, i)
        wall = (time.perf_counter() - t0) / a.counters * 1e3
        prof = nifs.flat_get_profile(ref)
        rec = {k: v for k, v in prof.items() if k.startswith("sketch_batch")}
        rec.update(candidates_per_query=round(prof["sketch_batch_candidates"] / max(1, prof["sketch_batch_queries"]), 3),
                   fallback_share=prof["sketch_batch_fallbacks"] / max(1, prof["sketch_batch_queries"]),
                   pass_ms_per_group=round(prof["sketch_batch_ms"] / max(1, prof["sketch_batch_launches"]), 4))
        rec.update(label=a.label, library=library, counters=True, rows=a.rows, dim=a.dim, metric=a.metric, limit=a.limit, groups=a.counters,
                   wall_ms_per_group_with_profiling=round(wall, 4))
        lines.append(rec)
    if a.callers:
        # bench.py's callers leg on this corpus: native threads loop on the handle, the coalescer forms what batches it
        # forms.  The threads' helper library must be the one linked against the library under test: it sits beside it.
        import ctypes as C
        take("default")
        lib_dir = os.path.dirname(os.environ.get("VETTORE_HIP_LIB") or os.path.join(ROOT, "vettore_amd", "lib", "x"))
        bench._CALLERS_LIB = None
        helper = C.CDLL(os.path.join(lib_dir, "libvt_callers.so"))
        helper.vt_callers_run.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_size_t, C.c_size_t, C.c_size_t, C.c_int,
                                          C.c_size_t, C.c_size_t, C.c_int, C.c_double, C.c_int,
                                          C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
        helper.vt_callers_run.restype = C.c_int
        bench._CALLERS_LIB = helper
        from vettore_amd import _lib
        qs = pool[:64]
        for threads in [int(v) for v in a.callers.split(",")]:
            bench.native_callers(a, _lib.load(), nifs, ref, threads, 0.3, qs, 0, 0)   # (untimed: the callers settle)
            res = bench.native_callers(a, _lib.load(), nifs, ref, threads, a.caller_seconds, qs, 0, 0)
            assert res is not None and res["verified"], res
            res.update(label=a.label, library=library, sweep=a.sweep, route="callers", rows=a.rows, dim=a.dim, metric=a.metric,
                       limit=a.limit, queries_per_batch=round(res["searches_in_batches"] / max(1, res["batches"]), 2))
            lines.append(res)
    text = "".join(json.dumps(ln) + "\n" for ln in lines)
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
