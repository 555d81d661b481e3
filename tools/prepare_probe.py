#!/usr/bin/env python3
"""tools/prepare_probe.py [--out profiles/prepare_rows.json] [--rows N] [--host-rows N] [--put-rows N] [--dim D]
                          [--parent-collection FILE]

What prepare rows (K14) costs, three measurements in one process, every timed call ending in a device
synchronise, warm-up first, the alternatives alternated, medians of the repeats.  Nothing is asserted.

1. The device form: --rows x --dim f32 rows in HBM, out of place, each mode with and without sign words: ms and
   (bytes read + bytes written) / s, counting every byte the call must move once (rows in, rows out, words out) -- the
   kernel reads the rows more than once (DESIGN says so), that is its business, not the caller's.  Beside it
   vt_device_read_peak of the same run and the ratio.
2. The host form on --host-rows rows: A = vt_prepare_rows(l2, with words) against B = vt_normalize_l2 followed by
   vt_compress_sign_bits, same input, alternated.
3. Collection.put_many of --put-rows embeddings.  With --parent-collection (a copy of the previous commit's
   vettore_amd/collection.py) the same batch also goes through that module, alternated: both run on the library of
   this build, whose vt_normalize_l2 and vt_compress_sign_bits -- all the older put_many calls -- are unchanged.
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("none", "l2", "zscore", "minmax")


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def device_form(a, out):
    import torch
    from vettore_amd import _lib, nifs
    n, d = a.rows, a.dim
    W = (d + 63) // 64
    gen = torch.Generator(device="cuda").manual_seed(14)
    x = torch.randn((n, d), generator=gen, device="cuda", dtype=torch.float32)
    y = torch.empty_like(x)
    words = torch.empty((n, W), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cases = [(m, w) for m in MODES for w in (True, False)]

    def call(mode, with_words):
        res = nifs.prepare_device_rows(mode, n, d, x.data_ptr(), d, y.data_ptr(), d, words.data_ptr() if with_words else 0)
        assert res == ("ok", ()), res

    for c in cases:
        call(*c)
    times = {c: [] for c in cases}
    for _ in range(a.reps):
        for c in cases:   # (interleaved: a drift of the box touches every case alike)
            times[c].append(timed(lambda: call(*c)))
    peak = C.c_double()
    st = _lib.load().vt_device_read_peak(nifs.DEVICE, 1 << 30, 20, C.byref(peak))
    assert st == 0
    rows = []
    for mode, with_words in cases:
        ms = median(times[mode, with_words])
        nbytes = 2 * n * d * 4 + (n * W * 8 if with_words else 0)
        gbps = nbytes / (ms * 1e-3) / 1e9
        rows.append({"mode": mode, "words": with_words, "ms": round(ms, 3), "min_ms": round(min(times[mode, with_words]), 3),
                     "bytes": nbytes, "gb_per_s": round(gbps, 1), "of_read_peak": round(gbps / peak.value, 3)})
    out["device_form"] = {"rows": n, "d": d, "reps": a.reps, "out_of_place": True,
                          "read_peak_gb_per_s": round(peak.value, 1), "cases": rows}
    del x, y, words
    torch.cuda.empty_cache()


def host_form(a, out):
    import numpy as np
    from vettore_amd import _lib, nifs
    L = _lib.load()
    n, d = a.host_rows, a.dim
    W = (d + 63) // 64
    x = np.random.default_rng(15).standard_normal((n, d), dtype=np.float32)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    y_a, w_a = np.empty_like(x), np.empty((n, W), dtype=np.uint64)
    y_b, w_b = np.empty_like(x), np.empty((n, W), dtype=np.uint64)

    def one_call():
        st = L.vt_prepare_rows(nifs.DEVICE, 1, n, d, x.ctypes.data_as(fp), y_a.ctypes.data_as(fp), w_a.ctypes.data_as(up), None)
        assert st == 0

    def two_calls():
        assert L.vt_normalize_l2(nifs.DEVICE, n, d, x.ctypes.data_as(fp), y_b.ctypes.data_as(fp)) == 0
        assert L.vt_compress_sign_bits(nifs.DEVICE, n, d, y_b.ctypes.data_as(fp), w_b.ctypes.data_as(up)) == 0

    for _ in range(2):
        one_call()
        two_calls()
    same = y_a.tobytes() == y_b.tobytes() and w_a.tobytes() == w_b.tobytes()
    ta, tb = [], []
    for _ in range(a.reps):
        ta.append(timed(one_call))
        tb.append(timed(two_calls))
    out["host_form"] = {"rows": n, "d": d, "reps": a.reps, "same_bytes": same,
                        "A_prepare_rows_l2_words_ms": round(median(ta), 2), "A_min_ms": round(min(ta), 2),
                        "B_normalize_l2_then_compress_sign_bits_ms": round(median(tb), 2), "B_min_ms": round(min(tb), 2),
                        "A_over_B": round(median(ta) / median(tb), 3)}


def put_many(a, out):
    import numpy as np
    from vettore_amd import collection as current
    parent = None
    if a.parent_collection:
        spec = importlib.util.spec_from_file_location("vettore_amd._parent_collection", a.parent_collection)
        parent = importlib.util.module_from_spec(spec)
        parent.__package__ = "vettore_amd"
        sys.modules[spec.name] = parent
        spec.loader.exec_module(parent)
    n, d = a.put_rows, a.dim
    x = np.random.default_rng(16).standard_normal((n, d), dtype=np.float32)
    vectors = [[float(v) for v in row] for row in x]

    def run(mod):
        made = mod.Collection.new(dimensions=d, metric="cosine")
        assert made[0] == "ok"
        embs = [mod.Embedding(id="doc%06d" % i, vector=v) for i, v in enumerate(vectors)]
        ms = timed(lambda: made[1].put_many(embs) == "ok" or sys.exit("put_many failed"))
        first = made[1].store[b"doc000000"]
        return ms, (np.asarray(first.vector, dtype=np.float32).tobytes(), first.binary_vector)

    run(current)   # (warm-up: the session's buffers, the index's first slab)
    cur, par, stored = [], [], []
    for _ in range(a.put_reps):
        ms, s = run(current)
        cur.append(ms)
        stored.append(s)
        if parent:
            ms, s = run(parent)
            par.append(ms)
            stored.append(s)
    out["put_many"] = {"rows": n, "d": d, "reps": a.put_reps, "this_commit_ms": round(median(cur), 1),
                       "parent_commit_ms": round(median(par), 1) if par else None,
                       "parent_over_this": round(median(par) / median(cur), 2) if par else None,
                       "same_first_row": all(s == stored[0] for s in stored)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--host-rows", type=int, default=100_000)
    ap.add_argument("--put-rows", type=int, default=10_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--put-reps", type=int, default=3)
    ap.add_argument("--parent-collection", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library: both bring a HIP runtime, torch's must come first)
    out = {"tool": "tools/prepare_probe.py"}
    device_form(a, out)
    host_form(a, out)
    put_many(a, out)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
