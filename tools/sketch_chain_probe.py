#!/usr/bin/env python3
"""tools/sketch_chain_probe.py -- one lone search per sketch tier (K1q, K1s, K1f, K1n through force_sketch /
force_sketch6) and one K1qm batch of four on a small cosine corpus, then one lone K1q search on an L2 corpus: the chains
a `rocprofv3 --kernel-trace` run shows (a tracing run on its own, no counters with it).

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python3 tools/sketch_chain_probe.py
    python3 tools/sketch_chain_probe.py --excerpt DIR/.../t_kernel_trace.csv > chain.txt

The excerpt lists every dispatch in order -- kernel, grid, workgroup, LDS bytes -- and nothing that differs from run to run,
so two builds launch the same chains exactly when their excerpts are equal (profiles/sketch_host/).  The profile counters
the searches leave are printed at the end of a run: which tier served which search."""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def excerpt(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))

    def col(r, *names):
        for n in names:
            if n in r:
                return int(r[n])
        return -1

    print("# pos kernel                                 grid          workgroup   lds_bytes")
    for i, r in enumerate(rows):
        m = re.search(r"(\w+_kernel|__amd_rocclr_\w+)", r["Kernel_Name"])
        name = m.group(1) if m else r["Kernel_Name"][:40]
        grid = "%dx%dx%d" % (col(r, "Grid_Size_X", "Grid_Size"), col(r, "Grid_Size_Y"), col(r, "Grid_Size_Z"))
        wg = "%dx%dx%d" % (col(r, "Workgroup_Size_X", "Workgroup_Size"), col(r, "Workgroup_Size_Y"), col(r, "Workgroup_Size_Z"))
        print("%5d %-38s %-13s %-11s %d" % (i, name, grid, wg, col(r, "LDS_Block_Size", "LDS_Block_Size_v")))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--excerpt":
        return excerpt(sys.argv[2])
    import numpy as np
    from vettore_amd import nifs

    rng = np.random.default_rng(20261020)
    n, d = 20000, 192
    x = rng.uniform(-1, 1, size=(n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    ids = [b"doc-%d" % (i + 1) for i in range(n)]
    qs = rng.uniform(-1, 1, size=(4, d)).astype(np.float32)
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    ref = nifs.flat_new_cosine()
    assert nifs.flat_load_matrix(ref, ids, x) == ("ok", ())
    nifs.flat_set_profiling(ref, True)
    for name, value in (("force_sketch", 1), ("force_sketch6", 1), ("force_sketch6", 2), ("force_sketch6", 3)):  # K1q, K1s, K1f, K1n
        nifs.debug_set(name, value)
        status, hits = nifs.flat_search(ref, qs[0], 10)
        assert status == "ok" and len(hits) == 10, hits
    nifs.debug_set("force_sketch6", 0)
    nifs.debug_set("force_sketch", 2)  # K1qm
    status, batch = nifs.flat_search_batch(ref, qs, 10)
    assert status == "ok" and len(batch) == 4
    prof = nifs.flat_get_profile(ref)
    l2 = nifs.flat_new_l2()
    assert nifs.flat_load_matrix(l2, ids, x) == ("ok", ())
    nifs.flat_set_profiling(l2, True)
    nifs.debug_set("force_sketch", 1)
    status, hits = nifs.flat_search(l2, qs[1], 10)
    assert status == "ok" and len(hits) == 10, hits
    prof_l2 = nifs.flat_get_profile(l2)
    nifs.debug_set("force_sketch", 0)
    keys = ("sketch_launches", "sketch6_launches", "sketch5_launches", "sketch4_launches", "sketch_batch_launches", "sketch_batch_queries",
            "sketch_fallbacks", "sketch6_fallbacks", "sketch5_fallbacks", "sketch4_fallbacks", "sketch_batch_fallbacks")
    print({k: prof[k] for k in keys}, {"l2_sketch_launches": prof_l2["sketch_launches"], "l2_sketch_fallbacks": prof_l2["sketch_fallbacks"]})


if __name__ == "__main__":
    main()
