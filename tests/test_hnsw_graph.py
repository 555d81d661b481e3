"""The host graph of the HNSW index (vettore_amd/csrc/host/vt_hnswgraph.h: plain C++ with no HIP call in it) built into
a stand-alone program with AddressSanitizer and UBSan (tests/hnswgraph_check.cpp) and fed what the device hands it: the
per-layer result lists of every insert of the restatement (tests/hnsw_ref.py), in shuffled order, with its deletes and
upserts.  After every step levels, entry and every adjacency list must be the restatement's -- although the header
prunes with the distances it kept and the restatement recomputes and sorts.  CPU only."""
import os
import random
import struct
import subprocess
import tempfile

import numpy as np

from hnsw_ref import L2, HnswIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(ref):
    parts = ["%d %d %d %d" % (ref.next, -1 if ref.entry is None else ref.entry,
                              -1 if ref.dimension is None else ref.dimension, len(ref.nodes))]
    for nid in sorted(ref.nodes):
        node = ref.nodes[nid]
        parts.append("|%d:%d;%s" % (nid, node.layer, ";".join(",".join(map(str, l)) for l in node.connections)))
    return " ".join(parts)


def insert_line(ref, rng, ext, vector):
    ref.insert(ext, vector)
    layers = (max(ref.last_lists) + 1) if ref.last_lists else 0
    words = ["I", ext.hex() or "-", str(len(vector)), str(layers)]
    for layer in range(layers):
        lst = list(ref.last_lists.get(layer, []))
        rng.shuffle(lst)
        words.append(str(len(lst)))
        for nid, dist in lst:
            words += [str(nid), struct.pack("<f", dist)[::-1].hex()]
    return " ".join(words)


def test_graph_header_follows_the_restatement_step_by_step():
    exe = os.path.join(tempfile.mkdtemp(), "hnswgraph_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "hnswgraph_check.cpp"), "-o", exe])
    rng = random.Random(20261018)
    nprng = np.random.default_rng(7)
    # tie-heavy: integer coordinates in -3..3; ids whose byte order differs from insertion order
    ref = HnswIndex(L2, m=4, m0=8, ef_construction=40, ef_search=16, max_level=12)
    script, expected = ["P 4 8 12"], []
    live = []
    for step in range(600):
        ext = b"n%d" % ((step * 7919) % 1000)
        script.append(insert_line(ref, rng, ext, nprng.integers(-3, 4, 16).astype(np.float32)))
        expected.append(dump(ref))
        live.append(ext)
        if step % 9 == 8:  # an upsert of a live id
            ext = rng.choice(live)
            script.append(insert_line(ref, rng, ext, nprng.integers(-3, 4, 16).astype(np.float32)))
            expected.append(dump(ref))
        if step % 13 == 12:  # a delete; now and then the entry itself
            ext = ref.nodes[ref.entry].external_id if step % 39 == 38 else rng.choice(live)
            live.remove(ext)
            ref.delete(ext)
            script.append("D " + ext.hex())
            expected.append(dump(ref))
    levels = [n.layer for n in ref.nodes.values()]
    assert max(levels) >= 3 and sum(1 for l in levels if l > 0) >= 100, (max(levels), sum(1 for l in levels if l > 0))
    # everything goes, one node comes back with another dimension: ids keep counting
    for ext in list(live):
        ref.delete(ext)
        script.append("D " + ext.hex())
        expected.append(dump(ref))
    assert ref.dimension is None
    script.append(insert_line(ref, rng, b"", np.float32([1.0, 2.0, 3.0])))
    expected.append(dump(ref))
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.splitlines()
    assert len(got) == len(expected)
    for i, (g, e) in enumerate(zip(got, expected)):
        assert g == e, "step %d (%s)" % (i, script[i + 1][:60])
