"""Batched search of the resident multi-vector store (vt_mv_top_k_batch, vt_mv_top_k_ids_batch, vt_mv_counters) without a
GPU: the new entry points are declared, exported and bound and refuse NULL arguments; and the planner that packs query
sets into K9rb's panels (vettore_amd/csrc/host/vt_mvbatch.h) -- plain C++ with no HIP call in it -- is built into a
stand-alone program with AddressSanitizer and UBSan (tests/mvbatch_check.cpp) and checked against a Python model over a
few thousand random batches."""
import ctypes as C
import os
import random
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vt_mv_top_k_batch", "vt_mv_top_k_ids_batch", "vt_mv_counters"]
FIRST, LAST = 1 << 8, 1 << 9


def test_every_new_name_is_declared_exported_and_bound():
    import vettore_amd._lib as L
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vettore_flat.h")).read(), flags=re.S)
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in L.SYMBOLS, name
    assert lib.vt_abi_version() == 4
    from vettore_amd import nifs
    from vettore_amd.collection import Collection
    from vettore_amd.mv_store import ResidentMultiVector
    for owner, names in ((nifs, ("mv_top_k_batch", "mv_top_k_ids_batch", "mv_counters")),
                         (ResidentMultiVector, ("top_k_batch", "top_k_ids_batch", "counters")),
                         (Collection, ("multi_vector_search_batch",))):
        for name in names:
            assert callable(getattr(owner, name)), name


def test_null_arguments():
    """Without a device no store can be made, so here the store is always NULL and the other arguments vary around it;
    a NULL `out` or offset array beside a real store is refused in tests/test_gpu_mv_batch.py
    (test_errors_stay_with_their_set)."""
    import vettore_amd._lib as L
    lib = L.load()
    off = (C.c_size_t * 2)(0, 0)
    one = (C.c_float * 1)(1.0)
    outs = (C.c_void_p * 1)()
    status = (C.c_int * 1)()
    # a NULL store, whatever else is there or missing
    for out in (outs, None):
        for set_off in (off, None):
            for st in (status, None):
                assert lib.vt_mv_top_k_batch(None, 1, set_off, one, off, 3, 1, out, st) == 19
                assert lib.vt_mv_top_k_batch(None, 0, set_off, one, off, 3, 1, out, st) == 19
                assert lib.vt_mv_top_k_ids_batch(None, 1, set_off, b"", off, set_off, one, off, 3, 1, out, st) == 19
    assert lib.vt_mv_top_k_batch(None, 1, off, one, off, 99, 1, outs, status) == 19   # before the metric is decoded
    assert not outs[0]
    assert lib.vt_mv_counters(None, None, None) == 19
    n = C.c_uint64(7)
    assert lib.vt_mv_counters(None, C.byref(n), C.byref(n)) == 19 and n.value == 7


def model_plan(counts, capacity, pass_slots, own_panel):
    """What vt_mvbatch.h promises: (panels, descriptors, single-path sets)."""
    cap_groups = capacity // pass_slots * pass_slots // 8
    panels, desc, single = [], [], []
    for b, c in enumerate(counts):
        ng = -(-c // 8)
        if c == 0 or ng > cap_groups:
            single.append(b)
            continue
        if not panels or own_panel or panels[-1][3] + ng > cap_groups:
            panels.append([b, 0, len(desc), 0])
        panels[-1][1] += 1
        panels[-1][3] += ng
        for g in range(ng):
            live = 8 if g + 1 < ng else c - 8 * g
            desc.append((b, live | (FIRST if g == 0 else 0) | (LAST if g + 1 == ng else 0)))
    return [tuple(p) for p in panels], desc, single


def check_invariants(counts, capacity, pass_slots, own_panel, panels, desc, single):
    cap_groups = capacity // pass_slots * pass_slots // 8
    seen = {}
    at = 0
    for first, sets, desc0, ndesc in panels:
        assert desc0 == at and 1 <= ndesc <= cap_groups and sets >= 1, (panels, capacity)
        assert desc[desc0][0] == first and (not own_panel or sets == 1)
        members = []
        for g in range(desc0, desc0 + ndesc):
            b, info = desc[g]
            if info & FIRST:
                assert b not in seen and (not members or b > members[-1])   # whole sets, in batch order, in one panel only
                seen[b] = []
                members.append(b)
            assert members and b == members[-1]                           # a set's groups are consecutive: no straddling
            seen[b].append(info)
        assert len(members) == sets and desc[desc0 + ndesc - 1][1] & LAST  # the panel ends with a whole set
        at += ndesc
    assert at == len(desc)
    for b, infos in seen.items():                                          # descriptors tile each set in order
        c = counts[b]
        assert len(infos) == -(-c // 8) and sum(i & 0xFF for i in infos) == c
        for g, info in enumerate(infos):
            assert (info & 0xFF) == (8 if g + 1 < len(infos) else c - 8 * g)
            assert bool(info & FIRST) == (g == 0) and bool(info & LAST) == (g + 1 == len(infos))
    assert sorted(list(seen) + single) == list(range(len(counts))) and single == sorted(single)
    for b in single:
        assert counts[b] == 0 or -(-counts[b] // 8) > cap_groups           # only what K9rb cannot take


def test_planner_against_a_model():
    exe = os.path.join(tempfile.mkdtemp(), "mvbatch_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "mvbatch_check.cpp"), "-o", exe])
    rng = random.Random(20261018)
    edge = (0, 1, 7, 8, 9, 33)
    cases = [((0, 1, 7, 8, 9, 33, 8, 1), 96, 32, 0), ((9, 9, 9, 33, 9, 16, 1), 32, 32, 0), ((9, 9, 9, 33, 9, 16, 1), 64, 32, 1),
             ((), 32, 32, 0), ((0,), 8, 8, 0), ((1,) * 300, 1952, 32, 0), ((4294967295, 1), 32, 32, 0), ((5, 5), 0, 32, 0),
             ((5, 5), 31, 32, 0)]
    for _ in range(3000):
        pass_slots = rng.choice((8, 16, 32))
        capacity = pass_slots * rng.choice((1, 1, 2, 3, 7, 61)) + rng.choice((0, 0, 5))   # one pass up to many, not always whole
        n = rng.choice((0, 1, 2, 5, 12, 40))
        counts = tuple(rng.choice(edge) if rng.random() < 0.7 else rng.randrange(0, 2 * capacity + 9) for _ in range(n))
        cases.append((counts, capacity, pass_slots, rng.randrange(2)))
    script = "".join("%d %d %d %d%s\n" % (cap, ps, own, len(cs), "".join(" %d" % c for c in cs)) for cs, cap, ps, own in cases)
    out = subprocess.run([exe], input=script, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-2000:])
    got = out.stdout.strip().split("\n")
    assert got[-1] == "ok" and len(got) == len(cases) + 1
    big = 0
    for line, (counts, capacity, pass_slots, own) in zip(got, cases):
        m = re.fullmatch(r"P((?: \S+)*) D((?: \S+)*) S((?: \S+)*)", line)
        assert m, line
        panels = [tuple(map(int, p.split("/"))) for p in m.group(1).split()]
        desc = [tuple(map(int, p.split("/"))) for p in m.group(2).split()]
        single = [int(p) for p in m.group(3).split()]
        check_invariants(counts, capacity, pass_slots, bool(own), panels, desc, single)
        assert (panels, desc, single) == model_plan(counts, capacity, pass_slots, bool(own)), (counts, capacity, pass_slots, own)
        big += any(c and -(-c // 8) * 8 > capacity for c in counts)
    assert big > 100, "the script hardly ever holds a set larger than a panel"
