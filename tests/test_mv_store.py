"""The resident multi-vector store (vt_mv_*, include/vettore_flat.h) without a GPU: the new entry points are declared,
exported and bound; they refuse NULL handles and a machine without a device; and the store's slot table
(vettore_amd/csrc/host/vt_mvstore.h) -- plain C++ with no HIP call in it -- is built into a stand-alone program with
AddressSanitizer and UBSan (tests/mvstore_check.cpp) and driven against a Python dict over a few thousand random puts,
upserts and deletes."""
import ctypes as C
import os
import random
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vt_mv_new", "vt_mv_free", "vt_mv_put_many", "vt_mv_delete", "vt_mv_len", "vt_mv_dimension", "vt_mv_top_k",
         "vt_mv_top_k_ids", "vt_mv_memory"]


def test_every_new_name_is_declared_exported_and_bound():
    import vettore_amd._lib as L
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vettore_flat.h")).read(), flags=re.S)
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in L.SYMBOLS, name
    assert lib.vt_abi_version() == 4


def test_null_handles_and_a_machine_without_a_device():
    import vettore_amd._lib as L
    lib = L.load()
    off = (C.c_size_t * 2)(0, 0)
    one = (C.c_float * 1)(1.0)
    out = C.c_void_p()
    assert lib.vt_mv_put_many(None, 1, b"", off, off, one, off) == 19
    assert lib.vt_mv_delete(None, b"x", 1) == 19
    assert lib.vt_mv_top_k(None, one, off, 0, 3, 1, C.byref(out)) == 19
    assert lib.vt_mv_top_k_ids(None, 0, b"", off, one, off, 0, 3, 1, C.byref(out)) == 19
    assert lib.vt_mv_memory(None, None, None, None, None, None) == 19
    assert lib.vt_mv_new(0, None) == 19
    assert lib.vt_mv_len(None) == 0 and lib.vt_mv_dimension(None) == -1
    lib.vt_mv_free(None)
    h = C.c_void_p()
    st = lib.vt_mv_new(0, C.byref(h))
    if lib.vt_device_count() == 0:
        assert st == 17 and not h.value                     # VT_ERR_DEVICE: no CPU fallback
        assert b"no CPU fallback" in lib.vt_last_error()
    else:
        assert st == 0 and h.value
        assert lib.vt_mv_len(h) == 0 and lib.vt_mv_dimension(h) == -1
        lib.vt_mv_free(h)


class Model:
    """What vt_mvstore.h promises, over a dict in insertion order (= the order of the last put)."""
    FIRST_ROWS = 4096

    def __init__(self, compactions=0):
        self.docs = {}
        self.used = self.dead = self.cap = 0
        self.compactions = compactions                      # (the handle's counter never goes back)

    def live_rows(self):
        return sum(self.docs.values())

    def settle(self):
        if self.used and self.live_rows() == 0:
            self.used = self.dead = self.cap = 0

    def put(self, docs):
        last = {i: k for k, (i, _) in enumerate(docs)}
        take = [(i, r) for k, (i, r) in enumerate(docs) if last[i] == k]
        if self.dead > self.used - self.dead:               # a put that finds more dead rows than live ones compacts first
            self.used, self.dead = self.used - self.dead, 0
            self.compactions += 1
        need = self.used + sum(r for _, r in take)
        if need > self.cap:
            self.cap = self.cap or self.FIRST_ROWS
            while self.cap < need:
                self.cap *= 2
        for i, r in take:
            if i in self.docs:
                self.dead += self.docs.pop(i)
            self.docs[i] = r
        self.used = need
        self.settle()

    def delete(self, i):
        if i in self.docs:
            self.dead += self.docs.pop(i)
            self.settle()

    def state(self):
        rank = {i: k for k, i in enumerate(sorted(self.docs, key=lambda s: s.encode()))}
        head = "len=%d dim=%d used=%d dead=%d cap=%d compactions=%d :" % (
            len(self.docs), 8 if self.live_rows() else -1, self.used, self.dead, self.cap, self.compactions)
        return head + "".join(" %s/%d/%d" % (i, r, rank[i]) for i, r in self.docs.items())


def test_slot_table_against_a_dict_model():
    exe = os.path.join(tempfile.mkdtemp(), "mvstore_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "mvstore_check.cpp"), "-o", exe])
    rng = random.Random(20261017)
    script, want = [], []
    compactions = 0
    for round_ in range(4):
        model = Model(compactions)
        universe = ["d%d" % i for i in range((12, 60, 300, 40)[round_])] + ["d", "d1x", "e"]
        big = (40, 200, 900, 3000)[round_]                  # rows per document: growth past 4 096 rows in every round
        for step in range(1500):
            op = rng.random()
            if op < 0.55:
                docs = [(rng.choice(universe), rng.choice((0, 0, 1, 2, rng.randrange(big))))
                        for _ in range(rng.choice((1, 1, 2, 5, 17)))]
                script.append("P %d %s" % (len(docs), " ".join("%s %d" % d for d in docs)))
                model.put(docs)
            else:
                i = rng.choice(universe + ["nobody"])
                script.append("D " + i)
                model.delete(i)
            if step % 7 == 0 or step == 1499:
                script.append("S")
                want.append(model.state())
        for i in list(model.docs):                          # deleting everything forgets rows, slab and dimension
            script.append("D " + i)
            model.delete(i)
        script.append("S")
        want.append(model.state())
        assert model.compactions > compactions + 3, "the script never compacts"
        compactions = model.compactions
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-2000:])
    got = out.stdout.strip().split("\n")
    assert got[-1] == "ok" and len(got) == len(want) + 1
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g[:300], w[:300])
