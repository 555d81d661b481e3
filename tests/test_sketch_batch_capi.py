"""K1qm's surface without a GPU: vt_profile ends with the seven counters of the group passes, in the
header and in the Python mirror alike, and the two settings that route batches take their new values."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vettore_flat.h")
NEW_FIELDS = [("sketch_batch_launches", C.c_uint64), ("sketch_batch_queries", C.c_uint64), ("sketch_batch_ms", C.c_double),
              ("sketch_batch_bytes", C.c_uint64), ("sketch_batch_candidates", C.c_uint64),
              ("sketch_batch_fallbacks", C.c_uint64), ("sketch_batch_tail_rescored", C.c_uint64)]


@pytest.fixture(scope="module")
def lib():
    import vettore_amd._lib as L
    return L.load()


def header_profile_fields():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct vt_profile \{(.*?)\} vt_profile;", text, flags=re.S) or \
        re.search(r"typedef struct\s*\{([^{}]*?)\} vt_profile;", text, flags=re.S)
    assert body, "include/vettore_flat.h has no vt_profile"
    return re.findall(r"\b(uint64_t|double)\s+([a-z0-9_]+)\s*;", body.group(1))


def test_the_profile_ends_with_the_group_counters():
    import vettore_amd._lib as L
    fields = list(L.Profile._fields_)
    assert fields[-len(NEW_FIELDS):] == NEW_FIELDS, fields[-len(NEW_FIELDS):]
    # ... behind everything an older binding knows: vt_flat_get_profile_sized copies a prefix
    assert fields[-len(NEW_FIELDS) - 1][0] == "sketch4_finished"
    # the mirror is the header's struct, field for field
    ctype = {"uint64_t": C.c_uint64, "double": C.c_double}
    assert [(name, ctype[t]) for t, name in header_profile_fields()] == fields
    assert all(C.sizeof(t) == 8 for _, t in fields) and C.sizeof(L.Profile) == 8 * len(fields)


def test_the_binding_reports_the_group_counters():
    """(flat_get_profile builds its dict from the mirror's fields: a search's counters come back under these names.)"""
    import vettore_amd._lib as L
    names = [n for n, _ in L.Profile._fields_]
    for name, _ in NEW_FIELDS:
        assert names.count(name) == 1, name
    for lone in ("sketch_launches", "sketch_ms", "sketch_bytes", "sketch_candidates", "sketch_fallbacks", "sketch_tail_rescored"):
        assert names.index(lone) < names.index("sketch_batch_launches"), lone


def test_the_two_settings_take_their_new_values(lib):
    v = C.c_long(-1)
    for name, default in ((b"force_sketch", 0), (b"sketch", 1)):
        assert lib.vt_debug_get(name, C.byref(v)) == 0 and v.value == default, (name, v.value)
        try:
            for value in (2, 1, 0, 2):
                assert lib.vt_debug_set(name, value) == 0, (name, value)
                assert lib.vt_debug_get(name, C.byref(v)) == 0 and v.value == value, (name, value, v.value)
        finally:
            assert lib.vt_debug_set(name, default) == 0
    # what the values mean is written where the settings are declared (tools/env_table.py copies it into DESIGN_APPENDIX A.10)
    env_h = open(os.path.join(ROOT, "vettore_amd", "csrc", "vt_env.h")).read()
    for name in ("sketch", "force_sketch"):
        line = next(ln for ln in env_h.splitlines() if '"%s"' % name in ln)
        assert "`2`" in line and "K1qm" in line, line
