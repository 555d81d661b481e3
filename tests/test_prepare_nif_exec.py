"""normalize_zscore/1, normalize_minmax/1 and prepare_rows/2 of the erl_nif shim, EXECUTED on the fake term runtime
(tests/muvera_nif_runtime.py: tests/nif_runtime.py with interned atoms) without a GPU: the table, rustler-style decode failures, and the error shapes that are decided
before a device is needed.  The same NIFs against the real library: tests/test_gpu_prepare_nif.py (-m gpu)."""
import pytest

import muvera_nif_runtime
from nif_runtime import ArgumentError, Atom, ImproperList

OK, ERROR = Atom("ok"), Atom("error")
NON_FINITE = b"vector contains a non-finite value"


@pytest.fixture(scope="module")
def rt():
    return muvera_nif_runtime.Runtime()   # (interned atoms: the shim knows its mode atoms by identity)


def test_the_table_holds_the_three_nifs(rt):
    funcs = rt.functions()
    for name, arity in (("normalize_zscore", 1), ("normalize_minmax", 1), ("prepare_rows", 2)):
        assert (name, arity) in funcs and funcs[name, arity] in (1, 2), name


def test_decode_failures_are_badarg(rt):
    for bad in ([1], [1.0, 2], [Atom("nan")], [1e39], [-1e39], Atom("x"), b"\x00\x00\x80\x3f",
                ImproperList([1.0], 2.0), (1.0, 2.0)):
        for name in ("normalize_zscore", "normalize_minmax"):
            with pytest.raises(ArgumentError):
                rt.call(name, bad)
        with pytest.raises(ArgumentError):
            rt.call("prepare_rows", Atom("l2"), [bad])
        with pytest.raises(ArgumentError):
            rt.call("prepare_rows", Atom("l2"), [[1.0], bad])
    # the mode is one of four atoms
    for mode in (Atom("l1"), Atom("nil"), 1, b"l2", [Atom("l2")]):
        with pytest.raises(ArgumentError):
            rt.call("prepare_rows", mode, [[1.0, 2.0]])
    # the vectors are a proper list of lists of one length
    for vectors in (Atom("x"), [1.0, 2.0], ImproperList([[1.0]], [2.0]), [[1.0, 2.0], [1.0]], [[1.0], [1.0, 2.0]], ([1.0],)):
        with pytest.raises(ArgumentError):
            rt.call("prepare_rows", Atom("zscore"), vectors)


def test_what_is_decided_before_a_device_is_needed(rt):
    """Empty batches and empty vectors are {:ok, ...}; a non-finite value is the reference's error string -- on a box
    without a GPU too, because the host checks every row before it reaches for a device."""
    nan, inf = float("nan"), float("inf")
    for mode in ("none", "l2", "zscore", "minmax"):
        assert rt.call("prepare_rows", Atom(mode), []) == (OK, [])
        assert rt.call("prepare_rows", Atom(mode), [[], []]) == (OK, [([], []), ([], [])])
        assert rt.call("prepare_rows", Atom(mode), [[1.0, 2.0], [3.0, nan]]) == (ERROR, NON_FINITE)
        for poison in (inf, -inf):   # (no such float on the BEAM; a double beyond f32's range does not decode)
            with pytest.raises(ArgumentError):
                rt.call("prepare_rows", Atom(mode), [[1.0, 2.0], [3.0, poison]])
    for name in ("normalize_zscore", "normalize_minmax"):
        assert rt.call(name, []) == (OK, [])                                  # distances.rs:648-649
        assert rt.call(name, [nan]) == (ERROR, NON_FINITE)                    # distances.rs:667-670
        for poison in (inf, -inf):
            with pytest.raises(ArgumentError):
                rt.call(name, [poison])
    assert rt.live_resources() == 0


def test_without_a_device_compute_calls_are_error_tuples_not_crashes(rt):
    import ctypes as C
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = C.CDLL(os.path.join(root, "vettore_amd", "lib", "libvettore_hip.so"))
    if lib.vt_device_count() > 0:
        return   # (a GPU is present: tests/test_gpu_prepare_nif.py runs the same calls for real)
    for call in (("normalize_zscore", [1.0, 2.0, 3.0]), ("normalize_minmax", [2.0, 4.0, 6.0]),
                 ("prepare_rows", Atom("l2"), [[3.0, 4.0]])):
        tag, msg = rt.call(*call)
        assert tag == ERROR and isinstance(msg, bytes) and b"no HIP device" in msg, call
