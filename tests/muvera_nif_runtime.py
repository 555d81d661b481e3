"""tests/nif_runtime.py over a term runtime whose atoms are interned (tests/stubs/erl_nif_fake_interned.c): the
MUVERA NIFs take `nil | integer` as their last argument, and the shim recognises nil the way NIFs do on the BEAM --
by the atom's identity --, which the plain fake runtime (a fresh term per enif_make_atom) cannot express.
`None` stands for nil.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import nif_runtime as base
from nif_runtime import ArgumentError, Atom  # noqa: F401

INTERNED = os.path.join(base.STUBS, "erl_nif_fake_interned.c")
OUT = os.path.join(base.BUILD, "vettore_gpu_nif_interned.so")


def build():
    srcs = [base.SHIM, base.FAKE, INTERNED, os.path.join(base.STUBS, "erl_nif.h"), os.path.join(base.ROOT, "include", "vettore_flat.h")]
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(s) for s in srcs):
        return OUT
    os.makedirs(base.BUILD, exist_ok=True)
    cmd = ["cc", "-std=c11", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I" + base.STUBS,
           "-I" + os.path.join(base.ROOT, "include"), base.SHIM, INTERNED, "-L" + base.LIBDIR, "-lvettore_hip",
           "-Wl,-rpath," + base.LIBDIR, "-o", OUT]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return OUT


class Runtime(base.Runtime):
    def __init__(self):
        saved, base.build = base.build, build
        try:
            super().__init__()
        finally:
            base.build = saved
        self.L.fake_atom_interned.restype = C.c_void_p
        self.L.fake_atom_interned.argtypes = [C.c_char_p]

    def to_term(self, env, v):
        if v is None:
            return self.L.fake_atom_interned(b"nil")
        if isinstance(v, Atom):
            return self.L.fake_atom_interned(str(v).encode())
        if isinstance(v, bool):
            return self.L.fake_atom_interned(b"true" if v else b"false")
        return super().to_term(env, v)
