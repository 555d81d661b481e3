/*
 * erl_nif_fake_interned.c -- the fake term runtime of erl_nif_fake.c with ONE difference: atoms are interned.
 *
 * On the BEAM an atom is an immediate term: enif_make_atom(env, "nil") gives the same ERL_NIF_TERM every time, and
 * NIFs compare atoms with `==` (that is how the shim tells Option's nil from an integer).  erl_nif_fake.c allocates a
 * fresh term per call, which is enough for building results but cannot express that identity.  This file includes it
 * unchanged, with its enif_make_atom renamed, and puts an interning one in front: one term per name, owned by an
 * environment that is never freed.  Test infrastructure only (tests/muvera_nif_runtime.py).
 */
#define enif_make_atom enif_make_atom_fresh
#include "erl_nif_fake.c"
#undef enif_make_atom

ERL_NIF_TERM enif_make_atom(ErlNifEnv *env, const char *name);
ERL_NIF_TERM fake_atom_interned(const char *name);

static ErlNifEnv g_atom_env;
static ERL_NIF_TERM g_atoms[256];
static int g_atom_count;

ERL_NIF_TERM fake_atom_interned(const char *name) {
  for (int i = 0; i < g_atom_count; ++i)
    if (strcmp(T(g_atoms[i])->v.atom, name) == 0) return g_atoms[i];
  if (g_atom_count == 256) abort();
  return g_atoms[g_atom_count++] = enif_make_atom_fresh(&g_atom_env, name);
}

ERL_NIF_TERM enif_make_atom(ErlNifEnv *env, const char *name) {
  (void)env;
  return fake_atom_interned(name);
}
