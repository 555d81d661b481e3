"""Python mirror of `Vettore.Encoding.Muvera` (lib/vettore/encoding/muvera.ex): MUVERA fixed-dimensional
encodings of multi-vector queries and documents, encoded on the GPU (vt_muvera_encode).

    encode_query(vectors, **config)      -> ("ok", [float]) | ("error", atom)
    encode_document(vectors, **config)   -> the same, averaging instead of summing
    encode_documents(sets, **config)     -> ("ok", (matrix, [atom or None per set])) | ("error", atom)   (extension)

Defaults, validation order and error atoms (as strings) are muvera.ex:42-51 and :83-105.  A configuration may
also be given as a list of (key, value) pairs -- an Elixir keyword list, where a repeated or unknown key is
"invalid_config".
"""
from __future__ import annotations

import math

from . import nifs

MAX_OUTPUT_DIMENSIONS = 16_777_216
U64_MAX = (1 << 64) - 1
F32_MAX = 3.4028234663852886e38
CONFIG_KEYS = ("dimension", "num_repetitions", "num_simhash_projections", "seed", "projection_dimension",
               "final_projection_dimension")
_MISSING = object()


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _positive(v):
    return _is_int(v) and v > 0


def _keyword(config):
    """muvera.ex:175-183 validate_keyword -> dict, or None for "invalid_config"."""
    if isinstance(config, dict):
        pairs = list(config.items())
    elif isinstance(config, (list, tuple)):
        pairs = list(config)
        if not all(isinstance(p, tuple) and len(p) == 2 and isinstance(p[0], str) for p in pairs):
            return None
    else:
        return None
    keys = [k for k, _ in pairs]
    if any(k not in CONFIG_KEYS for k in keys) or len(keys) != len(set(keys)):
        return None
    return dict(pairs)


def _finite_f32(v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return False
    return not (isinstance(v, float) and math.isnan(v)) and -F32_MAX <= v <= F32_MAX


def _prepare_vectors(vectors):
    """muvera.ex:153-173 -> (vectors as floats, dimension) or an atom."""
    if len(vectors) == 0:
        return "empty_vectors"
    first = vectors[0]
    if not isinstance(first, (list, tuple)) or len(first) == 0:
        return "invalid_vectors"
    dimension = len(first)
    if not all(isinstance(v, (list, tuple)) and len(v) == dimension for v in vectors):
        return "dimension_mismatch"
    if not all(_finite_f32(x) for v in vectors for x in v):
        return "invalid_vectors"
    return [[float(x) for x in v] for v in vectors], dimension


def _normalize_config(config, dimension):
    """muvera.ex:83-105 -> dict or an atom."""
    n = {
        "dimension": config.get("dimension", dimension),
        "num_repetitions": config.get("num_repetitions", 1),
        "num_simhash_projections": config.get("num_simhash_projections", 0),
        "seed": config.get("seed", 1),
        "projection_dimension": config.get("projection_dimension", dimension),
        "final_projection_dimension": config.get("final_projection_dimension"),
    }
    if not _is_int(n["dimension"]):
        return "invalid_dimension"
    if n["dimension"] != dimension:
        return "dimension_mismatch"
    if not _positive(n["num_repetitions"]):
        return "invalid_repetitions"
    if not (_is_int(n["num_simhash_projections"]) and 0 <= n["num_simhash_projections"] < 31):
        return "invalid_simhash_projections"
    if not (_is_int(n["seed"]) and 0 <= n["seed"] <= U64_MAX):
        return "invalid_seed"
    if not _positive(n["projection_dimension"]):
        return "invalid_projection_dimension"
    if n["final_projection_dimension"] is not None and not _positive(n["final_projection_dimension"]):
        return "invalid_final_projection_dimension"
    full = n["num_repetitions"] * (1 << n["num_simhash_projections"]) * n["projection_dimension"]
    if max(full, n["final_projection_dimension"] or full) > MAX_OUTPUT_DIMENSIONS:
        return "encoding_too_large"
    return n


def _native_error(reason):
    """muvera.ex:79-81: the native "encoding overflow" as an atom, anything else as it came."""
    return "encoding_overflow" if reason == "encoding overflow" else reason


def _args(n):
    return (n["dimension"], n["num_repetitions"], n["num_simhash_projections"], n["seed"], n["projection_dimension"],
            n["final_projection_dimension"])


def _encode(vectors, config, native):
    if not isinstance(vectors, (list, tuple)) or not isinstance(config, (dict, list, tuple)):
        return ("error", "invalid_vectors")
    config = _keyword(config)
    if config is None:
        return ("error", "invalid_config")
    prepared = _prepare_vectors(vectors)
    if isinstance(prepared, str):
        return ("error", prepared)
    vectors, dimension = prepared
    n = _normalize_config(config, dimension)
    if isinstance(n, str):
        return ("error", n)
    status, value = native(vectors, *_args(n))
    return (status, value) if status == "ok" else ("error", _native_error(value))


def encode_query(vectors, config=_MISSING, **kwargs):
    """Query side: per partition the sum of the projected vectors (muvera.ex:31-32)."""
    return _encode(vectors, kwargs if config is _MISSING else config, nifs.muvera_encode_query)


def encode_document(vectors, config=_MISSING, **kwargs):
    """Document side: per partition the running average of the projected vectors (muvera.ex:37-38)."""
    return _encode(vectors, kwargs if config is _MISSING else config, nifs.muvera_encode_document)


def encode_documents(sets, config=_MISSING, **kwargs):
    """Extension: many documents under one configuration in one native call.  Every set is prepared as
    encode_document prepares it; the configuration's dimension defaults to the first well-formed set's.
    ("ok", (float32 matrix [count][fde], [None or the set's atom])) -- a refused set keeps a zero row."""
    config = _keyword(kwargs if config is _MISSING else config)
    if not isinstance(sets, (list, tuple)):
        return ("error", "invalid_vectors")
    if config is None:
        return ("error", "invalid_config")
    prepared = [_prepare_vectors(s) if isinstance(s, (list, tuple)) else "invalid_vectors" for s in sets]
    dimension = next((p[1] for p in prepared if not isinstance(p, str)), config.get("dimension", 1))
    n = _normalize_config(config, dimension)
    if isinstance(n, str):
        return ("error", n)
    # a set the Elixir layer would refuse never reaches the native call: it goes in as an empty set and keeps its atom
    atoms = [p if isinstance(p, str) else ("dimension_mismatch" if p[1] != dimension else None) for p in prepared]
    native_sets = [[] if a is not None else p[0] for a, p in zip(atoms, prepared)]
    status, value = nifs.muvera_encode_batch(native_sets, nifs.MUVERA_DOCUMENT, *_args(n))
    if status != "ok":
        return ("error", _native_error(value))
    matrix, reasons = value
    return ("ok", (matrix, [a if a is not None else (None if r is None else _native_error(r)) for a, r in zip(atoms, reasons)]))
