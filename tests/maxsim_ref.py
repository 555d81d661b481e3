"""MaxSim as the reference composes it (multi_vector.rs:40-160, and its own score_oracle at :172-191): per query
vector the best similarity_value over the document's vectors, the maxima summed in f32 in query order -- built from
the CPU oracle's distances (oracle.compute / oracle.cosine), so a test can hold the device to it bit for bit.  The
lane order of every 8-float chunk is the oracle's (oracle.set_reduce_order): set it to the library's first."""
import numpy as np

import oracle

COSINE, INNER_PRODUCT, NEGATIVE_INNER_PRODUCT = 2, 3, 4


class MaxSimError(Exception):
    """Carries the reference's error string."""


def similarity_value(metric, raw):  # distances.rs:122-128
    raw = np.float32(raw)
    if metric in (COSINE, INNER_PRODUCT):
        return raw
    if metric == NEGATIVE_INNER_PRODUCT:
        return np.float32(-raw)
    return np.float32(np.float32(1.0) / (np.float32(1.0) + raw))


def pair(metric, q, t):
    try:
        raw = oracle.cosine(q, t) if metric == COSINE else oracle.compute(metric, q, t)
    except oracle.OracleError as e:
        raise MaxSimError(str(e))
    return similarity_value(metric, raw)


def score_validated(query, document, metric):  # multi_vector.rs:65-88
    total = np.float32(0.0)
    for q in query:
        best = np.float32(-np.inf)
        for t in document:
            best = max(best, pair(metric, q, t))
        with np.errstate(over="ignore"):
            total = np.float32(total + best)
        if not np.isfinite(total):
            raise MaxSimError("score overflow")
    return total


def _validate(vectors, dim):  # multi_vector.rs:152-160
    for v in vectors:
        if len(v) != dim:
            raise MaxSimError("dimension mismatch")
        if not np.all(np.isfinite(np.asarray(v, dtype=np.float32))):
            raise MaxSimError("vector contains a non-finite value")


def _validate_standalone(vectors):  # multi_vector.rs:142-150
    if not vectors:
        return
    if len(vectors[0]) == 0:
        raise MaxSimError("vectors must not be empty")
    _validate(vectors, len(vectors[0]))


def _decode(metric):
    if not 0 <= metric <= 8:
        raise MaxSimError("unknown metric")


def score(query, document, metric):  # multi_vector.rs:40-63
    _decode(metric)
    if not query:
        _validate_standalone(document)
        return np.float32(0.0)
    if len(query[0]) == 0:
        raise MaxSimError("vectors must not be empty")
    _validate(query, len(query[0]))
    if not document:
        return np.float32(0.0)
    _validate(document, len(query[0]))
    return score_validated(query, document, metric)


def top_k(documents, query, metric, limit):
    """multi_vector.rs:90-132 as a full sort: [(id bytes, score)] best first, or MaxSimError."""
    _decode(metric)
    _validate_standalone(query)
    scored = []
    for id_, vectors in documents:
        if not query:
            _validate_standalone(vectors)
            s = np.float32(0.0)
        elif not vectors:
            s = np.float32(0.0)
        else:
            _validate(vectors, len(query[0]))
            s = score_validated(query, vectors, metric)
        scored.append((id_.encode() if isinstance(id_, str) else bytes(id_), s))
    scored.sort(key=lambda h: (-float(h[1]), h[0]))  # (no score is NaN or -0.0: the sum starts at +0.0)
    return scored[:limit]
