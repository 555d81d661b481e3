"""Vettore.Distance.mmr_rerank/5 restated (lib/vettore_distance.ex:334-519), function by function, over the CPU oracle's
metrics.  Python floats are Erlang's doubles and Python integers Erlang's; every arithmetic step below is the
reference's, in its order.  TEST INFRASTRUCTURE ONLY: the product never imports it.

Elixir terms as Python values: a binary is `bytes` or `str`, a tuple a `tuple`, a list a `list`, an atom a `str`
("ok", "error", "invalid_mmr_args", ...); a metric is its name.
"""
from __future__ import annotations

import oracle

F32_MAX = 3.4028234663852886e38  # vettore_distance.ex:409

SIMILARITY_METRICS = ("cosine", "inner_product")
DISTANCE_METRICS = ("l2", "l2_squared", "negative_inner_product", "manhattan", "chebyshev", "hamming", "jaccard")

INVALID = ("error", "invalid_mmr_args")


def _is_number(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _is_binary(v) -> bool:
    return isinstance(v, (bytes, str))


def finite_number(value) -> bool:
    """:407-414 -- an integer or float within the f32 range (a NaN compares false both ways)."""
    return _is_number(value) and -F32_MAX <= value <= F32_MAX


def validate_metric(metric):
    """:586-590"""
    if isinstance(metric, str) and (metric in SIMILARITY_METRICS or metric in DISTANCE_METRICS):
        return "ok"
    return ("error", ("unknown_metric", metric))


def validate_mmr_embeddings(embeddings):
    """:347-387"""
    vectors, expected = {}, None
    for embedding in embeddings:
        if not (isinstance(embedding, tuple) and len(embedding) == 2):
            return INVALID
        id_, vector = embedding
        if not (_is_binary(id_) and len(id_) > 0 and isinstance(vector, list) and vector != []):
            return INVALID
        dimensions = len(vector)
        if id_ in vectors:
            return INVALID
        if expected not in (None, dimensions):
            return INVALID
        if not all(finite_number(v) for v in vector):
            return INVALID
        vectors[id_] = vector
        expected = expected or dimensions
    return ("ok", vectors)


def validate_mmr_initial(initial, vectors):
    """:389-405"""
    ids = set()
    for entry in initial:
        if not (isinstance(entry, tuple) and len(entry) == 2 and _is_binary(entry[0]) and len(entry[0]) > 0):
            return INVALID
        id_, score = entry
        if not (finite_number(score) and id_ in vectors and id_ not in ids):
            return INVALID
        ids.add(id_)
    return "ok"


def _native(metric, left, right):
    """native_pair (:639-647): float_vector, the NIF, normalize_native_error."""
    try:
        return ("ok", float(oracle.compute(oracle.METRIC_CODE[metric], [v / 1 for v in left], [v / 1 for v in right],
                                           checked=True)))
    except oracle.OracleError as e:
        return ("error", "metric_overflow" if str(e) == "metric overflow" else str(e))


def _cosine(left, right):
    """cosine/2 with the default normalize: :l2 (:146-152, :628-630) -> normalized_cosine_similarity, distances.rs:160-177"""
    try:
        return ("ok", float(oracle.cosine([v / 1 for v in left], [v / 1 for v in right])))
    except oracle.OracleError as e:
        return ("error", "metric_overflow" if str(e) == "metric overflow" else str(e))


def distance_similarity(res):
    """:516-519"""
    if res[0] == "ok":
        return ("ok", 1.0 / (1.0 + res[1]))
    return res


def pair_similarity(metric, left, right):
    """:489-514"""
    if metric == "cosine":
        return _cosine(left, right)
    if metric == "inner_product":
        return _native(metric, left, right)
    if metric == "negative_inner_product":
        res = _native(metric, left, right)
        return ("ok", -res[1] / 1) if res[0] == "ok" else res
    return distance_similarity(_native(metric, left, right))


def maximum_similarity(maximum, similarity):
    """:485-487 -- erlang:max/2 returns its first argument when the two compare equal"""
    if maximum is None:
        return similarity
    return similarity if similarity > maximum else maximum


def maximum_redundancy(id_, selected, vectors, metric, memo=None):
    """:464-483.  `memo`: pair_similarity is a pure function of the two vectors, and the reference asks for the same
    pair again in every later round; a call may remember its answers (errors included) instead of asking again."""
    if not selected:
        return ("ok", 0.0)
    maximum = None
    for selected_id, _score in selected:
        res = memo.get((id_, selected_id)) if memo is not None else None
        if res is None:
            res = pair_similarity(metric, vectors[id_], vectors[selected_id])
            if memo is not None:
                memo[(id_, selected_id)] = res
        if res[0] != "ok":
            return res
        maximum = maximum_similarity(maximum, res[1])
    return ("ok", maximum)


def mmr_score(alpha, query_score, redundancy):
    """:451 -- two products and a subtraction, each rounded; `/ 1` makes the result a float"""
    return (alpha * query_score - (1.0 - alpha) * redundancy) / 1


def score_mmr_candidates(remaining, selected, vectors, metric, alpha, memo=None):
    """:438-462"""
    scored = []
    for index, candidate in enumerate(remaining):
        id_, query_score = candidate
        res = maximum_redundancy(id_, selected, vectors, metric, memo)
        if res[0] != "ok":
            return res
        scored.append((candidate, index, mmr_score(alpha, query_score, res[1])))
    return ("ok", scored)


def do_mmr(remaining, vectors, metric, alpha, left, selected):
    """:416-436 -- `selected` newest first, as the reference conses it"""
    remaining = list(remaining)
    memo = {}
    while True:
        if left == 0 or not remaining:
            return ("ok", list(reversed(selected)))
        res = score_mmr_candidates(remaining, selected, vectors, metric, alpha, memo)
        if res[0] != "ok":
            return res
        best = None
        for entry in res[1]:  # Enum.max_by keeps the first maximum
            if best is None or entry[2] > best[2]:
                best = entry
        chosen, index, _ = best
        del remaining[index]
        left -= 1
        selected = [chosen] + selected


def mmr_rerank(initial, embeddings, metric, alpha, final_k):
    """:334-345"""
    if not (isinstance(initial, list) and isinstance(embeddings, list) and _is_number(alpha) and 0 <= alpha <= 1
            and isinstance(final_k, int) and not isinstance(final_k, bool) and final_k > 0):
        return INVALID
    res = validate_metric(metric)
    if res != "ok":
        return res
    res = validate_mmr_embeddings(embeddings)
    if res[0] != "ok":
        return res
    vectors = res[1]
    res = validate_mmr_initial(initial, vectors)
    if res != "ok":
        return res
    return do_mmr(initial, vectors, metric, alpha, final_k, [])


def order_of(initial, embeddings, metric, alpha, final_k):
    """What the C ABI answers for the same call: ("ok", indices into `initial` in order of choice) or the error."""
    res = mmr_rerank(initial, embeddings, metric, alpha, final_k)
    if res[0] != "ok":
        return res
    place = {entry[0]: i for i, entry in enumerate(initial)}
    return ("ok", [place[id_] for id_, _ in res[1]])


def order_of_rows(rows, scores, metric, alpha, final_k):
    """order_of for row i <-> entry i (vt_mmr_rerank's shape); rows: [n][d] floats, scores: n numbers."""
    ids = ["%06d" % i for i in range(len(scores))]
    initial = list(zip(ids, scores))
    embeddings = [(ids[i], [float(v) for v in rows[i]]) for i in range(len(ids))]
    return order_of(initial, embeddings, metric, alpha, final_k)
