"""tests/mmr_ref.py pinned to the reference's own expectations (tests/golden/mmr_ex.json: its doctests and ExUnit
assertions about mmr_rerank/5 and rerank/4), and to three properties the GPU path is held to through it: the score is
never fused, a round that never runs raises nothing, the last lone candidate's round still does.  CPU only."""
import math
from fractions import Fraction

import pytest

import mmr_ref
from support import load

GOLD = load("mmr_ex.json")


def _entries(entries):
    """A fixture list as the terms it stands for: [id, x] pairs are tuples, a bare string in their place an atom."""
    return [tuple(x) if isinstance(x, list) else x for x in entries]


def _expect(e):
    if e[0] == "ok":
        return ("ok", [tuple(x) for x in e[1]])
    return ("error", tuple(e[1]) if isinstance(e[1], list) else e[1])


@pytest.mark.parametrize("case", GOLD["cases"], ids=[c["source"].split(" (")[0] + "#%d" % i for i, c in enumerate(GOLD["cases"])])
def test_reference_expectations(case):
    got = mmr_ref.mmr_rerank(_entries(case["initial"]), _entries(case["embeddings"]), case["metric"], case["alpha"],
                             case["final_k"])
    assert got == _expect(case["expect"]), case["source"]


def test_fixture_covers_what_the_reference_asserts():
    assert GOLD["max_f32"] == mmr_ref.F32_MAX
    assert len(GOLD["cases"]) == 25
    metrics = {c["metric"] for c in GOLD["cases"] if c["source"].startswith("test/vector_algorithms_hardening_test.exs:188")}
    assert metrics == set(mmr_ref.SIMILARITY_METRICS) | set(mmr_ref.DISTANCE_METRICS)


def test_validation_order():
    ok_i, ok_e = [("a", 1.0)], [("a", [1.0])]
    # the guards come before the metric, the metric before the embeddings, the embeddings before the initial list
    assert mmr_ref.mmr_rerank(ok_i, ok_e, "nope", 1.5, 1) == mmr_ref.INVALID
    assert mmr_ref.mmr_rerank(ok_i, ok_e, "nope", 0.5, 0) == mmr_ref.INVALID
    assert mmr_ref.mmr_rerank(ok_i, ok_e, "nope", 0.5, 1.0) == mmr_ref.INVALID
    assert mmr_ref.mmr_rerank(ok_i, ok_e, "nope", True, 1) == mmr_ref.INVALID
    assert mmr_ref.mmr_rerank(ok_i, ok_e, "nope", float("nan"), 1) == mmr_ref.INVALID
    assert mmr_ref.mmr_rerank("a", ok_e, "nope", 0.5, 1) == mmr_ref.INVALID
    assert mmr_ref.mmr_rerank(ok_i, [("a", [])], "nope", 0.5, 1) == ("error", ("unknown_metric", "nope"))
    assert mmr_ref.mmr_rerank([("zz", 1.0)], [("a", [])], "l2", 0.5, 1) == mmr_ref.INVALID
    for bad in ([("", [1.0])], [("a", [1.0]), ("b", [1.0, 2.0])], [("a", [float("inf")])], [("a", [float("nan")])],
                [("a", [4e38])], [("a", [True])], [("a", (1.0,))], [(1, [1.0])], [("a", [1.0], 1)]):
        assert mmr_ref.mmr_rerank(ok_i, bad, "l2", 0.5, 1) == mmr_ref.INVALID, bad
    for bad in ([("", 1.0)], [("a", float("inf"))], [("a", float("nan"))], [("a", 4e38)], [("a", None)], [("b", 1.0)],
                [("a", 1.0), ("a", 1.0)], [("a",)]):
        assert mmr_ref.mmr_rerank(bad, ok_e, "l2", 0.5, 1) == mmr_ref.INVALID, bad
    # integers are numbers: as scores, as alpha, as coordinates
    assert mmr_ref.mmr_rerank([("a", 3), ("b", 2)], [("a", [1, 0]), ("b", [0, 1])], "l2", 1, 5) == ("ok", [("a", 3), ("b", 2)])
    assert mmr_ref.mmr_rerank([("a", 3), ("b", 2)], [("a", [1, 0]), ("b", [0, 1])], "l2", 0, 1) == ("ok", [("a", 3)])


def test_first_maximum_wins_and_scores_are_the_callers():
    rows = [("a", [1.0, 0.0]), ("b", [1.0, 0.0]), ("c", [1.0, 0.0])]
    initial = [("c", 0.5), ("a", 0.5), ("b", 0.5)]
    assert mmr_ref.mmr_rerank(initial, rows, "cosine", 0.5, 3) == ("ok", initial)
    assert mmr_ref.order_of(initial, rows, "cosine", 0.5, 2) == ("ok", [0, 1])
    # a zero vector's cosine is 0.0, not an error
    assert mmr_ref.pair_similarity("cosine", [0.0, 0.0], [1.0, 0.0]) == ("ok", 0.0)


# One case in which fusing alpha * s - (1 - alpha) * r into an FMA -- either product into the subtraction -- changes the
# selection.  Found with exact rational arithmetic (search_fma_case: fractions.Fraction, rounded to double where the
# hardware would round), kept here: after "a" = (1, 0) is chosen, "b" = (3, 4) has the f32 cosine 0.6 to it and a score
# that nearly cancels its penalty, "c" = (0, 1) has the cosine 0.0, so its MMR score is alpha * s exactly however it is
# computed.  c's score sits between b's thrice-rounded score and both of its once-less-rounded ones.
FMA_ALPHA = 0.3
FMA_ROWS = {"a": [1.0, 0.0], "b": [3.0, 4.0], "c": [0.0, 1.0]}
FMA_SCORES = {"a": 10.0, "b": 1.4062500018626451, "c": 0.006249946231643271}


def _three_ways(alpha, s, r):
    """alpha * s - (1 - alpha) * r as the reference rounds it, and with each product in turn fused into the subtraction."""
    beta = 1.0 - alpha
    p, q = alpha * s, beta * r
    unfused = p - q
    fused_left = float(Fraction(alpha) * Fraction(s) - Fraction(q))   # fma(alpha, s, -q)
    fused_right = float(Fraction(p) - Fraction(beta) * Fraction(r))   # fma(-beta, r, p)
    return unfused, fused_left, fused_right


def search_fma_case(alpha=FMA_ALPHA):
    r = mmr_ref.pair_similarity("cosine", FMA_ROWS["b"], FMA_ROWS["a"])[1]
    for i in range(1, 2000):
        s_b = 1.40625 + i * 2.0 ** -30  # alpha * s_b close to (1 - alpha) * r: the subtraction cancels, one rounding shows
        u, fl, fr = _three_ways(alpha, s_b, r)
        if not ((fl < u and fr < u) or (fl > u and fr > u)):
            continue
        lo, hi = (max(fl, fr), u) if fl < u else (u, min(fl, fr))
        mid = ((lo + hi) / 2) / alpha
        for j in range(-8, 9):
            s_c = mid
            for _ in range(abs(j)):
                s_c = math.nextafter(s_c, math.inf if j > 0 else -math.inf)
            if lo < alpha * s_c < hi:
                return s_b, s_c
    return None


def test_fusing_the_score_would_change_the_selection():
    assert search_fma_case() == (FMA_SCORES["b"], FMA_SCORES["c"])  # (the inputs kept above are what the search finds)
    alpha = FMA_ALPHA
    initial = [(k, FMA_SCORES[k]) for k in "abc"]
    rows = [(k, FMA_ROWS[k]) for k in "abc"]
    r_b = mmr_ref.pair_similarity("cosine", FMA_ROWS["b"], FMA_ROWS["a"])[1]
    r_c = mmr_ref.pair_similarity("cosine", FMA_ROWS["c"], FMA_ROWS["a"])[1]
    assert r_c == 0.0
    u_b, fl_b, fr_b = _three_ways(alpha, FMA_SCORES["b"], r_b)
    u_c, fl_c, fr_c = _three_ways(alpha, FMA_SCORES["c"], r_c)
    assert u_c == fl_c == fr_c
    # the reference chooses c in the second round; a kernel that fuses either way chooses b
    assert u_b < u_c and fl_b > u_c and fr_b > u_c
    assert mmr_ref.mmr_score(alpha, FMA_SCORES["b"], r_b) == u_b
    assert mmr_ref.mmr_rerank(initial, rows, "cosine", alpha, 2) == ("ok", [initial[0], initial[2]])
    assert mmr_ref.order_of(initial, rows, "cosine", alpha, 3) == ("ok", [0, 2, 1])


MAXF = mmr_ref.F32_MAX


def test_an_overflow_surfaces_only_in_a_round_that_runs():
    # a, then b: the pair (c, b) overflows under l2_squared, (c, a) and (b, a) do not
    rows = [("a", [0.0]), ("b", [1.5e19]), ("c", [-1.5e19])]
    initial = [("a", 3.0), ("b", 2.0), ("c", 1.0)]
    assert mmr_ref.pair_similarity("l2_squared", rows[2][1], rows[1][1]) == ("error", "metric_overflow")
    assert mmr_ref.pair_similarity("l2_squared", rows[1][1], rows[0][1])[0] == "ok"
    assert mmr_ref.pair_similarity("l2_squared", rows[2][1], rows[0][1])[0] == "ok"
    # final_k = 2: rounds 0 and 1 run, the pair (c, b) belongs to round 2, which never does
    assert mmr_ref.mmr_rerank(initial, rows, "l2_squared", 1.0, 2) == ("ok", [("a", 3.0), ("b", 2.0)])
    assert mmr_ref.mmr_rerank(initial, rows, "l2_squared", 1.0, 1) == ("ok", [("a", 3.0)])
    # final_k >= n: the last, lone candidate is still scored against the chosen, and fails the call with two results chosen
    assert mmr_ref.mmr_rerank(initial, rows, "l2_squared", 1.0, 3) == ("error", "metric_overflow")
    assert mmr_ref.mmr_rerank(initial, rows, "l2_squared", 1.0, 8) == ("error", "metric_overflow")
    # an f32 chain that overflows while the f64 recovery is representable is no error
    big = [("a", [3.0e38, 3.0e38]), ("b", [-3.0e38, 3.0e38])]
    assert mmr_ref.pair_similarity("manhattan", big[0][1], big[1][1])[0] == "error"
    half = [("a", [2.0e38, 0.0, 2.0e38]), ("b", [-1.0e38, 0.0, 1.0e38])]
    assert mmr_ref.pair_similarity("l2", half[0][1], half[1][1])[0] == "ok"
    assert mmr_ref.mmr_rerank([("a", 1.0), ("b", 0.5)], half, "l2", 0.5, 2) == ("ok", [("a", 1.0), ("b", 0.5)])
