"""GPU parity tests for K1qm: batches and meeting callers of 2..8 queries nominated from one pass over the int8 sketch of
the rows (vettore_amd/csrc/vt_sketch_batch.hip, host/vt_sketchbatch.h).

As in tests/test_gpu_sketch.py the sketch is an accelerator and must never show in a result: every list of a batch equals
flat_search of that query alone and the oracle's restatement of flat.rs:96-124, bits included -- for every metric the
sketch serves, group sizes on and off the compiled ones, limits up to the largest the path takes and one past it, a query
that must decline, rows that do not certify, after mutations, when the card "has no room", on a three-shard handle, and
for callers that meet on the handle.  The counters say which path ran: force_sketch = 2 sends batches on these small
corpora where the cost model sends rows of 256 MB and more; tests/test_sketch_batch_model.py shows in the model that the
corpora certify (or, for the spiky one, do not) before anything here relies on it.
"""
import numpy as np
import pytest

import sketch8_l2_ref as refl
import sketch_batch_cases as cases
import support
from test_gpu_parity import GpuIndex, bits, nifs, unwrap  # noqa: F401  (nifs: fixture)

pytestmark = pytest.mark.gpu

L2, L2SQ, COS, IP, NIP = cases.L2, cases.L2SQ, cases.COS, cases.IP, cases.NIP


def loaded(nifs, metric, ids, x, devices=None):
    g = GpuIndex(nifs, metric)
    if devices:
        g.ref = nifs.flat_new_sharded(metric, devices)
    unwrap(nifs.flat_load_matrix(g.ref, ids, x))
    nifs.flat_set_profiling(g.ref, True)
    return g


def moved(nifs, ref, before):
    after = nifs.flat_get_profile(ref)
    return {k: after[k] - before[k] for k in after}


def batch_equals_alone(nifs, ref, qs, k, want, note):
    """One batch; every list equals `want` (the lone answers).  Returns what the batch added to the profile."""
    before = nifs.flat_get_profile(ref)
    got = unwrap(nifs.flat_search_batch(ref, qs, k))
    delta = moved(nifs, ref, before)
    assert len(got) == len(qs)
    for i in range(len(qs)):
        assert bits(got[i]) == want[i], (note, k, len(qs), i)
    return delta


_ORACLE = {}


def oracle_lists(oracle_mod, which, metric, x, ids, qs, k):
    """The oracle's lists for the case's 17 queries, computed once per (corpus, metric, limit)."""
    key = (which, metric, k)
    if key not in _ORACLE:
        packed = oracle_mod.pack_ids(ids)
        _ORACLE[key] = [bits(oracle_mod.matrix_search(metric, x, packed, q, k)) for q in qs]
    return _ORACLE[key]


@pytest.mark.parametrize("which", cases.CORPORA)
@pytest.mark.parametrize("metric", cases.METRICS)
def test_batches_from_the_sketch_equal_searches_alone(nifs, oracle_mod, vt_debug, which, metric):
    """nq in {2, 3, 8, 9, 17} x limits {1, 10, 32}: one group pass per planned group, every query in one, none handed on,
    no lone pass -- and the lists are the lone searches' and the oracle's."""
    vt_debug.set("force_sketch", 2)
    x, ids, qs = cases.case(which, metric)
    g = loaded(nifs, metric, ids, x)
    d = x.shape[1]
    for k in cases.LIMITS:
        want = oracle_lists(oracle_mod, which, metric, x, ids, qs, k)
        alone = [bits(unwrap(nifs.flat_search(g.ref, q, k))) for q in qs]
        assert alone == want, (which, metric, k)
        gmax = cases.max_group(d, cases.list_k(k))
        for nq in cases.NQS:
            delta = batch_equals_alone(nifs, g.ref, qs[:nq], k, want, which)
            what = (which, metric, k, nq, {n: v for n, v in delta.items() if v})
            assert delta["sketch_batch_queries"] == nq, what
            assert delta["sketch_batch_launches"] == len(cases.plan(nq, gmax)), what
            assert delta["sketch_launches"] == 0 and delta["nominate_launches"] == 0, what
            assert delta["sketch_batch_fallbacks"] == 0 and delta["sketch_batch_tail_rescored"] == nq, what
            assert delta["sketch_batch_candidates"] >= nq * min(k, len(x)), what
            tiles = (len(x) + 63) // 64
            assert delta["sketch_batch_bytes"] == delta["sketch_batch_launches"] * tiles * (cases.ld8_of(d) // 16 + 1) * 1024, what
    assert nifs.flat_get_profile(g.ref)["sketch_builds"] == 1


@pytest.mark.parametrize("metric", [COS, L2])
def test_where_the_group_path_is_not_taken(nifs, oracle_mod, vt_debug, metric):
    """Limit 33; force_sketch = 1 (what it always meant: lone searches only); sketch = 2 and sketch = 0 under
    force_sketch = 2: no group pass, the same hits, and lone searches read the sketch or not as the setting says."""
    x, ids, qs = cases.case("uniform", metric)
    g = loaded(nifs, metric, ids, x)
    packed = oracle_mod.pack_ids(ids)
    want33 = [bits(oracle_mod.matrix_search(metric, x, packed, q, 33)) for q in qs[:8]]
    want10 = oracle_lists(oracle_mod, "uniform", metric, x, ids, qs, 10)
    for force, sketch, k, lone_reads in ((2, 1, 33, True), (1, 1, 10, True), (2, 2, 10, True), (2, 0, 10, False)):
        vt_debug.set("force_sketch", force)
        vt_debug.set("sketch", sketch)
        want = want33 if k == 33 else want10
        delta = batch_equals_alone(nifs, g.ref, qs[:8], k, want, (force, sketch))
        assert delta["sketch_batch_launches"] == 0 and delta["sketch_batch_queries"] == 0, (force, sketch, k, delta)
        assert delta["sketch_launches"] == 0, (force, sketch, k)  # (the searches a batch leaves over never read it)
        before = nifs.flat_get_profile(g.ref)
        assert bits(unwrap(nifs.flat_search(g.ref, qs[2], k))) == want[2]
        assert moved(nifs, g.ref, before)["sketch_launches"] == (1 if lone_reads else 0), (force, sketch, k)
    # and with the settings back at force_sketch = 2, sketch = 1 the same handle's batches share passes
    vt_debug.set("force_sketch", 2)
    vt_debug.set("sketch", 1)
    delta = batch_equals_alone(nifs, g.ref, qs[:8], 10, want10, "back")
    assert delta["sketch_batch_launches"] == 1 and delta["sketch_batch_queries"] == 8, delta


@pytest.mark.parametrize("metric", [IP, L2SQ])
def test_a_query_that_must_decline_leaves_its_group(nifs, oracle_mod, vt_debug, metric):
    """Unit rows and one query whose magnitude the lone path's overflow gate turns away (the dot family from
    ||q|| ||x|| >= 2^126, the L2 family from ||q|| + ||x|| >= 2^62): K1's own scan answers it, as it answers the lone call
    -- recovery in f64 included --, and the seven others travel in a group."""
    vt_debug.set("force_sketch", 2)
    n, d = 8000, 96
    x, ids = refl.corpus(n, d, 8400 + metric)
    x = refl.unit(x)
    qs = refl.unit(refl.queries(8401 + metric, x, 8))
    qs[5] = qs[5] * np.float32(2.0 ** 127 if metric == IP else 2.0 ** 63)
    g = loaded(nifs, metric, ids, x)
    packed = oracle_mod.pack_ids(ids)
    want = [bits(oracle_mod.matrix_search(metric, x, packed, q, 10)) for q in qs]
    before = nifs.flat_get_profile(g.ref)
    assert bits(unwrap(nifs.flat_search(g.ref, qs[5], 10))) == want[5]
    assert moved(nifs, g.ref, before)["sketch_launches"] == 0  # (the lone search declines too)
    delta = batch_equals_alone(nifs, g.ref, qs, 10, want, "decline")
    assert delta["sketch_batch_queries"] == 7 and delta["sketch_batch_launches"] == 1, delta
    assert delta["sketch_batch_fallbacks"] == 0 and delta["sketch_launches"] == 0, delta
    # two queries of which one declines: no group of one is run
    delta = batch_equals_alone(nifs, g.ref, qs[4:6], 10, want[4:6], "decline, two")
    assert delta["sketch_batch_queries"] == 0 and delta["sketch_batch_launches"] == 0, delta


@pytest.mark.parametrize("metric", [IP, L2])
def test_rows_that_do_not_certify_are_handed_on(nifs, oracle_mod, vt_debug, metric):
    """The spiky corpus (every slot of every list a candidate: the model says so): each query enters a group, none is
    answered by it, every one is counted as a fallback and answered by what batch_ready does with left-over queries."""
    vt_debug.set("force_sketch", 2)
    x, ids, qs = cases.spiky_case(metric)
    g = loaded(nifs, metric, ids, x)
    packed = oracle_mod.pack_ids(ids)
    want = [bits(oracle_mod.matrix_search(metric, x, packed, q, 10)) for q in qs]
    delta = batch_equals_alone(nifs, g.ref, qs, 10, want, "spiky")
    assert delta["sketch_batch_queries"] == 8 and delta["sketch_batch_launches"] == 1, delta
    assert delta["sketch_batch_fallbacks"] == 8 and delta["sketch_batch_tail_rescored"] == 0, delta


def test_mutations_between_batches_patch_the_column(nifs, oracle_mod, vt_debug):
    """Upserts, swap-deletes and an append between batches: the column is patched row by row under the batch's own
    preparation, and the batch sees the rows as they are."""
    vt_debug.set("force_sketch", 2)
    metric = L2
    x, ids, qs = cases.case("uniform", metric)
    ids = list(ids)
    g = loaded(nifs, metric, ids, x)

    def check(note, groups=1):
        packed = oracle_mod.pack_ids(ids)
        want = [bits(oracle_mod.matrix_search(metric, x, packed, q, 10)) for q in qs[:8]]
        delta = batch_equals_alone(nifs, g.ref, qs[:8], 10, want, note)
        assert delta["sketch_batch_launches"] == groups and delta["sketch_batch_queries"] == 8 * groups, (note, delta)
        return delta

    assert check("fresh")["sketch_builds"] == 1
    p0 = nifs.flat_get_profile(g.ref)
    for r in (0, 17, len(ids) - 1, 4500):  # upserts that become query 2's best hits: only a patched row lets them through
        x[r] = (qs[2] * (1.0 + 0.001 * (1 + r % 5))).astype(np.float32)
        unwrap(nifs.flat_insert(g.ref, ids[r], x[r]))
    check("upserts")
    for r in (5, 6000):  # swap-deletes
        unwrap(nifs.flat_delete(g.ref, ids[r]))
        last = len(ids) - 1
        x[r], ids[r] = x[last], ids[last]
        x, ids = x[:last], ids[:last]
    check("deletes")
    new = (qs[3] * 1.0005).astype(np.float32)
    unwrap(nifs.flat_insert(g.ref, b"zz-new", new))  # (sorts after every id: the ranks stay strictly current)
    x, ids = np.vstack([x, new[None]]), ids + [b"zz-new"]
    check("append")
    delta = {k: v for k, v in moved(nifs, g.ref, p0).items() if v and "sketch" in k}
    # the mutated rows were re-quantised in place by the batches' own preparation (the first mutation may double the slab,
    # and a slab that outgrew the column rebuilds it once: the column's policy)
    assert delta.get("sketch_patched_rows", 0) >= 3 and delta.get("sketch_builds", 0) <= 1, delta
    assert delta["sketch_batch_launches"] == 3 and delta.get("sketch_launches", 0) == 0, delta


def test_no_room_for_the_sketch_means_the_batch_runs_as_before(nifs, oracle_mod, request, vt_debug):
    """(test_refuse_sketch, libvettore_hip_hooks.so only: the test re-runs itself there.)"""
    if support.rerun_with_hooks_library(request):
        return
    vt_debug.set("test_refuse_sketch", 1)
    vt_debug.set("force_sketch", 2)
    for metric in (COS, L2SQ):
        x, ids, qs = cases.case("uniform", metric)
        g = loaded(nifs, metric, ids, x)
        want = oracle_lists(oracle_mod, "uniform", metric, x, ids, qs, 10)
        delta = batch_equals_alone(nifs, g.ref, qs[:8], 10, want, "refused")
        assert delta["sketch_batch_launches"] == 0 and delta["sketch_builds"] == 0 and delta["sketch_launches"] == 0, delta
        delta = batch_equals_alone(nifs, g.ref, qs[:9], 10, want, "refused, again")
        assert delta["sketch_batch_launches"] == 0 and delta["sketch_builds"] == 0, delta


@pytest.mark.parametrize("metric", [COS, L2])
def test_a_three_shard_handle(nifs, oracle_mod, vt_debug, metric):
    """Every shard's worker reaches batch_ready, so every shard's part of the batch shares passes over that shard's column:
    the merged lists are the oracle's."""
    vt_debug.set("force_sketch", 2)
    x, ids, qs = cases.case("ties", metric)
    g = loaded(nifs, metric, ids, x, devices=[0, 0, 0])
    want = oracle_lists(oracle_mod, "ties", metric, x, ids, qs, 10)
    for nq in (2, 9):
        delta = batch_equals_alone(nifs, g.ref, qs[:nq], 10, want, "sharded")
        # (three shards, each with its own groups over its own rows)
        assert delta["sketch_batch_launches"] == 3 * len(cases.plan(nq, 8)) and delta["sketch_batch_queries"] == 3 * nq, delta
        assert delta["nominate_launches"] == 0, delta


@pytest.mark.parametrize("metric", [COS, L2])
def test_callers_that_meet_share_a_pass(nifs, oracle_mod, request, vt_debug, metric):
    """Four native threads search at once and are held until all four have queued (test_coalesce_hold_until, the hooks
    build): they leave as one batch of four, which is one group pass; each gets the answer of its search alone."""
    if support.rerun_with_hooks_library(request):
        return
    vt_debug.set("coalesce_slots", 1)
    vt_debug.set("force_sketch", 2)
    x, ids, qs = cases.case("uniform", metric)
    g = loaded(nifs, metric, ids, x)
    want = oracle_lists(oracle_mod, "uniform", metric, x, ids, qs, 10)
    for i in range(4):
        assert bits(unwrap(nifs.flat_search(g.ref, qs[i], 10))) == want[i]
    b0, p0 = nifs.flat_coalesce_stats(g.ref), nifs.flat_get_profile(g.ref)
    wrong, failed = support.callers_meet(g.ref, qs[:4], 10, [0] * 4, rounds=1)
    b1, delta = nifs.flat_coalesce_stats(g.ref), moved(nifs, g.ref, p0)
    assert (wrong, failed) == (0, 0)
    assert (b1[0] - b0[0], b1[1] - b0[1]) == (1, 4), (b0, b1)
    assert delta["sketch_batch_queries"] == 4 and delta["sketch_batch_launches"] == 1 and delta["sketch_batch_fallbacks"] == 0, delta
    assert delta["nominate_launches"] == 0, delta
