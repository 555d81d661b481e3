"""What tests/test_gpu_sketch_batch.py relies on, shown in the numpy model of the int8 sketch before any kernel runs
(DESIGN.md 4.10): on its uniform and unit corpora every query of every batch is certified and rescored by its tail block
(so the share of fallbacks it asserts, zero, is a condition and not a cap), on its spiky corpus none is -- and the
restatement of the host's planner the tests count launches with is the one the C++ check pins down."""
import numpy as np
import pytest

import sketch_batch_cases as cases


@pytest.mark.parametrize("which", cases.CORPORA)
@pytest.mark.parametrize("metric", cases.METRICS)
def test_the_model_certifies_every_query_of_the_end_to_end_batches(which, metric):
    x, ids, qs = cases.case(which, metric)
    col = cases.Column(metric, x)
    d = x.shape[1]
    for k in cases.LIMITS:
        kp = cases.list_k(k)
        assert cases.max_group(d, kp) == 8
        # the grids the batches' groups run on, groups of 2..4 and of 5..8, on a card of 256 CUs
        grids = sorted({cases.group_blocks(d, kp, ng) for ng in range(2, 9)})
        for i, q in enumerate(qs):
            for blocks in grids:
                assert cases.outcome(col, q, k, blocks) == 1, (which, metric, k, i, blocks)


@pytest.mark.parametrize("metric", (cases.IP, cases.L2))
def test_the_model_leaves_spiky_rows_uncertified(metric):
    x, ids, qs = cases.spiky_case(metric)
    col = cases.Column(metric, x)
    for q in qs:
        for blocks in (512, 1024):
            assert cases.outcome(col, q, 10, blocks) != 1, (metric, blocks)


def test_the_planner_restated():
    assert cases.plan(9, 8) == [5, 4] and cases.plan(17, 8) == [6, 6, 5] and cases.plan(8, 8) == [8]
    assert cases.plan(3, 8) == [3] and cases.plan(2, 8) == [2] and cases.plan(1, 8) == [] and cases.plan(3, 2) == [2]
    for nq in range(2, 41):
        sizes = cases.plan(nq, 8)
        assert sum(sizes) == nq and len(sizes) == -(-nq // 8) and max(sizes) - min(sizes) <= 1 and min(sizes) >= 2
    assert [cases.max_group(d, 26) for d in (96, 128, 768, 1536, 8192, 32768)] == [8, 8, 8, 4, 2, 0]
    assert cases.group_blocks(96, 26, 8) == 512 and cases.group_blocks(96, 26, 4) == 1024 and cases.group_blocks(768, 26, 8) == 512
    assert np.all([cases.compiled_group(g) in (2, 4, 8) for g in range(2, 9)])
