"""The inputs of the selection kernels' tests are not vacuous (tests/select_cases.py, tests/select_ref.py), on the CPU.

tests/test_gpu_select_kernels.py compares K3 (csrc/vt_select.hip) with a sort.  That says something about a branch of
select_topk_kernel only if some input enters it, and random or search-made keys enter few.  Here the case table is labelled
with select_ref.route, a restatement of the kernel's digit walk, and every label must be reached in every launch form it
can be reached in:

  form        short  all-selected  whole-bin  exhausted-with-equals  cand  crowded
  lone          x         x            x               x              x      x
  two-level     x         x            x               x              x      -    (a slice holds about 1024 keys, a crowded
  list          -         x            x               x              x      x     bin more than 4096; the list form and the
  queries       x         x            x               x              x      -     first level have no one-key-per-thread path;
  lists         x         x            x               x              x      -     a query's list here stays below 4096 keys)

and the walk must end on exhausted varying bits among MORE equal keys than remain -- the suspected defect -- at the first
digit, on the LDS list and on the global keys, with a strictly smaller key past position 1024 of the block's list each time.
"""
import numpy as np
import pytest

import select_cases as sc
import select_ref as ref

ALL = ("short", "all-selected", "whole-bin", "exhausted-with-equals", "cand", "crowded")
APPLIES = {"lone": ALL, "two-level": ALL[:5], "list": ALL[1:], "queries": ALL[:5], "lists": ALL[:5]}


def labelled(form):
    for case in sc.of_form(form):
        for keys, k, lo, short_ok in sc.block_inputs(case):
            yield case, keys, k, lo, ref.route(keys, k, lo, short_ok)


@pytest.fixture(scope="module")
def table():
    return {form: list(labelled(form)) for form in APPLIES}


def test_case_names_are_unique_and_no_case_is_large():
    names = [c.name + "/" + c.form for c in sc.cases()]
    assert len(set(names)) == len(names)
    assert all(c.keys.size <= 20000 for c in sc.cases())
    assert {c.form for c in sc.cases()} == set(APPLIES)


@pytest.mark.parametrize("form", sorted(APPLIES))
def test_every_branch_is_reached_in_every_form_it_applies_to(table, form):
    reached = {}
    for case, _, _, _, labels in table[form]:
        for name in labels:
            reached.setdefault(name, case.name)
    print(form, reached)
    assert set(reached) == set(APPLIES[form])


def test_the_walk_resolves_several_digits_on_the_lds_list_and_on_the_global_keys(table):
    rounds = {"cand": set(), "crowded": set()}
    for rows in table.values():
        for _, _, _, _, labels in rows:
            for name in rounds:
                if name in labels:
                    rounds[name].add(labels[name])
    assert {1, 2} <= rounds["cand"] and max(rounds["cand"]) >= 3  # (the ladder family)
    assert {1, 2} <= rounds["crowded"]


def test_a_digit_is_cut_from_non_contiguous_varying_bits():
    keys = sc.bits(4097, 1)
    assert int(np.bitwise_or.reduce(keys) ^ np.bitwise_and.reduce(keys)) == (1 << 63) | 1
    assert ref.route(keys, 5)["cand"] == 1


@pytest.mark.parametrize("form", sorted(APPLIES))
def test_exhausted_cases_hold_a_smaller_key_past_position_1024(table, form):
    """More equal keys than remain to select, no varying bit left, and a strictly smaller live key whose thread reaches it in
    its second turn: with the bin's top for a threshold that key races the equals for a place."""
    ends = set()
    for case, keys, k, lo, labels in table[form]:
        # (a straggler list holds two or three values; other families end there too, without the late smaller key)
        if "exhausted-with-equals" not in labels or "straggler" not in case.name or len(set(keys.tolist())) > 3:
            continue
        want = ref.expected_topk(keys, k, lo)
        kth = want[-1][0]
        late = [pos for key, pos in want if key < kth and pos >= 1024]
        assert late, case.name
        assert sum(1 for x in keys if int(x) == kth) > sum(1 for key, _ in want if key == kth), case.name
        low_ones = all((kth >> b) & 1 for b in range(2))  # (the digit above ends at bit 2 in every straggler case)
        ends.add(("cand" if "cand" in labels else "crowded" if "crowded" in labels else "first", low_ones))
    places = ("first", "cand", "crowded") if "crowded" in APPLIES[form] else ("first", "cand")
    assert ends == {(p, ones) for p in places for ones in (False, True)}


def test_expected_topk_is_a_sort():
    for case in sc.cases():
        if "straggler" not in case.name and case.form != "lists":
            continue
        for keys, k, lo, _ in sc.block_inputs(case):
            live = sorted((int(x), i) for i, x in enumerate(keys) if int(x) != ref.EMPTY and (lo is None or int(x) > lo))
            assert ref.expected_topk(keys, k, lo) == live[:k]
    assert ref.expected_topk([5, ref.EMPTY, 3, 5, 3], 3) == [(3, 2), (3, 4), (5, 0)]
    assert ref.expected_topk([5, ref.EMPTY, 3, 5, 3], 9, lo=3) == [(5, 0), (5, 3)]
    assert ref.expected_topk([ref.EMPTY], 1) == []


def test_kth_threshold_counts_the_empties_and_masks_the_digits():
    keys = [7 << 31, ref.EMPTY, 3 << 31, 5 << 31 | 9]
    assert ref.kth_threshold(keys, 2, 64) == 5 << 31 | 9
    assert ref.kth_threshold(keys, 2, 33) == 5 << 31
    assert ref.kth_threshold(keys, 4, 64) == ref.EMPTY
    assert ref.kth_threshold(keys, 5, 33) == (ref.EMPTY >> 31) << 31


def test_route_follows_the_issues_hand_trace():
    keys = [0x200] * 1100 + [0x100]
    assert ref.route(keys, 3) == {"exhausted-with-equals": 1}
    assert ref.route(keys[:1024], 3) == {"short": 1}
    assert ref.route(keys[:1024], 3, one_key_per_thread=False) == {"all-selected": 1}
    assert ref.route(keys, 1) == {"whole-bin": 1}
    assert ref.route(keys, 2000) == {"all-selected": 1}
    assert ref.route(keys, 3, lo=0x200) == {"all-selected": 1}
