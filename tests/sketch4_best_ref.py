"""The numpy model of K1n's threshold from each list's best rows (vt_sketch_nibble.cuh nibble_best_rows,
vt_sketch4_rescore.hip best_select) beside the refine's rule it stands in for (sketch4_ref.exact_threshold), over lists as
the 4-bit pass leaves them: [lists][kp] slots, a slot's key(hi) word (optimistic), its key(lo) word (pessimistic) and the
exact key word of its row, 0xffffffff in an empty slot."""
import numpy as np

import sketch4_ref as ref4

EMPTY = np.uint32(0xFFFFFFFF)
KP = 64          # slots of a list
BEST_ROWS = 2    # rows a list's storing wave rescores


def owner_lists(n, blocks):
    """The list of every row as the 4-bit pass deals its tiles: 4 waves a block numbered across the blocks first, tile t to
    wave t mod waves, a list per pair of waves of a block (test_gpu_sketch_kernels.owner_list, width 4)."""
    w = (np.arange(n) // 64) % (4 * blocks)
    return 2 * (w % blocks) + (w // blocks) // 2


def deal(lists_of_rows, nlists, hi, lo, exact, rank=None):
    """The lists the pass leaves: list b keeps the KP rows of smallest (key(hi) word, id rank) among its own.  Returns
    rows[nlists][KP] (-1: empty) and the three word arrays in the same shape."""
    n = len(hi)
    rank = np.arange(n, dtype=np.uint64) if rank is None else np.asarray(rank, np.uint64)
    key = (np.asarray(hi, np.uint64) << np.uint64(32)) | rank
    order = np.lexsort((key, lists_of_rows))
    sorted_lists = lists_of_rows[order]
    first = np.searchsorted(sorted_lists, np.arange(nlists), side="left")
    last = np.searchsorted(sorted_lists, np.arange(nlists), side="right")
    rows = np.full((nlists, KP), -1, np.int64)
    for b in range(nlists):
        take = order[first[b]:min(last[b], first[b] + KP)]
        rows[b, :len(take)] = take
    live = rows >= 0
    pick = np.where(live, rows, 0)
    words = [np.where(live, np.asarray(w, np.uint32)[pick], EMPTY).astype(np.uint32) for w in (hi, lo, exact)]
    return rows, words[0], words[1], words[2]


def best_words(lo, exact, finite=None):
    """[lists][BEST_ROWS]: per list the exact words of its live slots of smallest key(lo) word, ties to the lower slot;
    0xffffffff where the list has no such slot or the row's value is not finite (finite[lists][kp], None: all are)."""
    lo, exact = np.asarray(lo, np.uint32), np.asarray(exact, np.uint32)
    out = np.full((lo.shape[0], BEST_ROWS), EMPTY, np.uint32)
    for b in range(lo.shape[0]):
        live = np.nonzero(lo[b] != EMPTY)[0]
        for j, slot in enumerate(live[np.argsort(lo[b][live], kind="stable")][:BEST_ROWS]):
            if finite is None or finite[b][slot]:
                out[b, j] = exact[b][slot]
    return out


def best_threshold(words, k):
    """Kt'': the k-th smallest of the words with multiplicity, empty words counting as 0xffffffff -- so 0xffffffff when
    fewer than k are live."""
    w = np.sort(np.asarray(words, np.uint32).reshape(-1))
    return int(w[k - 1]) if len(w) >= k else 0xFFFFFFFF


def refine_threshold(lo, exact, k):
    """Kt' of the chain this one replaces (the lowest word the refine may publish: sketch4_ref.exact_threshold)."""
    live = np.asarray(lo, np.uint32).reshape(-1) != EMPTY
    return ref4.exact_threshold(np.asarray(lo, np.uint32).reshape(-1)[live], None, np.asarray(exact, np.uint32).reshape(-1)[live], k)[1]


def candidates(hi, kt):
    """The rescoring kernel's rule, [lists][kp] booleans, and whether any list consists of candidates alone (refused)."""
    hi = np.asarray(hi, np.uint32)
    cand = (hi != EMPTY) & (hi <= np.uint32(kt))
    return cand, bool(cand.all(axis=1).any())
