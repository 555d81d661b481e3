"""What the selection kernels (csrc/vt_select.hip, K3) must return, in plain Python on Python integers.

  expected_topk   the only source of expected values for the selects, the sort and the merge: a sort.
  kth_threshold   the radix passes' threshold: the k-th smallest of the whole column, masked to the digits resolved.
  route           a restatement of select_topk_kernel's digit walk that LABELS an input with the branches it enters, so
                  that tests/test_select_model.py can show the case table reaches every one of them.  No expected value
                  comes from it.
"""
EMPTY = 0xFFFFFFFFFFFFFFFF  # vt_device.h kEmptyKey
M64 = EMPTY
SEL_CAND = 4096   # vt_select.hip kSelCand: the LDS candidate list (file-local there: this copy only labels inputs)
SHORT_MAX = 1024  # the one-key-per-thread path of a lone block


def expected_topk(keys, k, lo=None):
    """The first k of the live keys -- those != EMPTY and > lo -- in (key, position) order, as [(key, position)]."""
    live = [(int(key), i) for i, key in enumerate(keys) if int(key) != EMPTY and (lo is None or int(key) > lo)]
    live.sort()
    return live[:k]


def kth_threshold(keys, k, bits):
    """The k-th smallest (1-based) of the whole column, empties included as the histograms count them, masked to its top
    `bits` bits.  A column shorter than k has no k-th key: every digit falls to its last bin, all ones."""
    assert bits in (33, 64) and k >= 1
    mask = (M64 >> (64 - bits)) << (64 - bits)
    col = sorted(int(x) for x in keys)
    return (col[k - 1] if k <= len(col) else EMPTY) & mask


def route(keys, k, lo=None, one_key_per_thread=True):
    """The branches of select_topk_kernel that one block enters on `keys`: a dict label -> number.

      short                  the list has at most 1024 keys and the form allows the one-key-per-thread path
      all-selected           nvalid <= k, or no bit varies among the live keys
      cand: r                the first digit's bin went to the LDS list and r further digits were resolved there
      crowded: r             the first digit's bin held more than 4096 keys and r further digits were resolved globally
      whole-bin              the walk ended on a bin whose count is exactly what remained to select
      exhausted-with-equals  the walk ended because no varying bit was left, in a bin of MORE equal keys than remained
    A walk that ends at the first digit carries neither `cand` nor `crowded`."""
    keys = [int(x) for x in keys]
    if one_key_per_thread and len(keys) <= SHORT_MAX:
        return {"short": 1}
    live = [x for x in keys if x != EMPTY and (lo is None or x > lo)]
    if len(live) <= k:
        return {"all-selected": 1}
    bits_and, bits_or = M64, 0
    for x in live:
        bits_and &= x
        bits_or |= x
    var = bits_and ^ bits_or
    if var == 0:
        return {"all-selected": 1}

    def next_hb(shift):
        return (var & ((1 << shift) - 1)).bit_length() - 1

    labels = {}
    krem, hb = k, var.bit_length() - 1
    mask = ~var & M64
    prefix = bits_or & mask
    where, rounds = None, 0
    while True:
        width = min(hb + 1, 8)
        shift = hb + 1 - width
        dmask = (1 << width) - 1
        hist = [0] * 256
        for x in live:
            if x & mask == prefix:
                hist[(x >> shift) & dmask] += 1
        below = 0
        for b in range(256):
            if below + hist[b] >= krem:
                break
            below += hist[b]
        krem -= below
        prefix |= b << shift
        mask |= dmask << shift
        if where:
            rounds += 1
        if hist[b] == krem or next_hb(shift) < 0:
            labels["whole-bin" if hist[b] == krem else "exhausted-with-equals"] = 1
            if where:
                labels[where] = rounds
            return labels
        if not where:
            where = "cand" if hist[b] <= SEL_CAND else "crowded"
        hb = next_hb(shift)
