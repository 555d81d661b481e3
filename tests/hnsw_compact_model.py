"""A numpy restatement of K11c (vt_hnsw.hip: launch_hnsw_compact), the compaction of an HNSW slab and its device mirror,
and the hand-made mirrors its tests use.  tests/test_hnsw_plan.py checks the restatement against examples written out by
hand (CPU); tests/test_gpu_hnsw_compact_kernel.py holds the kernel to it word for word.

The mirror (vt_device.h, HnswDev): row r's layer-0 list is adj0[r] = [count, entries ..., unused words] with m0 + 1 words,
its list on layer l >= 1 the same with m + 1 words at upper[upoff[r] + (l - 1) * (m + 1)]; entries are rows."""
import numpy as np

NO_ROW = 0xFFFFFFFF
BEYOND, DEAD, COUNT, SHAPE = 0, 1, 2, 3   # the guards' status words


def plan_for(level, live_rows, m):
    """(src, new_upoff, new_upper) for the surviving old rows, ascending: host/vt_hnswplan.h's plan."""
    src = np.asarray(sorted(int(r) for r in live_rows), np.uint32)
    words = level[src].astype(np.uint64) * np.uint64(m + 1)
    ends = np.cumsum(words, dtype=np.uint64)
    new_upoff = (ends - words).astype(np.uint32)
    return src, new_upoff, int(ends[-1]) if len(src) else 0


def _list_image(lst, lim, stride, old_rows, remap, status):
    """The new image of one list of `stride` words: the count (clamped), the entries renumbered, zeros behind."""
    out = np.zeros(stride, np.uint32)
    cnt = int(lst[0])
    if cnt > lim:
        status[COUNT] = 1
        cnt = lim
    out[0] = cnt
    for k in range(1, cnt + 1):
        e = int(lst[k])
        if e >= old_rows:          # before the table is read
            status[BEYOND] = 1
            out[k] = NO_ROW
            continue
        out[k] = remap[e]
        if remap[e] == NO_ROW:
            status[DEAD] = 1
    return out


def compact(X, adj0, level, upoff, upper, m, m0, src, new_upoff, new_upper):
    """What the launch leaves in its output buffers: dict of outX, out_adj0, out_level, out_upoff, out_upper, remap, status."""
    old_rows, stride = X.shape
    rows = len(src)
    status = np.zeros(4, np.uint32)
    remap = np.full(old_rows, NO_ROW, np.uint32)
    for i, s in enumerate(src):
        if s >= old_rows:
            status[SHAPE] = 1
        else:
            remap[s] = i
    out = dict(outX=np.zeros((rows, stride), np.float32), out_adj0=np.zeros((rows, m0 + 1), np.uint32),
               out_level=np.zeros(rows, np.uint32), out_upoff=np.asarray(new_upoff, np.uint32).copy(),
               out_upper=np.zeros(new_upper, np.uint32), remap=remap, status=status)
    for i, s in enumerate(src):
        end = int(new_upoff[i + 1]) if i + 1 < rows else new_upper
        words = end - int(new_upoff[i])
        out["out_level"][i] = words // (m + 1)
        if s >= old_rows:
            continue
        out["outX"][i] = X[s]
        out["out_adj0"][i] = _list_image(adj0[s], m0, m0 + 1, old_rows, remap, status)
        if int(level[s]) * (m + 1) != words or (words and int(upoff[s]) + words > len(upper)):
            status[SHAPE] = 1
            continue
        for layer in range(words // (m + 1)):
            at, to = int(upoff[s]) + layer * (m + 1), int(new_upoff[i]) + layer * (m + 1)
            out["out_upper"][to:to + m + 1] = _list_image(upper[at:at + m + 1], m, m + 1, old_rows, remap, status)
    return out


def make_mirror(rng, rows, stride, m, m0, live):
    """A hand-made slab and mirror of `rows` rows whose lists name live rows only: levels 0..3 (three rows in eight above 0),
    counts from 0 to the full degree, the words behind a count garbage (a compaction must not carry them over), the
    upper-layer lists laid out in row order with a hole in front of every fourth row's (offsets are the mirror's to say)."""
    live = np.asarray(sorted(int(r) for r in live), np.uint32)
    X = rng.standard_normal((rows, stride)).astype(np.float32)
    level = rng.choice(np.asarray([0, 0, 0, 0, 0, 1, 2, 3], np.uint32), rows).astype(np.uint32)
    adj0 = rng.integers(0, 2**32, (rows, m0 + 1), dtype=np.uint64).astype(np.uint32)
    upoff = np.zeros(rows, np.uint32)
    at = 0
    for r in range(rows):
        if level[r] and r % 4 == 3:
            at += 3
        upoff[r] = at
        at += int(level[r]) * (m + 1)
    upper = rng.integers(0, 2**32, max(at, 1), dtype=np.uint64).astype(np.uint32)

    def fill(lst, lim):
        cnt = int(rng.choice([0, lim, lim // 2, 1])) if len(live) else 0
        lst[0] = cnt
        lst[1:1 + cnt] = rng.choice(live, cnt)

    for r in range(rows):
        fill(adj0[r], m0)
        for layer in range(int(level[r])):
            a = int(upoff[r]) + layer * (m + 1)
            fill(upper[a:a + m + 1], m)
    return dict(X=X, adj0=adj0, level=level, upoff=upoff, upper=upper)
