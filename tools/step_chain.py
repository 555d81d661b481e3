#!/usr/bin/env python3
"""tools/step_chain.py KERNEL_TRACE_CSV [ANCHOR] -- the chain of one lone search out of a `rocprofv3 --kernel-trace` of
`bench.py --gpus 1`: a step is everything from one launch of ANCHOR (default sketch_scan_kernel) to the next.  Prints, per
position in the chain, the kernel, the median / min / max of its duration and of the gap since the previous kernel's end
(us), then the median gap from a step's last kernel to the next step's ANCHOR (host time + blit) and the median step."""
import csv
import re
import sys
from collections import Counter


def short(name):
    m = re.search(r"(\w+_kernel)", name)
    return m.group(1) if m else name[:40]


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    anchor = sys.argv[2] if len(sys.argv) > 2 else "sketch_scan_kernel"
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]))
                for r in csv.DictReader(open(sys.argv[1])))
    starts = [i for i, e in enumerate(ev) if e[2] == anchor]
    steps = [ev[a:b] for a, b in zip(starts, starts[1:])]
    shape = Counter(tuple(e[2] for e in s) for s in steps).most_common(1)[0][0]
    steps = [s for s in steps if tuple(e[2] for e in s) == shape]
    keep = steps[len(steps) // 4:]  # (the warm-up and the first timed steps left out)
    print("# %d steps of shape %s; the last %d used" % (len(steps), " > ".join(shape), len(keep)))
    print("# pos kernel                          dur_med  dur_min  dur_max   gap_med  gap_min  gap_max  (us)")
    for i, name in enumerate(shape):
        d = [(s[i][1] - s[i][0]) / 1e3 for s in keep]
        g = [(s[i][0] - s[i - 1][1]) / 1e3 for s in keep] if i else [0.0]
        print("%5d %-30s %8.1f %8.1f %8.1f  %8.1f %8.1f %8.1f" % (i, name, med(d), min(d), max(d), med(g), min(g), max(g)))
    tail = [(b[0][0] - a[-1][1]) / 1e3 for a, b in zip(keep, keep[1:]) if b[0][0] - a[-1][1] < 1e6]
    whole = [(b[0][0] - a[0][0]) / 1e3 for a, b in zip(keep, keep[1:]) if b[0][0] - a[0][0] < 1e7]
    print("# last kernel's end -> next step's %s: median %.1f us, min %.1f" % (anchor, med(tail), min(tail)))
    print("# %s start -> next start: median %.1f us, min %.1f" % (anchor, med(whole), min(whole)))


if __name__ == "__main__":
    main()
