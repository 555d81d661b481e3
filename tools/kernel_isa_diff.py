#!/usr/bin/env python3
"""tools/kernel_isa_diff.py PARENT_DIR BRANCH_DIR -- are the device kernels of two checkouts the same code?

Compiles every csrc/*.hip of both trees to gfx950 assembly with the command `make -n` prints for the unit's object
(so with the unit's own flags), `-c` replaced by `--cuda-device-only -S`, and compares, over all units of a side:
the set of .amdhsa_kernel names; per kernel its .amdhsa_* descriptor lines (registers, scratch, LDS); per kernel the
instruction text between its label and its .Lfunc_end, local labels renumbered per function, comments dropped.
Prints the counts and the names that differ; exit status 1 when names or descriptors differ (text alone: listed).
No GPU needed.  What a refactor that only moves kernels between files commits as its proof (profiles/kernel_split/).
"""
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

LABEL = re.compile(r"\.(?:LBB\d+_\d+|Lfunc_end\d+|Ltmp\d+)")


def assemble(tree, unit, out):
    plan = subprocess.run(["make", "-C", tree, "-n", "-B", "vettore_amd/lib/%s.o" % unit], capture_output=True, text=True, check=True)
    cmd = next(line for line in plan.stdout.splitlines() if " -c " in line and "hipcc" in line).split(" 2>")[0]
    cmd = re.sub(r" -o \S+", " -o " + out, cmd.replace(" -c ", " --cuda-device-only -S "))
    subprocess.run(cmd, shell=True, cwd=tree, check=True, stderr=subprocess.DEVNULL)
    return out


def kernels(path):
    """{kernel name: (descriptor lines, normalised body lines)} of one assembly file."""
    lines = open(path).read().splitlines()
    desc, name = {}, None
    for line in lines:
        s = line.strip()
        if s.startswith(".amdhsa_kernel "):
            name = s.split()[1]
            desc[name] = []
        elif s == ".end_amdhsa_kernel":
            name = None
        elif name and s.startswith(".amdhsa_"):
            desc[name].append(s)
    found, i = {}, 0
    while i < len(lines):
        label = lines[i].split(":")[0] if lines[i][:1] == "_" else None  # (`name:   ; @name`)
        if label in desc:
            body, seen = [], {}
            for i in range(i + 1, len(lines)):
                s = lines[i].split(";")[0].strip()  # (comment lines and the loop notes behind labels)
                if s:
                    body.append(LABEL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), s))
                if s.startswith(".Lfunc_end"):
                    break
            found[label] = (desc[label], body)
        i += 1
    assert found.keys() == desc.keys(), path
    return found


def side(tree, files):
    per_unit = {u: kernels(f) for (t, u), f in files.items() if t == tree}
    merged = {}
    for u, ks in per_unit.items():
        assert not (merged.keys() & ks.keys()), "a kernel emitted by two units of %s" % tree
        merged.update(ks)
    return merged, {u: len(ks) for u, ks in per_unit.items()}


def main():
    parent_dir, branch_dir = (os.path.abspath(p) for p in sys.argv[1:3])
    jobs = [(t, os.path.basename(p)[:-4]) for t in (parent_dir, branch_dir) for p in sorted(glob.glob(os.path.join(t, "vettore_amd/csrc/*.hip")))]
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(int(os.environ.get("JOBS", "4"))) as pool:
        outs = pool.map(lambda j: assemble(j[0], j[1], os.path.join(tmp, "%d_%s.s" % (j[0] == branch_dir, j[1]))), jobs)
        files = dict(zip(jobs, outs))
        (parent, pu), (branch, bu) = side(parent_dir, files), side(branch_dir, files)
    for tag, units, ks in (("parent", pu, parent), ("branch", bu, branch)):
        print("%s: %d kernels in %d units (%s)" % (tag, len(ks), len(units), ", ".join("%s %d" % x for x in units.items())))
    only_p, only_b = sorted(parent.keys() - branch.keys()), sorted(branch.keys() - parent.keys())
    both = sorted(parent.keys() & branch.keys())
    bad_desc = [k for k in both if parent[k][0] != branch[k][0]]
    bad_text = [k for k in both if parent[k][0] == branch[k][0] and parent[k][1] != branch[k][1]]
    print("kernels on both sides: %d; identical (name, descriptor, instruction text): %d" % (len(both), len(both) - len(bad_desc) - len(bad_text)))
    for title, names in (("only in parent", only_p), ("only in branch", only_b), ("descriptor differs", bad_desc),
                         ("same descriptor, instruction text differs", bad_text)):
        print("%s: %d" % (title, len(names)))
        for n in names:
            print("  " + n)
    return 1 if only_p or only_b or bad_desc else 0


if __name__ == "__main__":
    sys.exit(main())
