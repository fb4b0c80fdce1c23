#!/usr/bin/env python3
"""Do two builds of the library hold the same GPU code?  No GPU needed.

    python tools/code_object_diff.py OLD/liblc3plus_hip.so NEW/liblc3plus_hip.so [--arch gfx950]

Each library holds one code object per kernel object file (tools/kernel_resources.py cuts them out).  The code objects of the two libraries are matched by
the set of kernel names each defines; per pair the tool says whether the .text sections are byte-identical and whether every kernel's metadata (VGPRs, AGPRs,
SGPRs, scratch, LDS, kernarg size) is equal.  Exit status 1 on any difference, and on any kernel that only one side has.  Machine code depends on the
compiler as much as on the sources: build both sides with the same hipcc, and keep no digest of either."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import FIELDS, code_objects, fatbin, object_kernels, section   # noqa: E402

META = FIELDS + (".kernarg_segment_size",)


def objects(path, arch):
    """{frozenset of kernel names: (.text bytes, {kernel: metadata})} over the code objects of a library"""
    out = {}
    for co in code_objects(fatbin(path), arch):
        k = object_kernels(co, META)
        if k:
            assert frozenset(k) not in out, "two code objects with the same kernels in %s" % path
            out[frozenset(k)] = (section(co, b".text") or b"", k)
    return out


def label(names):
    """an object is called after its one-wave encode kernel: every object file of the library defines exactly one"""
    ow = sorted(n for n in names if n.startswith("lc3_encode_kernel"))
    return ow[0] if ow else sorted(names)[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--arch", default="gfx950")
    a = ap.parse_args()
    old, new = objects(a.old, a.arch), objects(a.new, a.arch)
    bad = 0
    print("# code objects for %s: %d old, %d new; kernels: %d old, %d new" % (a.arch, len(old), len(new), sum(map(len, old)), sum(map(len, new))))
    print("%-36s %7s %9s  %-9s %s" % ("object (its one-wave kernel)", "kernels", "bytes", ".text", "metadata"))
    for names in sorted(set(old) & set(new), key=label):
        (t0, k0), (t1, k1) = old[names], new[names]
        moved = sorted(n for n in names if k0[n] != k1[n])
        bad += (t0 != t1) + bool(moved)
        print("%-36s %7d %9d  %-9s %s" % (label(names), len(names), len(t1), "identical" if t0 == t1 else "DIFFERS", "equal" if not moved else "DIFFERS: " + " ".join(moved)))
        if t0 != t1:
            print("#   .text %d -> %d bytes, first difference at byte %d" % (len(t0), len(t1), next((i for i, (x, y) in enumerate(zip(t0, t1)) if x != y), min(len(t0), len(t1)))))
    all_old, all_new = set().union(*old), set().union(*new)
    for side, objs, other in (("old", old, new), ("new", new, old)):
        for names in sorted(set(objs) - set(other), key=label):
            bad += 1
            print("# UNMATCHED in %s: the object of %s (%d kernels)" % (side, label(names), len(names)))
    for n in sorted(all_old ^ all_new):
        bad += 1
        print("# kernel only in %s: %s" % ("old" if n in all_old else "new", n))
    print("# %s" % ("%d differences" % bad if bad else "every code object byte-identical in .text and equal in metadata; same %d kernel names" % len(all_new)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
