#!/usr/bin/env python3
"""Merges the lines a run under LC3PLUS_LAUNCH_CENSUS=<path> appended to <path> - one block of "name count" lines per process that unloaded the library - into
one count per kernel, and lists the entry points of the library's gfx950 code object that no process launched.

    LC3PLUS_LAUNCH_CENSUS=/tmp/census.txt python -m pytest tests -m gpu
    python tools/launch_census_merge.py /tmp/census.txt [--lib audio_codec_amd/liblc3plus_hip.so] > profiles/launch_census_suite.txt

Needs no GPU.  Exit status 1 if a reported name is no kernel of the code object."""
import argparse
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def merge(path):
    n = collections.Counter()
    for line in open(path):
        w = line.split()
        if len(w) == 2 and not line.startswith("#"):
            n[w[0]] += int(w[1])
    return n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("census")
    ap.add_argument("--lib", default=os.path.join(ROOT, "audio_codec_amd", "liblc3plus_hip.so"))
    ap.add_argument("--title", default="")
    a = ap.parse_args()
    n = merge(a.census)
    kernels = sorted(kr.kernels(a.lib, "gfx950"))
    unknown = sorted(set(n) - set(kernels))
    unreached = [k for k in kernels if k not in n]
    print("# launch census%s: %d kernels in the code object, %d launched, %d never launched, %d launches" %
          (" (" + a.title + ")" if a.title else "", len(kernels), len(kernels) - len(unreached), len(unreached), sum(n.values())))
    for k in sorted(n):
        print("%s %d" % (k, n[k]))
    print("# never launched (%d):" % len(unreached))
    for k in unreached:
        print("# %s" % k)
    for k in unknown:
        print("# NOT A KERNEL OF THE CODE OBJECT: %s" % k)
    return 1 if unknown else 0


if __name__ == "__main__":
    sys.exit(main())
