"""Builds liblc3plus_hip.so and its sibling libraries (csrc/Makefile: SIBLINGS) in-tree (hipcc cross-compiles gfx950 without a GPU)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def build(verbose=False):
    cmd = ["make", "-j%d" % max(1, min(16, os.cpu_count() or 1)), "-C", os.path.join(HERE, "csrc")]   # the kernel objects, the runtime and the siblings, independent of each other
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return os.path.join(HERE, "liblc3plus_hip.so")
