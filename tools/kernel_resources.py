#!/usr/bin/env python3
"""Per-kernel resources of a HIP shared library, from the code-object metadata (no GPU needed).

    python tools/kernel_resources.py audio_codec_amd/liblc3plus_hip.so [--arch gfx950]
    python tools/kernel_resources.py NEW.so --against profiles/pcm_format_resources_parent.txt

Prints one line per kernel symbol, sorted by name: VGPRs (.vgpr_count), AGPRs, SGPRs, scratch bytes (.private_segment_fixed_size) and static LDS bytes
(.group_segment_fixed_size).  The library's .hip_fatbin section is a row of clang offload bundles, one per object file; the code object of the wanted
architecture is cut out of each and read with llvm-readelf --notes.  --against compares with a table printed earlier: exit status 1 if a kernel of that
table is missing here or grew in VGPRs, scratch or LDS."""
import argparse
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
HEAD = ("kernel", "vgpr", "agpr", "sgpr", "scratch", "lds")


def readelf():
    for c in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf"), shutil.which("llvm-readelf")):
        if c and os.path.exists(c):
            return c
    sys.exit("llvm-readelf not found (ROCM_PATH/llvm/bin or PATH)")


def section(d, want):
    """the bytes of section `want` of the ELF64 image d, or None"""
    assert d[:4] == b"\x7fELF" and d[4] == 2, "not an ELF64 file"
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", d, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]
    stroff = sec[shstrndx][4]
    for s in sec:
        if d[stroff + s[0]:d.index(b"\0", stroff + s[0])] == want:
            return d[s[4]:s[4] + s[5]]
    return None


def fatbin(path):
    fb = section(open(path, "rb").read(), b".hip_fatbin")
    if fb is None:
        sys.exit("no .hip_fatbin section in %s" % path)
    return fb


def code_objects(fb, arch):
    pos = fb.find(MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", fb, pos + len(MAGIC))
        q = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", fb, q)
            ident = fb[q + 24:q + 24 + idlen].decode()
            q += 24 + idlen
            if size and ident.startswith("hip") and ident.split("-")[-1].split(":")[0] == arch:
                yield fb[pos + off:pos + off + size]
        pos = fb.find(MAGIC, pos + 1)


def object_kernels(co, fields=FIELDS):
    """{kernel name: metadata values} of one code object"""
    out = {}
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co)
        f.flush()
        notes = subprocess.run([readelf(), "--notes", f.name], check=True, capture_output=True, text=True).stdout
    for block in re.split(r"\n\s+- \.", "\n" + notes):          # one list item of amdhsa.kernels per block
        vals = {m.group(1): m.group(2) for m in re.finditer(r"(\.[a-z_]+):\s+(\S+)", "." + block)}
        if ".symbol" in vals and ".name" in vals and ".vgpr_count" in vals:
            out[vals[".name"].strip("'\"")] = tuple(int(vals.get(k, "0")) for k in fields)
    return out


def kernels(path, arch):
    out = {}
    for co in code_objects(fatbin(path), arch):
        out.update(object_kernels(co))
    return out


def read_table(path):
    t = {}
    for line in open(path):
        w = line.split()
        if len(w) == len(HEAD) and w[0] != HEAD[0] and not line.startswith("#"):
            t[w[0]] = tuple(int(x) for x in w[1:])
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("library")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--against", help="a table printed earlier by this tool")
    a = ap.parse_args()
    k = kernels(a.library, a.arch)
    w = max([len(n) for n in k] + [6])
    print("# %s, %s: %d kernels" % (os.path.basename(a.library), a.arch, len(k)))
    print(("%-" + str(w) + "s %5s %5s %5s %8s %7s") % HEAD)
    for n in sorted(k):
        print(("%-" + str(w) + "s %5d %5d %5d %8d %7d") % ((n,) + k[n]))
    if a.against:
        bad = 0
        for n, old in sorted(read_table(a.against).items()):
            new = k.get(n)
            if new is None:
                print("# MISSING %s" % n); bad += 1
            elif new[0] > old[0] or new[3] > old[3] or new[4] > old[4]:
                print("# GREW %s: vgpr %d -> %d, scratch %d -> %d, lds %d -> %d" % (n, old[0], new[0], old[3], new[3], old[4], new[4])); bad += 1
        print("# against %s: %s" % (os.path.basename(a.against), "%d kernels grew or are missing" % bad if bad else "no kernel grew"))
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
