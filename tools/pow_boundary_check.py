#!/usr/bin/env python3
"""The device library's pow at the three call sites that still use it, against glibc's (float)pow((double), (double)), for EVERY argument
those sites can see.  Needs the GPU; run each part on its own, under a time limit:

    python tools/pow_boundary_check.py alpha          m_powf(alpha, k): all floats of [0.85, 1] x k = 0 ... 8 (the TNS LPC weighting), 2.3e7 evaluations
    python tools/pow_boundary_check.py pow2 [PART OF] m_powf(2, v): all floats of [-160, 160] (the regulariser, the decoder's SNS gains), 2.25e9 evaluations,
                                                      compared on the host in chunks; PART OF (0 2, 1 2): one of several runs over the range

Prints one line per part: arguments, how many differ in any bit, the first of them.  Exit status 1 when anything differs."""
import concurrent.futures
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK = 1 << 25
THREADS = 16


def host_lib():
    so = os.path.join(tempfile.mkdtemp(prefix="pow_boundary_"), "fastmath_host.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "audio_codec_amd", "csrc"),
                           os.path.join(ROOT, "tools", "fastmath_host.c"), "-o", so, "-lm"])
    H = C.CDLL(so)
    H.lc3m_host_eval.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_long]
    return H


def compare(L, H, pool, kind, host_kind, x, unit):
    """-> indices into x whose device and host results differ; the host side in THREADS slices, cut at multiples of `unit` so that i mod 9 stays what it is"""
    x = np.ascontiguousarray(x)
    dev, host = np.zeros_like(x), np.zeros_like(x)
    assert L.lc3hip_test_fastmath(kind, x.ctypes.data, dev.ctypes.data, x.size) == 0
    step = -(-x.size // THREADS // unit) * unit
    list(pool.map(lambda a: H.lc3m_host_eval(host_kind, x[a:].ctypes.data, host[a:].ctypes.data, min(step, x.size - a)), range(0, x.size, step)))
    return np.flatnonzero(dev.view(np.uint32) != host.view(np.uint32))


def bits(v):
    return int(np.array(v, np.float32).view(np.uint32))


def main():
    import audio_codec_amd
    L = audio_codec_amd.load_library()
    L.lc3hip_test_fastmath.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_longlong]
    H = host_lib()
    what = sys.argv[1]
    n = bad = 0
    first = []
    with concurrent.futures.ThreadPoolExecutor(THREADS) as pool:
        if what == "alpha":
            lo, hi = bits(0.85), bits(1.0)
            for a in range(lo, hi + 1, CHUNK // 9):
                u = np.arange(a, min(a + CHUNK // 9, hi + 1), dtype=np.uint32)
                x = np.repeat(u.view(np.float32), 9)
                d = compare(L, H, pool, 4, 7, x, 9)
                n += x.size; bad += d.size
                first += ["%08x^%d" % (u[i // 9], i % 9) for i in d[:8 - len(first)]]
            name = "alpha^k, alpha in [0.85, 1], k = 0 ... 8"
        else:
            part, of = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (0, 1)
            spans = [(0, bits(160.0) + 1), (0x80000000, bits(-160.0) + 1)]
            starts = [(a, min(a + CHUNK, hi)) for lo, hi in spans for a in range(lo, hi, CHUNK)]
            for a, b in starts[part::of]:
                u = np.arange(a, b, dtype=np.uint32)
                d = compare(L, H, pool, 3, 6, u.view(np.float32), 1)
                n += u.size; bad += d.size
                first += ["%08x" % u[i] for i in d[:8 - len(first)]]
            name = "2^v, v in [-160, 160], part %d of %d" % (part, of)
    print("%s: %d arguments, %d differ from glibc%s" % (name, n, bad, "".join(" " + f for f in first)), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
