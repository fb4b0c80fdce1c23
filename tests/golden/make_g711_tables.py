#!/usr/bin/env python3
"""Writes tests/golden/g711_tables.npz: the four G.711 tables of the wire sample types LC3PLUS_PCM_ULAW / LC3PLUS_PCM_ALAW, from the rule stated in
include/lc3plus_batch.h, restated here in numpy (no library code is called).

    ulaw_expand, alaw_expand     int16 [256]    code 0 ... 255 -> sample
    ulaw_compress, alaw_compress uint8 [65536]  sample -32768 ... 32767 (index = sample + 32768) -> code

The CRC32 of each table (the expansions as little-endian int16) is checked against the figure the rule was published with before the file is written:
the tests read the file, python's audioop - where it exists - agrees with it up to the sign symmetry of the mu-law compression."""
import os
import zlib

import numpy as np

CRC = {"ulaw_expand": 0x0C847A9F, "alaw_expand": 0x9D764657, "ulaw_compress": 0x6399D432, "alaw_compress": 0x9133796E}


def expand(c, alaw):
    c = np.asarray(c, np.int64)
    k = (c ^ 0x55) if alaw else (~c & 0xFF)
    e, q = (k >> 4) & 7, k & 15
    if alaw:
        m = np.where(e == 0, (2 * q + 1) << 3, ((2 * q + 33) << np.maximum(e - 1, 0)) << 3)
        return np.where(k & 0x80, m, -m).astype(np.int16)
    m = ((2 * q + 33) << (e + 2)) - 132
    return np.where(c & 0x80, m, -m).astype(np.int16)


def _log2(a):
    """floor(log2 a) of positive integers, exactly"""
    r = np.zeros(a.shape, np.int64)
    for b in range(1, 16):
        r[a >= (1 << b)] = b
    return r


def compress(x, alaw):
    x = np.asarray(x, np.int64)
    s = x < 0
    y = np.where(s, ~x, x)                                           # one's complement: -1 has magnitude 0
    if alaw:
        m = y >> 4
        e = _log2(np.maximum(m, 1)) - 3
        c7 = np.where(m <= 15, m, (np.maximum(e, 1) << 4) | ((m >> np.maximum(e - 1, 0)) & 15))
        return ((c7 | np.where(s, 0, 0x80)) ^ 0x55).astype(np.uint8)
    a = np.minimum((y >> 2) + 33, 8191)
    e = _log2(a) - 5
    q = (a >> (e + 1)) & 15
    return (np.where(s, 0, 0x80) | ((7 - e) << 4) | (15 - q)).astype(np.uint8)


def tables():
    codes, samples = np.arange(256), np.arange(-32768, 32768)
    return {"ulaw_expand": expand(codes, False), "alaw_expand": expand(codes, True), "ulaw_compress": compress(samples, False),
            "alaw_compress": compress(samples, True)}


def crc(t):
    return zlib.crc32(t.astype("<i2").tobytes() if t.dtype == np.int16 else t.tobytes())


if __name__ == "__main__":
    t = tables()
    for name, want in CRC.items():
        assert crc(t[name]) == want, (name, "%08x" % crc(t[name]))
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "g711_tables.npz"), **t)
