"""Writes tests/golden/s1_signal_classes.npz and tests/golden/signal_classes_sha256.json from the compiled ETSI reference (oracle/_ref): for every
geometry of tests/signal_classes.py the reference encoder's frames of every stream, and for the decoder's geometries one SHA-256 per stream of the
reference decoder's PCM and status on those frames damaged by signal_classes.damage.  The PCM is not stored: signal_classes regenerates it, and the
JSON pins one SHA-256 per (class, fs, N, T, bitdepth).  Run from the repository root where oracle/_ref is built."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import signal_classes as sc                                     # noqa: E402
from lc3_harness import Ref, RefDecoder, have_ref               # noqa: E402


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def pcm_digests():
    out = {}
    for g, (fs, ms, hr, ch, rates, depth) in sc.GEOMS.items():
        N = sc.frame_len(fs, ms)
        for k, x in sc.classes(fs, N, sc.T, depth).items():
            out["%s/%d/%d/%d/%d" % (k, fs, N, sc.T, depth)] = sha(x)
    return out


def decoder_digests(geom, frames):
    _, labels, rr = sc.streams(geom)
    bad, bfi = sc.damage(frames, labels, [sc.stream_bytes(geom, r) for r in rr])
    pcm, st = sc.decode(geom, RefDecoder, bad, bfi)
    return np.array([sha(pcm[b], st[b]) for b in range(len(rr))])


def main():
    assert have_ref(), "oracle/_ref is not built"
    data = {}
    for g in sc.GEOMS:
        data["frames/" + g] = sc.encode(g, Ref, dual_mono=True)
        if g in sc.DEC_GEOMS:
            data["dec/" + g] = decoder_digests(g, data["frames/" + g])
    np.savez_compressed(os.path.join(HERE, "s1_signal_classes.npz"), **data)
    with open(os.path.join(HERE, "signal_classes_sha256.json"), "w") as f:
        json.dump(pcm_digests(), f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
