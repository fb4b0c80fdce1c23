"""Writes tests/golden/d3_hostile_frames.npz from the compiled ETSI reference decoder (oracle/_ref) on the streams of tests/hostile_frames.py: per geometry
one SHA-256 over the arrays of streams(), one per stream over its payloads, the oracle's reason codes, the reference's per-frame status and one SHA-256 per
stream of its 16-bit PCM.  Neither payloads nor PCM are stored: hostile_frames regenerates the first, the digests pin the second.  Run from the repository
root where oracle/_ref is built."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hostile_frames as hf                                     # noqa: E402
from lc3_harness import RefDecoder, have_ref                    # noqa: E402


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def stream_digests(geom):
    frames, sizes, bfi, kind, reason = hf.streams(geom)
    return dict(sha=np.array(sha(frames, sizes, bfi, kind, reason)), payload=np.array([sha(frames[b]) for b in range(len(frames))]),
                reason=reason)


def decoder_digests(geom, dec_cls=None, **kw):
    frames, sizes, bfi, kind, reason = hf.streams(geom)
    o = hf.decode(geom, frames, sizes, bfi, dec_cls=dec_cls, **kw)
    return o["status"], np.array([sha(o["pcm"][b]) for b in range(len(frames))]), o


def main():
    assert have_ref(), "oracle/_ref is not built"
    data = {}
    for g in hf.GEOMS:
        for k, v in stream_digests(g).items():
            data["%s/%s" % (k, g)] = v
        data["status/" + g], data["pcm/" + g], _ = decoder_digests(g, RefDecoder)
    np.savez_compressed(os.path.join(HERE, "d3_hostile_frames.npz"), **data)


if __name__ == "__main__":
    main()
