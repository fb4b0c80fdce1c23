"""What the frame probe has to answer (test infrastructure, a plain helper beside hostile_frames.py): the record of include/lc3plus_batch.h "Frame probe"
composed from the CPU oracle's verdict on each channel's bytes.

The verdict on a channel's bytes depends on nothing but the bytes and the geometry, so each channel of a stream-frame goes through a MONO oracle decoder of
its own (OracleDecoder.last_reject, the trace) - also a second channel behind a refused first one, which a stereo decoder never parses - and the records of
both depths follow by the rule: FULL refuses for any reason, SIDE for reasons 1 - 4 alone, a later channel behind a refused one is skipped."""
import functools

import numpy as np

import hostile_frames as hf
from lc3_harness import OracleDecoder

WORDS = 48
ST_CONCEALED, ST_INVALID, ST_LOST, ST_SKIPPED = 1, 2, 4, 8
SIDE, FULL = 0, 1
SIDE_REASONS = (1, 2, 3, 4)
# words 3 ... 37 from the oracle's trace (lc3o_dec_trace): name, first word, count
FIELDS = (("bw_idx", 3, 1), ("lastnz", 4, 1), ("lsb_mode", 5, 1), ("gg_idx", 6, 1), ("fac_ns", 7, 1), ("nfilt", 8, 1), ("tns_order", 9, 2), ("tns_idx", 11, 16),
          ("scf_idx", 27, 7), ("ltpf", 34, 3), ("nres", 37, 1))
TNS_ORDER, TNS_IDX, NRES = 9, 11, 37


@functools.lru_cache(maxsize=None)
def _mono(fs, ms, hr):
    d = OracleDecoder(fs, 1, ms, hr, portable_math=True)
    return d, d.enable_trace()


@functools.lru_cache(maxsize=None)
def _chan(fs, ms, hr, payload):
    """(reason, body) of one channel's bytes: body = words 3 ... 47 as the trace has them after this frame (the side-information words are valid whenever the
    reason is not one of SIDE_REASONS: the oracle fills the trace behind dec_side)"""
    d, tr = _mono(fs, ms, hr)
    rc, _ = d.decode(np.frombuffer(payload, np.uint8))
    assert rc in (0, 2), rc
    why = d.last_reject()
    assert (rc == 2) == (why != 0)
    body = np.zeros(WORDS, np.int64)
    for name, at, n in FIELDS:
        v = getattr(tr[0], name)
        body[at:at + n] = list(v) if n > 1 else [v]
    return why, body


def records(fs, ms, hr, channels, payload):
    """payload: the bytes of one stream-frame (all channels; empty = lost) -> {SIDE: int64 [channels, WORDS], FULL: ...}.  The sizes the geometry refuses are
    not the oracle's to judge: invalid() below."""
    payload = bytes(bytearray(np.asarray(payload, np.uint8).tolist())) if not isinstance(payload, bytes) else payload
    out = {SIDE: np.zeros((channels, WORDS), np.int64), FULL: np.zeros((channels, WORDS), np.int64)}
    if len(payload) == 0:
        for r in out.values():
            r[:, 0] = ST_CONCEALED | ST_LOST
        return out
    at = 0
    refused = {SIDE: False, FULL: False}
    for c, z in enumerate(hf.channel_sizes(len(payload), channels)):
        why, body = _chan(fs, ms, hr, payload[at:at + z])
        at += z
        for depth, r in out.items():
            r[c, 2] = z
            if refused[depth]:
                r[c, 0] = ST_CONCEALED | ST_SKIPPED
            elif why and (depth == FULL or why in SIDE_REASONS):
                r[c, 0], r[c, 1] = ST_CONCEALED, why
                refused[depth] = True
            else:
                r[c, 3:] = body[3:]
                if depth == SIDE:                              # the two filter flags; nothing of the coded part
                    r[c, TNS_ORDER:TNS_ORDER + 2] = body[TNS_ORDER:TNS_ORDER + 2] > 0
                    r[c, TNS_IDX:TNS_IDX + 16] = 0
                    r[c, NRES] = 0
    return out


def invalid(channels):
    r = np.zeros((channels, WORDS), np.int64)
    r[:, 0] = ST_CONCEALED | ST_INVALID
    return r


@functools.lru_cache(maxsize=None)
def geom_items(geom):
    """the B x 24 stream-frames of hostile_frames.streams(geom), stream-major -> (payloads [bytes], {depth: int64 [n, channels, WORDS]}); read-only"""
    fs, ms, hr, ch, _ = hf.GEOMS[geom]
    frames, sizes, bfi, kind, reason = hf.streams(geom)
    B, T = sizes.shape
    pl = [frames[b, t, :sizes[b, t]].tobytes() for b in range(B) for t in range(T)]
    rec = [records(fs, ms, hr, ch, p) for p in pl]
    want = {d: np.stack([r[d] for r in rec]) for d in (SIDE, FULL)}
    # the stereo oracle's own verdict on the unflagged frames (hostile_frames.streams: reason [B * channels, T]) is the composed one
    for b in range(B):
        for t in range(T):
            if not bfi[b, t]:
                for c in range(ch):
                    assert want[FULL][b * T + t, c, 1] == reason[b * ch + c, t], (geom, b, t, c)
    for a in want.values():
        a.flags.writeable = False
    return pl, want
