"""What packet egress has to answer (test infrastructure, a plain helper beside ingest_ref.py): the rule of include/lc3plus_batch.h "Packet egress" restated in
numpy from the header's text - classify every cell, number it by position, keep the SENT ones in list order, scan their padded sizes, gather the bytes - and the
cases the tests run it on.

rule(case) -> dict with the keys of api.plan_egress.  A case is a dict: n_streams, n_frames, frames (uint8), frames_capacity, offsets, num_bytes [S, T],
max_frame_bytes, flags [S, T] or None, skip_mask, counts [S] or None, route_src [R] or None, seq_base [R], seq_bits, order, wire (the buffer's contents before the
call, or None: in place), wire_capacity, header_room, align.  Everything is drawn from np.random.RandomState integer draws, so the cases are bit-reproducible."""
import functools

import numpy as np

SENT, LOST, INVALID, SKIPPED, ABSENT, BAD_ROUTE, OVERFLOW = 1, 2, 4, 8, 16, 32, 64
PKT_OVERFLOW = 1
STATS_WORDS = 4
STREAM_MAJOR, FRAME_MAJOR = 0, 1
PACK_CAP = 8                                            # api.ENC_FL_PACK_CAP: the skip mask a sender passes
LIST = ("pkt_route", "pkt_seq", "pkt_frame", "pkt_offset", "pkt_size", "pkt_flags")
KEYS = LIST + ("n_packets", "wire_total", "next_seq", "stats", "cell_status")
OPTIONAL = ("pkt_flags", "wire_total", "next_seq", "stats", "cell_status")
WIRE_FILL = 0x5A


def rule(c):
    S, T, bits = c["n_streams"], c["n_frames"], c["seq_bits"]
    mod = 1 << bits
    raw_base = np.asarray(c["seq_base"], np.int64)
    R = raw_base.size
    src = np.arange(R) if c["route_src"] is None else np.asarray(c["route_src"], np.int64)
    bad = (src < 0) | (src >= S)
    s = np.where(bad, 0, src)
    cnt = np.full(S, T, np.int64) if c["counts"] is None else np.clip(np.asarray(c["counts"], np.int64), 0, T)
    c_r = np.where(bad, 0, cnt[s])
    t = np.arange(T, dtype=np.int64)
    nb, off = np.asarray(c["num_bytes"], np.int64)[s], np.asarray(c["offsets"], np.int64)[s]
    fl = np.asarray(c["flags"], np.int64)[s] if c["flags"] is not None else np.zeros((R, T), np.int64)
    front = (t[None, :] < c_r[:, None]) & ~bad[:, None]
    lost = front & (nb == 0)
    invalid = front & ~lost & ((nb < 0) | (nb > c["max_frame_bytes"]) | (off < 0) | (off > c["frames_capacity"] - nb))
    skipped = front & ~lost & ~invalid & ((fl & c["skip_mask"]) != 0)
    sent = front & ~lost & ~invalid & ~skipped
    status = np.full((R, T), ABSENT, np.int64)
    status[lost], status[invalid], status[skipped], status[sent] = LOST, INVALID, SKIPPED, SENT
    status[bad] = BAD_ROUTE
    seq = ((raw_base % mod)[:, None] + t[None, :]) % mod
    # the list: the SENT cells in list order
    rr, tt = np.meshgrid(np.arange(R), t, indexing="ij")
    if c["order"] == FRAME_MAJOR:
        pick = lambda a: a.T[sent.T]
    else:
        pick = lambda a: a[sent]
    p_r, p_t, p_nb, p_src, p_seq = pick(rr), pick(tt), pick(nb), pick(off), pick(seq)
    n = p_r.size
    h, align = c["header_room"], c["align"]
    size = h + p_nb
    wire = None
    if c["wire"] is None:
        offset, total, fit = p_src, int(p_nb.sum()), np.ones(n, bool)
    else:
        adv = (size + align - 1) // align * align
        offset = np.cumsum(adv) - adv
        total = int(adv.sum())
        fit = offset + size <= c["wire_capacity"]
        wire = np.array(c["wire"], np.uint8)
        k = np.flatnonzero(fit)
        lens = p_nb[k]
        within = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
        wire[np.repeat(offset[k] + h, lens) + within] = np.asarray(c["frames"], np.uint8)[np.repeat(p_src[k], lens) + within]
    over = np.zeros((R, T), bool)
    over[p_r[~fit], p_t[~fit]] = True
    status[over] |= OVERFLOW
    cells = R * T
    def full(a, dt):
        out = np.zeros(cells, dt)
        out[:n] = a.astype(np.int64).astype(dt) if dt != np.int32 else (a.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        return out
    base32 = (raw_base & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    nxt = (((raw_base % mod) + c_r) % mod & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    holes = (lost | invalid | skipped).sum(axis=1)
    return dict(pkt_route=full(p_r, np.int32), pkt_seq=full(p_seq, np.int32), pkt_frame=full(p_t, np.int32), pkt_offset=full(offset, np.int64),
                pkt_size=full(size, np.int32), pkt_flags=full(np.where(fit, 0, PKT_OVERFLOW), np.uint8), n_packets=n, wire_total=total,
                next_seq=np.where(bad, base32, nxt).astype(np.int32), stats=np.stack([c_r, sent.sum(axis=1), holes, over.sum(axis=1)], axis=1).astype(np.int32),
                cell_status=status.astype(np.uint8), wire=wire)


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def routes(rng, S, kind):
    """route_src by kind: "identity" (None), "fan" (0, 1 or 3 routes per stream in turn, shuffled) or "fan_bad" (the same with routes out of range among them)"""
    if kind == "identity":
        return None
    src = [s for s in range(S) for _ in range((0, 1, 3)[s % 3])] or [0]
    if kind == "fan_bad":
        src += [-1, S, S + 5, -(1 << 31), (1 << 31) - 1]
    return rng.permutation(np.array(src, np.int64)).astype(np.int32)


def drawn(seed, S, T, kind="identity", bits=16, order=STREAM_MAJOR, wire=None, sizes=(20, 401), with_flags=True, with_counts=True, hostile=True, cut=None):
    """S streams x T frames packed at every byte alignment with gaps of 0 ... 3 bytes, the last frame ending exactly at frames_capacity.  hostile: about one
    frame in 12 each is lost (size 0), has a negative size, a size above max_frame_bytes, a negative offset, or ends one byte or far beyond the capacity.
    flags: random bytes, the skip bit set in about one of four.  counts: -2 ... T + 3, so 0, negative, below, equal to and above n_frames all occur.
    bases: 65530 ... 65535 in turn with 16 bits, 2^32 - 3 ... with 32.  wire: None (in place) or (header_room, align).  cut: None - a wire buffer that holds
    every packet, with slack - or what the capacity is cut to: "inside" the last packet, at the "end" of the last but one, "zero", or "short" by one byte of
    the first packet."""
    rng = np.random.RandomState(seed)
    lo, hi = sizes
    nb = rng.randint(lo, hi, size=(S, T)).astype(np.int64)
    gaps = rng.randint(0, 4, size=S * T)
    gaps[0] += 1
    place = rng.permutation(S * T)                                   # where each frame lies in the buffer: any order
    length = nb.reshape(-1)[place]
    start = np.cumsum(length + gaps) - length
    off = np.zeros(S * T, np.int64)
    off[place] = start
    off = off.reshape(S, T)
    cap = int((start + length).max())
    frames = rng.randint(0, 256, size=cap).astype(np.uint8)
    max_bytes = hi - 1
    if hostile:
        what = rng.randint(0, 72, size=(S, T))
        nb[what == 0] = 0
        nb[what == 1] = -rng.randint(1, 1 << 31, size=int((what == 1).sum()))
        nb[what == 2] = max_bytes + 1 + rng.randint(0, 3, size=int((what == 2).sum())) * 100000
        off[what == 3] = -1 - rng.randint(0, 2, size=int((what == 3).sum())) * (1 << 40)
        off[what == 4] = (cap - nb + 1)[what == 4]
        off[what == 5] = (1 << 62) - 1
    flags = rng.randint(0, 256, size=(S, T)).astype(np.uint8) & np.where(rng.randint(0, 4, size=(S, T)) == 0, 0xFF, 0xFF ^ PACK_CAP).astype(np.uint8) if with_flags else None
    counts = rng.randint(-2, T + 4, size=S).astype(np.int32) if with_counts else None
    if with_counts and S >= 5:
        counts[:5] = [0, -1, max(T - 1, 0), T, T + 1]
    route_src = routes(rng, S, kind)
    R = S if route_src is None else route_src.size
    base = (65530 + np.arange(R) % 6) if bits == 16 else ((1 << 32) - 3 + np.arange(R) % 3) % (1 << 32)
    c = dict(n_streams=S, n_frames=T, frames=frames, frames_capacity=cap, offsets=off, num_bytes=nb.astype(np.int32), max_frame_bytes=max_bytes, flags=flags,
             skip_mask=PACK_CAP, counts=counts, route_src=route_src, seq_base=base.astype(np.int64), seq_bits=bits, order=order, wire=None, wire_capacity=0,
             header_room=0, align=1)
    if wire is not None:
        c["header_room"], c["align"] = wire
        c["wire"] = np.zeros(1, np.uint8)
        r = rule(dict(c, wire_capacity=0))                           # the packets' places do not depend on the capacity
        n, total = r["n_packets"], r["wire_total"]
        ends = r["pkt_offset"][:n] + r["pkt_size"][:n]
        wcap = {None: total + 5, "inside": int(ends[-1]) - 3 if n else 0, "end": int(ends[-2]) if n > 1 else 0, "zero": 0,
                "short": int(ends[0]) - 1 if n else 0}[cut]
        c["wire"] = np.full(total + 64, WIRE_FILL, np.uint8)         # bytes at and past wire_capacity belong to the buffer's owner too
        c["wire_capacity"] = wcap
    return _freeze(c)


def by_hand():
    """2 streams, 3 routes, 4 frames, base 65534, written out"""
    frames = np.arange(100, dtype=np.uint8)
    c = dict(n_streams=2, n_frames=4, frames=frames, frames_capacity=100, offsets=np.array([[0, 10, 20, 30], [40, 50, 60, 96]], np.int64),
             num_bytes=np.array([[10, 0, 10, 10], [5, 41, 5, 5]], np.int32), max_frame_bytes=40, flags=np.array([[0, 0, 8, 7], [0, 0, 0, 0]], np.uint8), skip_mask=8,
             counts=np.array([4, 3], np.int32), route_src=np.array([1, 0, 0], np.int32), seq_base=np.array([65534, 65534, 9], np.int64), seq_bits=16,
             order=STREAM_MAJOR, wire=None, wire_capacity=0, header_room=0, align=1)
    return _freeze(c)


WIRES = ((0, 1), (12, 4), (13, 1), (16, 16), (3, 64))
COPY_SIZES = tuple(range(1, 41)) + (63, 64, 65, 255, 256, 257, 400, 625, 1250)


def copy_case(wire, cut=None, seed=0):
    """The copy: one stream per source alignment 0 ... 15, one frame per size of COPY_SIZES, each frame behind a gap that puts it at its stream's alignment;
    with the destinations of WIRES every pair of source and destination alignment mod 16 occurs"""
    rng = np.random.RandomState(1000 + seed)
    S, T = 16, len(COPY_SIZES)
    nb = np.tile(np.array(COPY_SIZES, np.int64), (S, 1))
    off = np.zeros((S, T), np.int64)
    at = 0
    for t in range(T):
        for s in range(S):
            at += (s - at) % 16
            off[s, t] = at
            at += nb[s, t]
    frames = rng.randint(0, 256, size=at).astype(np.uint8)
    c = dict(n_streams=S, n_frames=T, frames=frames, frames_capacity=at, offsets=off, num_bytes=nb.astype(np.int32), max_frame_bytes=1250, flags=None, skip_mask=0,
             counts=None, route_src=None, seq_base=np.arange(S, dtype=np.int64), seq_bits=16, order=(STREAM_MAJOR, FRAME_MAJOR)[seed % 2], wire=np.zeros(1, np.uint8),
             wire_capacity=0, header_room=wire[0], align=wire[1])
    r = rule(c)
    n, total = r["n_packets"], r["wire_total"]
    ends = r["pkt_offset"][:n] + r["pkt_size"][:n]
    k = n // 2
    c["wire_capacity"] = {None: total, "inside": int(ends[k]) - 7, "end": int(ends[k]), "zero": 0, "short": int(ends[0]) - 1}[cut]
    c["wire"] = np.full(total + 64, WIRE_FILL, np.uint8)
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def cpu_cases():
    """name -> case, for the host plan; asserts that every status and both packet flags occur in them"""
    out = {"by_hand": by_hand()}
    k = 0
    for bits in (16, 32):
        for order in (STREAM_MAJOR, FRAME_MAJOR):
            for kind in ("identity", "fan", "fan_bad"):
                tag = "%d_%s_%s" % (bits, "fm" if order else "sm", kind)
                k += 1
                out["inplace_" + tag] = drawn(k, 7, 9, kind, bits, order)
                out["wire_" + tag] = drawn(100 + k, 6, 11, kind, bits, order, wire=WIRES[k % len(WIRES)])
                out["cut_" + tag] = drawn(200 + k, 5, 6, kind, bits, order, wire=WIRES[(k + 1) % len(WIRES)], cut=("inside", "end", "zero", "short")[k % 4])
    out["one_cell"] = drawn(301, 1, 1, hostile=False, with_counts=False)
    out["one_frame"] = drawn(302, 9, 1, "fan_bad", wire=(12, 4))
    out["one_route"] = drawn(303, 1, 30, wire=(3, 64), order=FRAME_MAJOR)
    out["plain"] = drawn(304, 4, 5, with_flags=False, with_counts=False, hostile=False)
    out["two_tiles"] = drawn(305, 40, 67, "fan", sizes=(1, 9), wire=(0, 1), order=FRAME_MAJOR)      # more than one tile of the scan
    for w in WIRES:
        out["copy_%d_%d" % w] = copy_case(w, seed=w[0])
    seen, flags = 0, 0
    for c in out.values():
        r = rule(c)
        seen |= int(np.bitwise_or.reduce(r["cell_status"].reshape(-1)))
        flags |= int(np.bitwise_or.reduce(r["pkt_flags"][:r["n_packets"]])) if r["n_packets"] else 0
    assert seen == 127 and flags == PKT_OVERFLOW, (seen, flags)
    return out


GPU_SHAPES = ((1, 1), (3, 5), (70, 67), (1, 300), (300, 1), (600, 130), (2100, 130))


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """name -> case, for the kernels: shapes that fill neither waves nor workgroups nor tiles; 600 x 130 needs 77 tiles of the scan, 2100 x 130 more tiles
    than the base kernel takes in one pass of its loop"""
    out = {}
    k = 0
    for S, T in GPU_SHAPES:
        big = S * T > 50000
        for order in (STREAM_MAJOR, FRAME_MAJOR):
            k += 1
            kind = "identity" if big or S < 3 else ("fan", "fan_bad")[order]
            bits = (16, 32)[k % 2]
            wire = None if big and order == STREAM_MAJOR else WIRES[k % len(WIRES)]
            out["%dx%d_%s" % (S, T, "fm" if order else "sm")] = drawn(400 + k, S, T, kind, bits, order, wire=wire, sizes=(1, 9) if big else (20, 401),
                                                                      cut="inside" if k % 3 == 0 else None, with_counts=S * T > 20 or order == FRAME_MAJOR,
                                                                      hostile=S * T > 1)
    out["3x5_identity_inplace"] = drawn(450, 3, 5, "identity", 16, STREAM_MAJOR)
    out["70x67_identity_wire32"] = drawn(451, 70, 67, "identity", 32, FRAME_MAJOR, wire=(16, 16))
    out["70x67_fan_inplace"] = drawn(452, 70, 67, "fan_bad", 16, FRAME_MAJOR)
    return out
