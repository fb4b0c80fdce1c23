"""RTP framing (include/lc3plus_batch.h "RTP framing"): the two rules once more, in numpy and struct, written from RFC 3550 5.1 / 5.3.1, RFC 5761 4 and the
header's text and not from csrc/lc3_rtp_shim.h - parse() and stamp() - with the generators of the datagram sets and packet lists that tests/test_rtp_cpu.py and
tests/test_gpu_rtp.py share.  Everything here is host data; nothing touches a device."""
import functools
import struct

import numpy as np

OK, RANGE, SHORT, VERSION, RTCP, HEADER, PADDING, PAYLOAD_ROOM, UNKNOWN_SSRC, PAYLOAD_TYPE = range(10)
STATS_WORDS = 16
STAMPED, ST_BAD_ROUTE, ST_OVERFLOW, ST_RANGE = 1, 2, 4, 8
MARKER_NEVER, MARKER_AFTER_HOLE = 0, 1
EGR_SENT, EGR_PKT_OVERFLOW, EGR_STATS_WORDS = 1, 1, 4
PARSE_KEYS = ("stream", "seq", "offsets", "num_bytes", "timestamp", "marker", "status", "stats")
WIRE_FILL = 0xA5


def _lower_bound(keys, x):
    """the search of the header's text over keys as they stand (unsigned values), sorted or not"""
    lo, hi = 0, len(keys)
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if keys[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    return lo


def parse_one(ring, capacity, off, size, keys, streams, n_streams, payload_type, payload_room):
    """one datagram -> (status, stream, seq, offset, num_bytes, timestamp, marker)"""
    bad = lambda st: (st, -1, 0, 0, 0, 0, 0)
    if off < 0 or size < 0 or off + size > capacity:
        return bad(RANGE)
    if size < 12:
        return bad(SHORT)
    d = bytes(ring[off:off + size])
    b0, b1, seq, ts, ssrc = struct.unpack(">BBHII", d[:12])
    if b0 >> 6 != 2:
        return bad(VERSION)
    if 192 <= b1 <= 223:
        return bad(RTCP)
    h = 12 + 4 * (b0 & 15)
    if h > size:
        return bad(HEADER)
    if b0 & 0x10:
        if h + 4 > size:
            return bad(HEADER)
        h += 4 + 4 * struct.unpack(">H", d[h + 2:h + 4])[0]
        if h > size:
            return bad(HEADER)
    pad = 0
    if b0 & 0x20:
        pad = d[-1]
        if pad == 0 or h + pad > size:
            return bad(PADDING)
    if size - h - pad < payload_room:
        return bad(PAYLOAD_ROOM)
    k = _lower_bound(keys, ssrc)
    if k >= len(keys) or keys[k] != ssrc or not 0 <= streams[k] < n_streams:
        return bad(UNKNOWN_SSRC)
    s = int(streams[k])
    if payload_type is not None and payload_type[s] >= 0 and payload_type[s] != (b1 & 127):
        return bad(PAYLOAD_TYPE)
    return OK, s, seq, off + h + payload_room, size - h - pad - payload_room, ts, b1 >> 7


def parse(c):
    """the parse rule over a case (see case()) -> dict of PARSE_KEYS as api.plan_rtp_parse gives them"""
    n = len(c["dg_offsets"])
    keys = [int(k) & 0xFFFFFFFF for k in c["ssrc_key"]]
    streams = [int(s) for s in c["ssrc_stream"]]
    pt = None if c["payload_type"] is None else [int(v) for v in c["payload_type"]]
    out = dict(stream=np.zeros(n, np.int32), seq=np.zeros(n, np.int32), offsets=np.zeros(n, np.int64), num_bytes=np.zeros(n, np.int32),
               timestamp=np.zeros(n, np.int32), marker=np.zeros(n, np.uint8), status=np.zeros(n, np.uint8), stats=np.zeros(STATS_WORDS, np.int32))
    for i in range(n):
        st, s, seq, off, nb, ts, m = parse_one(c["ring"], c["ring_capacity"], int(c["dg_offsets"][i]), int(c["dg_sizes"][i]), keys, streams, c["n_streams"], pt,
                                               c["payload_room"])
        out["status"][i], out["stream"][i], out["seq"][i], out["offsets"][i], out["num_bytes"][i], out["marker"][i] = st, s, seq, off, nb, m
        out["timestamp"][i] = np.uint32(ts).astype(np.int32)
        out["stats"][st] += 1
    return out


def datagram(seq=0, ts=0, ssrc=0, pt=96, marker=0, version=2, csrc=(), ext=None, pad=None, payload=b"", b1=None):
    """an RTP datagram: csrc a tuple of 32-bit values; ext None or (profile, words as bytes of 4 * length); pad None or the padding count (the P bit is set and
    pad bytes are appended, the last of them the count - 0 gives a P bit over a last byte of 0)"""
    b0 = version << 6 | (0x20 if pad is not None else 0) | (0x10 if ext is not None else 0) | len(csrc)
    d = struct.pack(">BBHII", b0, (marker << 7 | pt) if b1 is None else b1, seq & 0xFFFF, ts & 0xFFFFFFFF, ssrc & 0xFFFFFFFF)
    d += b"".join(struct.pack(">I", v) for v in csrc)
    if ext is not None:
        assert len(ext[1]) % 4 == 0
        d += struct.pack(">HH", ext[0], len(ext[1]) // 4) + ext[1]
    d += payload
    if pad is not None:
        d += bytes(max(pad - 1, 0)) + bytes([pad & 255]) if pad > 0 else b""
    return d


def case(datagrams, n_streams, ssrc_key, ssrc_stream, payload_type=None, payload_room=0, gaps=None, ring_capacity=None, tail=0):
    """datagrams (bytes each) laid into a ring one after the other, gaps[i] bytes of 0xEE in front of datagram i (default 0), tail bytes behind the last"""
    at, offs, parts = 0, [], []
    for i, d in enumerate(datagrams):
        g = 0 if gaps is None else int(gaps[i])
        parts.append(bytes([0xEE]) * g)
        at += g
        offs.append(at)
        parts.append(d)
        at += len(d)
    parts.append(bytes([0xEE]) * tail)
    ring = np.frombuffer(b"".join(parts), np.uint8).copy()
    return dict(n_streams=n_streams, ring=ring, ring_capacity=ring.size if ring_capacity is None else ring_capacity, dg_offsets=np.array(offs, np.int64),
                dg_sizes=np.array([len(d) for d in datagrams], np.int32), ssrc_key=np.array(ssrc_key, np.int64), ssrc_stream=np.array(ssrc_stream, np.int32),
                payload_type=None if payload_type is None else np.array(payload_type, np.int32), payload_room=payload_room)


KEYS5 = (0x00000010, 0x00000200, 0x7FFFFFFF, 0x80000001, 0xFFFFFFF0)        # ascending as uint32; as int32 the last two are negative
STREAMS5 = (3, 0, 9, 1, 2)                                                  # 9: outside the 4 streams


@functools.lru_cache(maxsize=None)
def crafted(payload_room=0):
    """the crafted datagram set over the table KEYS5 / STREAMS5 and 4 streams whose payload types are 96, any, 97, 96 -> (case, {label: item index})"""
    body = bytes(range(1, 21))
    full = dict(seq=0xFFFE, ts=0xFFFFFFF0, ssrc=0x80000001, pt=96, marker=1, csrc=(7, 8, 9), ext=(0xBEDE, bytes(range(8))), pad=5, payload=body)
    d, labels = [], {}

    def add(label, g):
        labels[label] = len(d)
        d.append(g)
    for cc in range(16):
        add("cc%d" % cc, datagram(seq=cc, ts=1000 + cc, ssrc=0x10, pt=96, csrc=tuple(range(cc)), payload=body))
    for words in (0, 1, 5):
        add("x%d" % words, datagram(seq=100 + words, ssrc=0x200, pt=5, marker=1, ext=(1, bytes(4 * words)), payload=body))
    add("pad1", datagram(seq=200, ssrc=0x10, pad=1, payload=body))
    add("pad_all", datagram(seq=201, ssrc=0x10, pad=20, payload=b""))          # the padding is the whole payload: an empty frame
    add("pad0", datagram(seq=202, ssrc=0x10, pad=0, payload=body[:-1] + b"\0"))
    large = bytearray(datagram(seq=203, ssrc=0x10, payload=body[:-1] + bytes([21])))      # 21 bytes of padding in 20 bytes of payload
    large[0] |= 0x20
    add("pad_large", bytes(large))
    whole = datagram(**full)
    assert len(whole) == 12 + 12 + 4 + 8 + 20 + 5
    for k in range(len(whole) + 1):
        add("cut%d" % k, whole[:k])
    for v in (0, 1, 3):
        add("v%d" % v, datagram(version=v, ssrc=0x10, payload=body))
    for b1 in (191, 192, 223, 224):
        add("b1_%d" % b1, datagram(ssrc=0x200, b1=b1, payload=body))
    add("room_exact", datagram(seq=300, ssrc=0x10, payload=bytes(payload_room)))
    add("room_short", datagram(seq=301, ssrc=0x10, payload=bytes(max(payload_room - 1, 0))))
    for k, ssrc in enumerate((0x0F, 0x11, 0x201, 0x7FFFFFFE, 0x80000000, 0x80000002, 0xFFFFFFEF, 0xFFFFFFF1, 0xFFFFFFFF, 0)):
        add("unknown%d" % k, datagram(seq=400 + k, ssrc=ssrc, payload=body))
    add("top_bit", datagram(seq=410, ssrc=0x80000001, payload=body))
    add("top_key", datagram(seq=411, ssrc=0xFFFFFFF0, pt=97, payload=body))
    add("stream_out", datagram(seq=412, ssrc=0x7FFFFFFF, payload=body))
    add("pt_mismatch", datagram(seq=420, ssrc=0x10, pt=97, payload=body))     # stream 3 takes 96
    add("pt_any", datagram(seq=421, ssrc=0x200, pt=33, payload=body))         # stream 0 takes any
    for a in range(4):
        add("align%d" % a, datagram(seq=500 + a, ts=0x01020304, ssrc=0x80000001, csrc=(1,), ext=(2, bytes(4)), pad=2, payload=body))
    gaps = [3] * len(d)                                                   # 3 mod 4 between datagrams of all lengths: every alignment occurs
    for a in range(4):
        i = labels["align%d" % a]
        at = sum(gaps[:i]) + sum(len(x) for x in d[:i])
        gaps[i] = 3 + (a - (at + 3)) % 4
    c = case(d, 4, KEYS5, STREAMS5, payload_type=(-1, 96, 97, 96), payload_room=payload_room, gaps=gaps, tail=5)
    for a in range(4):
        assert c["dg_offsets"][labels["align%d" % a]] % 4 == a
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c, labels


@functools.lru_cache(maxsize=None)
def random_set(n=20000, seed=7, table=5):
    """n datagrams of sizes 0 ... 80 of random bytes, at random gaps; a third of them with byte 0 forced to version 2 and an SSRC of the table, so that the
    later checks are reached; a few offsets and sizes out of range.  table: the number of senders (5: KEYS5; else `table` random keys, sorted) over 7 streams"""
    rng = np.random.RandomState(seed)
    if table == 5:
        keys, streams = np.array(KEYS5, np.int64), np.array(STREAMS5, np.int32)
    elif table == 1:
        keys, streams = np.array([0x80000001], np.int64), np.array([6], np.int32)
    else:
        keys = np.unique(np.concatenate([rng.randint(0, 2 ** 32, size=table + 64, dtype=np.int64), np.array(KEYS5, np.int64)]))[:table]
        assert keys.size == table
        streams = rng.randint(-1, 8, size=table).astype(np.int32)
    sizes = rng.randint(0, 81, size=n)
    d = []
    for i in range(n):
        b = bytearray(rng.randint(0, 256, size=int(sizes[i]), dtype=np.int64).astype(np.uint8).tobytes())
        if i % 3 == 0 and len(b) >= 12:
            b[0] = 0x80 | (b[0] & 0x3F if i % 2 else b[0] & 0x03)
            b[1] = b[1] & 0x7F if b[1] & 0x60 == 0x40 else b[1]
            b[8:12] = struct.pack(">I", int(keys[rng.randint(keys.size)]))
            if i % 9 == 0:
                b[1] = (b[1] & 0x80) | 96
            if b[0] & 0x20 and i % 2:
                b[-1] = rng.randint(0, 6)
        d.append(bytes(b))
    c = case(d, 7, keys, streams, payload_type=(96, -1, 96, -1, 200, 0, -1), payload_room=3, gaps=rng.randint(0, 6, size=n), tail=3)
    off, size = c["dg_offsets"].copy(), c["dg_sizes"].copy()
    cap = c["ring_capacity"]
    off[5], size[6], size[7], off[8] = -1, -1, cap, cap                    # negative offset, negative size, past the end, at the end with a size
    off[9], size[9] = cap - 12, 13
    off[10], size[10] = 2 ** 62, 2 ** 31 - 1
    off[11], size[11] = cap, 0                                           # in range, and SHORT
    c["dg_offsets"], c["dg_sizes"] = off, size
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def subset(c, idx):
    """the case with the items idx only (the ring stays)"""
    return dict(c, dg_offsets=np.ascontiguousarray(c["dg_offsets"][idx]), dg_sizes=np.ascontiguousarray(c["dg_sizes"][idx]))


# ---- stamp ----
def stamp(c):
    """the stamp rule over a case (see stamp_case()) -> dict of wire, pkt_status, next_ts, next_resume as api.plan_rtp_stamp gives them"""
    R, T = len(c["ssrc"]), c["n_frames"]
    m = len(c["pkt_route"])
    n = min(m if c["n_packets"] is None else c["n_packets"], m)
    wire = np.array(c["wire"], np.uint8)
    status = np.zeros(m, np.uint8)
    cs = c["cell_status"]
    for p in range(max(n, 0)):
        r, t, off, size = int(c["pkt_route"][p]), int(c["pkt_frame"][p]), int(c["pkt_offset"][p]), int(c["pkt_size"][p])
        if not 0 <= r < R:
            status[p] = ST_BAD_ROUTE
        elif c["pkt_flags"] is not None and c["pkt_flags"][p] & EGR_PKT_OVERFLOW:
            status[p] = ST_OVERFLOW
        elif off < 0 or size < c["header_room"] or off + size > c["wire_capacity"] or not 0 <= t < T:
            status[p] = ST_RANGE
        else:
            status[p] = STAMPED
            mark = 0
            if c["marker_mode"] == MARKER_AFTER_HOLE:
                mark = int(not cs[r, t - 1] & EGR_SENT) if t > 0 else int(c["resume"] is not None and c["resume"][r] != 0)
            ts = (int(c["ts_base"][r]) + t * c["ts_step"]) & 0xFFFFFFFF
            h = struct.pack(">BBHII", 0x80, mark << 7 | (int(c["payload_type"][r]) & 127), int(c["pkt_seq"][p]) & 0xFFFF, ts, int(c["ssrc"][r]) & 0xFFFFFFFF)
            at = off + c["header_room"] - c["payload_room"] - 12
            wire[at:at + 12] = np.frombuffer(h, np.uint8)
    next_ts, next_resume = np.zeros(R, np.int32), np.zeros(R, np.uint8)
    for r in range(R):
        cnt = T if c["route_stats"] is None else min(max(int(c["route_stats"][r, 0]), 0), T)
        next_ts[r] = np.uint32((int(c["ts_base"][r]) + cnt * c["ts_step"]) & 0xFFFFFFFF).astype(np.int32)
        if cs is not None:
            next_resume[r] = (0 if c["resume"] is None else c["resume"][r]) if cnt == 0 else int(not cs[r, cnt - 1] & EGR_SENT)
    return dict(wire=wire, pkt_status=status, next_ts=next_ts, next_resume=next_resume if cs is not None else None)


def stamp_case(n, seed, header_room=12, payload_room=0, marker_mode=MARKER_AFTER_HOLE, resume=True, route_stats=True, flags=True, slack=0, spare=0, shift=0):
    """a packet list of n + spare entries (n_packets = n) over 5 routes x 9 frames as an egress might leave it, with what it must not leave mixed in: routes
    -1 and 5, overflow flags, negative offsets, sizes below header_room, packets past wire_capacity, frames -1 and 9.  Packets lie one behind the other from
    `shift`, 1 ... 40 bytes of frame each, `slack` bytes apart; sequence numbers and timestamps wrap"""
    rng = np.random.RandomState(seed)
    R, T, m = 5, 9, n + spare
    route, frame = rng.randint(0, R, size=m).astype(np.int32), rng.randint(0, T, size=m).astype(np.int32)
    size = (header_room + rng.randint(1, 41, size=m)).astype(np.int32)
    off = (shift + np.concatenate([[0], np.cumsum(size[:-1] + slack)])).astype(np.int64)
    total = int(off[-1] + size[-1])
    cap = int(off[n - 1] + size[n - 1]) - (int(size[n - 1]) // 2 if n > 8 else 0)      # the last packet in front of n_packets does not fit
    fl = np.zeros(m, np.uint8)
    seq = (65530 + np.arange(m) * 3).astype(np.int64)
    if n > 8:
        k = rng.permutation(n - 1)[:8]
        route[k[0]], route[k[1]] = -1, R
        fl[k[2]] = 1
        fl[k[3]] = 2                                                     # not the overflow bit
        off[k[4]] = -4
        size[k[5]] = header_room - 1
        frame[k[6]], frame[k[7]] = -1, T
    cs = np.where(rng.rand(R, T) < 0.6, EGR_SENT, rng.choice([2, 4, 8, 16], size=(R, T))).astype(np.uint8)
    cs[0, :] = EGR_SENT | 64
    st = np.zeros((R, EGR_STATS_WORDS), np.int32)
    st[:, 0] = [T, 0, 4, T + 3, -2]
    st[:, 1:] = rng.randint(0, 9, size=(R, 3))
    return dict(pkt_route=route, pkt_seq=seq, pkt_frame=frame, pkt_offset=off, pkt_size=size, pkt_flags=fl if flags else None, n_packets=n,
                ssrc=np.array([0x10, 0x80000001, 0xFFFFFFF0, 0, 0x7FFFFFFF], np.int64), ts_base=np.array([0, 0xFFFFFF00, 0x7FFFFFF0, 480, 0xFFFFFFFF], np.int64),
                payload_type=np.array([96, 127, 0, 200, -1], np.int32), ts_step=480, n_frames=T, marker_mode=marker_mode,
                cell_status=cs if marker_mode == MARKER_AFTER_HOLE or resume else None, resume=np.array([1, 0, 7, 0, 1], np.uint8) if resume else None,
                route_stats=st if route_stats else None, wire=np.full(total + 24, WIRE_FILL, np.uint8), wire_capacity=cap, header_room=header_room,
                payload_room=payload_room)
