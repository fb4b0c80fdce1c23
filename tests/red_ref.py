"""Redundant audio (include/lc3plus_batch.h "Redundant audio") restated in numpy and plain Python from RFC 2198 section 3 and the header's text: the pack rule
(pack), the unpack rule (unpack), and the cases both test files share.  Nothing here calls the library."""
import struct

import numpy as np

MAX_DEPTH, MAX_BLOCK, MAX_TS_OFFSET = 4, 1023, 16383
PKT_OVERFLOW, PKT_BAD = 1, 2
STATS_WORDS, UNPACK_STATS_WORDS = 4, 16
OK, DROPPED, RANGE, SHORT, DEPTH, LENGTH, PAYLOAD_TYPE = range(7)
DROP_TYPE, DROP_OFFSET, DROP_EMPTY = 8, 9, 10
SENT, LOST, INVALID, SKIPPED = 1, 2, 4, 8
WIRE_FILL, TAIL_FILL = 0xA5, 0x3C
PACK_KEYS = ("red_offset", "red_size", "red_flags", "red_blocks", "wire_total", "route_stats", "tail_bytes", "tail_sizes", "wire")
UNPACK_KEYS = ("stream", "seq", "offsets", "num_bytes", "timestamp", "gen", "status", "stats")


# ---- the pack rule ----
def cell_class(c, s, t):
    """the egress's cell rule for frame (s, t) in front of its stream's count"""
    nb, off = int(c["num_bytes"][s, t]), int(c["offsets"][s, t])
    if nb == 0:
        return LOST
    if nb < 0 or nb > c["max_frame_bytes"] or off < 0 or off + nb > c["frames_capacity"]:
        return INVALID
    if c["flags"] is not None and int(c["flags"][s, t]) & c["skip_mask"]:
        return SKIPPED
    return SENT


def stream_count(c, s):
    T = c["offsets"].shape[1]
    return T if c["counts"] is None else min(max(int(c["counts"][s]), 0), T)


def tail_entry(c, s, g):
    """entry g of stream s's tail input as bytes, None where there is none"""
    if c["tail_sizes"] is None or g >= c["max_depth"]:
        return None
    v = int(c["tail_sizes"][s, g])
    if not 1 <= v <= min(MAX_BLOCK, c["tail_stride"]):
        return None
    return bytes(c["tail_bytes"][s, g, :v])


def generation(c, s, u):
    """frame u of stream s as a redundant block: its bytes, None where it does not exist"""
    if u >= 0:
        if cell_class(c, s, u) != SENT:
            return None
        o = int(c["offsets"][s, u])
        return bytes(c["frames"][o:o + int(c["num_bytes"][s, u])])
    return tail_entry(c, s, -u - 1)


def block_header(pt, ts_offset, length):
    """RFC 2198: F = 1, the block's payload type, a 14-bit timestamp offset, a 10-bit length"""
    return struct.pack(">I", 1 << 31 | (pt & 127) << 24 | (ts_offset & 0x3FFF) << 10 | (length & 0x3FF))


def pack(c):
    """-> dict of PACK_KEYS as api.plan_red_pack gives them with every optional output asked for"""
    S, T = c["offsets"].shape
    R = len(c["block_pt"])
    m = len(c["pkt_route"])
    n = min(max(int(c["n_packets"]), 0), m)
    hr, align, D = c["header_room"], c["align"], c["max_depth"]
    out = dict(red_offset=np.zeros(m, np.int64), red_size=np.zeros(m, np.int32), red_flags=np.zeros(m, np.uint8), red_blocks=np.zeros(m, np.uint8),
               route_stats=np.zeros((R, STATS_WORDS), np.int32), wire=np.array(c["wire"], np.uint8))
    run = 0
    for p in range(n):
        r, t = int(c["pkt_route"][p]), int(c["pkt_frame"][p])
        out["red_offset"][p] = run
        s = -1
        if 0 <= r < R and 0 <= t < T:
            s = r if c["route_src"] is None else int(c["route_src"][r])
        if not 0 <= s < S or t >= stream_count(c, s) or cell_class(c, s, t) != SENT:
            out["red_flags"][p] = PKT_BAD
            continue
        primary = generation(c, s, t)
        depth = D if c["depth"] is None else min(max(int(c["depth"][r]), 0), D)
        total = hr + 1 + len(primary)
        carried, missed = [], 0
        for j in range(1, depth + 1):
            b = generation(c, s, t - j)
            if b is None:
                continue
            if len(b) <= MAX_BLOCK and j * c["ts_step"] <= MAX_TS_OFFSET and total + 4 + len(b) <= c["max_packet_bytes"]:
                carried.append((j, b))
                total += 4 + len(b)
            else:
                missed += 1
        carried.reverse()                                             # oldest first
        pt = int(c["block_pt"][r])
        payload = b"".join(block_header(pt, j * c["ts_step"], len(b)) for j, b in carried) + bytes([pt & 127]) + b"".join(b for _, b in carried) + primary
        assert hr + len(payload) == total
        out["red_size"][p] = total
        out["red_blocks"][p] = sum(1 << (j - 1) for j, _ in carried)
        st = out["route_stats"][r]
        st[0] += 1; st[1] += len(carried); st[2] += sum(len(b) for _, b in carried); st[3] += missed
        if run + total <= c["wire_capacity"]:
            out["wire"][run + hr:run + total] = np.frombuffer(payload, np.uint8)
        else:
            out["red_flags"][p] = PKT_OVERFLOW
        run += (total + align - 1) // align * align
    out["wire_total"] = run
    stride = c["tail_stride"]
    tb, ts = np.array(c["tail_fill"], np.uint8).reshape(S, D, stride), np.zeros((S, D), np.int32)
    for s in range(S):
        cnt = stream_count(c, s)
        for g in range(D):
            u = cnt - 1 - g
            b = generation(c, s, u) if u >= 0 else tail_entry(c, s, g - cnt)
            if b is not None and len(b) <= MAX_BLOCK:
                ts[s, g] = len(b)
                tb[s, g, :len(b)] = np.frombuffer(b, np.uint8)
    out["tail_bytes"], out["tail_sizes"] = tb, ts
    return out


def list_of(c, order_by_frame=False):
    """the in-place egress's list for the tables of c: the SENT cells in front of each route's count -> (pkt_route, pkt_frame)"""
    S, T = c["offsets"].shape
    cells = []
    for r in range(len(c["block_pt"])):
        s = r if c["route_src"] is None else int(c["route_src"][r])
        if 0 <= s < S:
            cells += [(r, t) for t in range(stream_count(c, s)) if cell_class(c, s, t) == SENT]
    if order_by_frame:
        cells.sort(key=lambda x: (x[1], x[0]))
    return np.array([x[0] for x in cells], np.int32), np.array([x[1] for x in cells], np.int32)


SIZES = (1, 20, 1023, 1024)
PACK_CALLS = (dict(counts=(7, 2, 0), depth=(4, 3, 2, 1, 0), header_room=12, align=1, max_packet_bytes=12 + 1 + 1024 + 1100),
              dict(counts=(2, 0, 7), depth=(0, 1, 7, -2, 4), header_room=13, align=4, max_packet_bytes=1 << 30),
              dict(counts=(0, 7, 3), depth=None, header_room=15, align=16, max_packet_bytes=15 + 1 + 20 + 4 + 1023 + 4 + 20))


def pack_tables(call, seed=0):
    """the tables of one of three consecutive calls (call 0, 1, 2; no list, no tails yet): 3 streams, 5 routes - stream 0 sent twice, route 4 bad - 7 frames of 1,
    20, 1023 and 1024 bytes at source offsets of every residue mod 4 and mod 16, a LOST, an INVALID and a SKIPPED frame, counts 0, 2 or 3 (below the depth) and 7"""
    k = PACK_CALLS[call]
    rng = np.random.RandomState(100 + 10 * call + seed)
    S, T = 3, 7
    nb = np.array([[SIZES[(s + t + call) % 4] for t in range(T)] for s in range(S)], np.int32)
    busy = int(np.argmax(k["counts"]))                                # the stream with 7 frames
    if call == 1:
        nb[busy, 2:] = (20, 1023, 1, 20, 1023)                        # five frames in a row that can all be carried: a packet with four blocks
    flags = np.zeros((S, T), np.uint8)
    off = np.zeros((S, T), np.int64)
    at = 0
    for s in range(S):
        for t in range(T):
            at += 1 + (3 * s + 5 * t + call) % 7                      # gaps of 1 ... 7 bytes: every residue
            off[s, t] = at
            at += int(nb[s, t])
    frames = rng.randint(0, 256, at + 5).astype(np.uint8)
    if call == 1:                                                     # a LOST and an INVALID frame (its offset) in front of the five
        nb[busy, 0], off[busy, 1] = 0, -3
    else:                                                             # a LOST, an INVALID (its size) and a SKIPPED frame in the busy stream's middle
        nb[busy, 2], nb[busy, 4] = 0, 2000
        flags[busy, 5] = 8 | 1
    flags[busy, 3] = 1                                                # a flag outside skip_mask: sent
    return dict(n_streams=S, frames=frames, frames_capacity=frames.size - 2, offsets=off, num_bytes=nb, max_frame_bytes=1024, flags=flags, skip_mask=8,
                counts=np.array(k["counts"], np.int32), route_src=np.array([0, 1, 2, 0, 9], np.int32), block_pt=np.array([96, 97, 98, 99 + 128, 100], np.int32),
                depth=None if k["depth"] is None else np.array(k["depth"], np.int32), max_depth=4, ts_step=480, max_packet_bytes=k["max_packet_bytes"],
                header_room=k["header_room"], align=k["align"], tail_stride=1024)


def pack_case(call, n, tails=None, seed=0, spare=3):
    """tables of pack_tables(call) with a list of n packets - the call's own list with BAD entries among it, repeated to n - and `spare` entries behind n_packets;
    tails: (tail_bytes, tail_sizes) of the previous call or None; a wire buffer that the last packets overflow"""
    c = pack_tables(call, seed)
    route, frame = list_of(c)
    bad = [(4, 0), (5, 1), (-1, 0), (0, 7), (1, -1), (int(np.argmin(c["counts"])), 6), (int(np.argmax(c["counts"])), 0 if call == 1 else 2)]      # ... and a LOST frame
    cells = []
    for i, x in enumerate(zip(route.tolist(), frame.tolist())):
        cells.append(x)
        if i % 3 == 1 and bad:
            cells.append(bad.pop(0))
    cells += bad
    cells = [cells[i % len(cells)] for i in range(n)] + [(0, 0)] * spare
    c.update(pkt_route=np.array([x[0] for x in cells], np.int32), pkt_frame=np.array([x[1] for x in cells], np.int32), n_packets=n)
    S, D, stride = 3, c["max_depth"], c["tail_stride"]
    c["tail_bytes"], c["tail_sizes"] = tails if tails is not None else (None, None)
    c["tail_fill"] = np.full((S, D, stride), TAIL_FILL, np.uint8)
    c["wire"], c["wire_capacity"] = np.zeros(0, np.uint8), 1 << 40
    sized = pack(dict(c, wire=np.zeros(0, np.uint8), wire_capacity=-1))          # nothing fits: sizes and offsets only
    live = np.flatnonzero(sized["red_size"][:n] > 0)
    cap = int(sized["wire_total"]) if len(live) < 4 else int(sized["red_offset"][live[-2]] + sized["red_size"][live[-2]] - 1)
    c["wire_capacity"] = cap
    c["wire"] = np.full(int(sized["wire_total"]) + 64, WIRE_FILL, np.uint8)
    return c


# ---- the unpack rule ----
def red_payload(blocks, primary, primary_pt=96):
    """an RFC 2198 payload: blocks [(pt, ts_offset, bytes)] in wire order, then the primary"""
    return b"".join(block_header(pt, to, len(b)) for pt, to, b in blocks) + bytes([primary_pt & 127]) + b"".join(b for _, _, b in blocks) + bytes(primary)


def unpack(c):
    """-> dict of UNPACK_KEYS as api.plan_red_unpack gives them with every optional output asked for"""
    n, K = len(c["stream"]), c["max_red"] + 1
    out = dict(stream=np.full(n * K, -1, np.int32), seq=np.zeros(n * K, np.int32), offsets=np.zeros(n * K, np.int64), num_bytes=np.zeros(n * K, np.int32),
               timestamp=np.zeros(n * K, np.int32), gen=np.zeros(n * K, np.uint8), status=np.zeros(n, np.uint8), stats=np.zeros(UNPACK_STATS_WORDS, np.int32))
    ring = c["ring"]
    for i in range(n):
        out["status"][i] = st = _unpack_item(c, i, ring, out, i * K)
        out["stats"][st] += 1
    return out


def _unpack_item(c, i, ring, out, slot):
    s, off, size = int(c["stream"][i]), int(c["offsets"][i]), int(c["num_bytes"][i])
    if not 0 <= s < c["n_streams"]:
        return DROPPED
    if off < 0 or size < 0 or off + size > c["ring_capacity"]:
        return RANGE
    data = bytes(ring[off:off + size])
    heads, pos = [], 0
    while True:
        if pos >= size:
            return SHORT
        if not data[pos] & 0x80:
            break
        if pos + 4 > size:
            return SHORT
        w = struct.unpack(">I", data[pos:pos + 4])[0]
        heads.append((w >> 24 & 127, w >> 10 & 0x3FFF, w & 0x3FF))
        pos += 4
    pt = data[pos] & 127
    pos += 1
    if len(heads) > c["max_red"]:
        return DEPTH
    if pos + sum(h[2] for h in heads) > size:
        return LENGTH
    want = -1 if c["block_pt"] is None else int(c["block_pt"][s])
    if want >= 0 and want != pt:
        return PAYLOAD_TYPE
    seq = int(c["seq"][i]) & 0xFFFFFFFF
    ts = 0 if c["timestamp"] is None else int(c["timestamp"][i]) & 0xFFFFFFFF
    i32 = lambda v: int(np.uint32(v & 0xFFFFFFFF).view(np.int32))

    def put(k, seq_, at, nb, ts_, gen):
        out["stream"][k], out["seq"][k], out["offsets"][k], out["num_bytes"][k], out["timestamp"][k], out["gen"][k] = s, seq_, at, nb, i32(ts_), min(gen, 255)
    at = off + pos
    for k, (bpt, to, ln) in enumerate(heads):
        if want >= 0 and want != bpt:
            out["stats"][DROP_TYPE] += 1
        elif to == 0 or to % c["ts_step"]:
            out["stats"][DROP_OFFSET] += 1
        elif ln == 0:
            out["stats"][DROP_EMPTY] += 1
        else:
            g = to // c["ts_step"]
            put(slot + 1 + k, (seq - g) & 0xFFFF, at, ln, ts - to, g)
        at += ln
    put(slot, i32(seq), at, off + size - at, ts, 0)
    return OK


def _items(payloads, streams, n_streams, max_red, ts_step=480, block_pt=None, shift=True):
    """payloads laid into a ring one behind the other, item i at an offset of residue i mod 4 -> an unpack case"""
    ring, offs = bytearray(), []
    for i, p in enumerate(payloads):
        while shift and len(ring) % 4 != i % 4:
            ring.append(0xEE)
        offs.append(len(ring))
        ring += p
    n = len(payloads)
    return dict(n_streams=n_streams, stream=np.array(streams, np.int32), seq=(65533 + 7 * np.arange(n)) & 0xFFFF, offsets=np.array(offs, np.int64),
                num_bytes=np.array([len(p) for p in payloads], np.int32), timestamp=(0xFFFFF000 + 480 * np.arange(n)) & 0xFFFFFFFF,
                ring=np.frombuffer(bytes(ring) + b"\xEE" * 3, np.uint8).copy(), ring_capacity=len(ring), max_red=max_red, block_pt=block_pt, ts_step=ts_step)


def crafted_unpack(max_red=4):
    """-> (case, labels): valid packets of 0 ... 4 blocks at every alignment, a header list truncated at every byte, lengths past the payload, five headers, every
    per-block drop, the payload-type refusal, dropped and out-of-range items"""
    blk = lambda j, n=5, pt=96: (pt, 480 * j, bytes(range(16 * j, 16 * j + n)))
    P, S, lab = [], [], {}

    def add(name, payload, stream=0):
        lab[name] = len(P)
        P.append(payload)
        S.append(stream)
    for k in range(5):
        for a in range(4):                                            # four copies: every alignment, since item i lies at residue i mod 4
            add("valid%d_%d" % (k, a), red_payload([blk(j, 3 + j) for j in range(k, 0, -1)], bytes(range(200, 220))), stream=a % 2)
    full = red_payload([blk(j) for j in range(4, 0, -1)], b"\x01\x02")
    for cut in range(len(full) + 1):
        add("cut%d" % cut, full[:cut])
    add("length", red_payload([(96, 480, bytes(5))], b"")[:-1])
    add("length_big", block_header(96, 480, 1023) + bytes([96]) + bytes(40))
    add("five", red_payload([blk(j % 4 + 1) for j in range(5)], b"\x09"))
    add("five_cut", red_payload([blk(j % 4 + 1) for j in range(5)], b"\x09")[:18])
    add("six", red_payload([blk(j % 4 + 1) for j in range(6)], b"\x09"))
    add("drop_type", red_payload([blk(2, pt=97), blk(1)], b"\x07\x08"))
    add("drop_zero", red_payload([(96, 0, b"ab"), blk(1)], b"\x07\x08"))
    add("drop_odd", red_payload([(96, 481, b"ab"), (96, 16383, b"c"), blk(1)], b"\x07\x08"))
    add("drop_empty", red_payload([(96, 960, b""), blk(1)], b"\x07\x08"))
    add("drop_all", red_payload([(97, 0, b""), (96, 0, b""), (96, 960, b"")], b""))
    add("far", red_payload([(96, 480 * 34, b"xyz")], b"\x05"))
    add("pt", red_payload([blk(1)], b"\x07", primary_pt=97))
    add("pt_any", red_payload([blk(1, pt=5)], b"\x07", primary_pt=97), stream=2)
    add("empty_primary", red_payload([blk(1)], b""))
    add("no_f", bytes([96]) + bytes(30))
    add("dropped", full, stream=-1)
    add("stream_out", full, stream=3)
    c = _items(P, S, 3, max_red, block_pt=np.array([96, 96, -1], np.int32))
    for name, (off, size) in dict(neg=(-1, 5), neg_size=(0, -1), past=(c["ring_capacity"] - 4, 5), huge=(1 << 62, 1 << 30)).items():
        lab[name] = len(c["stream"])
        c["stream"] = np.append(c["stream"], 0).astype(np.int32)
        c["seq"], c["timestamp"] = np.append(c["seq"], 5), np.append(c["timestamp"], 5)
        c["offsets"], c["num_bytes"] = np.append(c["offsets"], off), np.append(c["num_bytes"], size).astype(np.int32)
    return c, lab


def random_unpack(n=1000, seed=1, max_red=4):
    """n items of seeded random bytes, sizes 0 ... 60; a third get a run of plausible headers in front so that the later checks are reached"""
    rng = np.random.RandomState(seed)
    P = []
    for i in range(n):
        b = bytearray(rng.randint(0, 256, rng.randint(0, 61)).astype(np.uint8).tobytes())
        if i % 3 == 0:
            k = int(rng.randint(0, 6))
            head = b"".join(block_header(int(rng.choice([96, 96, 96, 97])), int(rng.choice([0, 480, 960, 1440, 481])), int(rng.randint(0, 9))) for _ in range(k))
            head += bytes([int(rng.choice([96, 96, 97]))])
            b[:len(head)] = head
            b = b[:max(len(b), int(rng.randint(0, len(head) + 12)))]
        P.append(bytes(b))
    return _items(P, rng.randint(-1, 4, n), 3, max_red, block_pt=np.array([96, -1, 96], np.int32))


def subset(c, idx):
    """the case c with the items idx alone (the ring stays whole)"""
    return dict(c, **{k: np.asarray(c[k])[idx] for k in ("stream", "seq", "offsets", "num_bytes", "timestamp")})
