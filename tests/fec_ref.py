"""Generic FEC (RFC 5109) restated: the encode rule and the recover rule of include/lc3plus_batch.h "Generic FEC" in plain Python, written from the header's text
and not from the C - no tiles, no workspace, no shared helper.  encode(c) and recover(c) take a case (a dict of the calls' arguments as numpy arrays) and give
what api.plan_fec_encode / api.plan_fec_recover give; the case builders below serve tests/test_fec_cpu.py and tests/test_gpu_fec.py alike."""
import numpy as np

MAX_GROUP, STATE_WORDS, PKT_EMPTY, PKT_OVERFLOW, STAMPED = 16, 8, 2, 1, 1
(RECOVERED, DROPPED, RANGE, SHORT, HEADER, LENGTH, COMPLETE, MISSING, PARTIAL, OVERFLOW) = range(10)
STATS_WORDS = 16
FILL = 0x5A
ENCODE_KEYS = ("state", "acc", "fec_wire", "n_fec", "fec_route", "fec_seq", "fec_frame", "fec_offset", "fec_size", "fec_flags", "fec_mask", "next_fec_seq", "route_stats")
RECOVER_KEYS = ("ring", "rec_dg_offsets", "rec_dg_sizes", "rec_seq", "status", "stats")


def be(v, n):
    return int(v).to_bytes(n, "big")


def fec_packet(members, sn_base, positions, long_mask=False):
    """the FEC payload (FEC header, level header, level-0 payload) over RTP packets `members` (bytes) at group positions `positions`"""
    b0 = b1 = ts = ln = 0
    plen = max(len(m) - 12 for m in members)
    pay = bytearray(plen)
    mask = 0
    for m, i in zip(members, positions):
        b0 ^= m[0] & 0x3F
        b1 ^= m[1]
        ts ^= int.from_bytes(m[4:8], "big")
        ln ^= len(m) - 12
        for k, x in enumerate(m[12:]):
            pay[k] ^= x
        mask |= 1 << ((47 if long_mask else 15) - i)
    return bytes([b0 | (0x40 if long_mask else 0), b1]) + be(sn_base, 2) + be(ts, 4) + be(ln, 2) + be(plen, 2) + be(mask, 6 if long_mask else 2) + bytes(pay)


class _Group:
    def __init__(self, K, sn):
        self.K, self.sn, self.fill, self.mask, self.b01, self.ts, self.ln, self.max, self.dead, self.pay, self.last = K, sn & 0xFFFF, 0, 0, 0, 0, 0, 0, False, bytearray(), 0

    def add(self, pkt):
        if self.dead:
            return
        self.mask |= 0x8000 >> self.fill
        self.b01 ^= (pkt[0] & 0x3F) | pkt[1] << 8
        self.ts ^= int.from_bytes(pkt[4:8], "big")
        n = len(pkt) - 12
        self.ln ^= n
        self.max = max(self.max, n)
        if len(self.pay) < n:
            self.pay.extend(bytes(n - len(self.pay)))
        for k in range(n):
            self.pay[k] ^= pkt[12 + k]


def route_count(c, r):
    if c.get("route_stats") is None:
        return int(c["n_frames"])
    return int(min(max(int(c["route_stats"][r][0]), 0), c["n_frames"]))


def encode(c):
    R, T = len(c["seq_base"]), int(c["n_frames"])
    hr, pr, fhr = int(c.get("header_room", 12)), int(c.get("payload_room", 0)), int(c.get("fec_header_room", 12))
    wire = np.asarray(c["wire"], np.uint8)
    wcap = wire.size if c.get("wire_capacity") is None else int(c["wire_capacity"])
    fec_wire = np.array(c["fec_wire"], np.uint8)
    fcap = fec_wire.size if c.get("fec_capacity") is None else int(c["fec_capacity"])
    stride = int(c["fec_stride"])
    m = len(c["pkt_route"])
    n = m if c.get("n_packets") is None else min(max(int(c["n_packets"]), 0), m)
    Q = R * T if c.get("max_fec_packets") is None else int(c["max_fec_packets"])
    carry = c.get("state") is not None
    A = int(c["acc_stride"]) if carry else 0
    # the members: the lowest entry that names a cell
    cell = {}
    for p in range(n):
        r, t = int(c["pkt_route"][p]), int(c["pkt_frame"][p])
        if not 0 <= r < R or not 0 <= t < route_count(c, r):
            continue
        if c.get("pkt_status") is not None and not int(c["pkt_status"][p]) & STAMPED:
            continue
        off, size = int(c["pkt_offset"][p]), int(c["pkt_size"][p])
        if off < 0 or size < hr or size > 1 << 20 or off + size > wcap:
            continue
        a = off + hr - pr - 12
        if off + size - a - 12 > 65535:
            continue
        cell.setdefault((r, t), bytes(wire[a:off + size]))
    out = dict(state=np.zeros((R, STATE_WORDS), np.int32) if carry else None, acc=np.zeros((R, A), np.uint8) if carry else None, fec_wire=fec_wire,
               fec_route=np.zeros(Q, np.int32), fec_seq=np.zeros(Q, np.int32), fec_frame=np.zeros(Q, np.int32), fec_offset=np.zeros(Q, np.int64),
               fec_size=np.zeros(Q, np.int32), fec_flags=np.zeros(Q, np.uint8), fec_mask=np.zeros(Q, np.int32), next_fec_seq=np.zeros(R, np.int32),
               route_stats=np.zeros((R, 4), np.int32))
    q = 0
    for r in range(R):
        cnt = route_count(c, r)
        k = min(max(int(c["group"][r]), 0), MAX_GROUP)
        flush = c.get("flush") is not None and int(c["flush"][r]) != 0
        g = None
        if carry:
            st = [int(x) for x in c["state"][r]]
            if 1 <= st[1] <= MAX_GROUP and 1 <= st[0] < st[1]:
                g = _Group(st[1], st[2])
                g.fill = st[0]
                g.dead = st[7] < 0 or st[7] > A or st[7] > 65535
                if not g.dead:
                    g.mask = st[3] & 0xFFFF & ~(0xFFFF >> g.fill)
                    g.b01, g.ts, g.ln, g.max = st[4] & 0xFF3F, st[5] & 0xFFFFFFFF, st[6] & 0xFFFF, st[7]
                    g.pay = bytearray(np.asarray(c["acc"][r][:g.max], np.uint8).tobytes())
        if cnt == 0:
            if carry:
                out["state"][r] = c["state"][r]
                out["acc"][r] = c["acc"][r]
            out["next_fec_seq"][r] = np.uint32(int(c["fec_seq_base"][r]) & 0xFFFFFFFF).astype(np.int32)
            continue
        closed = []
        for t in range(cnt):
            if g is None:
                if k == 0:
                    break
                g = _Group(k, int(c["seq_base"][r]) + t)
            if (r, t) in cell:
                g.add(cell[(r, t)])
            g.fill += 1
            g.last = t
            if g.fill == g.K:
                closed.append(g)
                g = None
        if g is not None and flush and g.fill > 0:
            closed.append(g)
            g = None
        for gi, x in enumerate(closed):
            out["route_stats"][r, 0] += 1
            size = fhr + 14 + x.max if x.mask else 0
            off = q * stride
            flags = PKT_EMPTY if not x.mask else PKT_OVERFLOW if (q >= Q or size > stride or off + size > fcap) else 0
            if q < Q:
                out["fec_route"][q], out["fec_frame"][q], out["fec_offset"][q], out["fec_size"][q] = r, x.last, off, size
                out["fec_seq"][q] = np.uint32((int(c["fec_seq_base"][r]) + gi) & 0xFFFFFFFF).astype(np.int32)
                out["fec_flags"][q], out["fec_mask"][q] = flags, x.mask
            if not flags:
                body = bytes([x.b01 & 0x3F, x.b01 >> 8]) + be(x.sn, 2) + be(x.ts, 4) + be(x.ln, 2) + be(x.max, 2) + be(x.mask, 2) + bytes(x.pay) + bytes(x.max - len(x.pay))
                fec_wire[off + fhr:off + size] = np.frombuffer(body, np.uint8)
                out["route_stats"][r, 1] += 1
                out["route_stats"][r, 2] += bin(x.mask).count("1")
                out["route_stats"][r, 3] += x.max
            q += 1
        out["next_fec_seq"][r] = np.uint32((int(c["fec_seq_base"][r]) + len(closed)) & 0xFFFFFFFF).astype(np.int32)
        if carry and g is not None:
            if g.dead or g.max > A:
                out["state"][r] = [g.fill, g.K, g.sn, 0, 0, 0, 0, -1]
            else:
                out["state"][r] = np.array([g.fill, g.K, g.sn, g.mask, g.b01, g.ts, g.ln, g.max], np.int64).astype(np.uint32).view(np.int32)
                out["acc"][r, :len(g.pay)] = np.frombuffer(bytes(g.pay), np.uint8)
    out["n_fec"] = q
    return out


def recover(c):
    S, W = int(c["n_streams"]), int(c["window"])
    ring = np.array(c["ring"], np.uint8)
    cap = ring.size if c.get("ring_capacity") is None else int(c["ring_capacity"])
    n, m = len(c["stream"]), len(c["fec_stream"])
    table = {}
    for i in range(n):
        s = int(c["stream"][i])
        if 0 <= s < S:
            table.setdefault((s, int(c["seq"][i]) & (W - 1)), i)
    out = dict(ring=ring, rec_dg_offsets=np.zeros(m, np.int64), rec_dg_sizes=np.zeros(m, np.int32), rec_seq=np.zeros(m, np.int32), status=np.zeros(m, np.uint8),
               stats=np.zeros(STATS_WORDS, np.int32))
    src = np.array(c["ring"], np.uint8)                               # what the datagrams held before the call

    def present(s, sn):
        i = table.get((s, sn & (W - 1)))
        if i is None or int(c["stream"][i]) != s or int(c["seq"][i]) & 0xFFFF != sn:
            return None
        off, size = int(c["dg_offsets"][i]), int(c["dg_sizes"][i])
        if off < 0 or size < 12 or off + size > cap:
            return None
        return bytes(src[off:off + size])

    def verdict(f):
        s, off, size = int(c["fec_stream"][f]), int(c["fec_offsets"][f]), int(c["fec_num_bytes"][f])
        if not 0 <= s < S:
            return DROPPED
        if off < 0 or size < 0 or off + size > cap:
            return RANGE
        if size < 14:
            return SHORT
        h = bytes(src[off:off + size])
        L = h[0] >> 6 & 1
        hl = 18 if L else 14
        if size < hl:
            return SHORT
        plen = int.from_bytes(h[10:12], "big")
        mask = int.from_bytes(h[12:hl], "big")
        bits = 48 if L else 16
        if h[0] & 0x80 or mask == 0 or plen == 0:
            return HEADER
        if hl + plen > size:
            return LENGTH
        sn0 = int.from_bytes(h[2:4], "big")
        b0, b1, ts, ln = h[0] & 0x3F, h[1], int.from_bytes(h[4:8], "big"), int.from_bytes(h[8:10], "big")
        pay = bytearray(h[hl:hl + plen])
        missing = []
        for i in range(bits):
            if not mask >> (bits - 1 - i) & 1:
                continue
            sn = (sn0 + i) & 0xFFFF
            pkt = present(s, sn)
            if pkt is None:
                missing.append(sn)
                continue
            b0 ^= pkt[0] & 0x3F
            b1 ^= pkt[1]
            ts ^= int.from_bytes(pkt[4:8], "big")
            ln ^= (len(pkt) - 12) & 0xFFFF
            for k, x in enumerate(pkt[12:12 + plen]):
                pay[k] ^= x
        if not missing:
            return COMPLETE
        if len(missing) > 1:
            return MISSING
        if ln > plen:
            return PARTIAL
        slot = int(c["rec_offset"]) + f * int(c["rec_stride"])
        if 12 + ln > int(c["rec_stride"]) or slot + int(c["rec_stride"]) > cap:
            return OVERFLOW
        pkt = bytes([0x80 | b0, b1]) + be(missing[0], 2) + be(ts, 4) + be(int(c["ssrc"][s]) & 0xFFFFFFFF, 4) + bytes(pay[:ln])
        ring[slot:slot + len(pkt)] = np.frombuffer(pkt, np.uint8)
        out["rec_dg_offsets"][f], out["rec_dg_sizes"][f], out["rec_seq"][f] = slot, len(pkt), missing[0]
        return RECOVERED

    for f in range(m):
        st = verdict(f)
        out["status"][f] = st
        out["stats"][st] += 1
    return out


# ---- cases ----
def rtp_packet(rng, seq, size, ts=None, ssrc=0x01020304, pt=96):
    """a plain RTP packet of `size` bytes (>= 12), payload random"""
    ts = int(rng.randint(0, 1 << 31)) if ts is None else ts
    return bytes([0x80, pt]) + be(seq & 0xFFFF, 2) + be(ts & 0xFFFFFFFF, 4) + be(ssrc, 4) + rng.randint(0, 256, size - 12).astype(np.uint8).tobytes()


def encode_case(seed, R, T, group, lo=20, hi=400, align=1, header_room=12, payload_room=0, fec_header_room=12, holes=0.12, acc_stride=None, hostile=True,
                fec_stride=None, counts=None, flush=None, seq_base=None, fec_seq_base=None):
    """a stamped packet list over a wire buffer of random bytes (so every header bit is exercised): R routes x T positions, frames of lo ... hi bytes behind
    header_room bytes each, offsets rounded up to align, a share of holes; with `hostile` also duplicates, unstamped entries, entries out of range and bad routes"""
    rng = np.random.RandomState(seed)
    route, frame, offset, size, status = [], [], [], [], []
    at = 0
    cells = [(r, t) for r in range(R) for t in range(T)]
    for r, t in cells:
        if rng.rand() < holes:
            continue
        nb = int(rng.randint(lo, hi + 1))
        at = (at + align - 1) // align * align
        route.append(r), frame.append(t), offset.append(at), size.append(header_room + nb), status.append(STAMPED)
        at += header_room + nb
        if hostile and rng.rand() < 0.05:                             # a second entry for the cell: the first wins
            route.append(r), frame.append(t), offset.append(max(at - 40, 0)), size.append(header_room + 8), status.append(STAMPED)
        if hostile and rng.rand() < 0.05:
            kind = rng.randint(5)
            route.append([-1, R, r, r, r][kind]), frame.append([t, t, T, (t + 1) % T, (t + 2) % T][kind])
            offset.append([0, 0, 0, -1, at][kind]), size.append(header_room + [4, 4, 4, 4, 50][kind]), status.append([1, 1, 1, 1, 0 if kind == 4 and rng.rand() < 0.5 else 1][kind])
    wire = rng.randint(0, 256, at + 3).astype(np.uint8)
    m = len(route) + 3                                                # three entries behind n_packets
    pad = lambda a, dt: np.array(a + [0, 0, 0], dt)
    group = np.full(R, group, np.int32) if np.isscalar(group) else np.asarray(group, np.int32)
    stats = None
    if counts is not None:
        stats = np.zeros((R, 4), np.int32)
        stats[:, 0] = counts
    if fec_stride is None:
        fec_stride = (fec_header_room + 14 + hi + payload_room + 15) & ~15
    Q = R * T
    return dict(pkt_route=pad(route, np.int32), pkt_frame=pad(frame, np.int32), pkt_offset=pad(offset, np.int64), pkt_size=pad(size, np.int32),
                pkt_status=pad(status, np.uint8), n_packets=m - 3, wire=wire, wire_capacity=at, header_room=header_room, payload_room=payload_room, n_frames=T,
                seq_base=np.asarray(seq_base if seq_base is not None else (65530 + 1000 * np.arange(R)) & 0xFFFF, np.int32), route_stats=stats, group=group,
                flush=None if flush is None else np.asarray(flush, np.uint8), fec_seq_base=np.asarray(fec_seq_base if fec_seq_base is not None else 7 + np.arange(R), np.int32),
                state=None, acc=None, acc_stride=acc_stride, fec_wire=np.full(Q * fec_stride + 5, FILL, np.uint8), fec_capacity=Q * fec_stride, fec_stride=fec_stride,
                fec_header_room=fec_header_room, max_fec_packets=Q)


def with_state(c, state=None, acc=None, acc_stride=None):
    """the case joined to a stream: state / acc of the previous call, or an empty start"""
    R = len(c["seq_base"])
    A = int(acc_stride or c["acc_stride"] or 416)
    return dict(c, acc_stride=A, state=np.zeros((R, STATE_WORDS), np.int32) if state is None else state, acc=np.zeros((R, A), np.uint8) if acc is None else acc)


def owned(c, r):
    """the bytes of fec_wire a call may write: those of its written packets"""
    own = np.zeros(len(r["fec_wire"]), bool)
    for q in range(min(r["n_fec"], len(r["fec_size"]))):
        if r["fec_size"][q] and not r["fec_flags"][q]:
            own[r["fec_offset"][q] + c["fec_header_room"]:r["fec_offset"][q] + r["fec_size"][q]] = True
    return own


def recover_case(seed, S, n_groups, k, losses, window=1024, sizes=(20, 200), long_mask=False, rec_stride=None, shuffle=True):
    """media datagrams of S streams in n_groups groups of k with one FEC packet each in one ring; losses(stream, group) -> the positions dropped from that group.
    -> the case and, per FEC item, the lost packets"""
    rng = np.random.RandomState(seed)
    ring, dg, items, fec, lost = bytearray(), [], [], [], []
    for s in range(S):
        base = int(rng.randint(0, 1 << 16))
        for g in range(n_groups):
            pk = [rtp_packet(rng, base + g * k + i, int(rng.randint(sizes[0], sizes[1] + 1)), ssrc=0x1000 + s) for i in range(k)]
            drop = set(losses(s, g))
            for i, p in enumerate(pk):
                if i in drop:
                    continue
                ring.extend(bytes(int(rng.randint(0, 4))))
                dg.append((len(ring), len(p), s, (base + g * k + i) & 0xFFFF))
                ring.extend(p)
            ring.extend(bytes(int(rng.randint(0, 4))))
            f = fec_packet(pk, (base + g * k) & 0xFFFF, range(k), long_mask)
            fec.append((s, len(ring), len(f)))
            lost.append([pk[i] for i in sorted(drop)])
            ring.extend(f)
    if shuffle:
        order = rng.permutation(len(dg))
        dg = [dg[i] for i in order]
    rec_stride = rec_stride or (12 + sizes[1] + 3) & ~3
    rec_offset = (len(ring) + 3) & ~3
    ring.extend(bytes([FILL]) * (rec_offset - len(ring) + len(fec) * rec_stride + 4))
    c = dict(n_streams=S, ring=np.frombuffer(bytes(ring), np.uint8), dg_offsets=np.array([d[0] for d in dg], np.int64), dg_sizes=np.array([d[1] for d in dg], np.int32),
             stream=np.array([d[2] for d in dg], np.int32), seq=np.array([d[3] for d in dg], np.int32), fec_stream=np.array([f[0] for f in fec], np.int32),
             fec_offsets=np.array([f[1] for f in fec], np.int64), fec_num_bytes=np.array([f[2] for f in fec], np.int32), ssrc=0x1000 + np.arange(S), window=window,
             rec_offset=rec_offset, rec_stride=rec_stride, ring_capacity=len(ring) - 4)
    return c, lost


def crafted_recover(window=1024):
    """every status once by construction, a 48-bit mask, bytes of a further level, and a window collision -> the case and {label: (FEC item, status)}"""
    rng = np.random.RandomState(77)
    ring, dg, fec, lab = bytearray(bytes(3)), [], [], {}

    def media(s, sn, size, keep=True, ssrc=None):
        p = rtp_packet(rng, sn, size, ssrc=0x1000 + s)
        if keep:
            dg.append((len(ring), len(p), s, sn & 0xFFFF))
            ring.extend(p)
            ring.extend(bytes(int(rng.randint(0, 3))))
        return p

    def item(label, s, body, status, size=None, off=None):
        lab[label] = (len(fec), status)
        fec.append((s, len(ring) if off is None else off, len(body) if size is None else size))
        ring.extend(body)
        ring.extend(bytes(int(rng.randint(0, 3))))

    def group(s, sn, k, drop, size=lambda i: 30 + 7 * i):
        return [media(s, sn + i, 12 + size(i), i not in drop) for i in range(k)]
    pk = group(0, 100, 4, ())
    item("complete", 0, fec_packet(pk, 100, range(4)), COMPLETE)
    pk = group(0, 200, 4, (1,))
    item("recovered", 0, fec_packet(pk, 200, range(4)), RECOVERED)
    item("levels", 0, fec_packet(pk, 200, range(4)) + bytes(range(9)), RECOVERED)
    item("twice", 0, fec_packet(pk[:2], 200, range(2)), RECOVERED)     # a second item recovers the same packet
    pk = group(0, 300, 4, (0, 3))
    item("missing", 0, fec_packet(pk, 300, range(4)), MISSING)
    pk = group(0, 65534, 4, (2,))                                      # the sequence numbers wrap
    item("wrap", 0, fec_packet(pk, 65534, range(4)), RECOVERED)
    good = fec_packet(pk, 65534, range(4))
    item("dropped", -1, good, DROPPED)
    item("stream_out", 2, good, DROPPED)
    item("neg", 0, good, RANGE, off=-1)
    item("neg_size", 0, good, RANGE, size=-3)
    item("past", 0, good, RANGE, off=1 << 40)
    item("short13", 0, good, SHORT, size=13)
    item("short17", 0, bytes([good[0] | 0x40]) + good[1:], SHORT, size=17)
    item("e_bit", 0, bytes([good[0] | 0x80]) + good[1:], HEADER)
    item("mask0", 0, good[:12] + bytes(2) + good[14:], HEADER)
    item("plen0", 0, good[:10] + bytes(2) + good[12:], HEADER)
    item("length", 0, good, LENGTH, size=len(good) - 1)
    pk = group(0, 400, 3, (1,))
    f = fec_packet(pk, 400, range(3))
    plen = int.from_bytes(f[10:12], "big")
    want = (plen + 1) ^ (len(pk[0]) - 12) ^ (len(pk[2]) - 12)          # the recovered length comes out as plen + 1
    item("partial", 0, f[:8] + be(want, 2) + f[10:], PARTIAL)
    pk = group(0, 500, 3, (2,), size=lambda i: 40 + 30 * i)            # the lost packet has 100 bytes behind its header: more than a slot holds
    item("overflow", 0, fec_packet(pk, 500, range(3)), OVERFLOW)
    pk = group(1, 7000, 20, (17,), size=lambda i: 20 + 2 * i)
    item("long", 1, fec_packet(pk, 7000, range(20), True), RECOVERED)
    pk = group(1, 7100, 5, (4,))
    item("long_sparse", 1, fec_packet([pk[0], pk[2], pk[4]], 7100, (0, 2, 4), True), RECOVERED)
    dg.append((dg[0][0], dg[0][1], 1, (5002 + window) & 0xFFFF))      # an earlier item of stream 1 with the residue of 5002
    pk = group(1, 5000, 4, (1,))
    item("collision", 1, fec_packet(pk, 5000, range(4)), MISSING)
    pk = group(1, 6000, 2, (0,))
    item("slot_cut", 1, fec_packet(pk, 6000, range(2)), OVERFLOW)      # the last slot ends behind ring_capacity
    rec_stride = 12 + 80
    rec_offset = (len(ring) + 3) & ~3
    ring.extend(bytes([FILL]) * (rec_offset - len(ring) + len(fec) * rec_stride))
    c = dict(n_streams=2, ring=np.frombuffer(bytes(ring), np.uint8), dg_offsets=np.array([d[0] for d in dg], np.int64), dg_sizes=np.array([d[1] for d in dg], np.int32),
             stream=np.array([d[2] for d in dg], np.int32), seq=np.array([d[3] for d in dg], np.int32), fec_stream=np.array([f[0] for f in fec], np.int32),
             fec_offsets=np.array([f[1] for f in fec], np.int64), fec_num_bytes=np.array([f[2] for f in fec], np.int32), ssrc=0x1000 + np.arange(2), window=window,
             rec_offset=rec_offset, rec_stride=rec_stride, ring_capacity=len(ring) - 1)
    return c, lab
