"""Generic FEC, repair across calls, restated: the rule of include/lc3plus_batch.h "Generic FEC", REPAIR, in plain Python, written from the header's text and not
from the C - no workspace, no claims, no lanes: the steps one after the other over dicts and lists.  repair() takes what packet.plan_fec_repair takes and gives what
it gives; closure() is the fixed point of "a group with one member missing yields that member" over sets of numbers alone; Receiver lays a call's datagrams into
a ring in front of the history and serves tests/test_fec_repair_cpu.py and tests/test_gpu_fec_repair.py alike."""
import numpy as np

from fec_ref import fec_packet, rtp_packet  # noqa: F401  (the case builders of the tests use them through this module)

(RECOVERED, DROPPED, RANGE, SHORT, HEADER, LENGTH, COMPLETE, MISSING, PARTIAL, OVERFLOW, STALE, DUPLICATE, OVERSIZE, EXPIRED, TWIN) = range(15)
STORED = 0
STATS_WORDS, STATE_WORDS = 16, 4
STORES = ("ring", "med_seq", "med_size", "fec_store", "cell_seq", "cell_size", "cell_status", "state")
OUTPUTS = STORES + ("rec_dg_offsets", "rec_dg_sizes", "rec_seq", "item_status", "fec_status", "stats")


def d16(a, b):
    """d(a, b) = (int16)(a - b)"""
    v = (a - b) & 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def fec_fields(b):
    """the fields of an FEC payload: (b0, b1, sn base, ts, length recovery, plen, the protected positions, the header's bytes); None where it is too short"""
    if len(b) < 14 or (b[0] & 0x40 and len(b) < 18):
        return None
    long_mask = bool(b[0] & 0x40)
    bits = 48 if long_mask else 16
    mask = int.from_bytes(b[12:18 if long_mask else 14], "big")
    pos = [i for i in range(bits) if mask >> (bits - 1 - i) & 1]
    return b[0], b[1], int.from_bytes(b[2:4], "big"), int.from_bytes(b[4:8], "big"), int.from_bytes(b[8:10], "big"), int.from_bytes(b[10:12], "big"), pos, 18 if long_mask else 14


def repair(n_streams, stores, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, fec_seq, ssrc, passes=1, ring_capacity=None):
    S, H, P = int(n_streams), int(stores["med_slots"]), int(stores["fec_slots"])
    mo, ms, fs = int(stores["med_offset"]), int(stores["med_stride"]), int(stores["fec_stride"])
    ring = np.array(stores["ring"], np.uint8).reshape(-1)
    cap = ring.size if ring_capacity is None else int(ring_capacity)
    med_seq, med_size = np.array(stores["med_seq"], np.int32), np.array(stores["med_size"], np.int32)
    fec_store = np.array(stores["fec_store"], np.uint8)
    cell_seq, cell_size, cell_status = np.array(stores["cell_seq"], np.int32), np.array(stores["cell_size"], np.int32), np.array(stores["cell_status"], np.uint8)
    state = np.array(stores["state"], np.int32)
    n, m = len(stream), len(fec_stream)
    item_status, fec_status, stats = np.zeros(n, np.uint8), np.zeros(m, np.uint8), np.zeros(STATS_WORDS, np.int32)
    rec_off, rec_size, rec_seq = np.zeros(S * P, np.int64), np.zeros(S * P, np.int32), np.zeros(S * P, np.int32)

    def slot_at(s, j):
        return mo + (s * H + j) * ms

    # 1 usable
    def in_history(off, size):
        return size > 0 and off < mo + S * H * ms and off + size > mo

    def media_code(i):
        s, off, size = int(stream[i]), int(dg_offsets[i]), int(dg_sizes[i])
        if not 0 <= s < S:
            return DROPPED
        if off < 0 or size < 0 or off + size > cap or in_history(off, size):
            return RANGE
        if size < 12:
            return SHORT
        return OVERSIZE if size > ms else 0

    def fec_code(f):
        s, off, size = int(fec_stream[f]), int(fec_offsets[f]), int(fec_num_bytes[f])
        if not 0 <= s < S:
            return DROPPED
        if off < 0 or size < 0 or off + size > cap or in_history(off, size):
            return RANGE
        h = fec_fields(bytes(ring[off:off + size]))
        if h is None:
            return SHORT
        if h[0] & 0x80 or not h[6] or not h[5]:
            return HEADER
        if h[7] + h[5] > size:
            return LENGTH
        return OVERSIZE if size > fs else 0

    kinds = ((0, n, media_code, stream, seq, H), (1, m, fec_code, fec_stream, fec_seq, P))
    codes = [[code(i) for i in range(cnt)] for _, cnt, code, _, _, _ in kinds]
    # 2 heads
    valid, head = np.zeros((2, S), bool), np.zeros((2, S), np.int64)
    was = np.zeros((2, S), bool)
    for kind, cnt, _, strm, sq, _ in kinds:
        for s in range(S):
            usable = [int(sq[i]) & 0xFFFF for i in range(cnt) if not codes[kind][i] and int(strm[i]) == s]
            was[kind, s] = bool(int(state[s, 0]) >> kind & 1)
            if was[kind, s]:
                base = int(state[s, 1 + kind]) & 0xFFFF
            elif usable:
                base = usable[0]
            else:
                continue
            valid[kind, s] = True
            head[kind, s] = (base + max([0] + [d16(x, base) for x in usable])) & 0xFFFF

    def behind(s, sn):
        return d16(int(head[0, s]), sn) >= H

    def cell_fields(s, j):
        return fec_fields(bytes(fec_store[s, j, :int(cell_size[s, j])]))

    # 3 expiry
    for s in range(S):
        if valid[0, s]:
            for j in range(H):
                if not (was[0, s] and med_size[s, j] > 0 and ((int(head[0, s]) - int(med_seq[s, j])) & 0xFFFF) < H):
                    med_seq[s, j] = med_size[s, j] = 0
        if valid[1, s]:
            for j in range(P):
                live = was[1, s] and cell_size[s, j] > 0 and ((int(head[1, s]) - int(cell_seq[s, j])) & 0xFFFF) < P
                if live and valid[0, s]:
                    h = cell_fields(s, j)
                    live = not all(behind(s, (h[2] + i) & 0xFFFF) for i in h[6])
                if not live:
                    cell_seq[s, j] = cell_size[s, j] = cell_status[s, j] = 0
    # 4 admission
    fresh = set()                                                     # the cells stored in this call
    item_cell = {}
    for i in range(n):
        if codes[0][i]:
            item_status[i] = codes[0][i]
            continue
        s, sn, size, off = int(stream[i]), int(seq[i]) & 0xFFFF, int(dg_sizes[i]), int(dg_offsets[i])
        if ((int(head[0, s]) - sn) & 0xFFFF) >= H:
            item_status[i] = STALE
        elif med_size[s, sn & (H - 1)] > 0:
            item_status[i] = DUPLICATE
        else:
            j = sn & (H - 1)
            med_seq[s, j], med_size[s, j] = sn, size
            ring[slot_at(s, j):slot_at(s, j) + size] = ring[off:off + size].copy()
    for f in range(m):
        if codes[1][f]:
            fec_status[f] = codes[1][f]
            continue
        s, sn, size, off = int(fec_stream[f]), int(fec_seq[f]) & 0xFFFF, int(fec_num_bytes[f]), int(fec_offsets[f])
        if ((int(head[1, s]) - sn) & 0xFFFF) >= P:
            fec_status[f] = STALE
        elif cell_size[s, sn & (P - 1)] > 0:
            fec_status[f] = DUPLICATE
        else:
            j = sn & (P - 1)
            cell_seq[s, j], cell_size[s, j], cell_status[s, j] = sn, size, MISSING
            fec_store[s, j, :size] = ring[off:off + size]
            fresh.add((s, j))
            item_cell[f] = (s, j)
    # 5 passes
    for _ in range(int(passes)):
        seq0, size0, ring0 = med_seq.copy(), med_size.copy(), ring.copy()          # the history as the pass finds it
        writes = {}
        for s in range(S):
            if not valid[1, s]:
                continue
            for j in range(P):
                if cell_size[s, j] <= 0 or cell_status[s, j] != MISSING:
                    continue
                b0, b1, base, ts, ln, plen, pos, hl = cell_fields(s, j)
                numbers = [(base + i) & 0xFFFF for i in pos]
                present = [x for x in numbers if valid[0, s] and size0[s, x & (H - 1)] > 0 and int(seq0[s, x & (H - 1)]) & 0xFFFF == x]
                missing = [x for x in numbers if x not in present]
                if not missing:
                    st = COMPLETE
                elif valid[0, s] and any(behind(s, x) for x in missing if d16(x, int(head[0, s])) <= 0):
                    st = EXPIRED
                elif len(missing) > 1 or not valid[0, s] or d16(missing[0], int(head[0, s])) > 0:
                    st = MISSING
                else:
                    pay = bytearray(fec_store[s, j, hl:hl + plen].tobytes())
                    for x in present:
                        a = slot_at(s, x & (H - 1))
                        pk = bytes(ring0[a:a + int(size0[s, x & (H - 1)])])
                        b0 ^= pk[0] & 0x3F
                        b1 ^= pk[1]
                        ts ^= int.from_bytes(pk[4:8], "big")
                        ln ^= (len(pk) - 12) & 0xFFFF
                        for k, v in enumerate(pk[12:12 + plen]):
                            pay[k] ^= v
                    if ln > plen:
                        st = PARTIAL
                    elif 12 + ln > ms:
                        st = OVERFLOW
                    else:
                        st = RECOVERED
                        x = missing[0]
                        pkt = bytes([0x80 | (b0 & 0x3F), b1]) + x.to_bytes(2, "big") + ts.to_bytes(4, "big") + (int(ssrc[s]) & 0xFFFFFFFF).to_bytes(4, "big") + bytes(pay[:ln])
                        if (s, x) in writes:
                            st = TWIN
                        else:
                            writes[(s, x)] = (j, pkt)
                if st != MISSING:
                    cell_status[s, j] = st
                    if (s, j) not in fresh:
                        stats[st] += 1
        for (s, x), (j, pkt) in writes.items():
            k = x & (H - 1)
            ring[slot_at(s, k):slot_at(s, k) + len(pkt)] = np.frombuffer(pkt, np.uint8)
            med_seq[s, k], med_size[s, k] = x, len(pkt)
            rec_off[s * P + j], rec_size[s * P + j], rec_seq[s * P + j] = slot_at(s, k), len(pkt), x
    # 6 reports
    for f, (s, j) in item_cell.items():
        fec_status[f] = cell_status[s, j]
    for f in range(m):
        stats[fec_status[f]] += 1
    for s in range(S):
        if valid[0, s] or valid[1, s]:
            state[s] = (int(valid[0, s]) | int(valid[1, s]) << 1, head[0, s] if valid[0, s] else state[s, 1], head[1, s] if valid[1, s] else state[s, 2], 0)
    out = dict(ring=ring, med_seq=med_seq, med_size=med_size, fec_store=fec_store, cell_seq=cell_seq, cell_size=cell_size, cell_status=cell_status, state=state,
               rec_dg_offsets=rec_off, rec_dg_sizes=rec_size, rec_seq=rec_seq, item_status=item_status, fec_status=fec_status, stats=stats)
    out.update({k: stores[k] for k in ("med_offset", "med_slots", "med_stride", "fec_slots", "fec_stride")})
    return out


def closure(media, groups):
    """media: the delivered sequence numbers; groups: the protected numbers of every delivered FEC packet -> the numbers rebuilt at the fixed point of "a group
    with exactly one member missing yields that member" """
    have, rebuilt = set(media), set()
    while True:
        new = {next(iter(set(g) - have)) for g in groups if len(set(g) - have) == 1}
        if not new:
            return rebuilt
        have |= new
        rebuilt |= new


class Receiver:
    """A receiver's stores and the arrivals of its calls: `area` bytes in front of the history take a call's datagrams, at the byte alignment `align`.  call(fn,
    media, fec) lays the datagrams down - media: (stream, seq, RTP packet bytes), fec: (stream, fec_seq, FEC payload bytes) - and runs fn (packet.plan_fec_repair,
    repair above, or a DecBatch's fec_repair) on them; the stores it returns are the next call's."""

    def __init__(self, packet, n_streams, ssrc=None, med_slots=16, med_stride=416, fec_slots=4, fec_stride=432, area=1 << 14, fill=0, align=0, tail=0):
        self.S, self.area, self.align, self.fill = n_streams, (area + 15) & ~15, align, fill
        self.ssrc = np.arange(n_streams, dtype=np.int64) + 0x01020304 if ssrc is None else np.asarray(ssrc)
        ring = np.full(self.area + n_streams * med_slots * med_stride + tail, fill, np.uint8)
        self.stores = packet.fec_repair_stores(n_streams, ring, self.area, med_slots, med_stride, fec_slots, fec_stride)
        self.last = None

    def lay(self, media, fec):
        ring = np.array(self.stores["ring"], np.uint8)
        ring[:self.area] = self.fill
        at, lists = 16 + self.align, ([], [], [], [], [], [], [], [])
        for kind, items in ((0, media), (1, fec)):
            for s, sn, b in items:
                assert at + len(b) <= self.area, "the arrival area is too small for this call"
                ring[at:at + len(b)] = np.frombuffer(bytes(b), np.uint8)
                for lst, v in zip(lists[4 * kind:4 * kind + 4], (at, len(b), s, sn)):
                    lst.append(v)
                at += len(b)
                at += -(at - self.align) % 4                            # every datagram at the same byte alignment
        return ring, lists

    def call(self, fn, media=(), fec=(), passes=1, **kw):
        ring, (o, z, s, q, fo, fz, fs, fq) = self.lay(media, fec)
        self.last = fn(dict(self.stores, ring=ring), np.array(o, np.int64), np.array(z, np.int32), np.array(s, np.int32), np.array(q, np.int32), np.array(fs, np.int32),
                       np.array(fo, np.int64), np.array(fz, np.int32), np.array(fq, np.int32), self.ssrc, passes=passes, **kw)
        self.stores = {k: self.last[k] for k in self.stores}
        return self.last

    def packet_at(self, s, sn):
        """the stored media packet of that number, or None"""
        H, j = self.stores["med_slots"], sn & (self.stores["med_slots"] - 1)
        if self.stores["med_size"][s, j] <= 0 or int(self.stores["med_seq"][s, j]) != sn & 0xFFFF:
            return None
        a = self.stores["med_offset"] + (s * H + j) * self.stores["med_stride"]
        return bytes(self.stores["ring"][a:a + int(self.stores["med_size"][s, j])])


def ref(n_streams):
    """repair() with plan_fec_repair's argument order behind the stream count bound"""
    return lambda stores, *a, **kw: repair(n_streams, stores, *a, **kw)
