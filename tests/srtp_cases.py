"""The SRTP traffic both test files use (tests/test_srtp_cpu.py holds the host plans to tests/srtp_ref.py on it, tests/test_gpu_srtp.py the device to the host
plans): small lists built so that every path is taken - payloads around the AES block and packets around the SHA-1 padding boundary at all four byte
alignments, CSRCs and a header extension, rollover guesses in both directions, the window's edges, sources that have not started, forged and malformed
datagrams.  Every builder gives a dict: ring (uint8, GUARD bytes of 0xA5 on both sides and in every gap), offs, sizes, ssrc_key, keys (srtp_ref.Keys per
source), ctx [n, 64], state [n, 8], tag_len and expect {item: status} for the items whose status the scenario is about."""
import struct

import numpy as np

import srtp_ref as ref

GUARD = 32
FILL = 0xA5
# payload bytes: around one and two AES blocks, a long one, and with a 12-byte header those whose authenticated length (packet + 4) mod 64 is 54, 55, 56, 63, 0
PAYLOADS = (0, 1, 15, 16, 17, 31, 32, 33, 400, 38, 39, 40, 47, 48, 102, 103, 104, 111, 112)
# the same boundary with 15 CSRCs and a one-word extension (an 80-byte header)
PAYLOADS_LONG_HEADER = (0, 1, 16, 33, 34, 35, 36, 43, 44)
SSRCS = (0x00000011, 0x7FFFFFF0, 0x80000001, 0xDEADBEEF, 0xFFFFFFFE)        # ascending as uint32, on both sides of 2^31


def keys_for(k):
    return ref.Keys(bytes((31 * k + 7 * j + 1) & 255 for j in range(16)), bytes((13 * k + 5 * j + 3) & 255 for j in range(14)))


def state_block(started=0, roc=0, s_l=0, win=0, flags=0):
    return [flags | (1 if started else 0), roc, s_l, win & 0xFFFFFFFF, win >> 32, 0, 0, 0]


class Ring:
    """datagrams laid into a ring at chosen alignments"""

    def __init__(self):
        self.data, self.offs, self.sizes = bytearray([FILL] * GUARD), [], []

    def add(self, dg, align=None, gap=0):
        self.data += bytes([FILL] * gap)
        while align is not None and len(self.data) % 4 != align:
            self.data += bytes([FILL])
        self.offs.append(len(self.data))
        self.sizes.append(len(dg))
        self.data += dg
        return len(self.offs) - 1

    def done(self):
        return np.frombuffer(bytes(self.data) + bytes([FILL] * GUARD), np.uint8).copy(), np.array(self.offs, np.int64), np.array(self.sizes, np.int32)


def _case(ring, ssrcs, states, tag_len, expect, keys=None):
    r, offs, sizes = ring.done()
    keys = keys or [keys_for(k) for k in range(len(ssrcs))]
    return dict(ring=r, offs=offs, sizes=sizes, ssrc_key=np.array(ssrcs, np.uint32).view(np.int32), keys=keys, ctx=np.stack([k.ctx for k in keys]).view(np.int32),
                state=np.array(states, np.uint32).view(np.int32).reshape(-1, 8), tag_len=tag_len, expect=expect)


def _payload(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def shapes(tag_len, seed=1):
    """every payload size at every alignment, short and long headers, three started sources in order, neighbours touching"""
    rng = np.random.default_rng(seed)
    ssrcs = SSRCS[1:4]
    keys = [keys_for(k) for k in range(3)]
    roc, nxt = [0, 7, 0xFFFFFFFF], [100, 40000, 65000]
    states = [state_block(1, roc[k], nxt[k] - 1, 1) for k in range(3)]
    g, expect, k = Ring(), {}, 0
    for long_header, sizes in ((0, PAYLOADS), (1, PAYLOADS_LONG_HEADER)):
        for n in sizes:
            for align in range(4):
                s = k % 3
                k += 1
                extra = dict(csrc=tuple(range(1000, 1015)), ext=(0xBEDE, _payload(rng, 4))) if long_header else {}
                pkt = ref.rtp_packet(nxt[s], 160 * k, ssrcs[s], _payload(rng, n), marker=k & 1, padding=(3 if n == 17 else 0), **extra)
                i = g.add(ref.protect_packet(keys[s], pkt, roc[s], tag_len, ref.header_len(pkt)), align)
                expect[i] = ref.OK
                nxt[s] += 1
    return _case(g, ssrcs, states, tag_len, expect, keys)


def rollover(tag_len, seed=2):
    """guesses of ROC + 1 (S_L high, SEQ wrapped), ROC - 1 (S_L low, SEQ from before the wrap), ROC - 1 at ROC 0 (refused), and a wrap inside the list"""
    rng = np.random.default_rng(seed)
    ssrcs = SSRCS[:4]
    keys = [keys_for(k) for k in range(4)]
    states = [state_block(1, 5, 65533, 0b111), state_block(1, 9, 2, 0b1), state_block(1, 0, 3, 0b1), state_block(1, 0xFFFFFFFF, 65535, 1)]
    g, expect = Ring(), {}

    def put(s, seq, roc, want, gap=1):
        pkt = ref.rtp_packet(seq, 7, ssrcs[s], _payload(rng, 20 + seq % 7))
        expect[g.add(ref.protect_packet(keys[s], pkt, roc & 0xFFFFFFFF, tag_len), gap=gap)] = want
    for seq in (65534, 65535, 0, 1, 2):                              # source 0 crosses 65535 -> 0: the later ones are guessed at ROC + 1
        put(0, seq, 5 if seq > 60000 else 6, ref.OK)
    put(1, 65530, 8, ref.OK)                                         # guessed at ROC - 1: top - index = (9 << 16 | 2) - (8 << 16 | 65530) = 8, and bit 8 is clear
    put(1, 3, 9, ref.OK)
    put(1, 65535, 9, ref.AUTH)                                       # protected under ROC 9 but guessed at 8
    put(2, 65000, 0, ref.REPLAY_OLD)                                 # ROC - 1 at ROC 0: refused without authentication
    put(2, 4, 0, ref.OK)
    put(3, 0, 0, ref.REPLAY_OLD)                                     # ROC + 1 wraps to 0 in 32 bits: the 48-bit index does not go on, the key's life ends there
    return _case(g, ssrcs, states, tag_len, expect, keys)


def window(tag_len, seed=3):
    """deltas 0, 63 and 64 against a set and a clear window, an advance by less than 64 and one by 64 or more"""
    rng = np.random.default_rng(seed)
    ssrcs = SSRCS[:3]
    keys = [keys_for(k) for k in range(3)]
    top = 1000
    states = [state_block(1, 2, top, (1 << 63) | 1), state_block(1, 2, top, 1 | 1 << 5), state_block(1, 2, top, (1 << 64) - 1, flags=0x100)]
    g, expect = Ring(), {}

    def put(s, seq, want, roc=2):
        pkt = ref.rtp_packet(seq, 9, ssrcs[s], _payload(rng, 33))
        expect[g.add(ref.protect_packet(keys[s], pkt, roc, tag_len), gap=seq % 3)] = want
    put(0, top, ref.REPLAYED)                                        # delta 0, bit set
    put(0, top - 63, ref.REPLAYED)                                   # delta 63, bit set
    put(0, top - 64, ref.REPLAY_OLD)                                 # delta 64
    put(0, top - 62, ref.OK)                                         # delta 62, bit clear
    put(0, top - 62, ref.OK)                                         # twice inside one call: both OK (the one deviation from 3.3.2)
    put(1, top - 63, ref.OK)                                         # delta 63, clear
    put(1, top - 5, ref.REPLAYED)
    put(1, top + 3, ref.OK)                                          # advances the top by 3
    put(1, top + 1, ref.OK)
    put(2, top + 64, ref.OK)                                         # advances by 64: the old window is gone
    put(2, top + 64 + 70, ref.OK)                                    # and further: the first advance falls out of the window as well
    put(2, top + 64 + 70 - 63, ref.OK)
    return _case(g, ssrcs, states, tag_len, expect, keys)


def fresh(tag_len, seed=4):
    """sources that have not started: one whose first item is forged, one with a preset ROC, one with no accepted item, one that starts near the wrap"""
    rng = np.random.default_rng(seed)
    ssrcs = SSRCS[:4]
    keys = [keys_for(k) for k in range(4)]
    states = [state_block(), state_block(0, 77), state_block(0, 3, 1234, 0xF0F0, flags=0x40), state_block()]
    g, expect = Ring(), {}

    def put(s, seq, want, roc, forge=False):
        pkt = ref.rtp_packet(seq, 9, ssrcs[s], _payload(rng, 24))
        dg = bytearray(ref.protect_packet(keys[s], pkt, roc, tag_len))
        if forge:
            dg[-1] ^= 1
        expect[g.add(bytes(dg), gap=1)] = want
    put(0, 40000, ref.AUTH, 0, forge=True)                           # the first item gives S_L although it is forged
    put(0, 100, ref.OK, 1)                                           # so 100 is guessed at ROC + 1 ...
    put(0, 40001, ref.OK, 0)
    put(1, 500, ref.OK, 77)
    put(1, 499, ref.OK, 77)
    put(2, 9, ref.AUTH, 3, forge=True)                               # no accepted item: the state comes back word for word
    put(3, 65535, ref.OK, 0)
    put(3, 0, ref.OK, 1)
    return _case(g, ssrcs, states, tag_len, expect, keys)


def tampered(tag_len, seed=5):
    """one flipped bit in the header, in the payload and in the tag; and every malformed datagram of check 1 and 2"""
    rng = np.random.default_rng(seed)
    ssrcs = SSRCS[:2]
    keys = [keys_for(k) for k in range(2)]
    states = [state_block(1, 1, 10, 1), state_block()]
    g, expect = Ring(), {}
    seq = [11]

    def good(s=0, **kw):
        pkt = ref.rtp_packet(seq[0], 9, ssrcs[s], _payload(rng, 40), **kw)
        seq[0] += 1
        return bytearray(ref.protect_packet(keys[s], pkt, 1, tag_len, ref.header_len(pkt)))
    for at, bit in ((1, 0x01), (5, 0x80), (12, 0x10), (30, 0x02), (-1, 0x01), (-tag_len, 0x80)):
        dg = good()
        dg[at] ^= bit
        expect[g.add(bytes(dg), gap=3)] = ref.AUTH
    expect[g.add(bytes(good()), gap=0)] = ref.OK
    expect[g.add(bytes(good()[:11 + tag_len]))] = ref.SHORT
    dg = good(); dg[0] = 0x40 | (dg[0] & 0x3F); expect[g.add(bytes(dg))] = ref.VERSION
    dg = good(); dg[1] = 200; expect[g.add(bytes(dg))] = ref.RTCP
    dg = good(); dg[0] |= 15; expect[g.add(bytes(dg)[:40 + tag_len])] = ref.HEADER            # 15 CSRCs do not fit
    dg = good(); dg[0] |= 16; dg[14:16] = struct.pack(">H", 1000); expect[g.add(bytes(dg))] = ref.HEADER   # the extension runs past the end
    dg = good(); dg[8:12] = struct.pack(">I", 0x12345678); expect[g.add(bytes(dg))] = ref.UNKNOWN_SSRC
    c = _case(g, ssrcs, states, tag_len, expect, keys)
    n = len(c["offs"])
    c["offs"] = np.concatenate([c["offs"], [-1, c["ring"].size - 20, 8]]).astype(np.int64)      # outside the ring: before it, past its end, a negative size
    c["sizes"] = np.concatenate([c["sizes"], [30, 30, -5]]).astype(np.int32)
    for k in range(3):
        c["expect"][n + k] = ref.UN_RANGE
    return c


def crowd(tag_len, one_source, seed=6):
    """65 items of one source, or one item each of 65 sources; with 200 more behind so that the list needs more than one workgroup"""
    rng = np.random.default_rng(seed)
    S = 1 if one_source else 65
    ssrcs = [0x1000 + 0x03F0F0F1 * k for k in range(S)]
    keys = [keys_for(k % 5) for k in range(S)]
    states = [state_block(1, 1, 199, 1) if k % 2 == 0 else state_block() for k in range(S)]
    g, expect = Ring(), {}
    for i in range(65 + 200):
        s = i % S
        seq = 200 + (i // S)
        pkt = ref.rtp_packet(seq, i, ssrcs[s], _payload(rng, 5 + i % 23))
        expect[g.add(ref.protect_packet(keys[s], pkt, 1, tag_len), gap=i % 2)] = ref.OK
    for k in range(S):
        if k % 2:
            states[k] = state_block(0, 1)                            # not started, ROC preset to the sender's
    return _case(g, ssrcs, states, tag_len, expect, keys)


def _words(a):
    return (np.asarray(a).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def protect_list(tag_len, seed=11):
    """the stamp's view of a packet list: two routes, every payload size of srtp_cases at source offsets that take every alignment, SEQ crossing 65535, and one
    packet for every refusal; dst_stride is odd, so that the destinations take every alignment too"""
    rng = np.random.default_rng(seed)
    hr, pr = 19, 3
    # with payload_room 3 the packet is n + 15 bytes: n = 35, 36, 37, 44, 45 (and 64 more) give authenticated lengths (packet + 4) mod 64 of 54, 55, 56, 63, 0
    sizes = (list(PAYLOADS) + [35, 36, 37, 44, 45, 99, 100, 101, 108, 109, 500]) * 4 + [5] * 200      # more than one workgroup; 500: too long for a slot
    keys = [keys_for(0), keys_for(1)]
    ssrc, seq_base, roc = [0x80000001, 0x11], [65500, 3], [0xFFFFFFFF, 6]
    nxt = list(seq_base)
    wire = bytearray([FILL] * GUARD)
    route, off, size = [], [], []
    for i, n in enumerate(sizes):
        r = i % 2
        wire += bytes([FILL] * (i % 3))
        pkt = ref.rtp_packet(nxt[r], 960 * i, ssrc[r], rng.integers(0, 256, pr + n, dtype=np.uint8).tobytes(), marker=i & 1)
        nxt[r] += 1
        route.append(r); off.append(len(wire)); size.append(hr + n)
        wire += bytes([FILL] * (hr - pr - 12)) + pkt             # the header room's unused front, then the packet where the stamp writes it
    wire += bytes([FILL] * GUARD)
    m = len(sizes)
    status = np.ones(m, np.uint8)
    route, off, size = np.array(route, np.int32), np.array(off, np.int64), np.array(size, np.int32)
    stride = 12 + pr + 400 + tag_len + 1                               # the 400-byte payloads fit, the 500-byte ones do not: OVERFLOW
    if stride % 2 == 0:
        stride += 1
    expect = {i: (ref.OVERFLOW if n == 500 else ref.PROTECTED) for i, n in enumerate(sizes)}
    status[5] = 0; expect[5] = ref.NOT_STAMPED
    status[6] = 6; expect[6] = ref.NOT_STAMPED                         # other bits of the stamp's status do not count
    route[7] = 2; expect[7] = ref.BAD_ROUTE
    route[9] = -1; expect[9] = ref.BAD_ROUTE
    off[11] = -4; expect[11] = ref.RANGE
    off[13] = len(wire) - 10; expect[13] = ref.RANGE
    size[15] = hr - 1; expect[15] = ref.RANGE
    max_packets, n_packets = m + 3, m                                  # three entries behind the list's end
    pad = lambda a, v: np.concatenate([a, np.full(3, v, a.dtype)])
    slots = m - 2                                                      # the last two packets' slots end past dst_capacity
    expect[m - 1] = expect[m - 2] = ref.OVERFLOW
    return dict(route=pad(route, 0), off=pad(off, GUARD), size=pad(size, hr + 1), status=pad(status, 1), wire=np.frombuffer(bytes(wire), np.uint8).copy(), hr=hr, pr=pr,
                keys=keys, ctx=np.stack([k.ctx for k in keys]).view(np.int32), roc=_words(roc), seq_base=_words(seq_base), next_seq=_words(nxt), stride=stride,
                dst_capacity=slots * stride + stride - 1, tag_len=tag_len, max_packets=max_packets, n_packets=n_packets, expect=expect)


CASES = dict(shapes=shapes, rollover=rollover, window=window, fresh=fresh, tampered=tampered, crowd_one=lambda t: crowd(t, True), crowd_many=lambda t: crowd(t, False))


def split_lists(tag_len):
    """Lists for the split property - one call over a list equals two calls over its halves with the state carried over.  The stateless estimate and the
    sequential one agree where no item's guess or replay check depends on an item of the same call: here every source is started, its items ascend without a
    repeat, stay within 2^15 of S_L, and the cut falls anywhere.  -> (case, cut)"""
    rng = np.random.default_rng(7)
    ssrcs = SSRCS[:3]
    keys = [keys_for(k) for k in range(3)]
    states = [state_block(1, 4, 65500, 1), state_block(1, 0, 10, 0b101), state_block(1, 8, 30000, 1 << 40)]
    nxt, roc = [65501, 11, 30001], [4, 0, 8]
    g, expect = Ring(), {}
    for i in range(90):
        s = int(rng.integers(0, 3))
        nxt[s] += int(rng.integers(0, 3))                            # gaps
        seq = nxt[s] & 0xFFFF
        r = roc[s] + (nxt[s] >> 16)
        nxt[s] += 1
        pkt = ref.rtp_packet(seq, i, ssrcs[s], _payload(rng, 10 + i % 40))
        expect[g.add(ref.protect_packet(keys[s], pkt, r, tag_len), gap=i % 3)] = ref.OK
    return _case(g, ssrcs, states, tag_len, expect, keys), 41
