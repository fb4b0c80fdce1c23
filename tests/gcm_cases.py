"""The AES-GCM SRTP traffic both test files use (tests/test_gcm_cpu.py holds the host plans to tests/gcm_ref.py on it, tests/test_gpu_gcm.py the device to the
host plans): the seven scenarios of srtp_cases.CASES and its protect list rebuilt with GCM packets, the sources and routes alternating 16- and 32-byte keys
inside one call.  Payloads around one, two and three AES blocks, headers of 12 to 28 bytes so that the associated data ends at every place of a GHASH block and
spills into a second one, a header extension, all four byte alignments, rollover guesses in both directions, the window's edges, sources that have not started,
flipped bits and malformed datagrams, and lists longer than one workgroup.  Every builder gives a dict: ring (uint8, GUARD bytes of 0xA5 on both sides and in
the gaps), offs, sizes, ssrc_key, keys (gcm_ref.Keys per source), ctx [n, 128], state [n, 8] and expect {item: status}.  A scenario is built once per process
(the plain Python GHASH is slow): nobody writes into what a builder returned."""
import functools
import struct

import numpy as np

import gcm_ref as ref
from srtp_cases import FILL, GUARD, SSRCS, Ring, _payload, _words, state_block

PAYLOADS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 400)
CSRCS = (0, 1, 2, 3, 4)                                 # headers of 12, 16, 20, 24 and 28 bytes


@functools.lru_cache(maxsize=None)
def keys_for(k):
    """source or route k: a 16-byte master key for even k, a 32-byte one for odd k"""
    return ref.Keys(bytes((29 * k + 11 * j + 5) & 255 for j in range(32 if k & 1 else 16)), bytes((17 * k + 3 * j + 9) & 255 for j in range(12)))


def _case(ring, ssrcs, states, expect, keys=None):
    r, offs, sizes = ring.done()
    keys = keys or [keys_for(k) for k in range(len(ssrcs))]
    return dict(ring=r, offs=offs, sizes=sizes, ssrc_key=np.array(ssrcs, np.uint32).view(np.int32), keys=keys, ctx=np.stack([k.ctx for k in keys]).view(np.int32),
                state=np.array(states, np.uint32).view(np.int32).reshape(-1, 8), expect=expect)


@functools.lru_cache(maxsize=None)
def shapes(seed=1):
    """every payload size under every header length at every alignment, three started sources (16-, 32-, 16-byte keys) in order, neighbours touching; then an
    80-byte header (15 CSRCs and a one-word extension) and a padded packet"""
    rng = np.random.default_rng(seed)
    ssrcs = SSRCS[1:4]
    keys = [keys_for(k) for k in range(3)]
    roc, nxt = [0, 7, 0xFFFFFFFF], [100, 40000, 65000]
    states = [state_block(1, roc[k], nxt[k] - 1, 1) for k in range(3)]
    g, expect, k = Ring(), {}, 0

    def put(n, align, **extra):
        nonlocal k
        s = k % 3
        k += 1
        pkt = ref.rtp_packet(nxt[s], 160 * k, ssrcs[s], _payload(rng, n), marker=k & 1, **extra)
        expect[g.add(ref.protect_packet(keys[s], pkt, roc[s], ref.header_len(pkt)), align)] = ref.OK
        nxt[s] += 1
    for cc in CSRCS:
        for n in PAYLOADS:
            for align in range(4):
                put(n, align, csrc=tuple(range(1000, 1000 + cc)))
    for n in (0, 1, 16, 33):
        for align in range(4):
            put(n, align, csrc=tuple(range(1000, 1015)), ext=(0xBEDE, _payload(rng, 4)))
    put(17, 1, padding=3)
    put(20, 2, ext=(0xBEDE, b""))                                    # an extension of no words: a 16-byte header
    return _case(g, ssrcs, states, expect, keys)


@functools.lru_cache(maxsize=None)
def rollover(seed=2):
    """guesses of ROC + 1 (S_L high, SEQ wrapped), ROC - 1 (S_L low, SEQ from before the wrap), ROC - 1 at ROC 0 (refused), and a wrap inside the list"""
    rng = np.random.default_rng(seed)
    ssrcs = SSRCS[:4]
    keys = [keys_for(k) for k in range(4)]
    states = [state_block(1, 5, 65533, 0b111), state_block(1, 9, 2, 0b1), state_block(1, 0, 3, 0b1), state_block(1, 0xFFFFFFFF, 65535, 1)]
    g, expect = Ring(), {}

    def put(s, seq, roc, want, gap=1):
        pkt = ref.rtp_packet(seq, 7, ssrcs[s], _payload(rng, 20 + seq % 7))
        expect[g.add(ref.protect_packet(keys[s], pkt, roc & 0xFFFFFFFF), gap=gap)] = want
    for seq in (65534, 65535, 0, 1, 2):                              # source 0 crosses 65535 -> 0: the later ones are guessed at ROC + 1
        put(0, seq, 5 if seq > 60000 else 6, ref.OK)
    put(1, 65530, 8, ref.OK)                                         # guessed at ROC - 1, and bit 8 of the window is clear
    put(1, 3, 9, ref.OK)
    put(1, 65535, 9, ref.AUTH)                                       # protected under ROC 9 but guessed at 8: another IV
    put(2, 65000, 0, ref.REPLAY_OLD)                                 # ROC - 1 at ROC 0: refused without authentication
    put(2, 4, 0, ref.OK)
    put(3, 0, 0, ref.REPLAY_OLD)                                     # ROC + 1 wraps to 0 in 32 bits: the key's life ends there
    return _case(g, ssrcs, states, expect, keys)


@functools.lru_cache(maxsize=None)
def window(seed=3):
    """deltas 0, 63 and 64 against a set and a clear window, an advance by less than 64 and one by 64 or more"""
    rng = np.random.default_rng(seed)
    ssrcs = SSRCS[:3]
    keys = [keys_for(k) for k in range(3)]
    top = 1000
    states = [state_block(1, 2, top, (1 << 63) | 1), state_block(1, 2, top, 1 | 1 << 5), state_block(1, 2, top, (1 << 64) - 1, flags=0x100)]
    g, expect = Ring(), {}

    def put(s, seq, want, roc=2):
        pkt = ref.rtp_packet(seq, 9, ssrcs[s], _payload(rng, 33))
        expect[g.add(ref.protect_packet(keys[s], pkt, roc), gap=seq % 3)] = want
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
    return _case(g, ssrcs, states, expect, keys)


@functools.lru_cache(maxsize=None)
def fresh(seed=4):
    """sources that have not started: one whose first item is forged, one with a preset ROC, one with no accepted item, one that starts near the wrap"""
    rng = np.random.default_rng(seed)
    ssrcs = SSRCS[:4]
    keys = [keys_for(k) for k in range(4)]
    states = [state_block(), state_block(0, 77), state_block(0, 3, 1234, 0xF0F0, flags=0x40), state_block()]
    g, expect = Ring(), {}

    def put(s, seq, want, roc, forge=False):
        pkt = ref.rtp_packet(seq, 9, ssrcs[s], _payload(rng, 24))
        dg = bytearray(ref.protect_packet(keys[s], pkt, roc))
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
    return _case(g, ssrcs, states, expect, keys)


@functools.lru_cache(maxsize=None)
def tampered(seed=5):
    """one flipped bit in the header, in the payload's first and last byte, in the tag's first and last byte and in the SEQ, under a 16- and a 32-byte key; a
    datagram cut to 27 bytes; and every malformed datagram of checks 1 and 2"""
    rng = np.random.default_rng(seed)
    ssrcs = SSRCS[:2]
    keys = [keys_for(k) for k in range(2)]
    states = [state_block(1, 1, 10, 1), state_block(1, 1, 10, 1)]
    g, expect = Ring(), {}
    seq = [11]

    def good(s=0, **kw):
        pkt = ref.rtp_packet(seq[0], 9, ssrcs[s], _payload(rng, 40), **kw)
        seq[0] += 1
        return bytearray(ref.protect_packet(keys[s], pkt, 1, ref.header_len(pkt)))
    for s in range(2):
        # header (the marker bit, a timestamp byte), payload first and last, tag first and last, SEQ low byte
        for at, bit in ((1, 0x80), (5, 0x80), (12, 0x10), (12 + 39, 0x02), (-16, 0x80), (-1, 0x01), (3, 0x01)):
            dg = good(s)
            assert len(dg) == 12 + 40 + 16
            dg[at] ^= bit
            expect[g.add(bytes(dg), gap=3)] = ref.AUTH
        expect[g.add(bytes(good(s)), gap=0)] = ref.OK
        expect[g.add(bytes(good(s)[:27]))] = ref.SHORT
    expect[g.add(bytes(good(0, padding=0)[:28]))] = ref.AUTH          # 28 bytes: a header and a tag, no payload; the tag is not this packet's
    dg = good(); dg[0] = 0x40 | (dg[0] & 0x3F); expect[g.add(bytes(dg))] = ref.VERSION
    dg = good(); dg[1] = 200; expect[g.add(bytes(dg))] = ref.RTCP
    dg = good(); dg[0] |= 15; expect[g.add(bytes(dg)[:40 + 16])] = ref.HEADER                 # 15 CSRCs do not fit
    dg = good(); dg[0] |= 16; dg[14:16] = struct.pack(">H", 1000); expect[g.add(bytes(dg))] = ref.HEADER   # the extension runs past the end
    dg = good(); dg[8:12] = struct.pack(">I", 0x12345678); expect[g.add(bytes(dg))] = ref.UNKNOWN_SSRC
    c = _case(g, ssrcs, states, expect, keys)
    n = len(c["offs"])
    c["offs"] = np.concatenate([c["offs"], [-1, c["ring"].size - 20, 8]]).astype(np.int64)      # outside the ring: before it, past its end, a negative size
    c["sizes"] = np.concatenate([c["sizes"], [30, 30, -5]]).astype(np.int32)
    for k in range(3):
        c["expect"][n + k] = ref.UN_RANGE
    return c


@functools.lru_cache(maxsize=None)
def crowd(one_source, seed=6):
    """70 items of one source, or one item each of 70 sources; with 250 more behind: 320 items, more than one workgroup"""
    rng = np.random.default_rng(seed)
    S = 1 if one_source else 70
    ssrcs = [0x1000 + 0x03A0F0F1 * k for k in range(S)]
    keys = [keys_for(k % 6) for k in range(S)]
    states = [state_block(1, 1, 199, 1) if k % 2 == 0 else state_block(0, 1) for k in range(S)]      # odd: not started, ROC preset to the sender's
    g, expect = Ring(), {}
    for i in range(70 + 250):
        s = i % S
        seq = 200 + (i // S)
        pkt = ref.rtp_packet(seq, i, ssrcs[s], _payload(rng, 5 + i % 23))
        expect[g.add(ref.protect_packet(keys[s], pkt, 1), gap=i % 2)] = ref.OK
    return _case(g, ssrcs, states, expect, keys)


@functools.lru_cache(maxsize=None)
def protect_list(seed=11):
    """the stamp's view of a packet list: two routes (a 16- and a 32-byte key), every payload size at source offsets that take every alignment, SEQ crossing
    65535, and one packet for every refusal; dst_stride is odd, so that the destinations take every alignment too"""
    rng = np.random.default_rng(seed)
    hr, pr = 19, 3
    sizes = list(PAYLOADS + (13, 29, 45, 500)) * 4 + [5] * 260         # with payload_room 3: 16, 32 and 48 bytes of plaintext; 500: too long for a slot; 324 packets
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
    stride = 12 + pr + 400 + ref.TAG + 2                               # odd; the 400-byte payloads fit, the 500-byte ones do not: OVERFLOW
    assert stride % 2
    expect = {i: (ref.OVERFLOW if n == 500 else ref.PROTECTED) for i, n in enumerate(sizes)}
    status[5] = 0; expect[5] = ref.NOT_STAMPED
    status[6] = 6; expect[6] = ref.NOT_STAMPED                         # other bits of the stamp's status do not count
    route[7] = 2; expect[7] = ref.BAD_ROUTE
    route[9] = -1; expect[9] = ref.BAD_ROUTE
    off[11] = -4; expect[11] = ref.RANGE
    off[13] = len(wire) - 10; expect[13] = ref.RANGE
    size[17] = hr - 1; expect[17] = ref.RANGE
    max_packets, n_packets = m + 3, m                                  # three entries behind the list's end
    pad = lambda a, v: np.concatenate([a, np.full(3, v, a.dtype)])
    slots = m - 2                                                      # the last two packets' slots end past dst_capacity
    expect[m - 1] = expect[m - 2] = ref.OVERFLOW
    return dict(route=pad(route, 0), off=pad(off, GUARD), size=pad(size, hr + 1), status=pad(status, 1), wire=np.frombuffer(bytes(wire), np.uint8).copy(), hr=hr, pr=pr,
                keys=keys, ctx=np.stack([k.ctx for k in keys]).view(np.int32), roc=_words(roc), seq_base=_words(seq_base), next_seq=_words(nxt), stride=stride,
                dst_capacity=slots * stride + stride - 1, max_packets=max_packets, n_packets=n_packets, expect=expect)


CASES = dict(shapes=shapes, rollover=rollover, window=window, fresh=fresh, tampered=tampered, crowd_one=lambda: crowd(True), crowd_many=lambda: crowd(False))


@functools.lru_cache(maxsize=None)
def split_lists():
    """Lists for the split property - one call over a list equals two calls over its halves with the state carried over - as srtp_cases.split_lists has them:
    every source is started, its items ascend without a repeat, stay within 2^15 of S_L, and the cut falls anywhere.  -> (case, cut)"""
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
        expect[g.add(ref.protect_packet(keys[s], pkt, r), gap=i % 3)] = ref.OK
    return _case(g, ssrcs, states, expect, keys), 41
