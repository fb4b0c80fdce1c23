"""Secure RTP restated in plain Python (include/lc3plus_batch.h "Secure RTP"; RFC 3711 with AES_CM_128_HMAC_SHA1_80 / _32): AES-128 encryption written out,
HMAC-SHA1 from hashlib / hmac, the key derivation, protect, unprotect, the index estimate, the window and the state.  Shares no code with
audio_codec_amd/csrc/lc3_srtp_shim.h; tests/test_srtp_cpu.py pins the primitives here against the openssl program and the published vectors, and holds
lc3plus_plan_srtp_protect / lc3plus_plan_srtp_unprotect to this; tests/test_gpu_srtp.py holds the device to the plan functions."""
import hashlib
import hmac
import struct

import numpy as np

CTX_WORDS, STATE_WORDS, STATS_WORDS = 64, 8, 16
PROTECTED, NOT_STAMPED, BAD_ROUTE, RANGE, OVERFLOW = 1, 2, 4, 8, 16
OK, UN_RANGE, SHORT, VERSION, RTCP, HEADER, UNKNOWN_SSRC, REPLAY_OLD, REPLAYED, AUTH = range(10)
STAMPED = 1
MAX_PACKET = 1 << 20                                   # a payload has at most 2^16 keystream blocks: the counter lives in the IV's low 16 bits


# ---- AES-128 (FIPS-197), bytes in, bytes out ----
def _xtime(a):
    a <<= 1
    return (a ^ 0x11B) & 0xFF if a & 0x100 else a


def _mul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a, b = _xtime(a), b >> 1
    return r


def _make_sbox():
    box = []
    for x in range(256):
        inv = next((y for y in range(1, 256) if _mul(x, y) == 1), 0)     # the inverse by search
        s = inv
        for k in range(1, 5):
            s ^= ((inv << k) | (inv >> (8 - k))) & 0xFF
        box.append(s ^ 0x63)
    return box


SBOX = _make_sbox()


def aes_expand(key):
    w = [list(key[4 * i:4 * i + 4]) for i in range(4)]
    rc = 1
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = [SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= rc
            rc = _xtime(rc)
        w.append([a ^ b for a, b in zip(w[i - 4], t)])
    return [sum(w[4 * r:4 * r + 4], []) for r in range(11)]             # eleven round keys of 16 bytes, column after column


def aes_encrypt(key, block):
    rk = aes_expand(key)
    s = [b ^ k for b, k in zip(block, rk[0])]                           # s[4 * c + r]: column c, row r
    for rnd in range(1, 11):
        s = [SBOX[b] for b in s]
        s = [s[4 * ((c + r) % 4) + r] for c in range(4) for r in range(4)]      # ShiftRows
        if rnd < 10:
            m = []
            for c in range(4):
                a = s[4 * c:4 * c + 4]
                m += [_mul(a[r], 2) ^ _mul(a[(r + 1) % 4], 3) ^ a[(r + 2) % 4] ^ a[(r + 3) % 4] for r in range(4)]
            s = m
        s = [b ^ k for b, k in zip(s, rk[rnd])]
    return bytes(s)


def aes_cm(key, iv, n):
    """n bytes of the AES-CM keystream: block j is AES(iv + j), iv a 16-byte value whose low 16 bits are zero"""
    base = int.from_bytes(iv, "big")
    out = b""
    for j in range((n + 15) // 16):
        out += aes_encrypt(key, ((base + j) & ((1 << 128) - 1)).to_bytes(16, "big"))
    return out[:n]


# ---- RFC 3711 ----
def derive(master_key, master_salt, label, n):
    x = int.from_bytes(master_salt, "big") ^ (label << 48)
    return aes_cm(master_key, (x << 16).to_bytes(16, "big"), n)


def session_keys(master_key, master_salt):
    """-> (cipher key 16 bytes, auth key 20 bytes, salt 14 bytes), 4.3.1 with key derivation rate 0"""
    return derive(master_key, master_salt, 0, 16), derive(master_key, master_salt, 1, 20), derive(master_key, master_salt, 2, 14)


def packet_iv(salt, ssrc, index):
    return ((int.from_bytes(salt, "big") << 16) ^ (ssrc << 64) ^ (index << 16)).to_bytes(16, "big")


def tag_of(auth_key, data, roc, tag_len):
    return hmac.new(auth_key, bytes(data) + struct.pack(">I", roc & 0xFFFFFFFF), hashlib.sha1).digest()[:tag_len]


def _sha1_state(block):
    """the SHA-1 state behind one 64-byte block, five words (hashlib does not give midstates: the compression written out)"""
    h = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]
    w = list(struct.unpack(">16I", block))
    rot = lambda v, n: ((v << n) | (v >> (32 - n))) & 0xFFFFFFFF
    for t in range(16, 80):
        w.append(rot(w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16], 1))
    a, b, c, d, e = h
    for t in range(80):
        if t < 20:
            f, k = (b & c) | (~b & d), 0x5A827999
        elif t < 40:
            f, k = b ^ c ^ d, 0x6ED9EBA1
        elif t < 60:
            f, k = (b & c) | (b & d) | (c & d), 0x8F1BBCDC
        else:
            f, k = b ^ c ^ d, 0xCA62C1D6
        a, b, c, d, e = (rot(a, 5) + (f & 0xFFFFFFFF) + e + k + w[t]) & 0xFFFFFFFF, a, rot(b, 30), c, d
    return [(x + y) & 0xFFFFFFFF for x, y in zip(h, (a, b, c, d, e))]


def make_context(master_key, master_salt):
    """the 64 words of lc3plus_srtp_make_context, as uint32"""
    ke, ka, ks = session_keys(master_key, master_salt)
    words = []
    for rk in aes_expand(ke):
        words += list(struct.unpack(">4I", bytes(rk)))
    words += list(struct.unpack(">4I", ks + b"\0\0"))
    for fill in (0x36, 0x5C):
        words += _sha1_state(bytes(b ^ fill for b in ka + bytes(44)))
    return np.array(words + [0] * (CTX_WORDS - len(words)), np.uint32)


class Keys:
    """a source's or route's session keys beside its context"""

    def __init__(self, master_key, master_salt):
        self.ke, self.ka, self.ks = session_keys(master_key, master_salt)
        self.ctx = make_context(master_key, master_salt)


def protect_packet(keys, pkt, roc, tag_len, h=12):
    """an RTP packet (bytes) -> the SRTP packet"""
    seq, ssrc = struct.unpack(">H", pkt[2:4])[0], struct.unpack(">I", pkt[8:12])[0]
    stream = aes_cm(keys.ke, packet_iv(keys.ks, ssrc, (roc << 16) | seq), len(pkt) - h)
    body = bytes(pkt[:h]) + bytes(a ^ b for a, b in zip(pkt[h:], stream))
    return body + tag_of(keys.ka, body, roc, tag_len)


def protect(pkt_route, pkt_offset, pkt_size, pkt_status, n_packets, wire, header_room, payload_room, keys, roc, seq_base, next_seq, dst, dst_stride, tag_len):
    """-> dict like api.plan_srtp_protect's; keys: one Keys per route"""
    wire, dst = np.asarray(wire, np.uint8), np.array(dst, np.uint8)
    m, R = len(pkt_route), len(keys)
    out_offset, out_size, out_status = np.zeros(m, np.int64), np.zeros(m, np.int32), np.zeros(m, np.uint8)
    for p in range(min(int(n_packets), m)):
        out_offset[p] = p * dst_stride
        r, off, size = int(pkt_route[p]), int(pkt_offset[p]), int(pkt_size[p])
        if not int(pkt_status[p]) & STAMPED:
            out_status[p] = NOT_STAMPED
            continue
        if r < 0 or r >= R:
            out_status[p] = BAD_ROUTE
            continue
        if off < 0 or size < header_room or size > MAX_PACKET or off + size > wire.size:
            out_status[p] = RANGE
            continue
        a = off + header_room - payload_room - 12
        pkt = wire[a:off + size].tobytes()
        if len(pkt) + tag_len > dst_stride or (p + 1) * dst_stride > dst.size:
            out_status[p] = OVERFLOW
            continue
        seq = struct.unpack(">H", pkt[2:4])[0]
        b = int(seq_base[r]) & 0xFFFF
        roc_p = (int(roc[r]) + ((b + ((seq - b) & 0xFFFF)) >> 16)) & 0xFFFFFFFF
        out = protect_packet(keys[r], pkt, roc_p, tag_len)
        dst[p * dst_stride:p * dst_stride + len(out)] = np.frombuffer(out, np.uint8)
        out_size[p], out_status[p] = len(out), PROTECTED
    next_roc = None
    if next_seq is not None:
        next_roc = np.zeros(R, np.uint32)
        for r in range(R):
            b = int(seq_base[r]) & 0xFFFF
            next_roc[r] = (int(roc[r]) + ((b + ((int(next_seq[r]) - int(seq_base[r])) & 0xFFFF)) >> 16)) & 0xFFFFFFFF
        next_roc = next_roc.view(np.int32)
    return dict(dst=dst, out_offset=out_offset, out_size=out_size, out_status=out_status, next_roc=next_roc)


def guess(roc, s_l, seq):
    """RFC 3711 Appendix A -> (v, refused)"""
    if s_l < 32768:
        if seq - s_l > 32768:
            return (roc - 1) & 0xFFFFFFFF, roc == 0
        return roc, False
    return ((roc + 1) & 0xFFFFFFFF if s_l - 32768 > seq else roc), False


def _checks(ring, off, size, tag_len, ssrc_key):
    """checks 1 and 2 -> (status, source, h, seq, ssrc)"""
    if off < 0 or size < 0 or size > MAX_PACKET or off + size > ring.size:
        return UN_RANGE, -1, 0, 0, 0
    if size < 12 + tag_len:
        return SHORT, -1, 0, 0, 0
    n = size - tag_len
    d = ring[off:off + n].tobytes()
    if d[0] >> 6 != 2:
        return VERSION, -1, 0, 0, 0
    if 192 <= d[1] <= 223:
        return RTCP, -1, 0, 0, 0
    h = 12 + 4 * (d[0] & 15)
    if h > n:
        return HEADER, -1, 0, 0, 0
    if d[0] & 16:
        if h + 4 > n:
            return HEADER, -1, 0, 0, 0
        h += 4 + 4 * struct.unpack(">H", d[h + 2:h + 4])[0]
        if h > n:
            return HEADER, -1, 0, 0, 0
    ssrc = struct.unpack(">I", d[8:12])[0]
    where = [k for k, v in enumerate(ssrc_key) if (int(v) & 0xFFFFFFFF) == ssrc]
    if not where:
        return UNKNOWN_SSRC, -1, 0, 0, 0
    return OK, where[0], h, struct.unpack(">H", d[2:4])[0], ssrc


def unprotect(ring, dg_offsets, dg_sizes, ssrc_key, keys, state, tag_len):
    """-> dict like api.plan_srtp_unprotect's; keys: one Keys per source; state [n_ssrc, 8]"""
    ring = np.array(ring, np.uint8)
    state = (np.asarray(state).astype(np.int64) & 0xFFFFFFFF).reshape(-1, STATE_WORDS)
    n, S = len(dg_offsets), len(ssrc_key)
    items = [_checks(ring, int(dg_offsets[i]), int(dg_sizes[i]), tag_len, ssrc_key) for i in range(n)]
    first = {}
    for i, it in enumerate(items):
        if it[0] == OK:
            first.setdefault(it[1], i)
    sizes, status, index, stats = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.int64), np.zeros(STATS_WORDS, np.int32)
    accepted = [[] for _ in range(S)]
    for i, (st, s, h, seq, ssrc) in enumerate(items):
        if st == OK:
            off, size = int(dg_offsets[i]), int(dg_sizes[i])
            started = int(state[s, 0]) & 1
            roc, s_l = int(state[s, 1]), (int(state[s, 2]) & 0xFFFF if started else items[first[s]][3])
            v, refused = guess(roc, s_l, seq)
            idx = (v << 16) | seq
            top = (roc << 16) | s_l
            win = int(state[s, 3]) | int(state[s, 4]) << 32
            data = ring[off:off + size - tag_len].tobytes()
            if refused:
                st = REPLAY_OLD
            elif started and top - idx >= 64:
                st = REPLAY_OLD
            elif started and top - idx >= 0 and (win >> (top - idx)) & 1:
                st = REPLAYED
            elif not hmac.compare_digest(tag_of(keys[s].ka, data, v, tag_len), ring[off + size - tag_len:off + size].tobytes()):
                st = AUTH
            else:
                stream = aes_cm(keys[s].ke, packet_iv(keys[s].ks, ssrc, idx), len(data) - h)
                ring[off + h:off + len(data)] = np.frombuffer(bytes(a ^ b for a, b in zip(data[h:], stream)), np.uint8)
                sizes[i], index[i] = len(data), idx
                accepted[s].append(idx)
        status[i] = st
        stats[st] += 1
    out = state.copy()
    for s in range(S):
        if not accepted[s]:
            continue
        started = int(state[s, 0]) & 1
        top = (int(state[s, 1]) << 16) | (int(state[s, 2]) & 0xFFFF)
        win = int(state[s, 3]) | int(state[s, 4]) << 32
        top2 = max(accepted[s] + ([top] if started else []))
        win = (win << (top2 - top)) & ((1 << 64) - 1) if started and top2 - top < 64 else 0
        for idx in accepted[s]:
            if top2 - idx < 64:
                win |= 1 << (top2 - idx)
        out[s, 0] |= 1
        out[s, 1], out[s, 2], out[s, 3], out[s, 4] = top2 >> 16, top2 & 0xFFFF, win & 0xFFFFFFFF, win >> 32
    return dict(ring=ring, state=out.astype(np.uint32).view(np.int32).reshape(-1, STATE_WORDS), sizes=sizes, status=status, index=index, stats=stats)


# ---- building test traffic ----
def rtp_packet(seq, ts, ssrc, payload, pt=96, marker=0, csrc=(), ext=None, padding=0):
    """an RTP packet: ext = (profile, body of 4k bytes) or None; padding: pad bytes appended with the P bit"""
    b0 = 0x80 | (0x20 if padding else 0) | (0x10 if ext is not None else 0) | len(csrc)
    out = struct.pack(">BBHII", b0, marker << 7 | pt, seq & 0xFFFF, ts & 0xFFFFFFFF, ssrc & 0xFFFFFFFF)
    out += b"".join(struct.pack(">I", c) for c in csrc)
    if ext is not None:
        out += struct.pack(">HH", ext[0], len(ext[1]) // 4) + bytes(ext[1])
    out += bytes(payload)
    if padding:
        out += bytes(padding - 1) + bytes([padding])
    return out


def header_len(pkt):
    h = 12 + 4 * (pkt[0] & 15)
    if pkt[0] & 16:
        h += 4 + 4 * struct.unpack(">H", pkt[h + 2:h + 4])[0]
    return h
