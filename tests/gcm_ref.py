"""Secure RTP with the AEAD suites of RFC 7714 restated in plain Python (include/lc3plus_batch.h "Secure RTP, AEAD"): AES-128 and AES-256 encryption written
out, GHASH by SP 800-38D algorithm 1 bit by bit (no table), GCM, the key derivation of RFC 7714 11, the context, protect and unprotect.  Shares no code with
audio_codec_amd/csrc/lc3_gcm_shim.h; what is the same for every SRTP suite - the S-box, the receive checks 1 and 2, the index estimate, the test packets - is
srtp_ref's.  tests/test_gcm_cpu.py pins the primitives here against libcrypto, the openssl program and published vectors and holds the host plans to this;
tests/test_gpu_gcm.py holds the device to the host plans."""
import struct

import numpy as np

import srtp_ref as ref
from srtp_ref import (OK, UN_RANGE, SHORT, VERSION, RTCP, HEADER, UNKNOWN_SSRC, REPLAY_OLD, REPLAYED, AUTH, PROTECTED, NOT_STAMPED, BAD_ROUTE, RANGE, OVERFLOW,  # noqa: F401
                      STAMPED, MAX_PACKET, STATE_WORDS, STATS_WORDS, rtp_packet, header_len)

CTX_WORDS, TAG = 128, 16


# ---- AES (FIPS-197) for 16- and 32-byte keys, bytes in, bytes out ----
def aes_expand(key):
    """-> the round keys, 16 bytes each: 11 for a 16-byte key, 15 for a 32-byte key"""
    nk = len(key) // 4
    rounds = nk + 6
    w = [list(key[4 * i:4 * i + 4]) for i in range(nk)]
    rc = 1
    for i in range(nk, 4 * (rounds + 1)):
        t = list(w[i - 1])
        if i % nk == 0:
            t = [ref.SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= rc
            rc = ref._xtime(rc)
        elif nk > 6 and i % nk == 4:
            t = [ref.SBOX[b] for b in t]
        w.append([a ^ b for a, b in zip(w[i - nk], t)])
    return [sum(w[4 * r:4 * r + 4], []) for r in range(rounds + 1)]


def aes_encrypt(key, block):
    rk = aes_expand(key)
    last = len(rk) - 1
    s = [b ^ k for b, k in zip(block, rk[0])]                           # s[4 * c + r]: column c, row r
    for rnd in range(1, last + 1):
        s = [ref.SBOX[b] for b in s]
        s = [s[4 * ((c + r) % 4) + r] for c in range(4) for r in range(4)]      # ShiftRows
        if rnd < last:
            m = []
            for c in range(4):
                a = s[4 * c:4 * c + 4]
                m += [ref._mul(a[r], 2) ^ ref._mul(a[(r + 1) % 4], 3) ^ a[(r + 2) % 4] ^ a[(r + 3) % 4] for r in range(4)]
            s = m
        s = [b ^ k for b, k in zip(s, rk[rnd])]
    return bytes(s)


def aes_ctr(key, iv16, n):
    """n bytes of keystream: block j is AES(iv16 + j) as a 128-bit big-endian number (no carry leaves the low 32 bits in any use here)"""
    base = int.from_bytes(iv16, "big")
    out = b""
    for j in range((n + 15) // 16):
        out += aes_encrypt(key, ((base + j) & ((1 << 128) - 1)).to_bytes(16, "big"))
    return out[:n]


# ---- GCM (SP 800-38D) ----
R = 0xE1 << 120


def gf_mul(x, y):
    """algorithm 1: blocks as integers whose most significant bit is the block's first bit"""
    z, v = 0, y
    for i in range(128):
        if (x >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ R if v & 1 else v >> 1
    return z


def ghash(h, aad, c):
    y = 0
    pad = lambda b: bytes(b) + bytes(-len(b) % 16)
    data = pad(aad) + pad(c) + struct.pack(">QQ", 8 * len(aad), 8 * len(c))
    for k in range(0, len(data), 16):
        y = gf_mul(y ^ int.from_bytes(data[k:k + 16], "big"), h)
    return y.to_bytes(16, "big")


def gcm_encrypt(key, iv, aad, plain):
    """a 12-byte IV -> (ciphertext, the 16-byte tag)"""
    assert len(iv) == 12
    c = bytes(a ^ b for a, b in zip(plain, aes_ctr(key, iv + struct.pack(">I", 2), len(plain))))
    h = int.from_bytes(aes_encrypt(key, bytes(16)), "big")
    tag = bytes(a ^ b for a, b in zip(ghash(h, aad, c), aes_encrypt(key, iv + struct.pack(">I", 1))))
    return c, tag


def gcm_decrypt(key, iv, aad, c, tag):
    """-> the plaintext, or None where the tag does not hold"""
    h = int.from_bytes(aes_encrypt(key, bytes(16)), "big")
    want = bytes(a ^ b for a, b in zip(ghash(h, aad, c), aes_encrypt(key, iv + struct.pack(">I", 1))))
    if want != bytes(tag):
        return None
    return bytes(a ^ b for a, b in zip(c, aes_ctr(key, iv + struct.pack(">I", 2), len(c))))


# ---- RFC 7714 ----
def derive(master_key, master_salt, label, n):
    """RFC 7714 11: RFC 3711 4.3.1 with the 12-byte salt followed by two zero bytes, AES-CM under the master key of either size"""
    x = int.from_bytes(bytes(master_salt) + b"\0\0", "big") ^ (label << 48)
    return aes_ctr(master_key, (x << 16).to_bytes(16, "big"), n)


def session_keys(master_key, master_salt):
    """-> (session key of the master key's size, session salt of 12 bytes)"""
    return derive(master_key, master_salt, 0, len(master_key)), derive(master_key, master_salt, 2, 12)


def packet_iv(salt, ssrc, roc, seq):
    return bytes(a ^ b for a, b in zip(struct.pack(">HIIH", 0, ssrc & 0xFFFFFFFF, roc & 0xFFFFFFFF, seq & 0xFFFF), salt))


def make_context(master_key, master_salt):
    """the 128 words of lc3plus_srtp_gcm_make_context, as uint32"""
    ke, ks = session_keys(master_key, master_salt)
    words = []
    for rk in aes_expand(ke):
        words += list(struct.unpack(">4I", bytes(rk)))
    words += [0] * (60 - len(words)) + [len(ke) // 4 + 6] + list(struct.unpack(">3I", ks))
    h = int.from_bytes(aes_encrypt(ke, bytes(16)), "big")
    for e in range(16):                                                # e(x) * H, the nibble's highest bit the lowest power: the nibble at the block's front
        words += list(struct.unpack(">4I", gf_mul(e << 124, h).to_bytes(16, "big")))
    return np.array(words, np.uint32)


class Keys:
    """a source's or route's session keys beside its context"""

    def __init__(self, master_key, master_salt):
        self.ke, self.ks = session_keys(master_key, master_salt)
        self.ctx = make_context(master_key, master_salt)


def protect_packet(keys, pkt, roc, h=12):
    """an RTP packet (bytes) -> the SRTP packet: header, ciphertext, tag"""
    seq, ssrc = struct.unpack(">H", pkt[2:4])[0], struct.unpack(">I", pkt[8:12])[0]
    c, tag = gcm_encrypt(keys.ke, packet_iv(keys.ks, ssrc, roc, seq), pkt[:h], pkt[h:])
    return bytes(pkt[:h]) + c + tag


def protect(pkt_route, pkt_offset, pkt_size, pkt_status, n_packets, wire, header_room, payload_room, keys, roc, seq_base, next_seq, dst, dst_stride):
    """-> dict like api.plan_srtp_gcm_protect's; keys: one Keys per route"""
    wire, dst = np.asarray(wire, np.uint8), np.array(dst, np.uint8)
    m, nr = len(pkt_route), len(keys)
    out_offset, out_size, out_status = np.zeros(m, np.int64), np.zeros(m, np.int32), np.zeros(m, np.uint8)
    for p in range(min(int(n_packets), m)):
        out_offset[p] = p * dst_stride
        r, off, size = int(pkt_route[p]), int(pkt_offset[p]), int(pkt_size[p])
        if not int(pkt_status[p]) & STAMPED:
            out_status[p] = NOT_STAMPED
        elif r < 0 or r >= nr:
            out_status[p] = BAD_ROUTE
        elif off < 0 or size < header_room or size > MAX_PACKET or off + size > wire.size:
            out_status[p] = RANGE
        elif size - header_room + payload_room + 12 + TAG > dst_stride or (p + 1) * dst_stride > dst.size:
            out_status[p] = OVERFLOW
        else:
            pkt = wire[off + header_room - payload_room - 12:off + size].tobytes()
            seq = struct.unpack(">H", pkt[2:4])[0]
            b = int(seq_base[r]) & 0xFFFF
            roc_p = (int(roc[r]) + ((b + ((seq - b) & 0xFFFF)) >> 16)) & 0xFFFFFFFF
            out = protect_packet(keys[r], pkt, roc_p)
            dst[p * dst_stride:p * dst_stride + len(out)] = np.frombuffer(out, np.uint8)
            out_size[p], out_status[p] = len(out), PROTECTED
    next_roc = None
    if next_seq is not None:
        next_roc = np.zeros(nr, np.uint32)
        for r in range(nr):
            b = int(seq_base[r]) & 0xFFFF
            next_roc[r] = (int(roc[r]) + ((b + ((int(next_seq[r]) - int(seq_base[r])) & 0xFFFF)) >> 16)) & 0xFFFFFFFF
        next_roc = next_roc.view(np.int32)
    return dict(dst=dst, out_offset=out_offset, out_size=out_size, out_status=out_status, next_roc=next_roc)


def unprotect(ring, dg_offsets, dg_sizes, ssrc_key, keys, state):
    """-> dict like api.plan_srtp_gcm_unprotect's; keys: one Keys per source; state [n_ssrc, 8]"""
    ring = np.array(ring, np.uint8)
    state = (np.asarray(state).astype(np.int64) & 0xFFFFFFFF).reshape(-1, STATE_WORDS)
    n, S = len(dg_offsets), len(ssrc_key)
    items = [ref._checks(ring, int(dg_offsets[i]), int(dg_sizes[i]), TAG, ssrc_key) for i in range(n)]
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
            v, refused = ref.guess(roc, s_l, seq)
            idx = (v << 16) | seq
            top = (roc << 16) | s_l
            win = int(state[s, 3]) | int(state[s, 4]) << 32
            data = ring[off:off + size - TAG].tobytes()
            if refused:
                st = REPLAY_OLD
            elif started and top - idx >= 64:
                st = REPLAY_OLD
            elif started and top - idx >= 0 and (win >> (top - idx)) & 1:
                st = REPLAYED
            else:
                plain = gcm_decrypt(keys[s].ke, packet_iv(keys[s].ks, ssrc, v, seq), data[:h], data[h:], ring[off + size - TAG:off + size].tobytes())
                if plain is None:
                    st = AUTH
                else:
                    ring[off + h:off + len(data)] = np.frombuffer(plain, np.uint8)
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
