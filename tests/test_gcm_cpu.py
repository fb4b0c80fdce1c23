"""Secure RTP with AES-GCM without a GPU (include/lc3plus_batch.h "Secure RTP, AEAD"): the primitives of the plain Python restatement (gcm_ref.py) against
libcrypto through ctypes, the openssl program and two published vectors; the exported symbols and constants; lc3plus_srtp_gcm_make_context against the
restatement; lc3plus_plan_srtp_gcm_protect and lc3plus_plan_srtp_gcm_unprotect - the text the kernels run - against it on every output and every byte of the
lists of gcm_cases.py, 16- and 32-byte keys side by side; protect then unprotect gives the plaintext back; the split property; every refusal in the header's
order against a zero-filled block in place of a batch; a missing sibling library; and the host code once more in a program of its own under AddressSanitizer
+ UndefinedBehaviorSanitizer (tools/gcm_plan_driver.c).  Every comparison is equality."""
import ctypes as C
import ctypes.util
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import audio_codec_amd
from audio_codec_amd import api
import gcm_cases as cases
import gcm_ref as ref

NEW = ["lc3plus_srtp_gcm_make_context", "lc3plus_enc_batch_srtp_gcm_protect", "lc3plus_dec_batch_srtp_gcm_protect", "lc3plus_plan_srtp_gcm_protect",
       "lc3plus_dec_batch_srtp_gcm_unprotect", "lc3plus_plan_srtp_gcm_unprotect"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_codec_amd", "csrc")
STUB_DIR = os.path.join(ROOT, "audio_codec_amd", "_stub")
LC3_OK, LC3_ERROR, LC3_NULL_ERROR = 0, 1, 3
OPENSSL = shutil.which("openssl")
needs_openssl = pytest.mark.skipif(OPENSSL is None, reason="no openssl program")
CRYPTO = ctypes.util.find_library("crypto")
needs_libcrypto = pytest.mark.skipif(CRYPTO is None, reason="no libcrypto")


def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- the restatement's primitives against something independent ----
def test_published_vectors():
    """SP 800-38D's first two test cases (the GCM specification's test cases 1 and 2): a zero key and IV, no data, then one zero block"""
    assert ref.gcm_encrypt(bytes(16), bytes(12), b"", b"") == (b"", bytes.fromhex("58e2fccefa7e3061367f1d57a4e7455a"))
    assert ref.gcm_encrypt(bytes(16), bytes(12), b"", bytes(16)) == (bytes.fromhex("0388dace60b6a392f328c2b971b2fe78"), bytes.fromhex("ab6e47d42cec13bdf53a67b21257bddf"))
    assert ref.aes_encrypt(bytes(range(32)), bytes.fromhex("00112233445566778899aabbccddeeff")) == bytes.fromhex("8ea2b7ca516745bfeafc49904b496089")    # FIPS-197 C.3


class _Evp:
    """AES-GCM encryption by libcrypto's EVP interface"""

    def __init__(self):
        L = C.CDLL(CRYPTO)
        L.EVP_CIPHER_CTX_new.restype = C.c_void_p
        L.EVP_aes_128_gcm.restype = L.EVP_aes_256_gcm.restype = C.c_void_p
        L.EVP_CIPHER_CTX_free.argtypes = [C.c_void_p]
        L.EVP_EncryptInit_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p]
        L.EVP_EncryptUpdate.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
        L.EVP_EncryptFinal_ex.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
        L.EVP_CIPHER_CTX_ctrl.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        self.L = L

    def encrypt(self, key, iv, aad, plain):
        L, n = self.L, C.c_int(0)
        ctx = L.EVP_CIPHER_CTX_new()
        try:
            assert L.EVP_EncryptInit_ex(ctx, L.EVP_aes_128_gcm() if len(key) == 16 else L.EVP_aes_256_gcm(), None, None, None) == 1
            assert L.EVP_CIPHER_CTX_ctrl(ctx, 0x9, len(iv), None) == 1                                 # EVP_CTRL_AEAD_SET_IVLEN
            assert L.EVP_EncryptInit_ex(ctx, None, None, key, iv) == 1
            if aad:
                assert L.EVP_EncryptUpdate(ctx, None, C.byref(n), aad, len(aad)) == 1
            out = C.create_string_buffer(len(plain) + 16)
            got = 0
            if plain:
                assert L.EVP_EncryptUpdate(ctx, out, C.byref(n), plain, len(plain)) == 1
                got = n.value
            tail = C.create_string_buffer(16)
            assert L.EVP_EncryptFinal_ex(ctx, tail, C.byref(n)) == 1 and n.value == 0
            tag = C.create_string_buffer(16)
            assert L.EVP_CIPHER_CTX_ctrl(ctx, 0x10, 16, tag) == 1                                      # EVP_CTRL_AEAD_GET_TAG
            return out.raw[:got], tag.raw
        finally:
            L.EVP_CIPHER_CTX_free(ctx)


@needs_libcrypto
def test_gcm_equals_libcrypto():
    """both key sizes, associated data of 0 and 12 to 28 bytes, payloads of 0 to 80 bytes and a long one; and an SRTP packet of each key size as a whole"""
    evp = _Evp()
    rng = np.random.default_rng(1)
    for kb in (16, 32):
        for aad_len in (0, 12, 13, 15, 16, 17, 20, 24, 28):
            for n in (0, 1, 15, 16, 17, 31, 32, 33, 48, 80, 401):
                key, iv, aad, plain = _bytes(rng, kb), _bytes(rng, 12), _bytes(rng, aad_len), _bytes(rng, n)
                assert ref.gcm_encrypt(key, iv, aad, plain) == evp.encrypt(key, iv, aad, plain), (kb, aad_len, n)
                c, tag = ref.gcm_encrypt(key, iv, aad, plain)
                assert ref.gcm_decrypt(key, iv, aad, c, tag) == plain
                assert ref.gcm_decrypt(key, iv, aad, c, bytes([tag[0] ^ 1]) + tag[1:]) is None
    for k in range(2):
        keys = cases.keys_for(k)
        pkt = ref.rtp_packet(0xFFF0, 77, 0x80000001, _bytes(rng, 61), csrc=(1, 2))
        c, tag = evp.encrypt(keys.ke, ref.packet_iv(keys.ks, 0x80000001, 0xFFFFFFFE, 0xFFF0), pkt[:20], pkt[20:])
        assert ref.protect_packet(keys, pkt, 0xFFFFFFFE, 20) == pkt[:20] + c + tag


def _openssl(args, data=b""):
    return subprocess.run([OPENSSL] + args, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout


@needs_openssl
def test_gmac_equals_openssl():
    """the tag over an empty payload is GMAC over the associated data"""
    rng = np.random.default_rng(2)
    for n in (12, 16, 28, 75):
        key, iv, aad = _bytes(rng, 16), _bytes(rng, 12), _bytes(rng, n)
        out = _openssl(["mac", "-cipher", "AES-128-GCM", "-macopt", "hexkey:" + key.hex(), "-macopt", "hexiv:" + iv.hex(), "-binary", "GMAC"], aad)
        assert ref.gcm_encrypt(key, iv, aad, b"") == (b"", out)


@needs_openssl
def test_aes_256_block_and_keystream_equal_openssl():
    rng = np.random.default_rng(3)
    for _ in range(8):
        key, block = _bytes(rng, 32), _bytes(rng, 16)
        assert ref.aes_encrypt(key, block) == _openssl(["enc", "-aes-256-ecb", "-nopad", "-K", key.hex()], block)
    for kb, name in ((16, "-aes-128-ctr"), (32, "-aes-256-ctr")):
        for n in (1, 16, 17, 400):
            key, iv = _bytes(rng, kb), _bytes(rng, 12) + b"\0\0\0\2"
            assert ref.aes_ctr(key, iv, n) == _openssl(["enc", name, "-K", key.hex(), "-iv", iv.hex()], bytes(n))
    for kb in (16, 32):                                               # the key derivation is this keystream from the salt, the label in byte 7
        mk, ms = _bytes(rng, kb), _bytes(rng, 12)
        name = "-aes-128-ctr" if kb == 16 else "-aes-256-ctr"
        for label, n in ((0, kb), (2, 12)):
            x = bytearray(ms + bytes(4))
            x[7] ^= label
            assert ref.derive(mk, ms, label, n) == _openssl(["enc", name, "-K", mk.hex(), "-iv", bytes(x).hex()], bytes(n))


# ---- the interface ----
def test_symbols_are_exported():
    L = audio_codec_amd.load_library()
    text = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    for s in NEW:
        assert s in api.EXPORTS and hasattr(L, s) and re.search(r"\b%s\s*\(" % s, text), s
    for f in (api.srtp_gcm_make_context, api.Batch.srtp_gcm_protect_device, api.DecBatch.srtp_gcm_protect_device, api.DecBatch.srtp_gcm_unprotect_device,
              api.DecBatch.srtp_gcm_unprotect, api.plan_srtp_gcm_protect, api.plan_srtp_gcm_unprotect):
        assert callable(f)
    assert os.path.exists(os.path.join(ROOT, "audio_codec_amd", "liblc3plus_gcm_hip.so"))
    assert "the AEAD suites of RFC 7714, header-extension" not in text


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define\s+LC3PLUS_SRTP_GCM_(\w+)\s+\((\d+)\)", text)}
    assert header == dict(CTX_WORDS=128, TAG_BYTES=16)
    assert api.SRTP_GCM_CTX_WORDS == ref.CTX_WORDS == 128 and api.SRTP_GCM_TAG_BYTES == ref.TAG == 16


def test_make_context_equals_the_restatement():
    rng = np.random.default_rng(4)
    for kb in (16, 32):
        mk, ms = _bytes(rng, kb), _bytes(rng, 12)
        ctx = api.srtp_gcm_make_context(mk, ms)
        assert ctx.dtype == np.int32 and ctx.shape == (128,) and np.array_equal(ctx.view(np.uint32), ref.make_context(mk, ms))
        words = ctx.view(np.uint32)
        ke, ks = ref.session_keys(mk, ms)
        assert words[:kb // 4].astype(">u4").tobytes() == ke and words[60] == (10 if kb == 16 else 14) and words[61:64].astype(">u4").tobytes() == ks
        assert words[64 + 32:64 + 36].astype(">u4").tobytes() == ref.aes_encrypt(ke, bytes(16)) and not words[64:68].any()        # entry 8 is H, entry 0 is zero
        if kb == 16:
            assert not words[44:60].any()
    for k in range(6):
        assert np.array_equal(cases.keys_for(k).ctx.view(np.int32),
                              api.srtp_gcm_make_context(bytes((29 * k + 11 * j + 5) & 255 for j in range(32 if k & 1 else 16)), bytes((17 * k + 3 * j + 9) & 255 for j in range(12))))
    for key, salt in ((bytes(15), bytes(12)), (bytes(24), bytes(12)), (bytes(16), bytes(14))):
        with pytest.raises(ValueError):
            api.srtp_gcm_make_context(key, salt)
    L = audio_codec_amd.load_library()
    a = (C.c_uint8 * 512)()
    A = C.addressof(a)
    assert L.lc3plus_srtp_gcm_make_context(None, 16, A, A) == L.lc3plus_srtp_gcm_make_context(A, 16, None, A) == L.lc3plus_srtp_gcm_make_context(A, 16, A, None) == LC3_NULL_ERROR
    assert L.lc3plus_srtp_gcm_make_context(None, 7, A, A) == LC3_NULL_ERROR
    for kb in (0, 15, 24, 33, -16):
        assert L.lc3plus_srtp_gcm_make_context(A, kb, A, A) == LC3_ERROR and not any(a)


# ---- the plans against the restatement ----
def _plan_unprotect(c, **kw):
    return api.plan_srtp_gcm_unprotect(c["ring"], c["offs"], c["sizes"], c["ssrc_key"], c["ctx"], c["state"], **kw)


def _same(got, want, name):
    for k in want:
        bad = np.argwhere(np.asarray(got[k]).reshape(-1) != np.asarray(want[k]).reshape(-1))
        assert np.asarray(got[k]).shape == np.asarray(want[k]).shape and len(bad) == 0, (name, k, "first differing elements", bad[:6].ravel().tolist())


@pytest.mark.parametrize("which", sorted(cases.CASES))
def test_plan_unprotect_equals_the_restatement(which):
    c = cases.CASES[which]()
    assert {int(k.ctx[60]) for k in c["keys"]} == ({10} if which == "crowd_one" else {10, 14})           # both key sizes inside the one call
    got = _plan_unprotect(c)
    want = ref.unprotect(c["ring"], c["offs"], c["sizes"], c["ssrc_key"], c["keys"], c["state"])
    _same(got, want, which)
    for i, st in c["expect"].items():
        assert got["status"][i] == st, (which, i, int(got["status"][i]), st)
    refused = got["status"] != ref.OK
    assert (got["sizes"][refused] == 0).all() and (got["index"][refused] == 0).all()
    for i in np.flatnonzero(refused):                                 # not one byte of a refused item is changed
        o, n = int(c["offs"][i]), int(c["sizes"][i])
        if 0 <= o and n > 0 and o + n <= c["ring"].size:
            assert np.array_equal(got["ring"][o:o + n], c["ring"][o:o + n]), i
    ok = np.flatnonzero(~refused)
    assert np.array_equal(got["sizes"][ok], c["sizes"][ok] - 16)
    none = _plan_unprotect(c, optional=())
    assert none["status"] is None and none["index"] is None and none["stats"] is None
    assert np.array_equal(none["state"], got["state"]) and np.array_equal(none["ring"], got["ring"]) and np.array_equal(none["sizes"], got["sizes"])


def test_the_scenarios_cover_what_they_name():
    c = cases.shapes()
    h = np.array([ref.header_len(c["ring"][o:o + 100].tobytes()) for o in c["offs"]])
    pay = c["sizes"] - 16 - h
    for hl in (12, 16, 20, 24, 28):
        for n in cases.PAYLOADS:
            assert {int(o) % 4 for o in c["offs"][(h == hl) & (pay == n)]} == {0, 1, 2, 3}, (hl, n)
    assert (h == 80).any() and (c["ring"][c["offs"]] & 0x10).any()
    t = cases.tampered()
    st = np.array([t["expect"][i] for i in range(len(t["offs"]))])
    assert (st == ref.AUTH).sum() >= 14 and (t["sizes"][st == ref.SHORT] == 27).all() and (st == ref.SHORT).sum() == 2
    assert len(cases.crowd(True)["offs"]) >= 300 and len(cases.crowd(False)["offs"]) >= 300 and len(cases.protect_list()["route"]) >= 300


def test_the_window_is_the_hmac_rule_s():
    """lc3_gcm_shim.h restates the replay checks of lc3_srtp_shim.h's unprotect rule: on the scenarios that are about them the statuses, indices and states
    of the two plans agree item by item (the same SSRCs, SEQs, rollover counters and states; only the transform differs)"""
    import srtp_cases
    for which in ("rollover", "window", "fresh"):
        g, s = cases.CASES[which](), srtp_cases.CASES[which](10)
        a = _plan_unprotect(g)
        b = api.plan_srtp_unprotect(s["ring"], s["offs"], s["sizes"], s["ssrc_key"], s["ctx"], s["state"], 10)
        assert np.array_equal(g["state"], s["state"])
        for k in ("status", "index", "state", "stats"):
            assert np.array_equal(a[k], b[k]), (which, k)


def test_a_source_without_an_accepted_item_keeps_its_state():
    c = cases.fresh()
    got = _plan_unprotect(c)
    assert np.array_equal(got["state"][2], c["state"][2]) and c["state"][2].any()
    assert got["state"][0].tolist() == cases.state_block(1, 1, 100, 1)


def _plan_protect(c, dst0, **kw):
    return api.plan_srtp_gcm_protect(c["route"], c["off"], c["size"], c["status"], c["wire"], c["ctx"], c["roc"], c["seq_base"], dst0, c["stride"], c["hr"], c["pr"],
                                     n_packets=c["n_packets"], **kw)


def test_plan_protect_equals_the_restatement():
    c = cases.protect_list()
    dst0 = np.full(c["dst_capacity"], 0x6B, np.uint8)
    got = _plan_protect(c, dst0, next_seq=c["next_seq"])
    want = ref.protect(c["route"], c["off"], c["size"], c["status"], c["n_packets"], c["wire"], c["hr"], c["pr"], c["keys"], c["roc"].view(np.uint32), c["seq_base"],
                       c["next_seq"], dst0, c["stride"])
    _same(got, want, "protect")
    for i, st in c["expect"].items():
        assert got["out_status"][i] == st, (i, int(got["out_status"][i]), st)
    k = c["n_packets"]
    assert not got["out_size"][k:].any() and not got["out_status"][k:].any() and (got["out_size"][got["out_status"] != ref.PROTECTED] == 0).all()
    done = got["out_status"] == ref.PROTECTED
    assert np.array_equal(got["out_size"][done], c["size"][done] - c["hr"] + c["pr"] + 12 + 16)
    without = _plan_protect(c, dst0)
    assert without["next_roc"] is None and np.array_equal(without["dst"], got["dst"])


def test_protect_then_unprotect_gives_the_plaintext_back():
    c = cases.protect_list()
    p = _plan_protect(c, np.zeros(c["dst_capacity"], np.uint8))
    ssrc_key = np.array([0x11, 0x80000001], np.uint32).view(np.int32)                 # ascending: route 1, then route 0
    state = np.array([cases.state_block(0, 6), cases.state_block(0, 0xFFFFFFFF)], np.uint32).view(np.int32)
    u = api.plan_srtp_gcm_unprotect(p["dst"], p["out_offset"], p["out_size"], ssrc_key, c["ctx"][::-1], state)
    done = p["out_status"] == ref.PROTECTED
    assert done.sum() > 300 and np.array_equal(u["sizes"][done], p["out_size"][done] - 16) and (u["status"][done] == ref.OK).all()
    assert np.isin(u["status"][~done], (ref.SHORT, ref.UN_RANGE)).all()      # out_size 0; the slots past the destination lie outside the ring as well
    for i in np.flatnonzero(done):
        a = int(c["off"][i]) + c["hr"] - c["pr"] - 12
        o, n = int(p["out_offset"][i]), int(u["sizes"][i])
        assert np.array_equal(u["ring"][o:o + n], c["wire"][a:a + n]), i
    wrong = api.plan_srtp_gcm_unprotect(p["dst"], p["out_offset"], p["out_size"], ssrc_key, c["ctx"], state)            # each source under the other's key
    assert (wrong["status"][done] == ref.AUTH).all() and np.array_equal(wrong["ring"], p["dst"])


@pytest.mark.parametrize("cut", [1, 41, 89])
def test_split_calls_carry_the_state(cut):
    c, _ = cases.split_lists()
    whole = _plan_unprotect(c)
    first = _plan_unprotect(dict(c, offs=c["offs"][:cut], sizes=c["sizes"][:cut]))
    second = _plan_unprotect(dict(c, ring=first["ring"], offs=c["offs"][cut:], sizes=c["sizes"][cut:], state=first["state"]))
    assert np.array_equal(whole["state"], second["state"]) and np.array_equal(whole["ring"], second["ring"]) and (whole["status"] == ref.OK).all()
    for k in ("status", "index", "sizes"):
        assert np.array_equal(whole[k], np.concatenate([first[k], second[k]])), k
    again = _plan_unprotect(dict(c, ring=whole["ring"], state=whole["state"]))            # the same list once more: every item is a replay now
    assert set(again["status"].tolist()) <= {ref.REPLAYED, ref.REPLAY_OLD, ref.AUTH} and np.array_equal(again["state"], whole["state"])


# ---- the refusals ----
def test_refusals_in_the_header_s_order():
    """against a zero-filled block in place of a batch: a refusal returns before anything of the batch or the device is touched.  Every array is the same 64
    zero bytes (the destination another block), which no refused call may write"""
    L = audio_codec_amd.load_library()
    fake, a, d = (C.c_uint8 * 4096)(), (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    A, D, B = C.addressof(a), C.addressof(d), C.addressof(fake)
    names = ("max_packets", "n_packets", "pkt_route", "pkt_offset", "pkt_size", "pkt_status", "wire", "wire_capacity", "header_room", "payload_room", "n_routes", "ctx",
             "roc", "seq_base", "next_seq", "dst", "dst_capacity", "dst_stride", "out_offset", "out_size", "out_status", "next_roc")
    good = dict(max_packets=1, wire_capacity=64, header_room=12, payload_room=0, n_routes=1, dst=D, dst_capacity=64, dst_stride=32)

    def protect(fn, batch, **kw):
        v = dict({k: A for k in names}, **good)
        v.update(kw)
        args = [v[k] for k in names]
        return fn(*(([batch] if batch != "plan" else []) + args + ([None, 1] if batch != "plan" else [])))
    for fn in (L.lc3plus_enc_batch_srtp_gcm_protect, L.lc3plus_dec_batch_srtp_gcm_protect):
        assert protect(fn, None) == LC3_NULL_ERROR
        for k in ("n_packets", "pkt_route", "pkt_offset", "pkt_size", "pkt_status", "wire", "ctx", "roc", "seq_base", "dst", "out_offset", "out_size", "out_status", "next_seq"):
            assert protect(fn, B, **{k: None}) == LC3_NULL_ERROR, k
            assert protect(fn, B, max_packets=0, **{k: None}) == LC3_NULL_ERROR, k                      # NULL first
        assert protect(fn, B, next_seq=None, next_roc=None) == LC3_ERROR                               # passes every check: the block is no batch
        for bad in (dict(max_packets=0), dict(max_packets=-1), dict(max_packets=1 << 29), dict(wire_capacity=-1), dict(payload_room=-1), dict(header_room=11),
                    dict(header_room=14, payload_room=3), dict(n_routes=0), dict(dst_capacity=-1), dict(dst_stride=0), dict(dst_stride=(1 << 30) + 1),
                    dict(dst=A + 32, dst_capacity=16), dict(dst=A - 8, dst_capacity=9)):
            assert protect(fn, B, **bad) == LC3_ERROR, bad
    P = L.lc3plus_plan_srtp_gcm_protect
    assert protect(P, "plan", pkt_route=None) == LC3_NULL_ERROR and protect(P, "plan", n_routes=0) == LC3_ERROR and protect(P, "plan", dst=A) == LC3_ERROR
    unames = ("n_items", "ring", "ring_capacity", "dg_offsets", "dg_sizes", "n_ssrc", "ssrc_key", "ctx", "state_in", "state_out", "sizes_out", "status", "index", "stats")
    W = api.srtp_workspace_bytes(1, 1)
    ugood = dict(n_items=1, ring_capacity=64, n_ssrc=1)

    def unprotect(batch, workspace=D, workspace_bytes=W, **kw):
        v = dict({k: A for k in unames}, **ugood)
        v.update(kw)
        return L.lc3plus_dec_batch_srtp_gcm_unprotect(batch, *[v[k] for k in unames], workspace, workspace_bytes, None, 1)
    assert unprotect(None) == LC3_NULL_ERROR and unprotect(B, workspace=None) == LC3_NULL_ERROR
    for k in ("ring", "dg_offsets", "dg_sizes", "ssrc_key", "ctx", "state_in", "state_out", "sizes_out"):
        assert unprotect(B, **{k: None}) == LC3_NULL_ERROR, k
        assert unprotect(B, n_items=0, **{k: None}) == LC3_NULL_ERROR, k
    for bad in (dict(n_items=0), dict(n_items=-1), dict(n_items=1 << 29), dict(ring_capacity=-1), dict(n_ssrc=0), dict(n_ssrc=-4), dict(workspace_bytes=W - 1),
                dict(workspace_bytes=0)):
        assert unprotect(B, **bad) == LC3_ERROR, bad
    assert unprotect(B, status=None, index=None, stats=None) == LC3_ERROR                              # passes every check: the block is no batch
    U = L.lc3plus_plan_srtp_gcm_unprotect
    ok = [1, A, 64, A, A, 1, A, A, A, A, A, None, None, None]
    for at in (1, 3, 4, 6, 7, 8, 9, 10):
        assert U(*[None if k == at else v for k, v in enumerate(ok)]) == LC3_NULL_ERROR, at
    assert U(*([0] + ok[1:])) == LC3_ERROR and U(*(ok[:5] + [0] + ok[6:])) == LC3_ERROR and U(*(ok[:2] + [-1] + ok[3:])) == LC3_ERROR
    assert not any(fake) and not any(a) and not any(d)


# ---- a missing sibling, in a child process (the library is looked for once per process) ----
CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, %(root)r)
import audio_codec_amd
L = audio_codec_amd.load_library()
a, d = (C.c_uint64 * 8)(), (C.c_uint64 * 64)()
A, D = C.addressof(a), C.addressof(d)
L.lc3stub_reset()
enc, dec = C.c_void_p(), C.c_void_p()
assert L.lc3plus_enc_batch_create(C.byref(enc), 1, 48000, 1, 10.0, 0, (C.c_int * 1)(64000), 0) == 0
assert L.lc3plus_dec_batch_create(C.byref(dec), 1, 48000, 1, 10.0, 0, (C.c_int * 1)(80), 0) == 0
protect = [1] + [A] * 6 + [64, 12, 0, 1] + [A] * 4 + [D, 64, 32] + [A] * 4 + [None, 1]
calls = {
    "enc_srtp_gcm_protect": lambda: L.lc3plus_enc_batch_srtp_gcm_protect(enc, *protect),
    "dec_srtp_gcm_protect": lambda: L.lc3plus_dec_batch_srtp_gcm_protect(dec, *protect),
    "srtp_gcm_unprotect": lambda: L.lc3plus_dec_batch_srtp_gcm_unprotect(dec, 1, A, 64, A, A, 1, A, A, A, A, A, A, A, A, D, L.lc3plus_srtp_workspace_bytes(1, 1), None, 1),
}
assert L.lc3plus_srtp_workspace_bytes(1, 1) <= 512
for on in (0, 1, 1):                                                  # off: the device is refused, in front of the library; on, twice: the library is
    L.lc3stub_device_args(on)
    sys.stderr.flush()
    print("round", on, flush=True)
    sys.stderr.write("round %%d\n" %% on)
    for name in %(calls)r:
        print(name, calls[name](), flush=True)
assert not any(a) and not any(d)
L.lc3plus_enc_batch_destroy(enc); L.lc3plus_dec_batch_destroy(dec)
print("done")
"""
CALLS = ["enc_srtp_gcm_protect", "dec_srtp_gcm_protect", "srtp_gcm_unprotect"]


def test_a_missing_gcm_sibling_fails_its_calls_alone_and_is_named_once():
    """through the stub build, whose directory holds the host code and no kernel library: with the device granted the three GCM calls get as far as looking
    for liblc3plus_gcm_hip.so, return LC3_ERROR and nothing else, and stderr names the file once however often they are repeated"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "stub"])
    assert "liblc3plus_gcm_hip.so" not in os.listdir(STUB_DIR)
    env = dict(os.environ, LC3PLUS_HIP_LIB=os.path.join(STUB_DIR, "liblc3plus_stub.so"))
    r = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, calls=CALLS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, universal_newlines=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = r.stdout.split()
    assert out[-1] == "done"
    results = list(zip(out[:-1:2], out[1:-1:2]))
    assert results == sum(([("round", str(on))] + [(n, str(LC3_ERROR)) for n in CALLS] for on in (0, 1, 1)), [])
    err = r.stderr.splitlines()
    assert err[:err.index("round 1")] == ["round 0"]                    # a call the device refuses does not look for its library
    assert len([ln for ln in err if "liblc3plus_gcm_hip.so" in ln]) == 1 and len([ln for ln in err if "liblc3plus_" in ln]) == 1, r.stderr
    assert err[-1] == "round 1"                                         # nothing in the second round


# ---- the host code under the sanitizers, in a program of its own ----
@pytest.fixture(scope="module")
def driver():
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    subprocess.check_call(["make", "-s", "-C", CSRC, "gcm_driver"])
    return os.path.join(STUB_DIR, "gcm_plan_driver")


def _run(driver, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([driver] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, universal_newlines=True)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_driver_refusals_under_the_sanitizers(driver):
    assert _run(driver, "refuse").strip() == "refusals ok"


@pytest.mark.parametrize("seed,n", [(1, 1), (2, 64), (3, 700)])
def test_driver_roundtrip_under_the_sanitizers(driver, seed, n):
    """every buffer exactly as large as its capacity says; route 0 has a 16-byte key, route 1 a 32-byte one; the program itself checks that the plaintext comes
    back and that a damaged tag stops its item alone.  The contexts it prints are the restatement's on the keys it drew"""
    text = _run(driver, "roundtrip", seed, n)
    out = dict(line.split(" ", 1) for line in text.splitlines() if " " in line)
    x = seed
    draws = []
    for _ in range(16 + 12 + 32 + 12):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        draws.append((x >> 8) & 255)
    want = np.concatenate([ref.make_context(bytes(draws[:16]), bytes(draws[16:28])), ref.make_context(bytes(draws[28:60]), bytes(draws[60:72]))])
    assert np.array_equal(np.array(out["ctx"].split(), np.uint64).astype(np.uint32), want)
    assert out["stats"].split()[0] == str(n) and "damaged ok" in text
