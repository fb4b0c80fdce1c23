"""Secure RTP without a GPU (include/lc3plus_batch.h "Secure RTP"): the primitives of the plain Python restatement (srtp_ref.py) against the openssl program and
the published vectors (FIPS-197 C.1, RFC 3711 B.2 and B.3); the exported symbols and constants; lc3plus_srtp_make_context against the restatement;
lc3plus_plan_srtp_protect and lc3plus_plan_srtp_unprotect - the text the kernels run - against it on every output and every byte of the lists of srtp_cases.py;
protect then unprotect gives the plaintext back; the split property; every refusal in the header's order against a zero-filled block in place of a batch; and
the host code once more in a program of its own under AddressSanitizer + UndefinedBehaviorSanitizer (tools/srtp_plan_driver.c).  Every comparison is
equality."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import audio_codec_amd
from audio_codec_amd import api
import srtp_cases as cases
import srtp_ref as ref

NEW = ["lc3plus_srtp_make_context", "lc3plus_enc_batch_srtp_protect", "lc3plus_dec_batch_srtp_protect", "lc3plus_plan_srtp_protect",
       "lc3plus_dec_batch_srtp_unprotect", "lc3plus_plan_srtp_unprotect", "lc3plus_srtp_workspace_bytes"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_codec_amd", "csrc")
LC3_OK, LC3_ERROR, LC3_NULL_ERROR = 0, 1, 3
OPENSSL = shutil.which("openssl")
needs_openssl = pytest.mark.skipif(OPENSSL is None, reason="no openssl program")
# RFC 3711 B.3
MASTER_KEY, MASTER_SALT = bytes.fromhex("E1F97A0D3E018BE0D64FA32C06DE4139"), bytes.fromhex("0EC675AD498AFEEBB6960B3AABE6")
B3_CIPHER, B3_SALT = bytes.fromhex("C61E7A93744F39EE10734AFE3FF7A087"), bytes.fromhex("30CBBC08863D8C85D49DB34A9AE1")
B3_AUTH = bytes.fromhex("CEBE321F6FF7716B6FD4AB49AF256A156D38BAA4")
# RFC 3711 B.2
B2_KEY, B2_SALT = bytes.fromhex("2B7E151628AED2A6ABF7158809CF4F3C"), bytes.fromhex("F0F1F2F3F4F5F6F7F8F9FAFBFCFD")
B2_STREAM = bytes.fromhex("E03EAD0935C95E80E166B16DD92B4EB4" "D23513162B02D0F72A43A2FE4A5F97AB" "41E95B3BB0A2E8DD477901E4FCA894C0")


def _openssl(args, data):
    return subprocess.run([OPENSSL, "enc"] + args, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout


# ---- the restatement's primitives against something independent ----
def test_published_vectors():
    assert ref.aes_encrypt(bytes(range(16)), bytes.fromhex("00112233445566778899aabbccddeeff")) == bytes.fromhex("69c4e0d86a7b0430d8cdb78070b4c55a")    # FIPS-197 C.1
    assert ref.aes_cm(B2_KEY, ref.packet_iv(B2_SALT, 0, 0), 48) == B2_STREAM
    assert ref.session_keys(MASTER_KEY, MASTER_SALT) == (B3_CIPHER, B3_AUTH, B3_SALT)


@needs_openssl
def test_aes_block_equals_openssl():
    rng = np.random.default_rng(1)
    for _ in range(12):
        key, block = rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        assert ref.aes_encrypt(key, block) == _openssl(["-aes-128-ecb", "-nopad", "-K", key.hex()], block)


@needs_openssl
def test_keystream_equals_openssl():
    """the IV's low 16 bits are zero and a packet has fewer than 2^16 blocks, so AES-CM is plain big-endian CTR; and the published vectors hold under openssl
    too"""
    rng = np.random.default_rng(2)
    for n in (1, 16, 17, 400, 4099):
        key, salt = rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), rng.integers(0, 256, 14, dtype=np.uint8).tobytes()
        iv = ref.packet_iv(salt, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 48)))
        assert iv[14:] == b"\0\0" and ref.aes_cm(key, iv, n) == _openssl(["-aes-128-ctr", "-K", key.hex(), "-iv", iv.hex()], bytes(n))
    assert _openssl(["-aes-128-ctr", "-K", B2_KEY.hex(), "-iv", (B2_SALT + b"\0\0").hex()], bytes(48)) == B2_STREAM
    for label, want in ((0, B3_CIPHER), (1, B3_AUTH), (2, B3_SALT)):
        x = (int.from_bytes(MASTER_SALT, "big") ^ (label << 48)) << 16
        assert _openssl(["-aes-128-ctr", "-K", MASTER_KEY.hex(), "-iv", x.to_bytes(16, "big").hex()], bytes(len(want))) == want


# ---- the interface ----
def test_symbols_are_exported():
    L = audio_codec_amd.load_library()
    text = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    for s in NEW:
        assert s in api.EXPORTS and hasattr(L, s) and re.search(r"\b%s\s*\(" % s, text), s
    for f in (api.srtp_make_context, api.Batch.srtp_protect_device, api.DecBatch.srtp_protect_device, api.DecBatch.srtp_unprotect_device, api.DecBatch.srtp_unprotect,
              api.plan_srtp_protect, api.plan_srtp_unprotect, api.srtp_workspace_bytes):
        assert callable(f)
    assert os.path.exists(os.path.join(ROOT, "audio_codec_amd", "liblc3plus_srtp_hip.so"))


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define\s+LC3PLUS_SRTP_(\w+)\s+(\d+)", text)}
    want = dict(CTX_WORDS=64, PROTECTED=1, NOT_STAMPED=2, BAD_ROUTE=4, RANGE=8, OVERFLOW=16, STATE_WORDS=8, FLAGS=0, ROC=1, S_L=2, WIN_LO=3, WIN_HI=4, STARTED=1,
                OK=0, UN_RANGE=1, SHORT=2, VERSION=3, RTCP=4, HEADER=5, UNKNOWN_SSRC=6, REPLAY_OLD=7, REPLAYED=8, AUTH=9, STATS_WORDS=16)
    assert header == want
    for k, v in want.items():
        assert getattr(api, "SRTP_" + k) == v, k
        if hasattr(ref, k):
            assert getattr(ref, k) == v, k


def test_workspace_bytes():
    assert api.srtp_workspace_bytes(0, 1) == api.srtp_workspace_bytes(1, 0) == api.srtp_workspace_bytes(1 << 29, 1) == api.srtp_workspace_bytes(-1, 1) == 0
    for n, S in ((1, 1), (262144, 4096), ((1 << 29) - 1, 1), (5, 1 << 20)):
        w = api.srtp_workspace_bytes(n, S)
        assert 12 * n + 20 * S <= w <= 12 * n + 20 * S + 64, (n, S, w)


def test_make_context_equals_the_restatement():
    ctx = api.srtp_make_context(MASTER_KEY, MASTER_SALT)
    assert ctx.dtype == np.int32 and ctx.shape == (64,) and np.array_equal(ctx.view(np.uint32), ref.make_context(MASTER_KEY, MASTER_SALT))
    words = ctx.view(np.uint32)
    assert words[:4].astype(">u4").tobytes() == B3_CIPHER and words[44:48].astype(">u4").tobytes() == B3_SALT + b"\0\0" and not words[58:].any()
    for k in range(5):
        keys = cases.keys_for(k)
        assert np.array_equal(keys.ctx, api.srtp_make_context(bytes((31 * k + 7 * j + 1) & 255 for j in range(16)), bytes((13 * k + 5 * j + 3) & 255 for j in range(14))).view(np.uint32))
    with pytest.raises(ValueError):
        api.srtp_make_context(bytes(15), bytes(14))


# ---- the plans against the restatement ----
def _plan_unprotect(c, **kw):
    return api.plan_srtp_unprotect(c["ring"], c["offs"], c["sizes"], c["ssrc_key"], c["ctx"], c["state"], c["tag_len"], **kw)


def _same(got, want, name):
    for k in want:
        bad = np.argwhere(np.asarray(got[k]).reshape(-1) != np.asarray(want[k]).reshape(-1))
        assert np.asarray(got[k]).shape == np.asarray(want[k]).shape and len(bad) == 0, (name, k, "first differing elements", bad[:6].ravel().tolist())


@pytest.mark.parametrize("tag_len", [10, 4])
@pytest.mark.parametrize("which", sorted(cases.CASES))
def test_plan_unprotect_equals_the_restatement(which, tag_len):
    c = cases.CASES[which](tag_len)
    got = _plan_unprotect(c)
    want = ref.unprotect(c["ring"], c["offs"], c["sizes"], c["ssrc_key"], c["keys"], c["state"], tag_len)
    _same(got, want, which)
    for i, st in c["expect"].items():
        assert got["status"][i] == st, (which, i, int(got["status"][i]), st)
    refused = got["status"] != ref.OK
    assert (got["sizes"][refused] == 0).all() and (got["index"][refused] == 0).all()
    for i in np.flatnonzero(refused):                                 # not one byte of a refused item is changed
        o, n = int(c["offs"][i]), int(c["sizes"][i])
        if 0 <= o and n > 0 and o + n <= c["ring"].size:
            assert np.array_equal(got["ring"][o:o + n], c["ring"][o:o + n]), i
    none = _plan_unprotect(c, optional=())
    assert none["status"] is None and none["index"] is None and none["stats"] is None
    assert np.array_equal(none["state"], got["state"]) and np.array_equal(none["ring"], got["ring"]) and np.array_equal(none["sizes"], got["sizes"])


def test_a_source_without_an_accepted_item_keeps_its_state():
    c = cases.fresh(10)
    got = _plan_unprotect(c)
    assert np.array_equal(got["state"][2], c["state"][2]) and c["state"][2].any()
    assert got["state"][0].tolist() == cases.state_block(1, 1, 100, 1)           # started by its accepted items: the top is (1 << 16 | 100), 40001 lies far behind it


@pytest.mark.parametrize("tag_len", [10, 4])
def test_plan_protect_equals_the_restatement(tag_len):
    c = cases.protect_list(tag_len)
    dst0 = np.full(c["dst_capacity"], 0x6B, np.uint8)
    got = api.plan_srtp_protect(c["route"], c["off"], c["size"], c["status"], c["wire"], c["ctx"], c["roc"], c["seq_base"], dst0, c["stride"], tag_len, c["hr"], c["pr"],
                                next_seq=c["next_seq"], n_packets=c["n_packets"])
    want = ref.protect(c["route"], c["off"], c["size"], c["status"], c["n_packets"], c["wire"], c["hr"], c["pr"], c["keys"], c["roc"].view(np.uint32), c["seq_base"],
                       c["next_seq"], dst0, c["stride"], tag_len)
    _same(got, want, "protect")
    for i, st in c["expect"].items():
        assert got["out_status"][i] == st, (i, int(got["out_status"][i]), st)
    k = c["n_packets"]
    assert not got["out_size"][k:].any() and not got["out_status"][k:].any() and (got["out_size"][got["out_status"] != ref.PROTECTED] == 0).all()
    without = api.plan_srtp_protect(c["route"], c["off"], c["size"], c["status"], c["wire"], c["ctx"], c["roc"], c["seq_base"], dst0, c["stride"], tag_len, c["hr"], c["pr"],
                                    n_packets=k)
    assert without["next_roc"] is None and np.array_equal(without["dst"], got["dst"])


@pytest.mark.parametrize("tag_len", [10, 4])
def test_protect_then_unprotect_gives_the_plaintext_back(tag_len):
    c = cases.protect_list(tag_len)
    dst0 = np.zeros(c["dst_capacity"], np.uint8)
    p = api.plan_srtp_protect(c["route"], c["off"], c["size"], c["status"], c["wire"], c["ctx"], c["roc"], c["seq_base"], dst0, c["stride"], tag_len, c["hr"], c["pr"],
                              n_packets=c["n_packets"])
    ssrc_key = np.array([0x11, 0x80000001], np.uint32).view(np.int32)                 # ascending: route 1, then route 0
    state = np.array([cases.state_block(0, 6), cases.state_block(0, 0xFFFFFFFF)], np.uint32).view(np.int32)
    u = api.plan_srtp_unprotect(p["dst"], p["out_offset"], p["out_size"], ssrc_key, c["ctx"][::-1], state, tag_len)
    done = p["out_status"] == ref.PROTECTED
    assert done.sum() > 250 and np.array_equal(u["sizes"][done], p["out_size"][done] - tag_len) and (u["status"][done] == ref.OK).all()
    assert np.isin(u["status"][~done], (ref.SHORT, ref.UN_RANGE)).all()      # out_size 0; the slots past the destination lie outside the ring as well
    for i in np.flatnonzero(done):
        a = int(c["off"][i]) + c["hr"] - c["pr"] - 12
        o, n = int(p["out_offset"][i]), int(u["sizes"][i])
        assert np.array_equal(u["ring"][o:o + n], c["wire"][a:a + n]), i


@pytest.mark.parametrize("cut", [1, 41, 89])
def test_split_calls_carry_the_state(cut):
    """one unprotect call over a list equals two calls over its halves with the state carried over (srtp_cases.split_lists says on which lists the stateless
    estimate and the sequential one agree)"""
    c, _ = cases.split_lists(10)
    whole = _plan_unprotect(c)
    first = _plan_unprotect(dict(c, offs=c["offs"][:cut], sizes=c["sizes"][:cut]))
    second = _plan_unprotect(dict(c, ring=first["ring"], offs=c["offs"][cut:], sizes=c["sizes"][cut:], state=first["state"]))
    assert np.array_equal(whole["state"], second["state"]) and np.array_equal(whole["ring"], second["ring"]) and (whole["status"] == ref.OK).all()
    for k in ("status", "index", "sizes"):
        assert np.array_equal(whole[k], np.concatenate([first[k], second[k]])), k
    again = _plan_unprotect(dict(c, ring=whole["ring"], state=whole["state"]))            # the same list once more: every item is a replay now
    assert set(again["status"].tolist()) <= {ref.REPLAYED, ref.REPLAY_OLD, ref.AUTH} and np.array_equal(again["state"], whole["state"])


def test_checks_1_and_2_are_the_parse_s():
    """lc3_srtp_shim.h restates the parse's header checks and its SSRC search (it needs the table's place and the header's length, the parse gives a stream):
    on the malformed datagrams of srtp_cases.tampered, with the tag taken off the sizes, lc3plus_plan_rtp_parse refuses the same items for the same reasons"""
    same = {ref.SHORT: api.RTP_SHORT, ref.VERSION: api.RTP_VERSION, ref.RTCP: api.RTP_RTCP, ref.HEADER: api.RTP_HEADER, ref.UNKNOWN_SSRC: api.RTP_UNKNOWN_SSRC}
    for tag_len in (10, 4):
        c = cases.tampered(tag_len)
        got = _plan_unprotect(c)["status"]
        ok = got != ref.UN_RANGE                                      # (a size less its tag may fit where the whole did not)
        parse = api.plan_rtp_parse(len(c["ssrc_key"]), c["ring"], c["offs"][ok], c["sizes"][ok] - tag_len, c["ssrc_key"], np.arange(len(c["ssrc_key"])))["status"]
        seen = set()
        for s, p in zip(got[ok], parse):
            assert (same[s] == p) if s in same else (p not in same.values() and p != api.RTP_RANGE), (int(s), int(p))
            seen.add(int(s))
        assert set(same) <= seen
    big = np.zeros((1 << 20) + 64, np.uint8)                            # a datagram past 2^20 bytes is outside the rule: RANGE, whatever it holds
    big[0], big[1] = 0x80, 96
    u = api.plan_srtp_unprotect(big, [0, 0], [(1 << 20) + 1, 1 << 20], [0], cases.keys_for(0).ctx.view(np.int32).reshape(1, -1), np.zeros((1, 8), np.int32), 10)
    assert u["status"].tolist() == [ref.UN_RANGE, ref.AUTH] and np.array_equal(u["ring"], big)


# ---- the refusals ----
def test_refusals_in_the_header_s_order():
    """against a zero-filled block in place of a batch: a refusal returns before anything of the batch or the device is touched.  Every array is the same 64
    zero bytes (the destination another block), which no refused call may write"""
    L = audio_codec_amd.load_library()
    fake, a, d = (C.c_uint8 * 4096)(), (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    A, D, B = C.addressof(a), C.addressof(d), C.addressof(fake)
    names = ("max_packets", "n_packets", "pkt_route", "pkt_offset", "pkt_size", "pkt_status", "wire", "wire_capacity", "header_room", "payload_room", "n_routes", "ctx",
             "roc", "seq_base", "next_seq", "dst", "dst_capacity", "dst_stride", "tag_len", "out_offset", "out_size", "out_status", "next_roc")
    good = dict(max_packets=1, wire_capacity=64, header_room=12, payload_room=0, n_routes=1, dst=D, dst_capacity=64, dst_stride=32, tag_len=10)

    def protect(fn, batch, **kw):
        v = dict({k: A for k in names}, **good)
        v.update(kw)
        args = [v[k] for k in names]
        return fn(*(([batch] if batch != "plan" else []) + args + ([None, 1] if batch != "plan" else [])))
    for fn in (L.lc3plus_enc_batch_srtp_protect, L.lc3plus_dec_batch_srtp_protect):
        assert protect(fn, None) == LC3_NULL_ERROR
        for k in ("n_packets", "pkt_route", "pkt_offset", "pkt_size", "pkt_status", "wire", "ctx", "roc", "seq_base", "dst", "out_offset", "out_size", "out_status", "next_seq"):
            assert protect(fn, B, **{k: None}) == LC3_NULL_ERROR, k
            assert protect(fn, B, max_packets=0, tag_len=7, **{k: None}) == LC3_NULL_ERROR, k          # NULL first
        assert protect(fn, B, next_seq=None, next_roc=None) == LC3_ERROR                               # passes every check: the block is no batch
        for bad in (dict(max_packets=0), dict(max_packets=-1), dict(max_packets=1 << 29), dict(wire_capacity=-1), dict(payload_room=-1), dict(header_room=11),
                    dict(header_room=14, payload_room=3), dict(n_routes=0), dict(dst_capacity=-1), dict(dst_stride=0), dict(dst_stride=(1 << 30) + 1), dict(tag_len=0),
                    dict(tag_len=8), dict(tag_len=20), dict(dst=A + 32, dst_capacity=16), dict(dst=A - 8, dst_capacity=9)):
            assert protect(fn, B, **bad) == LC3_ERROR, bad
    assert protect(L.lc3plus_plan_srtp_protect, "plan", pkt_route=None) == LC3_NULL_ERROR and protect(L.lc3plus_plan_srtp_protect, "plan", tag_len=5) == LC3_ERROR
    assert protect(L.lc3plus_plan_srtp_protect, "plan", dst=A) == LC3_ERROR
    unames = ("n_items", "ring", "ring_capacity", "dg_offsets", "dg_sizes", "n_ssrc", "ssrc_key", "ctx", "state_in", "state_out", "tag_len", "sizes_out", "status", "index",
              "stats")
    W = api.srtp_workspace_bytes(1, 1)
    ugood = dict(n_items=1, ring_capacity=64, n_ssrc=1, tag_len=10)

    def unprotect(batch, workspace=D, workspace_bytes=W, **kw):
        v = dict({k: A for k in unames}, **ugood)
        v.update(kw)
        return L.lc3plus_dec_batch_srtp_unprotect(batch, *[v[k] for k in unames], workspace, workspace_bytes, None, 1)
    assert unprotect(None) == LC3_NULL_ERROR and unprotect(B, workspace=None) == LC3_NULL_ERROR
    for k in ("ring", "dg_offsets", "dg_sizes", "ssrc_key", "ctx", "state_in", "state_out", "sizes_out"):
        assert unprotect(B, **{k: None}) == LC3_NULL_ERROR, k
        assert unprotect(B, n_items=0, **{k: None}) == LC3_NULL_ERROR, k
    for bad in (dict(n_items=0), dict(n_items=-1), dict(n_items=1 << 29), dict(ring_capacity=-1), dict(n_ssrc=0), dict(n_ssrc=-4), dict(tag_len=0), dict(tag_len=12),
                dict(workspace_bytes=W - 1), dict(workspace_bytes=0)):
        assert unprotect(B, **bad) == LC3_ERROR, bad
    assert unprotect(B, status=None, index=None, stats=None) == LC3_ERROR                              # passes every check: the block is no batch
    assert not any(fake) and not any(a) and not any(d)
    assert L.lc3plus_srtp_make_context(None, A, A) == L.lc3plus_srtp_make_context(A, None, A) == L.lc3plus_srtp_make_context(A, A, None) == LC3_NULL_ERROR


# ---- the host code under the sanitizers, in a program of its own ----
@pytest.fixture(scope="module")
def driver():
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    subprocess.check_call(["make", "-s", "-C", CSRC, "srtp_driver"])
    return os.path.join(ROOT, "audio_codec_amd", "_stub", "srtp_plan_driver")


def _run(driver, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([driver] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, universal_newlines=True)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_driver_refusals_under_the_sanitizers(driver):
    assert _run(driver, "refuse").strip() == "refusals ok"


@pytest.mark.parametrize("seed,n,tag", [(1, 1, 10), (2, 64, 4), (3, 700, 10)])
def test_driver_roundtrip_under_the_sanitizers(driver, seed, n, tag):
    """every buffer exactly as large as its capacity says; the program itself checks that the plaintext comes back and that a damaged tag stops its item alone.
    The context it prints is the restatement's on the keys it drew"""
    out = dict(line.split(" ", 1) for line in _run(driver, "roundtrip", seed, n, tag).splitlines() if " " in line)
    x = seed
    draws = []
    for _ in range(30):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        draws.append((x >> 8) & 255)
    want = ref.make_context(bytes(draws[:16]), bytes(draws[16:30]))
    assert np.array_equal(np.array(out["ctx"].split(), np.uint64).astype(np.uint32), want)
    assert out["stats"].split()[0] == str(n) and "damaged ok" in _run(driver, "roundtrip", seed, n, tag)
