"""The wire sample types of the PCM format word (include/lc3plus_batch.h: LC3PLUS_PCM_S16_BE, _S24_3LE, _S24_3BE, _ULAW, _ALAW) on the host alone: exports
and constants, the format check, the element size, the conversion rule (lc3plus_pcm_to_native / lc3plus_pcm_from_native) against a numpy restatement of
the rule written here, the fixture tests/golden/g711_tables.npz and python's audioop, the slices a sharded call hands its shards for 1- and 3-byte elements
(tools/stub_shim.c), and the host functions under AddressSanitizer + UndefinedBehaviorSanitizer.  Every comparison is equality."""
import ctypes as C
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import audio_codec_amd
from audio_codec_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_codec_amd", "csrc")
F32, IL, CM = api.PCM_FLOAT32, api.PCM_INTERLEAVED, api.PCM_CHANNEL_MAJOR
WIRE = {"LC3PLUS_PCM_S16_BE": 0x81, "LC3PLUS_PCM_S24_3LE": 0x82, "LC3PLUS_PCM_S24_3BE": 0x83, "LC3PLUS_PCM_ULAW": 0x84, "LC3PLUS_PCM_ALAW": 0x85}
S16BE, S24LE, S24BE, ULAW, ALAW = 0x81, 0x82, 0x83, 0x84, 0x85
ELEM = {16: 2, 24: 4, 32: 4, F32: 4, S16BE: 2, S24LE: 3, S24BE: 3, ULAW: 1, ALAW: 1}
LC3_OK, LC3_ERROR, LC3_NULL_ERROR = 0, 1, 3
CRC = {"ulaw_expand": 0x0C847A9F, "alaw_expand": 0x9D764657, "ulaw_compress": 0x6399D432, "alaw_compress": 0x9133796E}


# ---- the rule, restated (section 2 of the feature's description; nothing of the library is called) ----
def expand(c, alaw):
    c = np.asarray(c, np.int64)
    k = (c ^ 0x55) if alaw else (~c & 0xFF)
    e, q = (k >> 4) & 7, k & 15
    if alaw:
        m = np.where(e == 0, (2 * q + 1) << 3, ((2 * q + 33) << np.maximum(e - 1, 0)) << 3)
        return np.where(k & 0x80, m, -m).astype(np.int16)
    m = ((2 * q + 33) << (e + 2)) - 132
    return np.where(c & 0x80, m, -m).astype(np.int16)


def _log2(a):
    r = np.zeros(a.shape, np.int64)
    for b in range(1, 16):
        r[a >= (1 << b)] = b
    return r


def compress(x, alaw):
    x = np.asarray(x, np.int64)
    s = x < 0
    y = np.where(s, ~x, x)
    if alaw:
        m = y >> 4
        e = _log2(np.maximum(m, 1)) - 3
        c7 = np.where(m <= 15, m, (np.maximum(e, 1) << 4) | ((m >> np.maximum(e - 1, 0)) & 15))
        return ((c7 | np.where(s, 0, 0x80)) ^ 0x55).astype(np.uint8)
    a = np.minimum((y >> 2) + 33, 8191)
    e = _log2(a) - 5
    q = (a >> (e + 1)) & 15
    return (np.where(s, 0, 0x80) | ((7 - e) << 4) | (15 - q)).astype(np.uint8)


def pack24(v, big):
    """int32 -> uint8 [..., 3]: saturated to 24 bits, then the low three bytes"""
    u = np.clip(np.asarray(v, np.int64), -8388608, 8388607) & 0xFFFFFF
    b = np.stack([u & 0xFF, (u >> 8) & 0xFF, u >> 16], axis=-1).astype(np.uint8)
    return b[..., ::-1].copy() if big else b


def unpack24(b, big):
    b = np.asarray(b, np.int64)
    if big:
        b = b[..., ::-1]
    u = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return np.where(u >= 1 << 23, u - (1 << 24), u).astype(np.int32)


CODES, SAMPLES = np.arange(256), np.arange(-32768, 32768)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "g711_tables.npz"))


# ---- 1. exports and constants ----
def test_symbols_are_exported_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", api.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in ("lc3plus_pcm_elem_bytes", "lc3plus_pcm_to_native", "lc3plus_pcm_from_native"):
        assert s in names and s in api.EXPORTS, s


def test_constants_match_the_header_and_the_kernels():
    for path, prefix in ((os.path.join(ROOT, "include", "lc3plus_batch.h"), "LC3PLUS_PCM_"), (os.path.join(CSRC, "lc3_plan.h"), "LC3D_PCM_")):
        text = open(path).read()
        for name, value in WIRE.items():
            m = re.search(r"#define\s+%s\s+(\S+)" % name.replace("LC3PLUS_PCM_", prefix), text)
            assert m and int(m.group(1), 0) == value, (path, name)
            assert getattr(api, name.replace("LC3PLUS_", "")) == value
    assert api.PCM_NAMES == {"s16be": S16BE, "s24_3le": S24LE, "s24_3be": S24BE, "ulaw": ULAW, "alaw": ALAW}


def test_format_check_accepts_the_wire_types_with_each_layout():
    lib = audio_codec_amd.load_library()
    for name, ty in api.PCM_NAMES.items():
        for lay in (0, IL, CM):
            assert lib.lc3plus_pcm_format_check(ty | lay) == 0, (ty, lay)
            assert api.pcm_format(ty, lay) == ty | lay and api.pcm_format(name, lay) == ty | lay


@pytest.mark.parametrize("word", [0, 8, 17, 16 | IL | CM, F32 | IL | CM, 16 | 0x400, F32 | 0x1000, 16 | F32, 24 | 32, IL, CM, -1, 16 | (1 << 30),   # test_pcm_format_cpu.py's
                                  56, 0x86, 0x7F, 0xFF, ULAW | IL | CM, S24LE | 0x400, ALAW | 0x1000, S16BE | (1 << 30), ULAW | 16, 1, 3])
def test_format_check_still_rejects(word):
    lib = audio_codec_amd.load_library()
    assert lib.lc3plus_pcm_format_check(word) != 0
    assert lib.lc3plus_pcm_elem_bytes(word) == -1


def test_elem_bytes_of_all_nine_types():
    lib = audio_codec_amd.load_library()
    assert len(ELEM) == 9
    for ty, n in ELEM.items():
        for lay in (0, IL, CM):
            assert lib.lc3plus_pcm_elem_bytes(ty | lay) == n, (ty, lay)
        assert np.dtype(api.pcm_dtype(ty)).itemsize * int(np.prod(api.pcm_shape(ty, 1, 1, 1, 1))) == n


def test_python_dtypes_and_shapes():
    assert api.pcm_dtype(ULAW) == np.uint8 and api.pcm_dtype(ALAW | IL) == np.uint8
    assert np.dtype(api.pcm_dtype(S16BE)) == np.dtype(">i2")
    assert api.pcm_dtype(S24LE) == np.uint8 and api.pcm_dtype(S24BE) == np.uint8
    assert api.pcm_shape(S24LE, 2, 3, 2, 5) == (2, 3, 2, 5, 3) and api.pcm_shape(S24BE | IL, 2, 3, 2, 5) == (2, 15, 2, 3)
    assert api.pcm_shape(S24LE | CM, 2, 3, 2, 5) == (2, 2, 15, 3) and api.pcm_shape(ULAW, 2, 3, 2, 5) == (2, 3, 2, 5)
    assert api.pcm_offset(ULAW | IL, 2, 4, 5, 1, 2, 1, 3) == api.pcm_offset(16 | IL, 2, 4, 5, 1, 2, 1, 3)          # element indices: unchanged by the type


# ---- 2. G.711, exhaustively ----
def test_fixture_is_the_rule_and_has_the_published_checksums(golden):
    for name, alaw in (("ulaw", False), ("alaw", True)):
        assert np.array_equal(golden[name + "_expand"], expand(CODES, alaw))
        assert np.array_equal(golden[name + "_compress"], compress(SAMPLES, alaw))
        assert golden[name + "_expand"].dtype == np.int16 and golden[name + "_compress"].dtype == np.uint8
        assert zlib.crc32(golden[name + "_expand"].astype("<i2").tobytes()) == CRC[name + "_expand"]
        assert zlib.crc32(golden[name + "_compress"].tobytes()) == CRC[name + "_compress"]
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_g711_tables
    finally:
        sys.path.pop(0)
    for name, t in make_g711_tables.tables().items():
        assert np.array_equal(t, golden[name]), name


@pytest.mark.parametrize("ty,name", [(ULAW, "ulaw"), (ALAW, "alaw")])
def test_g711_all_codes_and_all_samples(golden, ty, name):
    alaw = ty == ALAW
    got = api.pcm_to_native(ty, CODES.astype(np.uint8))
    assert got.dtype == np.int16
    assert np.array_equal(got, expand(CODES, alaw)) and np.array_equal(got, golden[name + "_expand"])
    got = api.pcm_from_native(ty | IL, SAMPLES.astype(np.int16))                  # a layout bit is ignored
    assert got.dtype == np.uint8
    assert np.array_equal(got, compress(SAMPLES, alaw)) and np.array_equal(got, golden[name + "_compress"])


def test_g711_round_trips(golden):
    a = golden["alaw_compress"][golden["alaw_expand"].astype(np.int64) + 32768]
    assert np.array_equal(a, CODES)
    u = golden["ulaw_compress"][golden["ulaw_expand"].astype(np.int64) + 32768]
    assert (u != CODES).nonzero()[0].tolist() == [0x7F] and u[0x7F] == 0xFF and golden["ulaw_expand"][0x7F] == 0


def test_g711_against_audioop(golden):
    """audioop negates in two's complement where the rule takes the one's complement: its mu-law compression is the rule's for x >= 0 and for x < 0 the
    rule is lin2ulaw(~x) ^ 0x80.  Where audioop does not exist (python 3.13), the fixture - checked above by its checksums - stands alone."""
    try:
        import audioop
    except ImportError:
        return
    codes = bytes(range(256))
    assert np.array_equal(np.frombuffer(audioop.ulaw2lin(codes, 2), "<i2"), golden["ulaw_expand"])
    assert np.array_equal(np.frombuffer(audioop.alaw2lin(codes, 2), "<i2"), golden["alaw_expand"])
    lin = SAMPLES.astype("<i2")
    assert np.array_equal(np.frombuffer(audioop.lin2alaw(lin.tobytes(), 2), np.uint8), golden["alaw_compress"])
    pos = np.frombuffer(audioop.lin2ulaw(np.where(SAMPLES < 0, ~SAMPLES, SAMPLES).astype("<i2").tobytes(), 2), np.uint8)
    assert np.array_equal(np.where(SAMPLES < 0, pos ^ 0x80, pos), golden["ulaw_compress"])
    plain = np.frombuffer(audioop.lin2ulaw(lin.tobytes(), 2), np.uint8)
    assert int((plain != golden["ulaw_compress"]).sum()) == 508 and (SAMPLES[plain != golden["ulaw_compress"]] < 0).all()


# ---- 3. packed 24 bits and big-endian 16 ----
def _values24():
    rng = np.random.default_rng(24)
    edge = [-2 ** 31, 2 ** 31 - 1, 2 ** 23, -2 ** 23, 2 ** 23 - 1, -2 ** 23 - 1, 0, -1, 1, 255, 256, -256, 65535, 65536, -65536, 0x123456, -0x123456]
    return np.concatenate([np.array(edge, np.int64), rng.integers(-2 ** 31, 2 ** 31, 4000), rng.integers(-2 ** 23, 2 ** 23, 4000)]).astype(np.int32)


@pytest.mark.parametrize("ty", [S24LE, S24BE])
def test_from_native_packed_24_saturates(ty):
    v = _values24()
    got = api.pcm_from_native(ty, v)
    assert got.dtype == np.uint8 and got.shape == v.shape + (3,)
    assert np.array_equal(got, pack24(v, ty == S24BE))
    first = {int(x): got[i].tolist() for i, x in enumerate(v[:5])}
    lo, hi = [0x00, 0x00, 0x80], [0xFF, 0xFF, 0x7F]
    if ty == S24BE:
        lo, hi = lo[::-1], hi[::-1]
    assert first[-2 ** 31] == lo and first[-2 ** 23] == lo and first[2 ** 31 - 1] == hi and first[2 ** 23] == hi and first[2 ** 23 - 1] == hi


@pytest.mark.parametrize("ty", [S24LE, S24BE])
def test_packed_24_round_trip(ty):
    v = _values24()
    back = api.pcm_to_native(ty, api.pcm_from_native(ty, v))
    assert back.dtype == np.int32 and np.array_equal(back, np.clip(v, -8388608, 8388607))
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 256, (5000, 3)).astype(np.uint8)                        # every byte pattern is a sample
    nat = api.pcm_to_native(ty, raw)
    assert np.array_equal(nat, unpack24(raw, ty == S24BE))
    assert np.array_equal(api.pcm_from_native(ty, nat), raw)
    odd = np.concatenate([np.zeros(1, np.uint8), raw.ravel()])[1:].reshape(-1, 3)  # a wire pointer one byte off every alignment
    assert odd.ctypes.data % 2 == 1
    assert np.array_equal(api.pcm_to_native(ty, odd), nat)


def test_s16_be_round_trip():
    x = SAMPLES.astype(np.int16)
    be = api.pcm_from_native(S16BE, x)
    assert be.dtype == np.dtype(">i2") and np.array_equal(be.view(np.uint8), x.astype(">i2").view(np.uint8))
    assert np.array_equal(be.view(np.uint8).reshape(-1, 2)[:, ::-1].copy().view("<i2").ravel(), x)     # the bytes swapped
    back = api.pcm_to_native(S16BE, be)
    assert back.dtype == np.int16 and np.array_equal(back, x)


def test_host_functions_refuse_what_they_must():
    lib = audio_codec_amd.load_library()
    src, dst = np.zeros(16, np.int32), np.zeros(64, np.uint8)
    for f in (lib.lc3plus_pcm_to_native, lib.lc3plus_pcm_from_native):
        for ty in (16, 24, 32, F32, 0, 0x86, ULAW | 0x400, S24LE | IL | 0x1000):
            assert f(ty, src.ctypes.data, 4, dst.ctypes.data) == LC3_ERROR, ty
        assert f(ULAW, None, 4, dst.ctypes.data) == LC3_NULL_ERROR and f(ULAW, src.ctypes.data, 4, None) == LC3_NULL_ERROR
        assert f(ULAW, src.ctypes.data, -1, dst.ctypes.data) == LC3_ERROR
        assert f(ALAW | CM, src.ctypes.data, 0, dst.ctypes.data) == LC3_OK
    assert not dst.any()
    with pytest.raises(api.LC3Error):
        api.pcm_to_native(16, np.zeros(4, np.int16))
    with pytest.raises(ValueError):
        api.pcm_to_native(S24LE, np.zeros(4, np.uint8))


# ---- 4. the slices of a sharded host call in a 1-byte and a 3-byte format (tools/stub_shim.c) ----
class Rec(C.Structure):                                              # lc3stub_rec
    _fields_ = [("ctx", C.c_int32), ("kind", C.c_int32), ("dec", C.c_int32), ("n_frames", C.c_int32), ("stride", C.c_int32), ("fmt", C.c_int32),
                ("on_device", C.c_int32), ("sync", C.c_int32), ("p", C.c_uint64 * 4), ("a", C.c_int64 * 3), ("b", C.c_int64 * 3), ("bytes", C.c_uint64),
                ("hip_stream", C.c_uint64)]


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-s", "-C", CSRC, "stub"])
    L = C.CDLL(os.path.join(ROOT, "audio_codec_amd", "_stub", "liblc3plus_stub.so"))
    api._declare_sharded(L)
    L.lc3plus_pcm_offset.argtypes = [C.c_int] * 8
    L.lc3plus_pcm_offset.restype = C.c_int64
    assert L.lc3stub_rec_sizeof() == C.sizeof(Rec)
    return L


def _log(L):
    n = L.lc3stub_log(None, 0)
    buf = (Rec * max(n, 1))()
    assert L.lc3stub_log(buf, n) == n
    return sorted([buf[i] for i in range(n)], key=lambda r: r.ctx)


@pytest.mark.parametrize("S,K", [(33, 2), (7, 3)])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("ty", [ULAW, S24LE, S24BE, S16BE])
def test_sharded_host_slices_in_bytes(stub, S, K, ch, ty):
    """shard i gets the pointer base + elem_bytes x (element index of its first stream), and the next shard's pointer lies exactly its block's bytes further"""
    L, N, T = stub, 480, 3
    eb = ELEM[ty]
    cfg = np.ascontiguousarray([64000 * ch] * S, np.int32)
    devs = np.zeros(K, np.int32)
    for lay in (0, IL, CM):
        fmt = ty | lay
        pcm = np.zeros(api.pcm_shape(fmt, S, T, ch, N), api.pcm_dtype(fmt))
        assert pcm.nbytes == S * T * ch * N * eb
        base = pcm.ctypes.data
        for kind in ("enc", "dec"):
            L.lc3stub_reset()
            h = C.c_void_p()
            cfg_k = cfg if kind == "enc" else np.ascontiguousarray([80 * ch] * S, np.int32)
            assert getattr(L, "lc3plus_%s_sharded_create" % kind)(C.byref(h), S, 48000, ch, 10.0, 0, cfg_k.ctypes.data, devs.ctypes.data, K) == 0
            buf, st = np.zeros((S, T, 80 * ch), np.uint8), np.zeros((S, T), np.uint8)
            L.lc3stub_reset()
            if kind == "enc":
                assert L.lc3plus_enc_sharded_encode(h, base, fmt, None, None, T, buf.ctypes.data, 80 * ch, None) == 0
            else:
                assert L.lc3plus_dec_sharded_decode(h, buf.ctypes.data, 80 * ch, None, None, T, base, fmt, st.ctypes.data) == 0
            log = [r for r in _log(L) if r.kind in (1, 2)]
            assert len(log) == K
            ptrs = [r.p[0] if kind == "enc" else r.p[1] for r in log]
            at = base
            for i in range(K):
                first, count = api.shard_block(S, K, i, L)
                assert ptrs[i] == base + eb * L.lc3plus_pcm_offset(fmt, ch, T, N, first, 0, 0, 0), (kind, lay, i)
                assert ptrs[i] == at, (kind, lay, i)
                assert log[i].fmt == fmt and log[i].n_frames == T
                at += count * T * ch * N * eb                        # the bytes of the block
            assert at == base + pcm.nbytes
            assert getattr(L, "lc3plus_%s_sharded_destroy" % kind)(h) == 0


# ---- 5. the host functions under the sanitizers ----
def _lib(name):
    p = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


def test_host_functions_are_clean_under_asan_and_ubsan():
    """the conversion tests of this file once more, in a child process against the sanitized build of lc3_host.c (`make asan`), as
    tests/test_host_sanitizers.py runs the host API: buffers of exactly n elements on both sides, so one byte too many is an error"""
    asan, ubsan = _lib("libasan.so"), _lib("libubsan.so")
    assert asan and ubsan, "gcc sanitizer runtimes not installed"
    subprocess.check_call(["make", "-s", "-C", CSRC])
    subprocess.check_call(["make", "-s", "-C", CSRC, "asan"])
    lib = os.path.join(ROOT, "audio_codec_amd", "_asan", "liblc3plus_hip.so")
    env = dict(os.environ, LD_PRELOAD=asan + ":" + ubsan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               LC3PLUS_HIP_LIB=lib)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider", "-k",
                          "g711_all or packed_24 or s16_be or refuse or elem_bytes or still_rejects"],
                         capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert out.returncode == 0 and " passed" in out.stdout and "runtime error" not in out.stderr, (out.stdout[-1500:], out.stderr[-3000:])
