"""Sharded batches (lc3plus_{enc,dec}_sharded_*, include/lc3plus_batch.h) without a GPU: the split, the create refusals of the product library, and the
host logic - which pointer, which slice of which array, which result, which thread - against a build of lc3_host.c whose HIP side is tools/stub_shim.c
(`make -C audio_codec_amd/csrc stub`): every call a shard makes is logged there instead of run.  The worker threads run under ThreadSanitizer in
tools/sharded_stub_driver.c.  Every comparison is equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from audio_codec_amd import api, sharding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_codec_amd", "csrc")
STUB_DIR = os.path.join(ROOT, "audio_codec_amd", "_stub")
LC3_OK, LC3_ERROR, LC3_NULL_ERROR, LC3_SAMPLERATE_ERROR, LC3_CHANNELS_ERROR, LC3_BITRATE_ERROR, LC3_NUMBYTES_ERROR, LC3_FRAMEMS_ERROR = 0, 1, 3, 4, 5, 6, 7, 9
LC3_BW_WARNING = 18
ENCODE, DECODE, GET_STATE, SET_STATE = 1, 2, 3, 4                    # record kinds of tools/stub_shim.c
STATE_BYTES = 32                                                     # per channel-stream in the stub

NEW = ["lc3plus_shard_block"] + ["lc3plus_enc_sharded_" + n for n in (
    "create", "destroy", "shards", "shard", "device", "owner", "input_samples", "num_bytes", "stride", "set_bitrate", "set_bandwidth", "bandwidth", "encode",
    "encode_device", "state_size", "get_state", "set_state", "last_kernel_ms")] + ["lc3plus_dec_sharded_" + n for n in (
    "create", "destroy", "shards", "shard", "device", "owner", "output_samples", "delay", "num_bytes", "set_num_bytes", "decode", "decode_device", "state_size",
    "get_state", "set_state", "last_kernel_ms")]


class Rec(C.Structure):                                              # lc3stub_rec
    _fields_ = [("ctx", C.c_int32), ("kind", C.c_int32), ("dec", C.c_int32), ("n_frames", C.c_int32), ("stride", C.c_int32), ("fmt", C.c_int32),
                ("on_device", C.c_int32), ("sync", C.c_int32), ("p", C.c_uint64 * 4), ("a", C.c_int64 * 3), ("b", C.c_int64 * 3), ("bytes", C.c_uint64),
                ("hip_stream", C.c_uint64)]


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-s", "-C", CSRC, "stub"])
    L = C.CDLL(os.path.join(STUB_DIR, "liblc3plus_stub.so"))
    api._declare_sharded(L)
    L.lc3plus_pcm_offset.argtypes = [C.c_int] * 8
    L.lc3plus_pcm_offset.restype = C.c_int64
    assert L.lc3stub_rec_sizeof() == C.sizeof(Rec)
    return L


def _log(L, kinds=(ENCODE, DECODE, GET_STATE, SET_STATE)):
    n = L.lc3stub_log(None, 0)
    buf = (Rec * max(n, 1))()
    assert L.lc3stub_log(buf, n) == n
    return [buf[i] for i in range(n) if buf[i].kind in kinds]


def _i32(x):
    return np.ascontiguousarray(x, dtype=np.int32)


def _create(L, kind, S, fs, ch, ms, hr, cfg, devices):
    h = C.c_void_p(0xDEAD)
    cfg = _i32(cfg) if cfg is not None else None
    dev = _i32(devices) if devices is not None else None
    rc = getattr(L, "lc3plus_%s_sharded_create" % kind)(C.byref(h), S, fs, ch, ms, hr, cfg.ctypes.data if cfg is not None else None,
                                                       dev.ctypes.data if dev is not None and dev.size else (None if dev is None else _i32([0]).ctypes.data),
                                                       len(devices) if devices is not None else 2)
    return rc, h


# ---- 1. the symbols ----
def test_new_symbols_are_exported_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", api.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in NEW:
        assert s in names, s
        assert s in api.EXPORTS, s


# ---- 2. the split ----
SIZES = list(range(71)) + [4096, 4097, 16384]


def test_shard_block_is_stream_block():
    for n in SIZES:
        for k in range(1, 10):
            at = 0
            for i in range(k):
                first, count = api.shard_block(n, k, i)
                assert (first, first + count) == sharding.stream_block(i, k, n), (n, k, i)
                assert first == at and count >= 0                  # the blocks tile [0, n) in order
                at += count
            assert at == n
            sizes = [api.shard_block(n, k, i)[1] for i in range(k)]
            assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)


def test_shard_block_bad_arguments():
    L = api.load_library()
    a, b = C.c_int(0), C.c_int(0)
    for n, k, i in ((-1, 2, 0), (4, 0, 0), (4, -1, 0), (4, 2, 2), (4, 2, -1)):
        assert L.lc3plus_shard_block(n, k, i, C.byref(a), C.byref(b)) == LC3_ERROR, (n, k, i)
    assert L.lc3plus_shard_block(4, 2, 0, None, C.byref(b)) == LC3_NULL_ERROR
    assert L.lc3plus_shard_block(4, 2, 0, C.byref(a), None) == LC3_NULL_ERROR


def test_owner_agrees_with_owner_of(stub):
    for n in [1, 2, 3, 7, 8, 9, 10, 33, 64, 70, 4097]:
        for k in range(1, 10):
            if k > n:
                continue
            for kind, cfg in (("enc", [64000] * n), ("dec", [80] * n)):
                rc, h = _create(stub, kind, n, 48000, 1, 10.0, 0, cfg, [0] * k)
                assert rc == 0 and h.value
                f = lambda x: getattr(stub, "lc3plus_%s_sharded_%s" % (kind, x))
                assert f("shards")(h) == k
                sh, lo = C.c_int(-1), C.c_int(-1)
                for s in (range(n) if n <= 70 else (0, 1, n // k - 1, min(n // k, n - 1), min(n // k + 1, n - 1), n // 2, n - 2, n - 1)):
                    assert f("owner")(h, s, C.byref(sh), C.byref(lo)) == 0
                    assert sh.value == sharding.owner_of(s, k, n), (n, k, s)
                    first, count = api.shard_block(n, k, sh.value, stub)
                    assert 0 <= lo.value < count and first + lo.value == s
                assert f("owner")(h, n, C.byref(sh), C.byref(lo)) == LC3_ERROR and f("owner")(h, -1, C.byref(sh), C.byref(lo)) == LC3_ERROR
                assert f("device")(h, k) == -1 and f("device")(h, 0) == 0 and not f("shard")(h, k) and f("shard")(h, k - 1)
                assert f("destroy")(h) == 0


# ---- 3. create refusals of the product library: none needs a device ----
def test_create_refusals_need_no_device():
    L = api.load_library()
    ok = dict(S=4, fs=48000, ch=1, ms=10.0, hr=0)
    for kind, good, bad, bad_code in (("enc", 64000, 1000, LC3_BITRATE_ERROR), ("dec", 80, 5, LC3_NUMBYTES_ERROR)):
        def create(devices, cfg=None, **kw):
            a = dict(ok, **kw)
            rc, h = _create(L, kind, a["S"], a["fs"], a["ch"], a["ms"], a["hr"], [good] * max(a["S"], 1) if cfg is None else cfg, devices)
            assert h.value is None, "the handle of a refused create is NULL"
            return rc
        assert create(None) == LC3_NULL_ERROR
        assert create([]) == LC3_ERROR                               # n_devices = 0
        assert create([0, -1]) == LC3_ERROR
        assert create([0, 0, 0, 0, 0]) == LC3_ERROR                  # more devices than streams
        assert create([0, 0], S=0) == LC3_ERROR
        assert create([0, 0], fs=47000) == LC3_SAMPLERATE_ERROR
        assert create([0, 0], ch=3) == LC3_CHANNELS_ERROR
        assert create([0, 0], ms=7.5) == LC3_FRAMEMS_ERROR
        assert create([0, 0], fs=16000, hr=1) == LC3_SAMPLERATE_ERROR
        assert create([0, 0], cfg=[good, good, good, bad]) == bad_code       # in the last shard's block
        # the unsharded create gives the same codes
        one = getattr(L, "lc3plus_%s_batch_create" % kind)
        h = C.c_void_p()
        cfg = (C.c_int * 4)(good, good, good, bad)
        assert one(C.byref(h), 4, 48000, 1, 10.0, 0, cfg, 0) == bad_code and one(C.byref(h), 4, 48000, 3, 10.0, 0, cfg, 0) == LC3_CHANNELS_ERROR
    h = C.c_void_p()
    assert L.lc3plus_enc_sharded_create(C.byref(h), 4, 48000, 1, 10.0, 0, None, _i32([0, 0]).ctypes.data, 2) == LC3_NULL_ERROR
    assert L.lc3plus_enc_sharded_create(None, 4, 48000, 1, 10.0, 0, _i32([64000] * 4).ctypes.data, _i32([0, 0]).ctypes.data, 2) == LC3_NULL_ERROR
    assert L.lc3plus_enc_sharded_destroy(None) == LC3_NULL_ERROR and L.lc3plus_dec_sharded_destroy(None) == LC3_NULL_ERROR


# ---- 4. the dispatch, against the stub ----
N, T = 480, 3
FORMATS = [t | l for t in (16, 24, 32, api.PCM_FLOAT32) for l in (0, api.PCM_INTERLEAVED, api.PCM_CHANNEL_MAJOR)]
SPLITS = [(33, 2), (7, 3)]


def _blocks(L, S, K):
    return [api.shard_block(S, K, i, L) for i in range(K)]


def _pcm_ptr(L, base, fmt, ch, first):
    return base + (2 if fmt & 0xFF == 16 else 4) * L.lc3plus_pcm_offset(fmt, ch, T, N, first, 0, 0, 0)


@pytest.mark.parametrize("S,K", SPLITS)
@pytest.mark.parametrize("ch", [1, 2])
def test_encode_hands_every_shard_its_slice(stub, S, K, ch):
    L = stub
    L.lc3stub_reset()
    rc, h = _create(L, "enc", S, 48000, ch, 10.0, 0, [64000 * ch] * S, [0] * K)
    assert rc == 0
    rows = np.arange(S * T, dtype=np.int32).reshape(S, T)
    sizes = 40 * ch + rows                                           # bytes of every stream-frame: all different
    rates, bws = _i32(sizes * 800), _i32(4000 + 10 * rows)
    stride = max(int(sizes.max()), 80 * ch)
    assert L.lc3plus_enc_sharded_stride(h) == 80 * ch and L.lc3plus_enc_sharded_input_samples(h) == N
    for fmt in FORMATS:
        pcm = np.zeros(api.pcm_shape(fmt, S, T, ch, N), api.pcm_dtype(fmt))
        out = np.zeros((S, T, stride), np.uint8)
        for br, bw in ((None, None), (rates, None), (None, bws), (rates, bws)):
            L.lc3stub_reset()
            nb = np.full((S, T), -7, np.int32)
            rc = L.lc3plus_enc_sharded_encode(h, pcm.ctypes.data, fmt, bw.ctypes.data if bw is not None else None, br.ctypes.data if br is not None else None,
                                              T, out.ctypes.data, stride, nb.ctypes.data)
            assert rc == 0
            log = sorted(_log(L), key=lambda r: r.ctx)
            assert [r.ctx % K for r in log] == list(range(K)) and all(r.kind == ENCODE for r in log)
            for i, (first, count) in enumerate(_blocks(L, S, K)):
                r = log[i]
                assert r.p[0] == _pcm_ptr(L, pcm.ctypes.data, fmt, ch, first), (fmt, i)
                assert r.p[1] == out.ctypes.data + first * T * stride
                assert (r.n_frames, r.stride, r.fmt, r.on_device, r.sync, r.hip_stream) == (T, stride, fmt, 0, 1, 0)
                last = first + count - 1
                assert list(r.a) == ([sizes[first, 0], sizes[first, 1], sizes[last, T - 1]] if br is not None else [-1, -1, -1])
                assert list(r.b) == ([bws[first, 0], bws[first, 1], bws[last, T - 1]] if bw is not None else [-1, -1, -1])
            # num_bytes: every shard wrote its rows
            if br is not None:
                assert (nb == sizes).all()
                for s in range(S):
                    assert L.lc3plus_enc_sharded_num_bytes(h, s) == sizes[s, T - 1]
                    assert L.lc3plus_enc_sharded_set_bitrate(h, s, 64000 * ch) == 0      # back to the start for the next round
            else:
                assert (nb == 80 * ch).all()
            if bw is not None:
                for s in (0, S // 2, S - 1):
                    assert L.lc3plus_enc_sharded_bandwidth(h, s) == bws[s, T - 1]
                    assert L.lc3plus_enc_sharded_set_bandwidth(h, s, 0) == 0
    assert L.lc3plus_enc_sharded_destroy(h) == 0


def test_refused_encode_logs_no_call_on_any_context(stub):
    L = stub
    for S, K in SPLITS:
        L.lc3stub_reset()
        rc, h = _create(L, "enc", S, 48000, 1, 10.0, 0, [64000] * S, [0] * K)
        assert rc == 0
        pcm, out, nb = np.zeros((S, T, N), np.int16), np.zeros((S, T, 400), np.uint8), np.zeros((S, T), np.int32)
        rates = np.full((S, T), 64000, np.int32); rates[S - 1, T - 1] = 1000            # a bad rate in the last shard's rows
        bws = np.full((S, T), 8000, np.int32)
        e = lambda **kw: L.lc3plus_enc_sharded_encode(h, kw.get("pcm", pcm).ctypes.data if kw.get("pcm", pcm) is not None else None, kw.get("fmt", 16),
                                                      kw["bw"].ctypes.data if kw.get("bw") is not None else None,
                                                      kw["br"].ctypes.data if kw.get("br") is not None else None, kw.get("T", T), out.ctypes.data,
                                                      kw.get("stride", 400), nb.ctypes.data)
        assert e(br=rates) == LC3_BITRATE_ERROR
        assert e(br=rates, bw=bws) == LC3_BITRATE_ERROR
        bad_bw = bws.copy(); bad_bw[S - 1, 0] = -5
        assert e(br=rates, bw=bad_bw) == LC3_ERROR                   # bandwidth values are checked before rates, as unsharded
        assert e(stride=79) == LC3_ERROR and e(T=0) == LC3_ERROR and e(fmt=17) == LC3_ERROR and e(pcm=None) == LC3_NULL_ERROR
        good = np.full((S, T), 64000, np.int32); good[S - 1, 1] = 96000
        assert e(br=good, stride=119) == LC3_ERROR                   # out_stride below the last shard's largest frame
        assert _log(L) == []
        refused = bws.copy(); refused[S - 1, 1] = 24000              # refused as set_bandwidth refuses it: the call runs, on every shard
        assert e(bw=refused) == LC3_BW_WARNING
        assert sorted(r.ctx for r in _log(L)) == list(range(K))
        assert L.lc3plus_enc_sharded_bandwidth(h, S - 1) == 8000
        assert L.lc3plus_enc_sharded_destroy(h) == 0


def test_a_failing_shard_does_not_stop_the_others(stub):
    L = stub
    L.lc3stub_reset()
    S, K = 7, 3
    rc, h = _create(L, "enc", S, 48000, 1, 10.0, 0, [64000] * S, [0] * K)
    rc2, d = _create(L, "dec", S, 48000, 1, 10.0, 0, [80] * S, [0] * K)
    assert rc == 0 and rc2 == 0                                      # contexts 0 - 2 the encoder's, 3 - 5 the decoder's
    pcm, out = np.zeros((S, T, N), np.int16), np.zeros((S, T, 80), np.uint8)
    st = np.zeros((S, T), np.uint8)
    L.lc3stub_fail_ctx(1)
    assert L.lc3plus_enc_sharded_encode(h, pcm.ctypes.data, 16, None, None, T, out.ctypes.data, 80, None) == LC3_ERROR
    assert sorted(r.ctx for r in _log(L)) == [0, 1, 2]
    L.lc3stub_fail_ctx(4)
    assert L.lc3plus_dec_sharded_decode(d, out.ctypes.data, 80, None, None, T, pcm.ctypes.data, 16, st.ctypes.data) == LC3_ERROR
    assert sorted(r.ctx for r in _log(L)) == [0, 1, 2, 3, 4, 5]
    L.lc3stub_fail_ctx(-1)
    assert L.lc3plus_enc_sharded_encode(h, pcm.ctypes.data, 16, None, None, T, out.ctypes.data, 80, None) == 0
    assert L.lc3plus_enc_sharded_destroy(h) == 0 and L.lc3plus_dec_sharded_destroy(d) == 0


@pytest.mark.parametrize("S,K", SPLITS)
@pytest.mark.parametrize("ch", [1, 2])
def test_decode_hands_every_shard_its_slice(stub, S, K, ch):
    L = stub
    L.lc3stub_reset()
    rc, h = _create(L, "dec", S, 48000, ch, 10.0, 0, [80 * ch] * S, [0] * K)
    assert rc == 0
    rows = np.arange(S * T, dtype=np.int32).reshape(S, T)
    sizes = _i32(40 * ch + rows)
    in_stride = max(int(sizes.max()), 80 * ch)
    bfi = ((rows % 5) == 2).astype(np.uint8)
    frames = np.zeros((S, T, in_stride), np.uint8)
    assert L.lc3plus_dec_sharded_output_samples(h) == N and L.lc3plus_dec_sharded_delay(h) > 0
    for fmt in FORMATS:
        pcm = np.zeros(api.pcm_shape(fmt, S, T, ch, N), api.pcm_dtype(fmt))
        for nb in (None, sizes):
            L.lc3stub_reset()
            status = np.zeros((S, T), np.uint8)
            rc = L.lc3plus_dec_sharded_decode(h, frames.ctypes.data, in_stride, nb.ctypes.data if nb is not None else None, bfi.ctypes.data, T,
                                              pcm.ctypes.data, fmt, status.ctypes.data)
            assert rc == 0
            log = sorted(_log(L), key=lambda r: r.ctx)
            assert len(log) == K and all(r.kind == DECODE for r in log)
            for i, (first, count) in enumerate(_blocks(L, S, K)):
                r = log[i]
                last = first + count - 1
                assert r.p[0] == frames.ctypes.data + first * T * in_stride
                assert r.p[1] == _pcm_ptr(L, pcm.ctypes.data, fmt, ch, first)
                assert r.p[2] == status.ctypes.data + first * T
                assert (r.n_frames, r.stride, r.fmt, r.on_device, r.sync) == (T, in_stride, fmt, 0, 1)
                assert list(r.b) == [bfi[first, 0], bfi[first, 1], bfi[last, T - 1]]
                if nb is None:
                    assert r.p[3] == bfi.ctypes.data + first * T and list(r.a) == [-1, -1, -1]
                else:                                                # the sizes the kernels take: 0 where the frame is lost
                    eff = np.where(bfi == 1, 0, sizes)
                    assert list(r.a) == [eff[first, 0], eff[first, 1], eff[last, T - 1]]
            if nb is not None:
                for s in range(S):
                    want = [sizes[s, t] for t in range(T) if not bfi[s, t]][-1]
                    assert L.lc3plus_dec_sharded_num_bytes(h, s) == want
                    assert L.lc3plus_dec_sharded_set_num_bytes(h, s, 80 * ch) == 0
    # a refused call logs nothing: a bad size, then a bad flag, in the last shard's rows; a stride below a stream's size
    L.lc3stub_reset()
    pcm, status = np.zeros((S, T, ch, N), np.int16), np.zeros((S, T), np.uint8)
    bad = sizes.copy(); bad[S - 1, T - 1] = 401 * ch
    call = lambda nb, fl, stride=in_stride: L.lc3plus_dec_sharded_decode(h, frames.ctypes.data, stride, nb.ctypes.data if nb is not None else None,
                                                                         fl.ctypes.data, T, pcm.ctypes.data, 16, status.ctypes.data)
    assert call(bad, bfi) == LC3_NUMBYTES_ERROR
    flags = bfi.copy(); flags[S - 1, 0] = 2
    assert call(sizes, flags) == LC3_ERROR
    assert call(None, bfi, 80 * ch - 1) == LC3_NUMBYTES_ERROR
    assert _log(L) == []
    assert L.lc3plus_dec_sharded_destroy(h) == 0


def test_state_slices_are_contiguous_and_in_shard_order(stub):
    L = stub
    for kind, cfg in (("enc", 64000), ("dec", 80)):
        for S, K in SPLITS:
            L.lc3stub_reset()
            rc, h = _create(L, kind, S, 48000, 2, 10.0, 0, [cfg * 2] * S, [0] * K)
            assert rc == 0
            f = lambda x: getattr(L, "lc3plus_%s_sharded_%s" % (kind, x))
            size = f("state_size")(h)
            assert size == STATE_BYTES * S * 2
            st = np.full(size + 8, 0xEE, np.uint8)
            assert f("get_state")(h, st.ctypes.data, size - 1) == LC3_ERROR and f("set_state")(h, st.ctypes.data, size + 1) == LC3_ERROR
            assert _log(L) == []
            assert f("get_state")(h, st.ctypes.data, size) == 0
            assert (st[size:] == 0xEE).all()
            at = 0
            for i, (first, count) in enumerate(_blocks(L, S, K)):    # the stub fills a shard's slice with its context number
                n = STATE_BYTES * count * 2
                assert at == STATE_BYTES * first * 2 and (st[at:at + n] == i).all()
                at += n
            assert at == size
            L.lc3stub_reset()
            assert f("set_state")(h, st.ctypes.data, size) == 0
            log = sorted(_log(L), key=lambda r: r.ctx)
            for i, (first, count) in enumerate(_blocks(L, S, K)):
                assert log[i].kind == SET_STATE and log[i].p[0] == st.ctypes.data + STATE_BYTES * first * 2 and log[i].bytes == STATE_BYTES * count * 2
                assert (log[i].a[0], log[i].a[2]) == (i, i)
            assert f("destroy")(h) == 0


def test_device_calls_queue_every_shard_before_any_wait(stub):
    L = stub
    L.lc3stub_reset()
    S, K = 7, 3
    rc, h = _create(L, "enc", S, 48000, 1, 10.0, 0, [64000] * S, [0] * K)
    assert rc == 0
    pcm = (C.c_void_p * K)(0x1000, 0x2000, 0x3000); out = (C.c_void_p * K)(0x4000, 0x5000, 0x6000); streams = (C.c_void_p * K)(0x10, None, 0x30)
    assert L.lc3plus_enc_sharded_encode_device(h, pcm, 16, T, out, 80, streams, 1) == 0
    log = _log(L, kinds=(ENCODE, 5))
    assert [(r.kind, r.ctx) for r in log] == [(ENCODE, 0), (ENCODE, 1), (ENCODE, 2), (5, 0), (5, 1), (5, 2)]
    assert [(r.p[0], r.p[1], r.hip_stream, r.on_device, r.sync) for r in log[:3]] == [(0x1000, 0x4000, 0x10, 1, 0), (0x2000, 0x5000, 0, 1, 0), (0x3000, 0x6000, 0x30, 1, 0)]
    L.lc3stub_reset()
    pcm[2] = None
    assert L.lc3plus_enc_sharded_encode_device(h, pcm, 16, T, out, 80, None, 0) == LC3_NULL_ERROR      # checked for all shards first
    assert L.lc3plus_enc_sharded_encode_device(h, None, 16, T, out, 80, None, 0) == LC3_NULL_ERROR
    assert _log(L, kinds=(ENCODE, 5)) == []
    assert L.lc3plus_enc_sharded_destroy(h) == 0


def test_python_mirror_on_the_stub(stub):
    sb = api.ShardedBatch(7, 48000, 2, 10.0, 0, [128000] * 7, [0, 0, 0], lib=stub)
    assert (sb.n_shards, sb.devices, sb.blocks, sb.owner(3)) == (3, [0, 0, 0], [(0, 3), (3, 2), (5, 2)], (1, 0))
    out = sb.encode(np.zeros((7, 2 * N, 2), np.float32), layout="interleaved", bitrates=np.full((7, 2), 96000))
    assert out.shape == (7, 2, 120) and (sb.last_num_bytes == 120).all()
    v = sb.shard(1)
    assert v.n_streams == 2 and v.num_bytes(0) == 120
    v.close()                                                        # a borrowed view: the shard lives on
    assert sb.num_bytes(3) == 120
    assert sb.get_state().size == sb.state_size
    sb.close()
    sd = api.ShardedDecBatch(7, 48000, 1, 10.0, 0, [80] * 7, [0, 0], lib=stub)
    pcm, st = sd.decode(np.zeros((7, 2, 80), np.uint8), bfi=np.zeros((7, 2), np.uint8))
    assert pcm.shape == (7, 2, 1, N) and sd.shard(1).n_streams == 3
    sd.close()


# ---- 5. the threads under ThreadSanitizer ----
def test_threads_are_clean_under_tsan(stub):
    out = subprocess.run([os.path.join(STUB_DIR, "sharded_stub_driver")], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1:exitcode=66"))
    assert out.returncode == 0 and "ThreadSanitizer" not in out.stderr and "ok" in out.stdout, (out.returncode, out.stdout[-500:], out.stderr[-3000:])


# ---- 6. the new host code under AddressSanitizer + UndefinedBehaviorSanitizer ----
def test_split_and_refusals_are_clean_under_asan_and_ubsan():
    if os.environ.get("LC3PLUS_SHARDED_ASAN_CHILD"):
        pytest.skip("this is the child")
    def lib(name):
        p = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
        return p if os.path.isabs(p) and os.path.exists(p) else None
    asan, ubsan = lib("libasan.so"), lib("libubsan.so")
    if not asan or not ubsan:
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC])
    subprocess.check_call(["make", "-s", "-C", CSRC, "asan"])
    env = dict(os.environ, LD_PRELOAD=asan + ":" + ubsan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               LC3PLUS_HIP_LIB=os.path.join(ROOT, "audio_codec_amd", "_asan", "liblc3plus_hip.so"), LC3PLUS_SHARDED_ASAN_CHILD="1")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider", "-k",
                          "test_shard_block_is_stream_block or test_shard_block_bad_arguments or test_create_refusals_need_no_device"],
                         capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert out.returncode == 0 and "3 passed" in out.stdout and "runtime error" not in out.stderr, (out.stdout[-1500:], out.stderr[-3000:])
