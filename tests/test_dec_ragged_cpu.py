"""Per-stream frame counts of the batched decoder (include/lc3plus_batch.h: lc3plus_dec_batch_set_frame_counts) on the host alone: the exports, the clamp
(lc3plus_dec_plan_counts) against numpy's clip with its argument errors, and through the stub build (tools/stub_shim.c) the setter's pointer reaching the
shim, the decode calls that refuse while counts are on - nothing queued - and work again after NULL, and the setter through a shard handle.  Every
comparison is equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import audio_codec_amd
from audio_codec_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_codec_amd", "csrc")
LC3_OK, LC3_ERROR, LC3_NULL_ERROR = 0, 1, 3
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
NEW = ("lc3plus_dec_batch_set_frame_counts", "lc3plus_dec_plan_counts")


# ---- 1. exports ----
def test_symbols_are_exported_declared_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", api.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    for s in NEW:
        assert s in names and s in api.EXPORTS, s
        assert re.search(r"\b%s\(" % s, header), s
    plan = open(os.path.join(CSRC, "lc3_plan.h")).read()
    assert int(re.search(r"#define\s+LC3D_DEC_ST_ABSENT\s+(\d+)", plan).group(1)) == api.DEC_ST_ABSENT == 8
    assert hasattr(api.DecBatch, "set_frame_counts")


# ---- 2. the clamp ----
@pytest.mark.parametrize("T", [1, 6, 16, 4096, I32_MAX])
def test_plan_counts_is_numpy_clip(T):
    rng = np.random.default_rng(T % 1000)
    counts = np.array([I32_MIN, I32_MIN + 1, -1, 0, 1, T - 1, T, min(T + 1, I32_MAX), I32_MAX - 1, I32_MAX] + [int(x) for x in rng.integers(-40, 40, 64)],
                      np.int64).astype(np.int32)
    got = api.dec_plan_counts(counts, T)
    assert got.dtype == np.int32 and (got == np.clip(counts.astype(np.int64), 0, T)).all()


def test_plan_counts_arguments():
    f = audio_codec_amd.load_library().lc3plus_dec_plan_counts
    c, e = np.array([3, -2, 9], np.int32), np.full(3, 77, np.int32)
    assert f(None, 0, 4, None) == LC3_OK                                # no stream: nothing is read or written
    assert f(None, 3, 4, e.ctypes.data) == LC3_NULL_ERROR
    assert f(c.ctypes.data, 3, 4, None) == LC3_NULL_ERROR
    assert f(c.ctypes.data, -1, 4, e.ctypes.data) == LC3_ERROR
    assert f(c.ctypes.data, 3, 0, e.ctypes.data) == LC3_ERROR
    assert f(c.ctypes.data, 3, -5, e.ctypes.data) == LC3_ERROR
    assert (e == 77).all()                                              # a refused call writes nothing
    assert f(c.ctypes.data, 3, 4, e.ctypes.data) == LC3_OK and e.tolist() == [3, 0, 4]
    with pytest.raises(api.LC3Error):
        api.dec_plan_counts([1, 2], 0)


# ---- 3. the host logic through the stub build ----
class Rec(C.Structure):                                              # lc3stub_rec (tools/stub_shim.c)
    _fields_ = [("ctx", C.c_int32), ("kind", C.c_int32), ("dec", C.c_int32), ("n_frames", C.c_int32), ("stride", C.c_int32), ("fmt", C.c_int32),
                ("on_device", C.c_int32), ("sync", C.c_int32), ("p", C.c_uint64 * 4), ("a", C.c_int64 * 3), ("b", C.c_int64 * 3), ("bytes", C.c_uint64),
                ("hip_stream", C.c_uint64)]


STUB_DECODE, STUB_WAIT, STUB_COUNTS = 2, 5, 7


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-s", "-C", CSRC, "stub"])
    L = C.CDLL(os.path.join(ROOT, "audio_codec_amd", "_stub", "liblc3plus_stub.so"))
    api._declare_sharded(L)
    L.lc3plus_dec_batch_set_frame_counts.argtypes = [C.c_void_p, C.c_void_p]
    L.lc3plus_dec_batch_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int]
    L.lc3plus_dec_batch_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_int]
    L.lc3plus_dec_batch_decode_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_int]
    L.lc3plus_dec_batch_decode_traced.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.lc3plus_dec_batch_decode_sizes_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                        C.c_void_p, C.c_int]
    L.lc3plus_dec_trace_sizeof.restype = C.c_int
    L.lc3plus_dec_batch_destroy.argtypes = [C.c_void_p]
    assert L.lc3stub_rec_sizeof() == C.sizeof(Rec)
    return L


def _log(L):
    n = L.lc3stub_log(None, 0)
    buf = (Rec * max(n, 1))()
    assert L.lc3stub_log(buf, n) == n
    return [buf[i] for i in range(n)]


def _dec(L, S=3, ch=2):
    L.lc3stub_reset()
    d = C.c_void_p()
    nb = np.ascontiguousarray([80 * ch] * S, np.int32)
    assert L.lc3plus_dec_batch_create(C.byref(d), S, 48000, ch, C.c_float(10.0), 0, nb.ctypes.data_as(C.c_void_p), 0) == 0
    return d


def test_setter_reaches_the_shim_and_null_switches_off(stub):
    L = stub
    d = _dec(L)
    L.lc3stub_reset()
    assert L.lc3plus_dec_batch_set_frame_counts(None, 0x5000) == LC3_NULL_ERROR
    assert _log(L) == []
    assert L.lc3plus_dec_batch_set_frame_counts(d, 0x5000) == LC3_OK
    assert L.lc3plus_dec_batch_set_frame_counts(d, None) == LC3_OK
    assert [(r.kind, r.dec, r.p[0]) for r in _log(L)] == [(STUB_COUNTS, 1, 0x5000), (STUB_COUNTS, 1, 0)]
    L.lc3plus_dec_batch_destroy(d)


def test_other_decode_calls_refuse_while_counts_are_on(stub):
    """decode, decode_sizes and the traced call return LC3_ERROR and reach no shim function; the device-size call goes through; after NULL all work again"""
    L = stub
    S, ch, T, N = 3, 2, 4, 480
    d = _dec(L, S, ch)
    pcm, fr, st = np.zeros((S, T, ch, N), np.int16), np.zeros((S, T, 80 * ch), np.uint8), np.zeros((S, T), np.uint8)
    nb = np.full((S, T), 80 * ch, np.int32)
    tr = np.zeros(S * ch * T * L.lc3plus_dec_trace_sizeof(), np.uint8)
    pp, fp = pcm.ctypes.data, fr.ctypes.data

    def calls():
        return [L.lc3plus_dec_batch_decode(d, fp, 0, 80 * ch, None, T, pp, 0, 16, st.ctypes.data, None, 1),
                L.lc3plus_dec_batch_decode(d, fp, 1, 80 * ch, None, T, pp, 1, 16, None, None, 0),
                L.lc3plus_dec_batch_decode_sizes(d, fp, 0, 80 * ch, nb.ctypes.data, None, T, pp, 0, 16, st.ctypes.data, None, 1),
                L.lc3plus_dec_batch_decode_traced(d, fp, 80 * ch, None, T, pp, 16, st.ctypes.data, tr.ctypes.data)]

    L.lc3stub_reset()
    assert calls() == [LC3_OK] * 4                                      # off: as ever
    assert [r.kind for r in _log(L)] == [STUB_DECODE] * 4
    assert L.lc3plus_dec_batch_set_frame_counts(d, 0x5000) == LC3_OK
    L.lc3stub_reset()
    assert calls() == [LC3_ERROR] * 4
    assert _log(L) == []                                                # nothing queued, nothing read back
    assert L.lc3plus_dec_batch_decode(None, fp, 0, 80 * ch, None, T, pp, 0, 16, None, None, 1) == LC3_NULL_ERROR
    assert L.lc3plus_dec_batch_decode_sizes_device(d, fp, 80 * ch, nb.ctypes.data, None, T, pp, 16, None, None, 0) == LC3_OK
    assert L.lc3plus_dec_batch_set_frame_counts(d, None) == LC3_OK
    L.lc3stub_reset()
    assert calls() == [LC3_OK] * 4
    assert [r.kind for r in _log(L)] == [STUB_DECODE] * 4
    L.lc3plus_dec_batch_destroy(d)


def test_shard_handle_and_sharded_calls(stub):
    """the borrowed handle of a shard takes the setter (local indices: its own context); both sharded decode calls then refuse before any shard is touched,
    and work again after NULL"""
    L = stub
    S, K, ch, T, N = 6, 2, 1, 3, 480
    h = C.c_void_p()
    nb0, devs = np.ascontiguousarray([80] * S, np.int32), np.zeros(K, np.int32)
    L.lc3stub_reset()
    assert L.lc3plus_dec_sharded_create(C.byref(h), S, 48000, ch, 10.0, 0, nb0.ctypes.data, devs.ctypes.data, K) == 0
    sh1 = L.lc3plus_dec_sharded_shard(h, 1)
    pcm, fr, st = np.zeros((S, T, ch, N), np.int16), np.zeros((S, T, 80), np.uint8), np.zeros((S, T), np.uint8)
    nb = np.full((S, T), 80, np.int32)
    fptr = (C.c_void_p * K)(fr.ctypes.data, fr.ctypes.data + fr.nbytes // 2)
    pptr = (C.c_void_p * K)(pcm.ctypes.data, pcm.ctypes.data + pcm.nbytes // 2)

    def calls():
        return [L.lc3plus_dec_sharded_decode(h, fr.ctypes.data, 80, None, None, T, pcm.ctypes.data, 16, st.ctypes.data),
                L.lc3plus_dec_sharded_decode(h, fr.ctypes.data, 80, nb.ctypes.data, None, T, pcm.ctypes.data, 16, st.ctypes.data),
                L.lc3plus_dec_sharded_decode_device(h, fptr, 80, T, pptr, 16, None, 1)]

    L.lc3stub_reset()
    assert L.lc3plus_dec_batch_set_frame_counts(sh1, 0x9000) == LC3_OK
    assert [(r.kind, r.ctx, r.p[0]) for r in _log(L)] == [(STUB_COUNTS, 1, 0x9000)]
    L.lc3stub_reset()
    assert calls() == [LC3_ERROR] * 3
    assert _log(L) == []                                                # shard 0, which has no counts, was not touched either
    assert L.lc3plus_dec_batch_set_frame_counts(sh1, None) == LC3_OK
    L.lc3stub_reset()
    assert calls() == [LC3_OK] * 3
    kinds = [r.kind for r in _log(L)]
    assert kinds.count(STUB_DECODE) == 3 * K and set(kinds) <= {STUB_DECODE, STUB_WAIT}
    assert L.lc3plus_dec_sharded_destroy(h) == 0
