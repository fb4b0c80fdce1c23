"""Per-stream frame counts of the batched encoder (include/lc3plus_batch.h: lc3plus_enc_batch_set_frame_counts) on the host alone: the exports, the host
plan lc3plus_enc_plan_rates_ragged against lc3plus_enc_plan_rates_lenient cut at each stream's count, the packed offsets of ragged sizes, and through the
stub build (tools/stub_shim.c) the setter's pointer reaching the shim, the encode calls that refuse while counts are on - nothing queued - and work again
after NULL, and the setter through a shard handle.  Every comparison is equality."""
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
NEW = ("lc3plus_enc_batch_set_frame_counts", "lc3plus_enc_plan_rates_ragged")
ABSENT = 32


# ---- 1. exports ----
def test_symbols_are_exported_declared_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", api.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    for s in NEW:
        assert s in names and s in api.EXPORTS, s
        assert re.search(r"\b%s\(" % s, header), s
    plan = open(os.path.join(CSRC, "lc3_plan.h")).read()
    assert int(re.search(r"#define\s+LC3D_ENC_FL_ABSENT\s+(\d+)", plan).group(1)) == api.ENC_FL_ABSENT == ABSENT
    assert int(re.search(r"#define\s+LC3PLUS_ENC_FL_ABSENT\s+(\d+)", header).group(1)) == ABSENT
    assert hasattr(api.Batch, "set_frame_counts")


# ---- 2. the host plan ----
GEOMS = [(48000, 1, 10.0, 0, [40000, 64000, 96000, 128000]), (48000, 2, 10.0, 0, [128800, 160800, 96000]), (16000, 1, 2.5, 0, [64000, 128000, 160000]),
         (96000, 1, 10.0, 1, [149600, 256000, 400000])]


def _words(g, S, T, seed):
    """random rates and bandwidths [S, T], about a fifth of them values the rule refuses"""
    fs, ch, ms, hr, rates = g
    rng = np.random.default_rng(seed)
    br = rng.choice(np.array(rates + [0, -1, 1, I32_MAX, I32_MIN], np.int64), size=(S, T), p=[0.8 / len(rates)] * len(rates) + [0.04] * 5).astype(np.int32)
    bws = [0, 4000, 8000, 12000, 16000, 20000, 24000]
    bw = rng.choice(np.array(bws + [-1, 7, I32_MAX, I32_MIN], np.int64), size=(S, T), p=[0.8 / len(bws)] * len(bws) + [0.05] * 4).astype(np.int32)
    start = [rates[s % len(rates)] for s in range(S)]
    return br, (None if hr else bw), start


# (rates alone in the high-resolution mode, which has no bandwidth controller)
@pytest.mark.parametrize("g,mode", [(g, m) for g in GEOMS for m in ("r", "b", "rb") if not (g[3] and "b" in m)], ids=lambda v: v if isinstance(v, str) else "%d_%d_%g" % v[:3])
def test_dense_counts_and_null_equal_the_lenient_plan(g, mode):
    fs, ch, ms, hr, rates = g
    S, T = 7, 9
    br, bw, start = _words(g, S, T, 3)
    kw = dict(bitrates=br if "r" in mode else None, bandwidths=bw if "b" in mode else None, out_stride=600)
    want = api.enc_plan_rates_lenient(fs, ch, ms, hr, start, [0] * S, **kw)
    assert want[0] == LC3_OK and (want[3] != 0).any()
    for counts in (None, [T] * S, [T + 5] * S, [I32_MAX] * S):
        got = api.enc_plan_rates_ragged(fs, ch, ms, hr, start, [0] * S, counts=counts, **kw)
        assert got[0] == LC3_OK
        for a, b in zip(got[1:], want[1:]):
            assert (a == b).all()
    # the errors of the lenient plan are the ragged plan's
    bad = api.enc_plan_rates_lenient(fs, ch, ms, hr, [1] * S, [0] * S, **kw)[0]
    assert bad != LC3_OK and api.enc_plan_rates_ragged(fs, ch, ms, hr, [1] * S, [0] * S, counts=[T] * S, **kw)[0] == bad


@pytest.mark.parametrize("g", GEOMS[:3], ids=lambda g: "%d_%d_%g" % g[:3])
def test_counts_cut_the_plan_and_absent_inputs_do_not_matter(g):
    fs, ch, ms, hr, rates = g
    S, T = 8, 6
    br, bw, start = _words(g, S, T, 5)
    counts = np.array([0, 1, 3, 6, -3, T + 9, I32_MIN, I32_MAX], np.int32)
    c = np.clip(counts.astype(np.int64), 0, T)
    rc, nb, inf, fl, end = api.enc_plan_rates_ragged(fs, ch, ms, hr, start, [8000] * S, bitrates=br, bandwidths=bw, out_stride=600, counts=counts)
    assert rc == LC3_OK
    # the same with every absent entry a refused value
    br2, bw2 = br.copy(), bw.copy()
    for s in range(S):
        br2[s, c[s]:] = -1; bw2[s, c[s]:] = -1
    again = api.enc_plan_rates_ragged(fs, ch, ms, hr, start, [8000] * S, bitrates=br2, bandwidths=bw2, out_stride=600, counts=counts)
    for a, b in zip((rc, nb, inf, fl, end), again):
        assert np.array_equal(a, b)
    # stream by stream: the lenient plan of its present frames alone
    for s in range(S):
        n = int(c[s])
        assert (nb[s, n:] == 0).all() and (inf[s, n:] == 0).all() and (fl[s, n:] == ABSENT).all()
        if n == 0:
            assert end[s] == start[s]                                   # the start is kept
            continue
        w = api.enc_plan_rates_lenient(fs, ch, ms, hr, [start[s]], [8000], bitrates=br[s:s + 1, :n], bandwidths=bw[s:s + 1, :n], out_stride=600)
        assert w[0] == LC3_OK
        assert (nb[s, :n] == w[1][0]).all() and (inf[s, :n] == w[2][0]).all() and (fl[s, :n] == w[3][0]).all() and end[s] == w[4][0]
        assert not (fl[s, :n] & ABSENT).any()


def test_plan_with_neither_rates_nor_bandwidths_and_its_arguments():
    S, T = 4, 5
    rc, nb, inf, fl, end = api.enc_plan_rates_ragged(48000, 1, 10.0, 0, [64000, 96000, 128000, 64000], [0, 8000, 0, 0], counts=[5, 2, 0, 9], n_frames=T)
    assert rc == LC3_OK
    assert nb.tolist() == [[80] * 5, [120, 120, 0, 0, 0], [0] * 5, [80] * 5]
    assert inf.tolist() == [[0] * 5, [8000, 8000, 0, 0, 0], [0] * 5, [0] * 5]
    assert fl.tolist() == [[0] * 5, [0, 0, 32, 32, 32], [32] * 5, [0] * 5] and end.tolist() == [64000, 96000, 128000, 64000]
    f = audio_codec_amd.load_library().lc3plus_enc_plan_rates_ragged
    i = lambda n, v=0: np.full(n, v, np.int32)
    sr, sb, o1, o2, o3, o4, cn = i(S, 64000), i(S), i(S * T, 77), i(S * T, 77), np.full(S * T, 77, np.uint8), i(S, 77), i(S, 2)
    a = lambda **k: f(48000, 1, C.c_float(10.0), 0, k.get("S", S), k.get("sr", sr.ctypes.data), sb.ctypes.data, None, None, k.get("T", T), 300,
                      k.get("o1", o1.ctypes.data), o2.ctypes.data, o3.ctypes.data, o4.ctypes.data, cn.ctypes.data)
    assert a(sr=None) == LC3_NULL_ERROR and a(o1=None) == LC3_NULL_ERROR
    assert a(S=0) == LC3_ERROR and a(T=0) == LC3_ERROR
    assert (o1 == 77).all() and (o3 == 77).all() and (o4 == 77).all()   # a refused call writes nothing
    assert a() == LC3_OK and o1.reshape(S, T).tolist() == [[80, 80, 0, 0, 0]] * S
    # the lenient plan still wants one of the two
    assert api.load_library().lc3plus_enc_plan_rates_lenient(48000, 1, C.c_float(10.0), 0, S, sr.ctypes.data, sb.ctypes.data, None, None, T, 300, o1.ctypes.data,
                                                             o2.ctypes.data, o3.ctypes.data, o4.ctypes.data) == LC3_NULL_ERROR


@pytest.mark.parametrize("order", [api.PACK_STREAM_MAJOR, api.PACK_FRAME_MAJOR])
def test_packed_offsets_of_ragged_sizes(order):
    """an absent frame has size 0: its offset is the running offset at its place in the order, total is the sum over the present frames"""
    rc, nb, _, fl, _ = api.enc_plan_rates_ragged(48000, 1, 10.0, 0, [64000, 96000, 128000], [0] * 3, counts=[3, 0, 1], n_frames=3)
    assert rc == LC3_OK and nb.tolist() == [[80, 80, 80], [0, 0, 0], [160, 0, 0]]
    rc, offs, total, ovf = api.plan_packed(nb, order=order, capacity=300)
    assert rc == LC3_OK and total == 400
    if order == api.PACK_STREAM_MAJOR:
        assert offs.tolist() == [[0, 80, 160], [240, 240, 240], [240, 400, 400]]
        assert ovf.tolist() == [[0, 0, 0], [0, 0, 0], [8, 8, 8]]        # (the host hook knows no counts: the device reports exactly 32 for the absent ones)
    else:
        assert offs.tolist() == [[0, 240, 320], [80, 320, 400], [80, 320, 400]]
        assert ovf.tolist() == [[0, 8, 8], [0, 8, 8], [0, 8, 8]]


# ---- 3. the host logic through the stub build ----
class Rec(C.Structure):                                              # lc3stub_rec (tools/stub_shim.c)
    _fields_ = [("ctx", C.c_int32), ("kind", C.c_int32), ("dec", C.c_int32), ("n_frames", C.c_int32), ("stride", C.c_int32), ("fmt", C.c_int32),
                ("on_device", C.c_int32), ("sync", C.c_int32), ("p", C.c_uint64 * 4), ("a", C.c_int64 * 3), ("b", C.c_int64 * 3), ("bytes", C.c_uint64),
                ("hip_stream", C.c_uint64)]


STUB_ENCODE, STUB_WAIT, STUB_COUNTS = 1, 5, 7


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-s", "-C", CSRC, "stub"])
    L = C.CDLL(os.path.join(ROOT, "audio_codec_amd", "_stub", "liblc3plus_stub.so"))
    api._declare_sharded(L)
    V, I = C.c_void_p, C.c_int
    L.lc3plus_enc_batch_set_frame_counts.argtypes = [V, V]
    L.lc3plus_enc_batch_create.argtypes = [C.POINTER(V), I, I, I, C.c_float, I, V, I]
    L.lc3plus_enc_batch_encode.argtypes = [V, V, I, I, I, V, I, I, V, I]
    L.lc3plus_enc_batch_encode_bitrates.argtypes = [V, V, I, I, V, I, V, I, I, V, V, I]
    L.lc3plus_enc_batch_encode_bandwidths.argtypes = [V, V, I, I, V, V, I, V, I, I, V, V, I]
    L.lc3plus_enc_batch_encode_traced.argtypes = [V, V, I, I, V, I, V]
    L.lc3plus_enc_batch_encode_bitrates_traced.argtypes = [V, V, I, V, I, V, I, V]
    L.lc3plus_enc_batch_encode_rates_device.argtypes = [V, V, I, V, V, I, V, I, V, V, V, I]
    L.lc3plus_enc_batch_encode_packed.argtypes = [V, V, I, V, V, I, I, V, C.c_int64, V, V, V, V, V, I]
    L.lc3plus_trace_sizeof.restype = I
    L.lc3plus_enc_batch_destroy.argtypes = [V]
    L.lc3plus_enc_sharded_shard.restype = V
    L.lc3plus_enc_sharded_shard.argtypes = [V, I]
    assert L.lc3stub_rec_sizeof() == C.sizeof(Rec)
    return L


def _log(L):
    n = L.lc3stub_log(None, 0)
    buf = (Rec * max(n, 1))()
    assert L.lc3stub_log(buf, n) == n
    return [buf[i] for i in range(n)]


def _enc(L, S=3, ch=2):
    L.lc3stub_reset()
    e = C.c_void_p()
    br = np.ascontiguousarray([64000 * ch] * S, np.int32)
    assert L.lc3plus_enc_batch_create(C.byref(e), S, 48000, ch, C.c_float(10.0), 0, br.ctypes.data_as(C.c_void_p), 0) == 0
    return e


def test_setter_reaches_the_shim_and_null_switches_off(stub):
    L = stub
    e = _enc(L)
    L.lc3stub_reset()
    assert L.lc3plus_enc_batch_set_frame_counts(None, 0x5000) == LC3_NULL_ERROR
    assert _log(L) == []
    assert L.lc3plus_enc_batch_set_frame_counts(e, 0x5000) == LC3_OK
    assert L.lc3plus_enc_batch_set_frame_counts(e, None) == LC3_OK
    assert [(r.kind, r.dec, r.p[0]) for r in _log(L)] == [(STUB_COUNTS, 0, 0x5000), (STUB_COUNTS, 0, 0)]
    L.lc3plus_enc_batch_destroy(e)


def test_other_encode_calls_refuse_while_counts_are_on(stub):
    """encode, encode_bitrates, encode_bandwidths and the traced calls return LC3_ERROR and reach no shim function; the two calls with flags in device memory
    go through (encode_packed with neither rates nor bandwidths too); after NULL all work again"""
    L = stub
    S, ch, T, N = 3, 2, 4, 480
    e = _enc(L, S, ch)
    pcm, out = np.zeros((S, T, ch, N), np.int16), np.zeros((S, T, 80 * ch), np.uint8)
    br, bw, nb = np.full((S, T), 64000 * ch, np.int32), np.full((S, T), 8000, np.int32), np.zeros((S, T), np.int32)
    tr = np.zeros(S * ch * T * L.lc3plus_trace_sizeof(), np.uint8)
    pp, op, st = pcm.ctypes.data, out.ctypes.data, 80 * ch

    def calls():
        return [L.lc3plus_enc_batch_encode(e, pp, 0, 16, T, op, st, 0, None, 1),
                L.lc3plus_enc_batch_encode(e, pp, 1, 16, T, op, st, 1, None, 0),
                L.lc3plus_enc_batch_encode_bitrates(e, pp, 0, 16, br.ctypes.data, T, op, st, 0, nb.ctypes.data, None, 1),
                L.lc3plus_enc_batch_encode_bandwidths(e, pp, 0, 16, bw.ctypes.data, None, T, op, st, 0, None, None, 1),
                L.lc3plus_enc_batch_encode_bandwidths(e, pp, 1, 16, bw.ctypes.data, br.ctypes.data, T, op, st, 1, None, None, 0),
                L.lc3plus_enc_batch_encode_traced(e, pp, 16, T, op, st, tr.ctypes.data),
                L.lc3plus_enc_batch_encode_bitrates_traced(e, pp, 16, br.ctypes.data, T, op, st, tr.ctypes.data)]

    L.lc3stub_reset()
    assert calls() == [LC3_OK] * 7                                      # off: as ever
    assert [r.kind for r in _log(L)] == [STUB_ENCODE] * 7
    assert L.lc3plus_enc_batch_set_frame_counts(e, 0x5000) == LC3_OK
    L.lc3stub_reset()
    assert calls() == [LC3_ERROR] * 7
    assert _log(L) == []                                                # nothing queued, nothing read back
    assert L.lc3plus_enc_batch_encode(None, pp, 0, 16, T, op, st, 0, None, 1) == LC3_NULL_ERROR
    assert L.lc3plus_enc_batch_encode_rates_device(e, pp, 16, br.ctypes.data, None, T, op, st, None, None, None, 0) == LC3_OK
    assert L.lc3plus_enc_batch_encode_rates_device(e, pp, 16, None, None, T, op, st, None, None, None, 0) == LC3_NULL_ERROR      # slotted: one of the two, as ever
    assert L.lc3plus_enc_batch_encode_packed(e, pp, 16, None, None, T, 0, op, out.nbytes, None, None, None, None, None, 0) == LC3_OK
    assert L.lc3plus_enc_batch_set_frame_counts(e, None) == LC3_OK
    L.lc3stub_reset()
    assert calls() == [LC3_OK] * 7
    assert [r.kind for r in _log(L)][-7:] == [STUB_ENCODE] * 7          # (the first reads the configuration back: the device calls above left it on the device)
    L.lc3plus_enc_batch_destroy(e)


def test_shard_handle_and_sharded_calls(stub):
    """the borrowed handle of a shard takes the setter (local indices: its own context); both sharded encode calls then refuse before any shard is touched,
    and work again after NULL"""
    L = stub
    S, K, ch, T, N = 6, 2, 1, 3, 480
    h = C.c_void_p()
    br0, devs = np.ascontiguousarray([64000] * S, np.int32), np.zeros(K, np.int32)
    L.lc3stub_reset()
    assert L.lc3plus_enc_sharded_create(C.byref(h), S, 48000, ch, 10.0, 0, br0.ctypes.data, devs.ctypes.data, K) == 0
    sh1 = L.lc3plus_enc_sharded_shard(h, 1)
    pcm, out = np.zeros((S, T, ch, N), np.int16), np.zeros((S, T, 80), np.uint8)
    br, bw = np.full((S, T), 64000, np.int32), np.full((S, T), 8000, np.int32)
    pptr = (C.c_void_p * K)(pcm.ctypes.data, pcm.ctypes.data + pcm.nbytes // 2)
    optr = (C.c_void_p * K)(out.ctypes.data, out.ctypes.data + out.nbytes // 2)

    def calls():
        return [L.lc3plus_enc_sharded_encode(h, pcm.ctypes.data, 16, None, None, T, out.ctypes.data, 80, None),
                L.lc3plus_enc_sharded_encode(h, pcm.ctypes.data, 16, None, br.ctypes.data, T, out.ctypes.data, 80, None),
                L.lc3plus_enc_sharded_encode(h, pcm.ctypes.data, 16, bw.ctypes.data, br.ctypes.data, T, out.ctypes.data, 80, None),
                L.lc3plus_enc_sharded_encode_device(h, pptr, 16, T, optr, 80, None, 1)]

    L.lc3stub_reset()
    assert L.lc3plus_enc_batch_set_frame_counts(sh1, 0x9000) == LC3_OK
    assert [(r.kind, r.ctx, r.p[0]) for r in _log(L)] == [(STUB_COUNTS, 1, 0x9000)]
    L.lc3stub_reset()
    assert calls() == [LC3_ERROR] * 4
    assert _log(L) == []                                                # shard 0, which has no counts, was not touched either
    assert L.lc3plus_enc_batch_set_frame_counts(sh1, None) == LC3_OK
    L.lc3stub_reset()
    assert calls() == [LC3_OK] * 4
    kinds = [r.kind for r in _log(L)]
    assert kinds.count(STUB_ENCODE) == 4 * K and set(kinds) <= {STUB_ENCODE, STUB_WAIT}
    assert L.lc3plus_enc_sharded_destroy(h) == 0
