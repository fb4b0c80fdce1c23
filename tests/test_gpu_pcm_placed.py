"""GPU tests of placed PCM (include/lc3plus_batch.h: lc3plus_{enc,dec}_batch_set_pcm_placement): frame (s, t) of a device-pointer call lies at an element
offset read from device memory.

Every comparison is exact.  The yardstick is the dense call of the same build on the gathered PCM (encoder) or scattered into the arena (decoder), and for
one case per geometry the CPU oracle.  The arenas, the gathers and the scatters are built here in numpy from the address rule as the header states it, never
with the library's host functions.  Each case runs as two consecutive calls of T frames (T = 4: the one-wave kernel, T = 64: the pipelined path).  Everything
is handled as bytes: an element is eb bytes, a frame channels * N elements."""
import ctypes as C
import functools

import numpy as np
import pytest

from lc3_harness import make_dec_case, oracle_decode_streams
from test_gpu_dec_varsize_device import _Hip
from test_gpu_pcm_format import _amd, _api, _oracle_bytes, _pcm16, _same
from test_gpu_pcm_wire import ALAW, DEPTH, G8, G8S, G16, G16S, G44, G48, G48ST, G96, S16BE, S24BE, S24LE, ULAW, _wire_input, to_native

pytestmark = pytest.mark.gpu

F32, IL, CM = 0x80, 0x100, 0x200
NATIVE = [16, 24, 32, F32]
WIRE = [S16BE, S24LE, S24BE, ULAW, ALAW]
TYPES = NATIVE + WIRE
EB = {16: 2, 24: 4, 32: 4, F32: 4, S16BE: 2, S24LE: 3, S24BE: 3, ULAW: 1, ALAW: 1}
GEOMS = [G8, G8S, G16, G16S, G44, G48, G48ST, G96]                      # those of tests/test_gpu_pcm_wire.py
TS = [4, 64]
CANARY = 0xA5
ENC_FL_PCM_PLACE, DEC_ST_PCM_PLACE = 16, 4
I64_MAX = 2 ** 63 - 1


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


def _upload(dev, ptr, arr):
    arr = np.ascontiguousarray(arr)
    assert dev.hip.hipMemcpy(C.c_void_p(ptr), C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), C.c_int(1)) == 0


# ---- input: elements as bytes [S, frames, C, N, eb], and the native array they stand for ----
def _input(ty, g, frames, seed, streams=3):
    if ty in WIRE:
        w, nat = _wire_input(ty, g, frames, seed, streams=streams)
        return w, nat
    x = _pcm16(g, frames, seed=seed, streams=streams)
    rng = np.random.default_rng(seed + 7)
    if ty == 24:
        x = (x.astype(np.int32) << 8) + rng.integers(0, 256, x.shape).astype(np.int32)
    elif ty == 32:
        x = (x.astype(np.int32) << 16) + rng.integers(0, 65536, x.shape).astype(np.int32)
    elif ty == F32:
        x = (x.astype(np.float32) + rng.integers(0, 256, x.shape).astype(np.float32) / 256.0) / np.float32(32768.0)
    x = np.ascontiguousarray(x)
    return x.view(np.uint8).reshape(x.shape + (x.dtype.itemsize,)), x


# ---- the address rule, restated: a frame's channels * N elements from its offset on, [C][N] with no layout bit, [N][C] interleaved ----
def _frame_flat(fr, lay):
    """fr [C, N, eb] -> bytes in placement order"""
    return np.ascontiguousarray(fr.transpose(1, 0, 2) if lay == IL else fr).reshape(-1)


def _scatter(arena, offs, xb, lay, cap):
    """writes every valid frame of xb [S, T, C, N, eb] into the byte arena at its offset (elements); returns the validity [S, T]"""
    S, T, Cn, N, eb = xb.shape
    fe = Cn * N
    ok = np.zeros((S, T), bool)
    for s in range(S):
        for t in range(T):
            o = int(offs[s, t])
            if 0 <= o and o + fe <= cap:
                arena[o * eb:(o + fe) * eb] = _frame_flat(xb[s, t], lay)
                ok[s, t] = True
    return ok


def _gather(arena, offs, lay, Cn, N, eb):
    S, T = offs.shape
    out = np.zeros((S, T, Cn, N, eb), np.uint8)
    for s in range(S):
        for t in range(T):
            o = int(offs[s, t])
            fr = arena[o * eb:(o + Cn * N) * eb]
            out[s, t] = fr.reshape(N, Cn, eb).transpose(1, 0, 2) if lay == IL else fr.reshape(Cn, N, eb)
    return out


def _inv(offs, cap, fe):
    """the validity rule, restated: 0 <= offset and offset + channels * N <= capacity"""
    return np.array([[not (0 <= int(o) and int(o) + fe <= cap) for o in row] for row in offs])


def _dense_offsets(S, T, fe):
    return (np.arange(S * T, dtype=np.int64) * fe).reshape(S, T)


def _ring_plan(S, T, fe, seed, k):
    """per-stream rings of R = T + 2 frames (R < 2 T: the first two calls wrap), random start positions, the ring bases of every second stream shifted by
    an odd number of elements -> (offsets [S, T] of call k, capacity in elements)"""
    api = _api()
    R = T + 2
    rng = np.random.default_rng(seed)
    starts = rng.integers(5, R, S)
    stride = R * fe + 8
    shift = np.array([0 if s % 2 == 0 else (1, 3, 5)[(s // 2) % 3] for s in range(S)], np.int64)
    offs = api.ring_offsets((starts + k * T) % R, T, R, fe, stride) + shift[:, None]
    for s in range(S):                                                  # restated: the helper is what the header says
        for t in range(T):
            assert offs[s, t] == s * stride + ((int(starts[s]) + k * T + t) % R) * fe + shift[s]
    assert k > 1 or all(int(starts[s] + k * T) % R + T > R for s in range(S)), "a call does not wrap"
    return offs, S * stride + 8


# ---- encoder runs ----
def _batch(g, S, rates=None):
    fs, ms, hr, ch, rate = g
    return _amd().Batch(S, fs, ch, ms, hr, rates if rates is not None else [rate] * S, device=0)


def _enc_dense(dev, g, xb, ty, T, rates=None, state=False):
    """xb [S, n T, C, N, eb] in consecutive dense device-pointer calls of T frames (default layout) -> bytes [S, n T, stride]"""
    S = xb.shape[0]
    bat = _batch(g, S, rates)
    try:
        stride, outs = bat.stride, []
        for k in range(xb.shape[1] // T):
            d_out = dev.zeros(S * T * stride)
            bat.encode_device(dev.put(xb[:, k * T:(k + 1) * T]), ty, T, d_out, stride, sync=True)
            outs.append(dev.get(d_out, (S, T, stride), np.uint8))
        got = np.concatenate(outs, axis=1)
        return (got, bat.get_state()) if state else got
    finally:
        bat.close()


def _enc_placed(dev, g, xb, ty, lay, T, plan, rates=None, state=False, base_shift=0):
    """the same frames through placed calls: plan(k) -> (offsets [S, T], capacity); one arena and one offsets array in device memory, rewritten between the
    calls as a server's capture would.  The arena is random bytes wherever no frame of the call lies.  base_shift: bytes the pcm pointer is off its allocation."""
    S, _, Cn, N, eb = xb.shape
    bat = _batch(g, S, rates)
    try:
        stride, outs = bat.stride, []
        cap0 = max(plan(k)[1] for k in range(xb.shape[1] // T))
        d_arena, d_offs = dev.zeros(base_shift + cap0 * eb + 64), dev.zeros(S * T * 8)
        rng = np.random.default_rng(99)
        for k in range(xb.shape[1] // T):
            offs, cap = plan(k)
            arena = rng.integers(0, 256, cap0 * eb + 64, dtype=np.uint8)
            if ty == F32:
                arena.view(np.float32)[:] = 0.25                        # (random bytes would be NaNs here and there: nothing reads them, but keep them plain)
            _scatter(arena, offs, xb[:, k * T:(k + 1) * T], lay, cap)
            _upload(dev, d_arena + base_shift, arena)
            _upload(dev, d_offs, offs.astype(np.int64))
            bat.set_pcm_placement(d_offs, cap)
            d_out = dev.zeros(S * T * stride)
            bat.encode_device(d_arena + base_shift, ty | lay, T, d_out, stride, sync=True)
            outs.append(dev.get(d_out, (S, T, stride), np.uint8))
        got = np.concatenate(outs, axis=1)
        return (got, bat.get_state()) if state else got
    finally:
        bat.close()


# ---- decoder runs ----
def _dec_dense(dev, g, frames, nbytes, bfi, T, ty, state=False):
    """-> (elements as bytes [S, n T, C, N, eb], status [S, n T]) of consecutive dense calls with sizes and flags in device memory"""
    fs, ms, hr, ch, rate = g
    S = frames.shape[0]
    d = _amd().DecBatch(S, fs, ch, ms, hr, nbytes, device=0)
    try:
        eb, out, sts = EB[ty], [], []
        nb = np.repeat(np.asarray(nbytes, np.int32)[:, None], T, axis=1)
        for k in range(frames.shape[1] // T):
            d_pcm, d_st = dev.zeros(S * T * ch * d.N * eb), dev.zeros(S * T)
            d.decode_device_sizes(dev.put(frames[:, k * T:(k + 1) * T]), frames.shape[2], T, d_pcm, dev.put(nb), dev.put(bfi[:, k * T:(k + 1) * T]), d_st, bps=ty, sync=True)
            out.append(dev.get(d_pcm, (S, T, ch, d.N, eb), np.uint8))
            sts.append(dev.get(d_st, (S, T), np.uint8))
        res = np.concatenate(out, axis=1), np.concatenate(sts, axis=1)
        return res + (d.get_state(),) if state else res
    finally:
        d.close()


def _dec_placed(dev, g, frames, nbytes, bfi, T, ty, lay, plan, guard=96, state=False):
    """placed calls into one arena pre-filled with the canary, guard bytes in front of and behind it -> per call (arena bytes, offsets, capacity, status), and
    the check that the guards are untouched"""
    fs, ms, hr, ch, rate = g
    S = frames.shape[0]
    d = _amd().DecBatch(S, fs, ch, ms, hr, nbytes, device=0)
    try:
        eb, res = EB[ty], []
        nb = np.repeat(np.asarray(nbytes, np.int32)[:, None], T, axis=1)
        for k in range(frames.shape[1] // T):
            offs, cap = plan(k)
            total = guard + cap * eb + guard
            d_buf, d_st, d_offs = dev.put(np.full(total, CANARY, np.uint8)), dev.zeros(S * T), dev.put(offs.astype(np.int64))
            d.set_pcm_placement(d_offs, cap)
            d.decode_device_sizes(dev.put(frames[:, k * T:(k + 1) * T]), frames.shape[2], T, d_buf + guard, dev.put(nb), dev.put(bfi[:, k * T:(k + 1) * T]), d_st, bps=ty | lay,
                                  sync=True)
            got = dev.get(d_buf, (total,), np.uint8)
            assert (got[:guard] == CANARY).all() and (got[guard + cap * eb:] == CANARY).all(), ("guard bytes were written", k)
            res.append((got[guard:guard + cap * eb], offs, cap, dev.get(d_st, (S, T), np.uint8)))
        return (res, d.get_state()) if state else res
    finally:
        d.close()


def _check_dec(res, want, T, lay, Cn, N, eb, invalid=None):
    """every valid frame of every call holds the dense call's elements; every other byte of the arena is still the canary"""
    for k, (arena, offs, cap, st) in enumerate(res):
        image = np.full(arena.size, CANARY, np.uint8)
        ok = _scatter(image, offs, want[:, k * T:(k + 1) * T], lay, cap)
        if invalid is not None:
            assert np.array_equal(~ok, invalid[:, k * T:(k + 1) * T])
        bad = np.flatnonzero(arena != image)
        assert bad.size == 0, ("call", k, "first differing bytes", bad[:6].tolist(), "of", arena.size)


@functools.lru_cache(maxsize=None)
def _dec_case(g, T, S=3, seed=23):
    """frames with loss and corruption (the CPU oracle encodes them: once per geometry and length)"""
    fs, ms, hr, ch, rate = g
    return make_dec_case(fs, ms, hr, ch, [rate] * S, 2 * T, seed=seed)


# the sample types and layouts of a geometry: with one channel the interleaved addresses are those of no layout, so mono geometries take it once (G48)
def _cross(types, geoms):
    return [pytest.param(ty, lay, g, id="%#x-%#x-%d-%g-%dch" % (ty, lay, g[0], g[1], g[3])) for g in geoms for lay in ((0, IL) if g[3] > 1 or g is G48 else (0,))
            for ty in types]


RING_ALL = [(16, 0), (16, IL), (F32, 0), (24, IL), (32, 0), (S24LE, 0), (S16BE, IL), (ULAW, 0), (ALAW, IL), (S24BE, 0)]
RING_FEW = [(16, 0), (F32, 0), (S24LE, 0), (ULAW, 0)]
RINGS = [pytest.param(ty, lay, g, id="%#x-%#x-%d-%g-%dch" % (ty, lay, g[0], g[1], g[3])) for g in GEOMS
         for ty, lay in (RING_ALL if g in (G48, G16S, G48ST) else RING_FEW)]


# ---- 1. identity ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("ty,lay,g", _cross(TYPES, GEOMS))
def test_encoder_dense_offsets_give_the_dense_bytes(dev, ty, lay, g, T):
    S = 3
    xb, nat = _input(ty, g, 2 * T, seed=61, streams=S)
    fe = xb.shape[2] * xb.shape[3]
    want = _enc_dense(dev, g, xb, ty, T)
    got = _enc_placed(dev, g, xb, ty, lay, T, lambda k: (_dense_offsets(S, T, fe), S * T * fe))
    _same(got, want, "the dense call")
    if ty in (16, ULAW) and lay == 0:                                  # one case per geometry (and a wire type) against the CPU oracle
        _same(got, _oracle_bytes(g, nat, DEPTH.get(ty, ty)), "oracle")


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("ty,lay,g", _cross(TYPES, GEOMS))
def test_decoder_dense_offsets_give_the_dense_pcm(dev, ty, lay, g, T):
    fs, ms, hr, ch, rate = g
    frames, nbytes, bfi = _dec_case(g, T)
    S = frames.shape[0]
    want, wst = _dec_dense(dev, g, frames, nbytes, bfi, T, ty)
    N, fe = want.shape[3], ch * want.shape[3]
    res = _dec_placed(dev, g, frames, nbytes, bfi, T, ty, lay, lambda k: (_dense_offsets(S, T, fe), S * T * fe))
    _check_dec(res, want, T, lay, ch, N, EB[ty])
    assert np.array_equal(np.concatenate([r[3] for r in res], axis=1), wst)
    if ty == 16 and lay == 0:
        o, ost = oracle_decode_streams(frames, nbytes, bfi, fs, ms, hr, ch, bps=16)
        assert np.array_equal(want.view(np.int16)[..., 0], o) and np.array_equal(wst, ost)


# ---- 2. rings -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("ty,lay,g", RINGS)
def test_encoder_reads_rings_that_wrap(dev, ty, lay, g, T):
    S = 4
    xb, nat = _input(ty, g, 2 * T, seed=63, streams=S)
    fe = xb.shape[2] * xb.shape[3]
    want = _enc_dense(dev, g, xb, ty, T)
    got = _enc_placed(dev, g, xb, ty, lay, T, lambda k: _ring_plan(S, T, fe, 7, k))
    _same(got, want, "the dense call on the gathered PCM")
    if ty == 16 and lay == 0:
        _same(got, _oracle_bytes(g, nat, 16), "oracle")


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("ty,lay,g", RINGS)
def test_decoder_writes_rings_that_wrap_and_nothing_else(dev, ty, lay, g, T):
    fs, ms, hr, ch, rate = g
    frames, nbytes, bfi = _dec_case(g, T, S=4, seed=25)
    want, wst = _dec_dense(dev, g, frames, nbytes, bfi, T, ty)
    N = want.shape[3]
    res = _dec_placed(dev, g, frames, nbytes, bfi, T, ty, lay, lambda k: _ring_plan(4, T, ch * N, 9, k))
    _check_dec(res, want, T, lay, ch, N, EB[ty])
    assert np.array_equal(np.concatenate([r[3] for r in res], axis=1), wst)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("ty", [16, F32, ULAW])
def test_pcm_pointer_off_its_alignment_with_even_offsets(dev, ty, T):
    """aligned element offsets from a pointer that is not: the wide-or-not choice is made from the byte address"""
    g, S = G48, 3
    xb, _ = _input(ty, g, 2 * T, seed=65, streams=S)
    fe = xb.shape[2] * xb.shape[3]
    want = _enc_dense(dev, g, xb, ty, T)
    got = _enc_placed(dev, g, xb, ty, 0, T, lambda k: (_dense_offsets(S, T, fe), S * T * fe), base_shift=EB[ty])
    _same(got, want, "the dense call")


# ---- 3. simulcast ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g,rates", [(G48, [32000, 64000, 128000]), (G16S, [48000, 64000, 96000]), (G96, [200000, 256000, 400000]), (G8, [24000, 32000, 64000])])
def test_simulcast_three_rates_share_one_row_of_offsets(dev, g, rates, T):
    xb1, _ = _input(16, g, 2 * T, seed=67, streams=1)
    xb = np.repeat(xb1, 3, axis=0)                                      # the dense call's copies
    fe = xb.shape[2] * xb.shape[3]
    want = _enc_dense(dev, g, xb, 16, T, rates=rates)
    row = (np.arange(T, dtype=np.int64) * fe + 3)[None, :]
    got = _enc_placed(dev, g, xb, 16, 0, T, lambda k: (np.repeat(row, 3, axis=0), T * fe + 3), rates=rates)
    _same(got, want, "three dense streams on copied PCM")
    assert not np.array_equal(got[0], got[1])


def test_hop_shorter_than_a_frame(dev):
    """input frames may overlap: every stream reads windows that advance by half a frame"""
    g, T, S = G16, 8, 3
    xb1, _ = _input(16, g, 2 * T + 1, seed=69, streams=1)
    sig = xb1.reshape(-1, 2)                                            # one signal, as bytes per sample
    N = xb1.shape[3]
    hop = N // 2
    win = np.stack([sig[(s + t) * hop:(s + t) * hop + N] for s in range(S) for t in range(2 * T)]).reshape(S, 2 * T, 1, N, 2)
    want = _enc_dense(dev, g, win, 16, T)
    bat = _batch(g, S)
    try:
        d_sig, outs = dev.put(sig), []
        for k in range(2):
            offs = np.array([[(s + k * T + t) * hop for t in range(T)] for s in range(S)], np.int64)
            bat.set_pcm_placement(dev.put(offs), sig.shape[0])
            d_out = dev.zeros(S * T * bat.stride)
            bat.encode_device(d_sig, 16, T, d_out, bat.stride, sync=True)
            outs.append(dev.get(d_out, (S, T, bat.stride), np.uint8))
    finally:
        bat.close()
    _same(np.concatenate(outs, axis=1), want, "the dense call on the copied windows")


# ---- 4. invalid offsets ---------------------------------------------------------------------------------------------------------------------------

def _invalid_plan(S, T, fe, k):
    """dense offsets with a negative one, one ending an element past the capacity and INT64_MAX, in first, middle and last frames"""
    offs = _dense_offsets(S, T, fe)
    cap = S * T * fe
    bad = {(0, 0): -1, (1, T // 2): cap - fe + 1, (2, T - 1): I64_MAX, (1, 0): -fe, (0, T - 1): cap, (2, T // 2): -I64_MAX - 1} if k == 0 else \
          {(0, T // 2): I64_MAX, (1, T - 1): -1, (2, 0): cap - fe + 1}
    for (s, t), v in bad.items():
        offs[s, t] = v
    return offs, cap


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g", [G48, G16S, G96, G8S, G44])
@pytest.mark.parametrize("ty,lay", [(16, 0), (F32, IL), (S24LE, 0)])
def test_encoder_takes_silence_for_invalid_frames_and_flags_them(dev, ty, lay, g, T):
    S = 3
    fs, ms, hr, ch, rate = g
    xb, _ = _input(ty, g, 2 * T, seed=71, streams=S)
    fe = xb.shape[2] * xb.shape[3]
    inv = np.concatenate([_inv(*_invalid_plan(S, T, fe, k), fe) for k in range(2)], axis=1)
    assert inv.sum() == 9 and inv[:, 0].any() and inv[:, T - 1].any() and inv[:, T // 2].any()
    zeroed = xb.copy()
    zeroed[inv] = 0                                                     # the zero of these sample types is all-zero bytes (G.711: the test below)
    want = _enc_dense(dev, g, zeroed, ty, T)
    # through encode_rates_device, which reports flags: constant rates, so the bytes are those of encode()
    bat = _batch(g, S)
    try:
        stride, outs, flags = bat.stride, [], []
        for k in range(2):
            offs, cap = _invalid_plan(S, T, fe, k)
            guard = 4096
            arena = np.full(guard + cap * EB[ty] + guard, 0x5A, np.uint8)
            body = arena[guard:guard + cap * EB[ty]]
            _scatter(body, offs, xb[:, k * T:(k + 1) * T], lay, cap)
            d_arena = dev.put(arena)
            bat.set_pcm_placement(dev.put(offs), cap)
            d_out, d_fl, d_nb = dev.zeros(S * T * stride), dev.put(np.full((S, T), 0xEE, np.uint8)), dev.zeros(S * T * 4)
            bat.encode_device_rates(d_arena + guard, ty | lay, T, d_out, stride, d_bitrates_ptr=dev.put(np.full((S, T), rate, np.int32)), d_num_bytes_ptr=d_nb,
                                    d_flags_ptr=d_fl, sync=True)
            outs.append(dev.get(d_out, (S, T, stride), np.uint8))
            flags.append(dev.get(d_fl, (S, T), np.uint8))
            assert np.array_equal(dev.get(d_arena, arena.shape, np.uint8), arena), "the encoder wrote into the PCM buffer or its guards"
    finally:
        bat.close()
    _same(np.concatenate(outs, axis=1), want, "the dense call with those frames zeroed")
    assert np.array_equal(np.concatenate(flags, axis=1), np.where(inv, ENC_FL_PCM_PLACE, 0).astype(np.uint8))


@pytest.mark.parametrize("T", TS)
def test_encoder_invalid_g711_frames_are_silence_not_code_zero(dev, T):
    """mu-law: silence is the sample 0, not the byte 0 (which expands to -32124)"""
    g, S, ty = G16, 3, ULAW
    xb, nat = _input(ty, g, 2 * T, seed=73, streams=S)
    fe = xb.shape[2] * xb.shape[3]
    inv = np.concatenate([_inv(*_invalid_plan(S, T, fe, k), fe) for k in range(2)], axis=1)
    z = nat.copy()
    z[inv] = 0
    z = np.ascontiguousarray(z)
    want = _enc_dense(dev, g, z.view(np.uint8).reshape(z.shape + (2,)), 16, T)
    got = _enc_placed(dev, g, xb, ty, 0, T, lambda k: _invalid_plan(S, T, fe, k))
    _same(got, want, "the int16 call with those frames zeroed")


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g", [G48, G16S, G96, G8S, G44])
@pytest.mark.parametrize("ty,lay", [(16, 0), (F32, IL), (S24LE, 0), (ULAW, IL)])
def test_decoder_skips_invalid_frames_and_reports_them(dev, ty, lay, g, T):
    fs, ms, hr, ch, rate = g
    frames, nbytes, bfi = _dec_case(g, T, seed=27)
    S = frames.shape[0]
    want, wst = _dec_dense(dev, g, frames, nbytes, bfi, T, ty)
    N, fe = want.shape[3], ch * want.shape[3]
    res = _dec_placed(dev, g, frames, nbytes, bfi, T, ty, lay, lambda k: _invalid_plan(S, T, fe, k), guard=4096)
    inv = np.concatenate([_inv(*_invalid_plan(S, T, fe, k), fe) for k in range(2)], axis=1)
    _check_dec(res, want, T, lay, ch, N, EB[ty], invalid=inv)          # later frames of those streams equal the dense call's: the streams advanced
    st = np.concatenate([r[3] for r in res], axis=1)
    assert np.array_equal(st, wst | np.where(inv, DEC_ST_PCM_PLACE, 0).astype(np.uint8))


def test_host_status_keeps_its_meaning_and_capacity_zero_writes_nothing(dev):
    """decode() with device pointers and no device status: nothing reports the invalid frames; capacity 0 makes every frame invalid"""
    g, T, S = G16S, 8, 3
    fs, ms, hr, ch, rate = g
    frames, nbytes, bfi = _dec_case(g, T, seed=29)
    bfi0 = np.zeros_like(bfi)
    want, _ = _dec_dense(dev, g, frames, nbytes, bfi0, T, 16)
    N = want.shape[3]
    d = _amd().DecBatch(S, fs, ch, ms, hr, nbytes, device=0)
    try:
        n = S * T * ch * N * 2
        d_buf = dev.put(np.full(n, CANARY, np.uint8))
        d.set_pcm_placement(dev.put(_dense_offsets(S, T, ch * N)), 0)
        d.decode_device(dev.put(frames[:, :T]), frames.shape[2], T, d_buf, bps=16, sync=True)
        assert (dev.get(d_buf, (n,), np.uint8) == CANARY).all()
        d.set_pcm_placement(None)
        d.decode_device(dev.put(frames[:, T:]), frames.shape[2], T, d_buf, bps=16, sync=True)
        assert np.array_equal(dev.get(d_buf, (S, T, ch, N, 2), np.uint8), want[:, T:]), "the streams did not advance through the unwritten call"
    finally:
        d.close()


# ---- 5. with the other features -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [8, 64])
@pytest.mark.parametrize("packed", [False, True])
def test_device_rates_and_bandwidths_and_packed_output_from_rings(dev, packed, T):
    g, S, ty, lay = G16S, 4, 16, IL
    fs, ms, hr, ch, rate = g
    xb, _ = _input(ty, g, 2 * T, seed=75, streams=S)
    fe = xb.shape[2] * xb.shape[3]
    rng = np.random.default_rng(3)
    rates = rng.choice([32000, 48000, 64000, 96000, 128000, 5], size=(S, 2 * T)).astype(np.int32)      # 5: refused, flagged, the carried rate stays
    bws = rng.choice([0, 4000, 8000], size=(S, 2 * T)).astype(np.int32)
    res = {}
    for name in ("dense", "placed"):
        bat = _batch(g, S)
        try:
            parts, stride, cap_out = [], 400, S * T * 400
            for k in range(2):
                part = xb[:, k * T:(k + 1) * T]
                if name == "dense":
                    d_pcm, word = dev.put(part), ty
                    bat.set_pcm_placement(None)
                else:
                    offs, cap = _ring_plan(S, T, fe, 11, k)
                    arena = np.zeros(cap * 2, np.uint8)
                    _scatter(arena, offs, part, lay, cap)
                    d_pcm, word = dev.put(arena), ty | lay
                    bat.set_pcm_placement(dev.put(offs), cap)
                d_r, d_b = dev.put(rates[:, k * T:(k + 1) * T]), dev.put(bws[:, k * T:(k + 1) * T])
                d_nb, d_fl = dev.zeros(S * T * 4), dev.zeros(S * T)
                if packed:
                    d_out, d_off, d_tot = dev.zeros(cap_out), dev.zeros(S * T * 8), dev.zeros(8)
                    bat.encode_device_packed(d_pcm, word, T, d_out, cap_out, 0, d_bitrates_ptr=d_r, d_bandwidths_ptr=d_b, d_offsets_ptr=d_off, d_total_ptr=d_tot,
                                             d_num_bytes_ptr=d_nb, d_flags_ptr=d_fl, sync=True)
                    parts.append((dev.get(d_out, (cap_out,), np.uint8), dev.get(d_off, (S, T), np.int64), dev.get(d_tot, (1,), np.int64),
                                  dev.get(d_nb, (S, T), np.int32), dev.get(d_fl, (S, T), np.uint8)))
                else:
                    d_out = dev.zeros(S * T * stride)
                    bat.encode_device_rates(d_pcm, word, T, d_out, stride, d_bitrates_ptr=d_r, d_bandwidths_ptr=d_b, d_num_bytes_ptr=d_nb, d_flags_ptr=d_fl, sync=True)
                    parts.append((dev.get(d_out, (S, T, stride), np.uint8), dev.get(d_nb, (S, T), np.int32), dev.get(d_fl, (S, T), np.uint8)))
            res[name] = parts
        finally:
            bat.close()
    for k in range(2):
        for i, (a, b) in enumerate(zip(res["dense"][k], res["placed"][k])):
            assert np.array_equal(a, b), (k, i)
        assert res["dense"][k][-1].any() and not (res["placed"][k][-1] & ENC_FL_PCM_PLACE).any()


def test_packed_output_without_rates_flags_invalid_frames(dev):
    g, S, T, ty = G48, 3, 8, 16
    xb, _ = _input(ty, g, T, seed=77, streams=S)
    fe = xb.shape[2] * xb.shape[3]
    offs, cap = _invalid_plan(S, T, fe, 0)
    inv = _inv(offs, cap, fe)
    zeroed = xb.copy()
    zeroed[inv] = 0
    out = {}
    for name in ("dense", "placed"):
        bat = _batch(g, S)
        try:
            cap_out = S * T * bat.stride
            arena = np.zeros(cap * 2, np.uint8)
            _scatter(arena, offs, xb, 0, cap)
            if name == "placed":
                bat.set_pcm_placement(dev.put(offs), cap)
            d_out, d_off, d_fl = dev.zeros(cap_out), dev.zeros(S * T * 8), dev.put(np.full((S, T), 0xEE, np.uint8))
            bat.encode_device_packed(dev.put(arena if name == "placed" else zeroed), ty, T, d_out, cap_out, 0, d_offsets_ptr=d_off, d_flags_ptr=d_fl, sync=True)
            out[name] = (dev.get(d_out, (cap_out,), np.uint8), dev.get(d_off, (S, T), np.int64), dev.get(d_fl, (S, T), np.uint8))
        finally:
            bat.close()
    assert np.array_equal(out["dense"][0], out["placed"][0]) and np.array_equal(out["dense"][1], out["placed"][1])
    assert not out["dense"][2].any() and np.array_equal(out["placed"][2], np.where(inv, ENC_FL_PCM_PLACE, 0).astype(np.uint8))


@pytest.mark.parametrize("T", [8, 64])
def test_decode_packed_into_rings(dev, T):
    g, ty, lay = G16S, F32, 0
    fs, ms, hr, ch, rate = g
    frames, nbytes, bfi = _dec_case(g, T, S=4, seed=31)
    S = frames.shape[0]
    want, wst = _dec_dense(dev, g, frames, nbytes, bfi, T, ty)
    N, fe, eb = want.shape[3], ch * want.shape[3], 4
    nbf = int(nbytes[0])
    d = _amd().DecBatch(S, fs, ch, ms, hr, nbytes, device=0)
    try:
        res = []
        for k in range(2):
            fr = frames[:, k * T:(k + 1) * T]
            order = np.random.default_rng(k).permutation(S * T)
            fo = np.zeros(S * T, np.int64)
            fo[order] = np.arange(S * T) * (nbf + 3) + 1              # any offsets: odd, out of order, with gaps
            packed = np.zeros(S * T * (nbf + 3) + 8, np.uint8)
            for i in range(S * T):
                packed[fo[i]:fo[i] + nbf] = fr.reshape(S * T, -1)[i, :nbf]
            offs, cap = _ring_plan(S, T, fe, 13, k)
            total = 64 + cap * eb + 64
            d_buf, d_st = dev.put(np.full(total, CANARY, np.uint8)), dev.zeros(S * T)
            d.set_pcm_placement(dev.put(offs), cap)
            d.decode_device_packed(dev.put(packed), packed.size, dev.put(fo.reshape(S, T)), T, d_buf + 64, dev.put(np.full((S, T), nbf, np.int32)), nbf,
                                   d_bfi_ptr=dev.put(bfi[:, k * T:(k + 1) * T]), d_status_ptr=d_st, bps=ty | lay, sync=True)
            got = dev.get(d_buf, (total,), np.uint8)
            assert (got[:64] == CANARY).all() and (got[64 + cap * eb:] == CANARY).all()
            res.append((got[64:64 + cap * eb], offs, cap, dev.get(d_st, (S, T), np.uint8)))
    finally:
        d.close()
    _check_dec(res, want, T, lay, ch, N, eb)
    assert np.array_equal(np.concatenate([r[3] for r in res], axis=1), wst)


@pytest.mark.parametrize("g,T", [(G48, 16), (G48, 6), (G16S, 16), (G96, 12)])
def test_three_calls_in_flight_under_the_input_ready_promise(dev, g, T):
    """K calls queued on one stream without a wait, each with its own arena and offsets (the promise covers both) = one continuous dense encode; then the
    decoder the same way"""
    S, K, ty = 64, 4, 16
    fs, ms, hr, ch, rate = g
    xb, _ = _input(ty, g, K * T, seed=79, streams=S)
    fe = xb.shape[2] * xb.shape[3]
    want = _enc_dense(dev, g, xb, ty, T)
    bat = _batch(g, S)
    s = dev.stream()
    try:
        bat.set_input_ready(True)
        stride, outs = bat.stride, []
        for k in range(K):
            offs, cap = _ring_plan(S, T, fe, 15, k)
            arena = np.zeros(cap * 2, np.uint8)
            _scatter(arena, offs, xb[:, k * T:(k + 1) * T], 0, cap)
            d_out = dev.zeros(S * T * stride)
            bat.set_pcm_placement(dev.put(offs), cap)
            bat.encode_device(dev.put(arena), ty, T, d_out, stride, hip_stream=s, sync=False)
            outs.append(d_out)
        dev.stream_sync(s)
        got = np.concatenate([dev.get(o, (S, T, stride), np.uint8) for o in outs], axis=1)
    finally:
        bat.close()
    _same(got, want, "the continuous dense encode")
    fr = np.ascontiguousarray(want)                                     # the decoder on the same frames
    nbytes = [fr.shape[2]] * S
    dd, dp = _amd().DecBatch(S, fs, ch, ms, hr, nbytes, device=0), _amd().DecBatch(S, fs, ch, ms, hr, nbytes, device=0)
    try:
        N = dd.N
        dp.set_input_ready(True)
        bufs = []
        for k in range(K):
            offs, cap = _ring_plan(S, T, ch * N, 17, k)
            d_buf = dev.put(np.full(cap * 2, CANARY, np.uint8))
            dp.set_pcm_placement(dev.put(offs), cap)
            dp.decode_device(dev.put(fr[:, k * T:(k + 1) * T]), fr.shape[2], T, d_buf, bps=16, hip_stream=s, sync=False)
            bufs.append((d_buf, offs, cap))
        dev.stream_sync(s)
        for k, (d_buf, offs, cap) in enumerate(bufs):
            d_pcm = dev.zeros(S * T * ch * N * 2)
            dd.decode_device(dev.put(fr[:, k * T:(k + 1) * T]), fr.shape[2], T, d_pcm, bps=16, sync=True)
            dense = dev.get(d_pcm, (S, T, ch, N, 2), np.uint8)
            image = np.full(cap * 2, CANARY, np.uint8)
            _scatter(image, offs, dense, 0, cap)
            assert np.array_equal(dev.get(d_buf, (cap * 2,), np.uint8), image), k
    finally:
        dd.close()
        dp.close()


@pytest.mark.parametrize("T", TS)
def test_reset_streams_between_placed_calls(dev, T):
    g, S, ty = G48, 4, 16
    xb, _ = _input(ty, g, 2 * T, seed=81, streams=S)
    fe = xb.shape[2] * xb.shape[3]
    res = {}
    for name in ("dense", "placed"):
        bat = _batch(g, S)
        try:
            outs = []
            for k in range(2):
                part = xb[:, k * T:(k + 1) * T]
                if name == "placed":
                    offs, cap = _ring_plan(S, T, fe, 19, k)
                    arena = np.zeros(cap * 2, np.uint8)
                    _scatter(arena, offs, part, 0, cap)
                    bat.set_pcm_placement(dev.put(offs), cap)
                    d_pcm = dev.put(arena)
                else:
                    d_pcm = dev.put(part)
                d_out = dev.zeros(S * T * bat.stride)
                bat.encode_device(d_pcm, ty, T, d_out, bat.stride, sync=True)
                outs.append(dev.get(d_out, (S, T, bat.stride), np.uint8))
                if k == 0:
                    bat.reset_streams([1, 3])
            res[name] = (np.concatenate(outs, axis=1), bat.get_state())
        finally:
            bat.close()
    _same(res["placed"][0], res["dense"][0], "the dense calls with the same reset")
    assert np.array_equal(res["placed"][1], res["dense"][1])
    fresh = _enc_dense(dev, g, xb[:, T:], ty, T)
    assert np.array_equal(res["placed"][0][1, T:], fresh[1]) and not np.array_equal(res["placed"][0][0, T:], fresh[0])


@pytest.mark.parametrize("T", TS)
def test_sharded_batch_on_one_device_twice(dev, T):
    """devices {0, 0}: each shard gets its placement through the borrowed handle, with offsets for its own block of streams into an arena of its own"""
    amd = _amd()
    g, S, ty = G16S, 5, 16
    fs, ms, hr, ch, rate = g
    xb, _ = _input(ty, g, 2 * T, seed=83, streams=S)
    fe = xb.shape[2] * xb.shape[3]
    want = _enc_dense(dev, g, xb, ty, T)
    sb = amd.ShardedBatch(S, fs, ch, ms, hr, [rate] * S, [0, 0])
    try:
        stride, outs = sb.stride, []
        blocks = [_api().shard_block(S, 2, i) for i in range(2)]
        for k in range(2):
            pcm_ptrs, out_ptrs = [], []
            for i, (first, count) in enumerate(blocks):
                offs, cap = _ring_plan(count, T, fe, 21 + i, k)
                arena = np.zeros(cap * 2, np.uint8)
                _scatter(arena, offs, xb[first:first + count, k * T:(k + 1) * T], IL, cap)
                sb.shard(i).set_pcm_placement(dev.put(offs), cap)
                pcm_ptrs.append(dev.put(arena))
                out_ptrs.append(dev.zeros(count * T * stride))
            sb.encode_device(pcm_ptrs, ty | IL, T, out_ptrs, stride, sync=True)
            outs.append(np.concatenate([dev.get(p, (c, T, stride), np.uint8) for p, (_, c) in zip(out_ptrs, blocks)], axis=0))
    finally:
        sb.close()
    _same(np.concatenate(outs, axis=1), want, "the unsharded dense call")


# ---- 6. state -------------------------------------------------------------------------------------------------------------------------------------

def _enc_state_rows(state, g, N, ncs):
    """get_state's bytes as words [channel-stream][LC3D_STATE_WORDS], with the words in front of the MDCT memory set to 0.

    The MDCT / resampler memory is the last N - la_zeros samples of the previous frame, right-aligned in a slot of 300 words (600 in the large layout:
    csrc/lc3_plan.h, LC3D_ST_XPREV).  No kernel reads the slot's words in front of it.  A pipelined call of any kind, dense or placed, hands the slot over from
    the LDS of the front kernel's last wave, which fills only the memory itself: where N - la_zeros is less than the slot, the words in front are what that LDS
    held before, and differ from run to run of one and the same dense call.  They are no state, so they are left out of the comparison here; every other word
    is compared, and the test goes on to show that two batches which take the two states encode alike."""
    fs, ms, hr, ch, rate = g
    la = {10.0: 3 * N // 8, 5.0: N // 4, 2.5: 0}[ms]                    # la_zeros of the frame length (csrc/lc3_tables.h: lc3t_cfg)
    ml = N - la
    mc = 600 if N > 480 or ml > 300 else 300                            # LC3D_LAYOUT_BIG
    rows = state.view(np.uint32).reshape(ncs, mc + 660).copy()          # LC3D_STATE_WORDS
    rows[:, :mc - ml] = 0
    return rows


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g", [G48, G16S, G96, G8S])
def test_two_placed_calls_equal_one_dense_call_and_leave_its_state(dev, g, T):
    S, ty = 3, 16
    fs, ms, hr, ch, rate = g
    xb, _ = _input(ty, g, 2 * T, seed=85, streams=S)
    N, fe = xb.shape[3], xb.shape[2] * xb.shape[3]
    want, wstate = _enc_dense(dev, g, xb, ty, 2 * T, state=True)
    got, gstate = _enc_placed(dev, g, xb, ty, 0, T, lambda k: _ring_plan(S, T, fe, 23, k), state=True)
    _same(got, want, "one dense call of 2 T frames")
    assert gstate.size == wstate.size
    assert np.array_equal(_enc_state_rows(gstate, g, N, S * ch), _enc_state_rows(wstate, g, N, S * ch)), "get_state after the placed calls differs from the dense call's"
    cont = []                                                           # the two states, whole, carry on alike
    for st in (wstate, gstate):
        bat = _batch(g, S)
        try:
            bat.set_state(st)
            d_out = dev.zeros(S * T * bat.stride)
            bat.encode_device(dev.put(xb[:, :T]), ty, T, d_out, bat.stride, sync=True)
            cont.append(dev.get(d_out, (S, T, bat.stride), np.uint8))
        finally:
            bat.close()
    _same(cont[1], cont[0], "the batch that took the dense call's state")
    frames, nbytes, bfi = _dec_case(g, T, seed=33)
    dense, dst, dstate = _dec_dense(dev, g, frames, nbytes, bfi, 2 * T, ty, state=True)
    N = dense.shape[3]
    res, pstate = _dec_placed(dev, g, frames, nbytes, bfi, T, ty, 0, lambda k: _ring_plan(S, T, ch * N, 25, k), state=True)
    _check_dec(res, dense, T, 0, ch, N, 2)
    assert np.array_equal(pstate, dstate), "get_state after the placed decodes differs from the dense call's"


# ---- refusals on the device build -------------------------------------------------------------------------------------------------------------------

def test_refused_calls_leave_the_batch_unchanged(dev):
    api = _api()
    g, T, S = G16S, 4, 2
    fs, ms, hr, ch, rate = g
    x = _pcm16(g, 2 * T, seed=87, streams=S)
    fresh, bat = _batch(g, S), _batch(g, S)
    try:
        assert np.array_equal(bat.encode(x[:, :T]), fresh.encode(x[:, :T]))
        bat.set_pcm_placement(dev.put(_dense_offsets(S, T, ch * x.shape[3])), S * T * ch * x.shape[3])
        for call in (lambda: bat.encode(x[:, T:]), lambda: bat.encode_traced(x[:, T:]),
                     lambda: bat.encode_device(dev.put(x[:, T:]), 16 | CM, T, dev.zeros(S * T * bat.stride), bat.stride, sync=True)):
            with pytest.raises(api.LC3Error) as e:
                call()
            assert e.value.code == 1
        with pytest.raises(api.LC3Error) as e:
            bat.set_pcm_placement(dev.put(np.zeros(4, np.int64)), -1)
        assert e.value.code == 1
        bat.set_pcm_placement(None)
        assert np.array_equal(bat.encode(x[:, T:]), fresh.encode(x[:, T:])), "a refused call moved the stream's state"
    finally:
        bat.close()
        fresh.close()
