"""GPU tests of the wire sample types of the PCM format word (include/lc3plus_batch.h: LC3PLUS_PCM_S16_BE, _S24_3LE, _S24_3BE, _ULAW, _ALAW).

Every comparison is exact.  Encoder: a call in a wire type gives the bytes of the same call on the converted int16 / int32 array, and the CPU oracle's.
Decoder: the output is the rule - bytes swapped, saturated to 24 bits, G.711 compressed - applied to the 16- or 24-bit output of the same frames, and to
the oracle's.  The expectations are built here in numpy from a restatement of the rule and from tests/golden/g711_tables.npz, never with the library's
host functions.  Each case runs as two consecutive calls of T frames (T = 4: the one-wave kernel, T = 64: the pipelined path)."""
import os

import numpy as np
import pytest

from lc3_harness import Oracle, make_dec_case, oracle_decode_streams
from test_gpu_dec_varsize_device import _Hip
from test_gpu_pcm_format import _amd, _api, _from_layout, _oracle_bytes, _pcm16, _same, _to_layout

pytestmark = pytest.mark.gpu

S16BE, S24LE, S24BE, ULAW, ALAW = 0x81, 0x82, 0x83, 0x84, 0x85
TYPES = [S16BE, S24LE, S24BE, ULAW, ALAW]
ELEM = {S16BE: 2, S24LE: 3, S24BE: 3, ULAW: 1, ALAW: 1}
DEPTH = {S16BE: 16, S24LE: 24, S24BE: 24, ULAW: 16, ALAW: 16}       # the integer format a type stands for
IL, CM = 0x100, 0x200
# fs, frame_ms, hrmode, channels, total bitrate per stream
G8 = (8000, 10.0, 0, 1, 32000)
G8S = (8000, 2.5, 0, 1, 64000)            # N = 20: a frame of 20 / 40 / 60 bytes, no whole 16-byte piece fits
G16 = (16000, 10.0, 0, 1, 32000)
G48 = (48000, 10.0, 0, 1, 64000)
G16S = (16000, 10.0, 0, 2, 64000)
G48ST = (48000, 10.0, 0, 2, 128000)
G96 = (96000, 10.0, 1, 1, 256000)
G44 = (44100, 10.0, 0, 1, 64000)
TS = [4, 64]
B = 3
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g711_tables.npz"))


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


# ---- the rule in numpy: native [..] <-> wire bytes [.., elem_bytes] ----
def to_wire(ty, v):
    """what the decoder writes for the integer output v (int16, or int32 at 24 bits), as uint8 [..., elem_bytes]"""
    v = np.asarray(v)
    if ty in (ULAW, ALAW):
        return GOLD["ulaw_compress" if ty == ULAW else "alaw_compress"][v.astype(np.int64) + 32768][..., None]
    if ty == S16BE:
        u = v.astype(np.int64) & 0xFFFF
        return np.stack([u >> 8, u & 0xFF], axis=-1).astype(np.uint8)
    u = np.clip(v.astype(np.int64), -8388608, 8388607) & 0xFFFFFF
    b = np.stack([u & 0xFF, (u >> 8) & 0xFF, u >> 16], axis=-1).astype(np.uint8)
    return b[..., ::-1].copy() if ty == S24BE else b


def to_native(ty, w):
    """the integer a wire element stands for: w uint8 [..., elem_bytes] -> int16 / int32 [...]"""
    w = np.asarray(w, np.int64)
    if ty in (ULAW, ALAW):
        return GOLD["ulaw_expand" if ty == ULAW else "alaw_expand"][w[..., 0]]
    if ty == S16BE:
        u = (w[..., 0] << 8) | w[..., 1]
        return np.where(u >= 1 << 15, u - (1 << 16), u).astype(np.int16)
    if ty == S24BE:
        w = w[..., ::-1]
    u = w[..., 0] | (w[..., 1] << 8) | (w[..., 2] << 16)
    return np.where(u >= 1 << 23, u - (1 << 24), u).astype(np.int32)


def _wire_input(ty, g, frames, seed, streams=B):
    """(wire uint8 [S, frames, C, N, eb], native [S, frames, C, N]): G.711 input that uses all 256 codes, random 24-bit PCM for the packed types"""
    x = _pcm16(g, frames, seed=seed, streams=streams)
    if ty in (ULAW, ALAW):
        codes = GOLD["ulaw_compress" if ty == ULAW else "alaw_compress"][x.astype(np.int64) + 32768]
        flat = codes.reshape(-1)
        flat[5:5 + 256] = np.arange(256, dtype=np.uint8)              # (a frame is at least 20 samples: the codes cross frames and streams of every case)
        assert np.unique(codes).size == 256
        w = codes[..., None]
    elif ty == S16BE:
        w = to_wire(ty, x)
    else:
        rng = np.random.default_rng(seed + 100)
        i24 = (x.astype(np.int32) << 8) + rng.integers(0, 256, x.shape).astype(np.int32)
        w = to_wire(ty, i24)
    nat = to_native(ty, w)
    assert np.array_equal(to_wire(ty, nat), w) or ty == ULAW             # (mu-law code 0x7f, negative zero, does not come back)
    return np.ascontiguousarray(w), np.ascontiguousarray(nat)


def _lay5(w, lay):
    """wire bytes [S, T, C, N, eb] in the default layout -> the bytes of layout bit lay, flat"""
    S, T, Cn, N, eb = w.shape
    if lay == IL:
        w = w.transpose(0, 1, 3, 2, 4)
    elif lay == CM:
        w = w.transpose(0, 2, 1, 3, 4)
    return np.ascontiguousarray(w).reshape(-1)


def _unlay5(flat, lay, S, T, Cn, N, eb):
    if lay == IL:
        return flat.reshape(S, T, N, Cn, eb).transpose(0, 1, 3, 2, 4)
    if lay == CM:
        return flat.reshape(S, Cn, T, N, eb).transpose(0, 2, 1, 3, 4)
    return flat.reshape(S, T, Cn, N, eb)


def _encode_device(dev, g, arr, word, T, pad_bytes=0, wire=False):
    """arr [S, 2 T, C, N(, eb)] in two consecutive device-pointer calls of T frames in format word -> bytes [S, 2 T, stride]; pad_bytes shifts the device
    pointer off its allocation boundary"""
    fs, ms, hr, ch, rate = g
    S, lay = arr.shape[0], word & 0x300
    bat = _amd().Batch(S, fs, ch, ms, hr, [rate] * S, device=0)
    try:
        stride = bat.stride
        outs = []
        for k in range(2):
            part = arr[:, k * T:(k + 1) * T]
            body = _lay5(part, lay) if wire else _to_layout(part, lay).view(np.uint8).ravel()
            d_pcm = dev.put(np.concatenate([np.zeros(pad_bytes, np.uint8), body])) + pad_bytes
            d_out = dev.zeros(S * T * stride)
            bat.encode_device(d_pcm, word, T, d_out, stride, sync=True)
            outs.append(dev.get(d_out, (S, T, stride), np.uint8))
        return np.concatenate(outs, axis=1)
    finally:
        bat.close()


def _check_encoder(dev, g, ty, lay, T, seed, pad_bytes=0, oracle=True):
    w, nat = _wire_input(ty, g, 2 * T, seed)
    got = _encode_device(dev, g, w, ty | lay, T, pad_bytes=pad_bytes, wire=True)
    _same(got, _encode_device(dev, g, nat, DEPTH[ty], T), "the call on the converted integers")
    if oracle:
        _same(got, _oracle_bytes(g, nat, DEPTH[ty]), "oracle")


# ---- encoder ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g", [G8, G8S, G16, G48])
@pytest.mark.parametrize("ty", [ULAW, ALAW])
def test_g711_input_gives_the_int16_bytes(dev, ty, g, T):
    _check_encoder(dev, g, ty, 0, T, seed=31)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g,lay", [(G48, 0), (G48ST, IL), (G48ST, CM), (G96, 0), (G44, 0)])
@pytest.mark.parametrize("ty", [S16BE, S24LE, S24BE])
def test_big_endian_and_packed_input_gives_the_integer_bytes(dev, ty, g, lay, T):
    _check_encoder(dev, g, ty, lay, T, seed=33)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("ty", [S16BE, S24LE, S24BE])
def test_wide_pieces_with_a_remainder_from_an_aligned_pointer(dev, ty, T):
    """N = 20 from an aligned pointer: a run holds whole pieces (two 16-byte pieces of S16_BE where the frame lies on 16 bytes, five dword triples of packed 24
    bits) and, for S16_BE, four samples the per-sample loop takes"""
    _check_encoder(dev, G8S, ty, 0, T, seed=34)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("pad", [1, 3])
@pytest.mark.parametrize("g", [G48, G8S, G16S])
@pytest.mark.parametrize("ty", TYPES)
def test_device_pointer_off_every_alignment(dev, ty, g, pad, T):
    """wire elements carry no alignment requirement: a pointer one byte and three bytes off a 16-byte boundary takes the per-sample loads"""
    _check_encoder(dev, g, ty, 0, T, seed=35, pad_bytes=pad, oracle=False)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("ty", TYPES)
def test_host_pointers_every_layout(ty, T):
    amd, api = _amd(), _api()
    g = G48ST
    fs, ms, hr, ch, rate = g
    w, nat = _wire_input(ty, g, 2 * T, seed=37)
    N = w.shape[3]

    def run(arr, word, layout):
        bat = amd.Batch(B, fs, ch, ms, hr, [rate] * B, device=0)
        try:
            outs = []
            for k in range(2):
                part = arr[:, k * T:(k + 1) * T]
                if arr is w:
                    a = _lay5(part, api.PCM_LAYOUTS[layout]).view(api.pcm_dtype(word)).reshape(api.pcm_shape(word | api.PCM_LAYOUTS[layout], B, T, ch, N))
                else:
                    a = _to_layout(part, api.PCM_LAYOUTS[layout])
                outs.append(bat.encode(a, bitdepth=word, layout=layout))
            return np.concatenate(outs, axis=1)
        finally:
            bat.close()
    want = run(nat, DEPTH[ty], None)
    _same(want, _oracle_bytes(g, nat, DEPTH[ty]), "oracle")
    for layout in (None, "interleaved", "channel_major"):
        _same(run(w, ty, layout), want, layout)


@pytest.mark.parametrize("ty,S", [(ULAW, 2048), (S24LE, 768)])
def test_host_pointers_large_call_in_runs(ty, S):
    """a host call large enough to go up in several overlapped runs of frames (more than 64 MB of PCM in 1- and 3-byte elements): the default and the
    interleaved layout keep the runs, the channel-major one goes up in one piece"""
    amd, api = _amd(), _api()
    g = G16S
    fs, ms, hr, ch, rate = g
    T = 112
    w0, nat0 = _wire_input(ty, g, T, seed=39, streams=64)
    rep = S // 64
    w, nat = np.tile(w0, (rep, 1, 1, 1, 1)), np.tile(nat0, (rep, 1, 1, 1))
    assert w.nbytes > (2 << 25)

    def run(arr, word, layout):
        bat = amd.Batch(S, fs, ch, ms, hr, [rate] * S, device=0)
        try:
            lay = api.PCM_LAYOUTS[layout]
            a = _lay5(arr, lay).view(api.pcm_dtype(word)).reshape(api.pcm_shape(word | lay, S, T, ch, arr.shape[3])) if arr is w else _to_layout(arr, lay)
            return bat.encode(a, bitdepth=word, layout=layout)
        finally:
            bat.close()
    want = run(nat, DEPTH[ty], None)
    for layout in (None, "interleaved", "channel_major"):
        _same(run(w, ty, layout), want, layout)


@pytest.mark.parametrize("ty,lay", [(ULAW, IL), (S24BE, CM), (S16BE, 0)])
def test_device_rates_with_a_wire_format(dev, ty, lay):
    g, T = G16S, 8
    fs, ms, hr, ch, rate = g
    w, nat = _wire_input(ty, g, 2 * T, seed=41)
    rng = np.random.default_rng(1)
    rates = rng.choice([32000, 48000, 64000, 96000, 128000], size=(B, 2 * T)).astype(np.int32)
    res = {}
    for name, arr, word in (("native", nat, DEPTH[ty]), ("wire", w, ty | lay)):
        bat = _amd().Batch(B, fs, ch, ms, hr, [rate] * B, device=0)
        try:
            stride = 400
            parts = []
            for k in range(2):
                part = arr[:, k * T:(k + 1) * T]
                d_pcm = dev.put(_lay5(part, lay) if name == "wire" else np.ascontiguousarray(part))
                d_out, d_nb, d_fl = dev.zeros(B * T * stride), dev.zeros(B * T * 4), dev.zeros(B * T)
                bat.encode_device_rates(d_pcm, word, T, d_out, stride, d_bitrates_ptr=dev.put(rates[:, k * T:(k + 1) * T]), d_num_bytes_ptr=d_nb,
                                        d_flags_ptr=d_fl, sync=True)
                parts.append((dev.get(d_out, (B, T, stride), np.uint8), dev.get(d_nb, (B, T), np.int32), dev.get(d_fl, (B, T), np.uint8)))
            res[name] = parts
        finally:
            bat.close()
    for k in range(2):
        for a, b in zip(res["native"][k], res["wire"][k]):
            assert np.array_equal(a, b), k
        assert res["native"][k][1].min() > 0


@pytest.mark.parametrize("ty,lay", [(ALAW, IL), (S24LE, 0)])
def test_device_packed_with_a_wire_format(dev, ty, lay):
    g, T = G16S, 8
    fs, ms, hr, ch, rate = g
    w, nat = _wire_input(ty, g, 2 * T, seed=43)
    res = {}
    cap = B * T * 400
    for name, arr, word in (("native", nat, DEPTH[ty]), ("wire", w, ty | lay)):
        bat = _amd().Batch(B, fs, ch, ms, hr, [rate] * B, device=0)
        try:
            parts = []
            for k in range(2):
                part = arr[:, k * T:(k + 1) * T]
                d_pcm = dev.put(_lay5(part, lay) if name == "wire" else np.ascontiguousarray(part))
                d_out, d_off, d_nb, d_tot = dev.zeros(cap), dev.zeros(B * T * 8), dev.zeros(B * T * 4), dev.zeros(8)
                bat.encode_device_packed(d_pcm, word, T, d_out, cap, 0, d_offsets_ptr=d_off, d_total_ptr=d_tot, d_num_bytes_ptr=d_nb, sync=True)
                parts.append((dev.get(d_out, (cap,), np.uint8), dev.get(d_off, (B, T), np.int64), dev.get(d_nb, (B, T), np.int32), dev.get(d_tot, (1,), np.int64)))
            res[name] = parts
        finally:
            bat.close()
    for k in range(2):
        for a, b in zip(res["native"][k], res["wire"][k]):
            assert np.array_equal(a, b), k
        assert res["native"][k][3][0] > 0


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("ty", [ULAW, S24BE])
def test_sharded_host_call_on_one_device_twice(ty, T):
    """devices = {0, 0}: the shards' slices are cut in bytes of 1- and 3-byte elements"""
    amd, api = _amd(), _api()
    g = G16S
    fs, ms, hr, ch, rate = g
    S = 5
    w, nat = _wire_input(ty, g, 2 * T, seed=45, streams=S)
    N = w.shape[3]
    for layout in (None, "interleaved"):
        lay = api.PCM_LAYOUTS[layout]
        sb = amd.ShardedBatch(S, fs, ch, ms, hr, [rate] * S, [0, 0])
        one = amd.Batch(S, fs, ch, ms, hr, [rate] * S, device=0)
        try:
            for k in range(2):
                part = w[:, k * T:(k + 1) * T]
                a = _lay5(part, lay).view(api.pcm_dtype(ty)).reshape(api.pcm_shape(ty | lay, S, T, ch, N))
                got = sb.encode(a, bitdepth=ty, layout=layout)
                _same(got, one.encode(np.ascontiguousarray(nat[:, k * T:(k + 1) * T]), bitdepth=DEPTH[ty]), ("sharded", layout, k))
        finally:
            one.close()
            sb.close()


# ---- decoder ----------------------------------------------------------------------------------------------------------------------------------------

def _dec_case(g, T, seed=23):
    fs, ms, hr, ch, rate = g
    return make_dec_case(fs, ms, hr, ch, [rate] * B, 2 * T, seed=seed)


def _overshoot_case(g, T):
    """frames of full-scale 24-bit square waves (CPU oracle encoder at 24 bits): their decoded output exceeds the 24-bit range on both sides"""
    fs, ms, hr, ch, rate = g
    N = int(fs * ms / 1000)
    t = np.arange(2 * T * N)
    x = np.zeros((B, ch, 2 * T * N), np.int32)
    for b in range(B):
        for c in range(ch):
            x[b, c] = np.where((t // (40 + 24 * b + 10 * c)) % 2 == 0, 8388607, -8388608)
    pcm = np.ascontiguousarray(x.reshape(B, ch, 2 * T, N).transpose(0, 2, 1, 3))
    per = []
    for b in range(B):
        o = Oracle(fs, ch, ms, hr, rate, portable_math=True)
        per.append(np.stack([o.encode(pcm[b, k], 24) for k in range(2 * T)]))
    frames = np.stack(per)
    return frames, [frames.shape[2]] * B, np.zeros((B, 2 * T), np.uint8)


def _decode_device(dev, g, frames, nbytes, bfi, T, word, pad_bytes=0, guard=64, streams=B):
    """two consecutive device calls with sizes and flags in device memory, the output pointer pad_bytes off its allocation -> (elements as bytes in the
    default layout [S, 2 T, C, N, eb], [(bytes in front, bytes behind)] of every call: guard bytes of 0xA5 each)"""
    api = _api()
    fs, ms, hr, ch, rate = g
    d = _amd().DecBatch(streams, fs, ch, ms, hr, nbytes, device=0)
    try:
        eb = np.dtype(api.pcm_dtype(word)).itemsize * (3 if (word & 0xFF) in (S24LE, S24BE) else 1)
        n = streams * T * ch * d.N * eb
        out, guards = [], []
        stride = frames.shape[2]
        nb = np.repeat(np.asarray(nbytes, np.int32)[:, None], T, axis=1)
        for k in range(2):
            d_buf = dev.put(np.full(pad_bytes + guard + n + guard, 0xA5, np.uint8))
            d.decode_device_sizes(dev.put(frames[:, k * T:(k + 1) * T]), stride, T, d_buf + pad_bytes + guard, dev.put(nb), dev.put(bfi[:, k * T:(k + 1) * T]), None,
                                  bps=word, sync=True)
            got = dev.get(d_buf, (pad_bytes + guard + n + guard,), np.uint8)
            out.append(_unlay5(got[pad_bytes + guard:pad_bytes + guard + n], word & 0x300, streams, T, ch, d.N, eb))
            guards.append((got[:pad_bytes + guard], got[pad_bytes + guard + n:]))
        return np.concatenate(out, axis=1), guards
    finally:
        d.close()


def _native_bytes(y):
    """an integer output [S, T, C, N] as little-endian bytes [S, T, C, N, itemsize] - the shape _decode_device returns"""
    y = np.ascontiguousarray(y)
    return y.view(np.uint8).reshape(y.shape + (y.dtype.itemsize,))


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g", [G16S, G48, G8S, G96])
@pytest.mark.parametrize("ty", TYPES)
def test_decoder_output_is_the_rule_on_the_integer_output(dev, ty, g, T):
    """frames with loss and corruption"""
    fs, ms, hr, ch, rate = g
    frames, nbytes, bfi = _dec_case(g, T)
    depth = DEPTH[ty]
    y, _ = _decode_device(dev, g, frames, nbytes, bfi, T, depth)
    y = np.ascontiguousarray(y).view(np.int16 if depth == 16 else np.int32)[..., 0]
    o, ost = oracle_decode_streams(frames, nbytes, bfi, fs, ms, hr, ch, bps=depth)
    assert ost.any(), "the case conceals nothing"
    got, guards = _decode_device(dev, g, frames, nbytes, bfi, T, ty)
    bad = np.argwhere((got != to_wire(ty, y)).any(axis=(2, 3, 4)))
    assert len(bad) == 0, ("the integer output of this build", bad[:6].tolist())
    bad = np.argwhere((got != to_wire(ty, o)).any(axis=(2, 3, 4)))
    assert len(bad) == 0, ("oracle", bad[:6].tolist())
    for front, behind in guards:
        assert (front == 0xA5).all() and (behind == 0xA5).all()


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g", [G16S, G48])
@pytest.mark.parametrize("ty", [S24LE, S24BE])
def test_packed_24_output_saturates_on_both_sides(dev, ty, g, T):
    fs, ms, hr, ch, rate = g
    frames, nbytes, bfi = _overshoot_case(g, T)
    y, _ = _decode_device(dev, g, frames, nbytes, bfi, T, 24)
    y = np.ascontiguousarray(y).view(np.int32)[..., 0]
    o, _ = oracle_decode_streams(frames, nbytes, bfi, fs, ms, hr, ch, bps=24)
    assert np.array_equal(y, o)
    assert (y > 8388607).any() and (y < -8388608).any(), "the integer output stays inside 24 bits: saturation is not exercised"
    for lay in (0, IL, CM):
        got, _ = _decode_device(dev, g, frames, nbytes, bfi, T, ty | lay)
        assert np.array_equal(got, to_wire(ty, y)), lay
        v = to_native(ty, got)
        assert v.max() == 8388607 and v.min() == -8388608


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("lay", [0, IL, CM])
@pytest.mark.parametrize("ty", TYPES)
def test_decoder_writes_not_one_byte_more(dev, ty, lay, T):
    """Stereo, every layout, the output pointer one byte off alignment: guard bytes in front of and behind the buffer are untouched, and every byte inside
    it is the expected one (inside a call the byte behind a channel-frame's last is the first of another channel-frame: a store that ran over would have to
    be repaired by that frame's own wave to go unseen - the single-frame calls below leave no such wave)."""
    g = G16S
    frames, nbytes, bfi = _dec_case(g, T, seed=29)
    y, _ = _decode_device(dev, g, frames, nbytes, bfi, T, DEPTH[ty])
    y = np.ascontiguousarray(y).view(np.int16 if DEPTH[ty] == 16 else np.int32)[..., 0]
    for pad in (1, 0):
        got, guards = _decode_device(dev, g, frames, nbytes, bfi, T, ty | lay, pad_bytes=pad)
        assert np.array_equal(got, to_wire(ty, y)), (lay, pad)
        for front, behind in guards:
            assert (front == 0xA5).all() and (behind == 0xA5).all(), ("bytes outside the buffer were written", lay, pad)


@pytest.mark.parametrize("g", [G48, G8S, G16])
@pytest.mark.parametrize("ty", TYPES)
def test_guard_bytes_behind_every_channel_frame(dev, ty, g):
    """One mono stream decoded one frame per call, each call into a buffer of its own with guard bytes on both sides, aligned and one byte off: the byte
    directly behind every channel-frame's last byte is a guard byte, in all three layouts (one channel: the same addresses)."""
    fs, ms, hr, ch, rate = g
    n_fr = 6
    frames, nbytes, bfi = make_dec_case(fs, ms, hr, ch, [rate], n_fr, seed=47)
    depth = DEPTH[ty]
    want = {}
    for word in (depth, ty, ty | IL, ty | CM):
        for pad in (0, 1):
            if word == depth and pad:
                continue
            parts = []
            d = _amd().DecBatch(1, fs, ch, ms, hr, nbytes, device=0)
            try:
                eb = ELEM[ty] if word != depth else depth // 8 if depth == 16 else 4
                n = d.N * eb
                nb = np.asarray(nbytes, np.int32).reshape(1, 1)
                for t in range(n_fr):
                    d_buf = dev.put(np.full(pad + 32 + n + 32, 0xA5, np.uint8))
                    d.decode_device_sizes(dev.put(frames[:, t:t + 1]), frames.shape[2], 1, d_buf + pad + 32, dev.put(nb), dev.put(bfi[:, t:t + 1]), None, bps=word, sync=True)
                    got = dev.get(d_buf, (pad + 32 + n + 32,), np.uint8)
                    assert (got[:pad + 32] == 0xA5).all() and (got[pad + 32 + n:] == 0xA5).all(), (word, pad, t)
                    parts.append(got[pad + 32:pad + 32 + n].reshape(d.N, eb))
            finally:
                d.close()
            want[(word, pad)] = np.stack(parts)
    y = np.ascontiguousarray(want[(depth, 0)]).view(np.int16 if depth == 16 else np.int32)[..., 0]
    for key, got in want.items():
        if key[0] != depth:
            assert np.array_equal(got, to_wire(ty, y)), key


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("ty", TYPES)
def test_decoder_host_pointers_every_layout(ty, T):
    """DecBatch.decode and ShardedDecBatch.decode (devices {0, 0}) into host arrays of the wire dtype and shape"""
    amd, api = _amd(), _api()
    g = G16S
    fs, ms, hr, ch, rate = g
    frames, nbytes, bfi = _dec_case(g, T, seed=27)
    for layout in (None, "interleaved", "channel_major"):
        lay = api.PCM_LAYOUTS[layout]
        d, dn = amd.DecBatch(B, fs, ch, ms, hr, nbytes, device=0), amd.DecBatch(B, fs, ch, ms, hr, nbytes, device=0)
        sd = amd.ShardedDecBatch(B, fs, ch, ms, hr, nbytes, [0, 0])
        try:
            for k in range(2):
                fr, fl = frames[:, k * T:(k + 1) * T], bfi[:, k * T:(k + 1) * T]
                y, st = dn.decode(fr, fl, bps=DEPTH[ty])
                want = to_wire(ty, y)
                for dec in (d, sd):
                    got, gst = dec.decode(fr, fl, bps=ty, layout=layout)
                    assert got.dtype == api.pcm_dtype(ty) and got.shape == api.pcm_shape(ty | lay, B, T, ch, dn.N)
                    got = _unlay5(np.ascontiguousarray(got).view(np.uint8).reshape(-1), lay, B, T, ch, dn.N, ELEM[ty])
                    assert np.array_equal(got, want), (layout, k, type(dec).__name__)
                    assert np.array_equal(gst, st)
        finally:
            sd.close()
            dn.close()
            d.close()


@pytest.mark.parametrize("lay", [0, CM])
@pytest.mark.parametrize("ty", TYPES)
def test_stereo_single_frame_calls_hold_exactly_their_bytes(dev, ty, lay):
    """One stereo stream decoded one frame per call, pointer aligned and one byte off: with one frame per call the byte behind channel 0's frame is channel 1's
    first in both layouts and the byte behind channel 1's frame is a guard byte; the whole content is compared."""
    g = G16S
    fs, ms, hr, ch, rate = g
    n_fr = 6
    frames, nbytes, bfi = make_dec_case(fs, ms, hr, ch, [rate], n_fr, seed=49)
    res = {}
    for word, pad in ((DEPTH[ty], 0), (ty | lay, 0), (ty | lay, 1)):
        d = _amd().DecBatch(1, fs, ch, ms, hr, nbytes, device=0)
        try:
            eb = ELEM[ty] if word != DEPTH[ty] else (2 if DEPTH[ty] == 16 else 4)
            n = ch * d.N * eb
            nb = np.asarray(nbytes, np.int32).reshape(1, 1)
            parts = []
            for t in range(n_fr):
                d_buf = dev.put(np.full(pad + 32 + n + 32, 0xA5, np.uint8))
                d.decode_device_sizes(dev.put(frames[:, t:t + 1]), frames.shape[2], 1, d_buf + pad + 32, dev.put(nb), dev.put(bfi[:, t:t + 1]), None, bps=word, sync=True)
                got = dev.get(d_buf, (pad + 32 + n + 32,), np.uint8)
                assert (got[:pad + 32] == 0xA5).all() and (got[pad + 32 + n:] == 0xA5).all(), (word, pad, t)
                parts.append(got[pad + 32:pad + 32 + n].reshape(ch, d.N, eb))
        finally:
            d.close()
        res[(word, pad)] = np.stack(parts)
    y = np.ascontiguousarray(res[(DEPTH[ty], 0)]).view(np.int16 if DEPTH[ty] == 16 else np.int32)[..., 0]
    for pad in (0, 1):
        assert np.array_equal(res[(ty | lay, pad)], to_wire(ty, y)), pad


@pytest.mark.parametrize("T", TS)
def test_ulaw_round_trip_that_never_leaves_the_device(dev, T):
    """decode to mu-law, encode from that very buffer at another bitrate on the same HIP stream with sync = 0: the bytes of the same round trip taken
    through the host in int16 and numpy"""
    amd = _amd()
    g = G16S
    fs, ms, hr, ch, rate = g
    rate2 = rate // 2 + 16000
    frames, nbytes, bfi = _dec_case(g, T)
    word = ULAW | CM
    dec = amd.DecBatch(B, fs, ch, ms, hr, nbytes, device=0)
    enc = amd.Batch(B, fs, ch, ms, hr, [rate2] * B, device=0)
    s = dev.stream()
    try:
        stride, n = enc.stride, B * T * ch * dec.N
        nb = np.repeat(np.asarray(nbytes, np.int32)[:, None], T, axis=1)
        calls = [(dev.put(frames[:, k * T:(k + 1) * T]), dev.put(nb), dev.put(bfi[:, k * T:(k + 1) * T]), dev.zeros(n), dev.zeros(B * T * stride)) for k in range(2)]
        for d_fr, d_nb, d_bfi, d_pcm, d_out in calls:
            dec.decode_device_sizes(d_fr, frames.shape[2], T, d_pcm, d_nb, d_bfi, None, bps=word, hip_stream=s, sync=False)
            enc.encode_device(d_pcm, word, T, d_out, stride, hip_stream=s, sync=False)
        dev.stream_sync(s)
        got = np.concatenate([dev.get(c[4], (B, T, stride), np.uint8) for c in calls], axis=1)
    finally:
        enc.close()
        dec.close()
    d = amd.DecBatch(B, fs, ch, ms, hr, nbytes, device=0)
    enc = amd.Batch(B, fs, ch, ms, hr, [rate2] * B, device=0)
    try:
        want = []
        for k in range(2):
            y, _ = d.decode(frames[:, k * T:(k + 1) * T], bfi[:, k * T:(k + 1) * T], bps=16)
            back = to_native(ULAW, to_wire(ULAW, y))                      # what the mu-law buffer holds, expanded
            want.append(enc.encode(np.ascontiguousarray(back), bitdepth=16))
        want = np.concatenate(want, axis=1)
    finally:
        enc.close()
        d.close()
    _same(got, want, "device round trip against the host round trip")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ty", TYPES)
def test_traced_calls_refuse_the_wire_types_and_change_nothing(ty):
    amd, api = _amd(), _api()
    g, T = G16S, 4
    fs, ms, hr, ch, rate = g
    w, nat = _wire_input(ty, g, 2 * T, seed=51, streams=1)
    N = w.shape[3]
    fresh = amd.Batch(1, fs, ch, ms, hr, [rate], device=0)
    bat = amd.Batch(1, fs, ch, ms, hr, [rate], device=0)
    try:
        a = np.ascontiguousarray(nat[:, :T])
        first = bat.encode(a, bitdepth=DEPTH[ty])
        assert np.array_equal(first, fresh.encode(a, bitdepth=DEPTH[ty]))
        wa = _lay5(w[:, T:], 0).view(api.pcm_dtype(ty)).reshape(api.pcm_shape(ty, 1, T, ch, N))
        with pytest.raises(api.LC3Error) as e:
            bat.encode_traced(wa, bitdepth=ty)
        assert e.value.code == 1
        b = np.ascontiguousarray(nat[:, T:])
        assert np.array_equal(bat.encode(b, bitdepth=DEPTH[ty]), fresh.encode(b, bitdepth=DEPTH[ty])), "the refused call moved the stream's state"
    finally:
        bat.close()
        fresh.close()
    frames, nbytes, bfi = make_dec_case(fs, ms, hr, ch, [rate], 2 * T, seed=53)
    fresh = amd.DecBatch(1, fs, ch, ms, hr, nbytes, device=0)
    dec = amd.DecBatch(1, fs, ch, ms, hr, nbytes, device=0)
    try:
        y0, _ = dec.decode(frames[:, :T], bfi[:, :T], bps=DEPTH[ty])
        assert np.array_equal(y0, fresh.decode(frames[:, :T], bfi[:, :T], bps=DEPTH[ty])[0])
        with pytest.raises(api.LC3Error) as e:
            dec.decode_traced(frames[:, T:], bfi[:, T:], bps=ty)
        assert e.value.code == 1
        assert np.array_equal(dec.decode(frames[:, T:], bfi[:, T:], bps=DEPTH[ty])[0], fresh.decode(frames[:, T:], bfi[:, T:], bps=DEPTH[ty])[0])
    finally:
        dec.close()
        fresh.close()
