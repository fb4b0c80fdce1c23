"""GPU tests of the PCM format word (include/lc3plus_batch.h: LC3PLUS_PCM_FLOAT32, LC3PLUS_PCM_INTERLEAVED, LC3PLUS_PCM_CHANNEL_MAJOR) of the batch calls.

Every comparison is exact.  The yardstick is the CPU oracle and, beside it, the integer path of the same build: float input that lies on the 16-, 24- or
32-bit grid must give the bytes of the integer call, float output must round to the integers of the integer call, and a layout changes addresses only.
Each case runs as two consecutive calls of T frames (T = 4: the one-wave kernel, T = 64: the pipelined path), so that the loads of the previous frame's
tail are covered.  Device buffers through ctypes (test_gpu_dec_varsize_device._Hip): the tests do not depend on torch."""
import numpy as np
import pytest

from lc3_harness import Oracle, make_dec_case, oracle_decode_streams, synth_pcm
from test_gpu_dec_varsize_device import _Hip

pytestmark = pytest.mark.gpu

# fs, frame_ms, hrmode, channels, total bitrate per stream
G48 = (48000, 10.0, 0, 1, 64000)          # front4 and the 48 kHz resampler
G16S = (16000, 10.0, 0, 2, 64000)         # stereo
G48S = (48000, 2.5, 0, 1, 128000)         # frontm
G96 = (96000, 10.0, 1, 1, 256000)         # high resolution, the large layout
G48ST = (48000, 10.0, 0, 2, 128000)       # stereo on the front4 / 48 kHz resampler path
GEOMS = [G48, G16S, G48S, G96, G48ST]
TS = [4, 64]
B = 3


def _amd():
    import audio_codec_amd
    return audio_codec_amd


def _api():
    from audio_codec_amd import api
    return api


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


def _frame_len(fs, ms):
    return int((48000 if fs == 44100 else fs) * ms / 1000)


def _pcm16(g, frames, seed=3, streams=B):
    """[streams, frames, channels, N] int16, every channel a signal of its own"""
    fs, ms, hr, ch, rate = g
    N = _frame_len(fs, ms)
    return np.ascontiguousarray(synth_pcm(streams * ch, frames, N, fs, seed=seed).reshape(streams, ch, frames, N).transpose(0, 2, 1, 3))


def _to_layout(x, lay):
    """x [S, T, C, N] in the default layout -> the array of layout bit lay"""
    api = _api()
    S, T, Cn, N = x.shape
    if lay == api.PCM_INTERLEAVED:
        return np.ascontiguousarray(x.transpose(0, 1, 3, 2).reshape(S, T * N, Cn))
    if lay == api.PCM_CHANNEL_MAJOR:
        return np.ascontiguousarray(x.transpose(0, 2, 1, 3).reshape(S, Cn, T * N))
    return np.ascontiguousarray(x)


def _from_layout(y, lay, S, T, Cn, N):
    api = _api()
    if lay == api.PCM_INTERLEAVED:
        return y.reshape(S, T, N, Cn).transpose(0, 1, 3, 2)
    if lay == api.PCM_CHANNEL_MAJOR:
        return y.reshape(S, Cn, T, N).transpose(0, 2, 1, 3)
    return y.reshape(S, T, Cn, N)


def _oracle_bytes(g, pcm, bitdepth):
    """pcm [S, frames, C, N] through one CPU oracle encoder per stream, frame by frame -> [S, frames, nbytes]"""
    fs, ms, hr, ch, rate = g
    out = []
    for b in range(pcm.shape[0]):
        o = Oracle(fs, ch, ms, hr, rate, portable_math=True)
        assert o.N == pcm.shape[3]
        out.append(np.stack([o.encode(pcm[b, t], bitdepth) for t in range(pcm.shape[1])]))
    return np.stack(out)


def _encode_device(dev, g, x, sample, lay, T, pad_bytes=0):
    """x [S, 2 T, C, N] in two consecutive device-pointer calls of T frames in format sample | lay -> bytes [S, 2 T, stride]; pad_bytes shifts the device
    pointer off its 256-byte allocation boundary."""
    fs, ms, hr, ch, rate = g
    S = x.shape[0]
    bat = _amd().Batch(S, fs, ch, ms, hr, [rate] * S, device=0)
    try:
        stride = bat.stride
        outs = []
        for k in range(2):
            a = _to_layout(x[:, k * T:(k + 1) * T], lay)
            raw = np.concatenate([np.zeros(pad_bytes, np.uint8), a.view(np.uint8).ravel()])
            d_pcm = dev.put(raw) + pad_bytes
            d_out = dev.zeros(S * T * stride)
            bat.encode_device(d_pcm, sample | lay, T, d_out, stride, sync=True)
            outs.append(dev.get(d_out, (S, T, stride), np.uint8))
        return np.concatenate(outs, axis=1)
    finally:
        bat.close()


def _same(got, want, what):
    n = min(got.shape[2], want.shape[2])
    bad = np.argwhere((got[:, :, :n] != want[:, :, :n]).any(axis=2))
    assert len(bad) == 0, (what, "first differing (stream, frame)", bad[:6].tolist())


# ---- encoder ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g", GEOMS)
def test_float_on_the_16_bit_grid_gives_the_int16_bytes(dev, g, T):
    api = _api()
    x = _pcm16(g, 2 * T)
    f = (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    got = _encode_device(dev, g, f, api.PCM_FLOAT32, 0, T)
    _same(got, _encode_device(dev, g, x, 16, 0, T), "int16 call")
    _same(got, _oracle_bytes(g, x, 16), "oracle")


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g", GEOMS)
def test_float_on_the_24_bit_grid_gives_the_24_bit_bytes(dev, g, T):
    api = _api()
    rng = np.random.default_rng(24)
    x = _pcm16(g, 2 * T, seed=5)
    i24 = (x.astype(np.int32) << 8) + rng.integers(0, 256, x.shape).astype(np.int32)
    f = (i24.astype(np.float32) / np.float32(1 << 23)).astype(np.float32)
    got = _encode_device(dev, g, f, api.PCM_FLOAT32, 0, T)
    _same(got, _encode_device(dev, g, i24, 24, 0, T), "bitdepth-24 call")
    _same(got, _oracle_bytes(g, i24, 24), "oracle at 24 bits")


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g", GEOMS)
def test_quiet_float_finer_than_the_24_bit_grid_gives_the_32_bit_bytes(dev, g, T):
    """i / 2^31 with |i| < 2^23: no rounding happens on the way in"""
    api = _api()
    rng = np.random.default_rng(32)
    x = _pcm16(g, 2 * T, seed=7)
    i32 = (x.astype(np.int32) << 7) + rng.integers(0, 128, x.shape).astype(np.int32)
    assert np.abs(i32).max() < (1 << 23)
    f = (i32.astype(np.float32) / np.float32(2.0 ** 31)).astype(np.float32)
    got = _encode_device(dev, g, f, api.PCM_FLOAT32, 0, T)
    _same(got, _encode_device(dev, g, i32, 32, 0, T), "bitdepth-32 call")


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g", [G16S, G48ST])
@pytest.mark.parametrize("sample", ["int16", "float32"])
def test_layouts_change_addresses_only(dev, g, T, sample):
    api = _api()
    x = _pcm16(g, 2 * T, seed=9)
    if sample == "float32":
        x, word = (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32), api.PCM_FLOAT32
    else:
        word = 16
    want = _encode_device(dev, g, x, word, 0, T)
    for lay in (api.PCM_INTERLEAVED, api.PCM_CHANNEL_MAJOR):
        _same(_encode_device(dev, g, x, word, lay, T), want, "layout %#x" % lay)


@pytest.mark.parametrize("g", [G48, G16S])
def test_with_one_channel_the_three_layouts_are_the_same(dev, g):
    """mono: the three layouts are the same addresses"""
    api = _api()
    T = 4
    x = _pcm16((g[0], g[1], g[2], 1, 64000), 2 * T, seed=2)
    gm = (g[0], g[1], g[2], 1, 64000)
    f = (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    want = _encode_device(dev, gm, x, 16, 0, T)
    for lay in (api.PCM_INTERLEAVED, api.PCM_CHANNEL_MAJOR):
        _same(_encode_device(dev, gm, f, api.PCM_FLOAT32, lay, T), want, lay)
        _same(_encode_device(dev, gm, x, 16, lay, T), want, lay)


def test_device_rates_float_interleaved(dev):
    api = _api()
    g, T = G16S, 8
    fs, ms, hr, ch, rate = g
    x = _pcm16(g, 2 * T, seed=11)
    f = (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    rng = np.random.default_rng(1)
    rates = rng.choice([32000, 48000, 64000, 96000, 128000], size=(B, 2 * T)).astype(np.int32)
    res = {}
    for name, arr, word, lay in (("int16", x, 16, 0), ("float", f, api.PCM_FLOAT32, api.PCM_INTERLEAVED)):
        bat = _amd().Batch(B, fs, ch, ms, hr, [rate] * B, device=0)
        try:
            stride = 400
            parts = []
            for k in range(2):
                d_pcm = dev.put(_to_layout(arr[:, k * T:(k + 1) * T], lay))
                d_out, d_nb, d_fl = dev.zeros(B * T * stride), dev.zeros(B * T * 4), dev.zeros(B * T)
                bat.encode_device_rates(d_pcm, word | lay, T, d_out, stride, d_bitrates_ptr=dev.put(rates[:, k * T:(k + 1) * T]), d_num_bytes_ptr=d_nb,
                                        d_flags_ptr=d_fl, sync=True)
                parts.append((dev.get(d_out, (B, T, stride), np.uint8), dev.get(d_nb, (B, T), np.int32), dev.get(d_fl, (B, T), np.uint8)))
            res[name] = parts
        finally:
            bat.close()
    for k in range(2):
        for a, b in zip(res["int16"][k], res["float"][k]):
            assert np.array_equal(a, b), k
        assert res["int16"][k][1].min() > 0


def test_device_packed_float_interleaved(dev):
    api = _api()
    g, T = G16S, 8
    fs, ms, hr, ch, rate = g
    x = _pcm16(g, 2 * T, seed=13)
    f = (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    res = {}
    cap = B * T * 400
    for name, arr, word, lay in (("int16", x, 16, 0), ("float", f, api.PCM_FLOAT32, api.PCM_INTERLEAVED)):
        bat = _amd().Batch(B, fs, ch, ms, hr, [rate] * B, device=0)
        try:
            parts = []
            for k in range(2):
                d_pcm = dev.put(_to_layout(arr[:, k * T:(k + 1) * T], lay))
                d_out, d_off, d_nb, d_tot = dev.zeros(cap), dev.zeros(B * T * 8), dev.zeros(B * T * 4), dev.zeros(8)
                bat.encode_device_packed(d_pcm, word | lay, T, d_out, cap, 0, d_offsets_ptr=d_off, d_total_ptr=d_tot, d_num_bytes_ptr=d_nb, sync=True)
                parts.append((dev.get(d_out, (cap,), np.uint8), dev.get(d_off, (B, T), np.int64), dev.get(d_nb, (B, T), np.int32), dev.get(d_tot, (1,), np.int64)))
            res[name] = parts
        finally:
            bat.close()
    for k in range(2):
        for a, b in zip(res["int16"][k], res["float"][k]):
            assert np.array_equal(a, b), k
        assert res["int16"][k][3][0] > 0


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g", [G48, G48S, G16S])
@pytest.mark.parametrize("sample", ["int16", "float32"])
def test_pointer_four_bytes_off_a_16_byte_boundary(dev, g, T, sample):
    """the guard of the wide loads: the same bytes from a pointer that is only 4-byte aligned"""
    api = _api()
    x = _pcm16(g, 2 * T, seed=15)
    if sample == "float32":
        x, word = (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32), api.PCM_FLOAT32
    else:
        word = 16
    want = _encode_device(dev, g, x, word, 0, T)
    _same(_encode_device(dev, g, x, word, 0, T, pad_bytes=4), want, "pointer + 4")


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g,lay", [(G48, 0), (G48S, 0), (G48ST, "interleaved"), (G16S, "channel_major")])
def test_nan_and_infinities_are_taken_as_zero(dev, g, lay, T):
    api = _api()
    lay = api.PCM_LAYOUTS[lay] if lay else 0
    x = _pcm16(g, 2 * T, seed=17)
    f = (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    rng = np.random.default_rng(4)
    bad = f.copy()
    flat = bad.reshape(-1)
    idx = rng.choice(flat.size, size=max(12, flat.size // 97), replace=False)
    flat[idx] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(idx.size) % 3]
    zeroed = f.copy()
    zeroed.reshape(-1)[idx] = 0.0
    assert not np.isfinite(bad).all()
    _same(_encode_device(dev, g, bad, api.PCM_FLOAT32, lay, T), _encode_device(dev, g, zeroed, api.PCM_FLOAT32, lay, T), "NaN / inf as 0")


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g", [G16S, G48ST])
def test_host_pointers_pageable_every_layout(g, T):
    amd = _amd()
    fs, ms, hr, ch, rate = g
    x = _pcm16(g, 2 * T, seed=19)
    f = (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)

    def run(arr, layout):
        bat = amd.Batch(B, fs, ch, ms, hr, [rate] * B, device=0)
        try:
            lay = _api().PCM_LAYOUTS[layout]
            return np.concatenate([bat.encode(_to_layout(arr[:, k * T:(k + 1) * T], lay), layout=layout) for k in range(2)], axis=1)
        finally:
            bat.close()
    want = run(x, None)
    _same(want, _oracle_bytes(g, x, 16), "oracle")
    for layout in (None, "interleaved", "channel_major"):
        _same(run(f, layout), want, layout)


def test_host_pointers_large_call_in_runs():
    """a host call large enough to go up in several overlapped runs of frames (more than 64 MB of PCM): the interleaved layout keeps the runs, the
    channel-major one goes up in one piece"""
    amd = _amd()
    g = G16S
    fs, ms, hr, ch, rate = g
    S, T = 512, 112
    x = _pcm16(g, T, seed=21, streams=S)
    f = (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    assert f.nbytes > (2 << 25)

    def run(arr, layout):
        bat = amd.Batch(S, fs, ch, ms, hr, [rate] * S, device=0)
        try:
            return bat.encode(_to_layout(arr, _api().PCM_LAYOUTS[layout]), layout=layout)
        finally:
            bat.close()
    want = run(x, None)
    for layout in (None, "interleaved", "channel_major"):
        _same(run(f, layout), want, layout)


def test_three_channels_do_not_exist_in_this_codec():
    """The address rule holds for any channel count (tests/test_pcm_format_cpu.py checks it with three), but no encoder or decoder of three channels can be
    made: the library refuses them as the reference does (lc3_channels_supported: one or two), and so does the CPU oracle - there is nothing a three-channel
    GPU case could be compared with.  Should either side ever accept three channels, this test fails and the layout cases above want a three-channel twin."""
    amd, api = _amd(), _api()
    assert amd.load_library().lc3_channels_supported(3) == 0
    with pytest.raises(api.LC3Error):
        amd.Batch(1, 48000, 3, 10.0, 0, [192000], device=0)
    with pytest.raises(api.LC3Error):
        amd.DecBatch(1, 48000, 3, 10.0, 0, [240], device=0)
    with pytest.raises(RuntimeError):
        Oracle(48000, 3, 10.0, 0, 192000, portable_math=True)


def test_every_other_word_is_an_error_and_traced_calls_stay_integer(dev):
    amd, api = _amd(), _api()
    fs, ms, hr, ch, rate = G16S
    bat = amd.Batch(1, fs, ch, ms, hr, [rate], device=0)
    dec = amd.DecBatch(1, fs, ch, ms, hr, [bat.stride], device=0)
    try:
        d_pcm, d_out = dev.zeros(4 * ch * bat.N * 4), dev.zeros(4 * 400)
        for word in (0, 8, 17, 16 | 0x300, api.PCM_FLOAT32 | 0x400, api.PCM_INTERLEAVED):
            with pytest.raises(api.LC3Error):
                bat.encode_device(d_pcm, word, 4, d_out, 400, sync=True)
            with pytest.raises(api.LC3Error):
                dec.decode_device(d_out, 400, 4, d_pcm, bps=word, sync=True)
        with pytest.raises(api.LC3Error):
            bat.encode_traced(np.zeros((1, 2, ch, bat.N), np.int16), bitdepth=16 | api.PCM_INTERLEAVED)
    finally:
        dec.close()
        bat.close()


# ---- decoder ----------------------------------------------------------------------------------------------------------------------------------------

def _rha(v):
    """round half away from zero, float64 (np.round rounds half to even)"""
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def _dec_case(g, T):
    fs, ms, hr, ch, rate = g
    frames, nbytes, bfi = make_dec_case(fs, ms, hr, ch, [rate] * B, 2 * T, seed=23)
    return frames, nbytes, bfi


def _decode_host(g, frames, nbytes, bfi, T, bps, layout=None):
    """two consecutive host calls of T frames -> (pcm in the default layout [B, 2 T, C, N], status)"""
    fs, ms, hr, ch, rate = g
    d = _amd().DecBatch(B, fs, ch, ms, hr, nbytes, device=0)
    try:
        pcm, st = [], []
        for k in range(2):
            y, s = d.decode(frames[:, k * T:(k + 1) * T], bfi[:, k * T:(k + 1) * T], bps=bps, layout=layout)
            pcm.append(_from_layout(y, _api().PCM_LAYOUTS[layout], B, T, ch, d.N)); st.append(s)
        return np.concatenate(pcm, axis=1), np.concatenate(st, axis=1)
    finally:
        d.close()


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g", GEOMS)
def test_float_output_rounds_to_the_integer_outputs(g, T):
    api = _api()
    fs, ms, hr, ch, rate = g
    frames, nbytes, bfi = _dec_case(g, T)
    y, st = _decode_host(g, frames, nbytes, bfi, T, api.PCM_FLOAT32)
    assert y.dtype == np.float32
    y = y.astype(np.float64)
    p16, st16 = _decode_host(g, frames, nbytes, bfi, T, 16)
    o16, ost = oracle_decode_streams(frames, nbytes, bfi, fs, ms, hr, ch, bps=16)
    r16 = np.clip(_rha(y * 32768.0), -32768.0, 32767.0).astype(np.int16)
    assert (st == st16).all() and (st == ost).all()
    assert st.any(), "the case conceals nothing"
    bad = np.argwhere((r16 != p16).any(axis=(2, 3)))
    assert len(bad) == 0, ("bps 16", bad[:6].tolist())
    bad = np.argwhere((r16 != o16).any(axis=(2, 3)))
    assert len(bad) == 0, ("oracle", bad[:6].tolist())
    assert np.abs(y).max() < 256.0                       # inside what an int32 at 24 bits holds: the out-of-range conversion is not what this test is about
    p24, _ = _decode_host(g, frames, nbytes, bfi, T, 24)
    bad = np.argwhere((_rha(y * float(1 << 23)).astype(np.int64) != p24.astype(np.int64)).any(axis=(2, 3)))
    assert len(bad) == 0, ("bps 24", bad[:6].tolist())


def _decode_device(dev, g, frames, nbytes, bfi, T, word, lay, sentinel_elems=64):
    """two consecutive device calls with sizes and flags in device memory -> (pcm in the default layout, the elements behind each buffer)"""
    api = _api()
    fs, ms, hr, ch, rate = g
    d = _amd().DecBatch(B, fs, ch, ms, hr, nbytes, device=0)
    try:
        dt = api.pcm_dtype(word)
        n = B * T * ch * d.N
        sent = np.full(sentinel_elems, 0x5A5A if dt == np.int16 else 0x5A5A5A5A, np.uint32).astype(dt) if dt != np.float32 else np.full(sentinel_elems, -123.25, np.float32)
        pcm, tails = [], []
        stride = frames.shape[2]
        nb = np.repeat(np.asarray(nbytes, np.int32)[:, None], T, axis=1)
        for k in range(2):
            d_pcm = dev.put(np.concatenate([np.zeros(n, dt), sent]))
            d.decode_device_sizes(dev.put(frames[:, k * T:(k + 1) * T]), stride, T, d_pcm, dev.put(nb), dev.put(bfi[:, k * T:(k + 1) * T]), None, bps=word | lay, sync=True)
            got = dev.get(d_pcm, (n + sentinel_elems,), dt)
            pcm.append(_from_layout(got[:n], lay, B, T, ch, d.N)); tails.append((got[n:], sent))
        return np.concatenate(pcm, axis=1), tails
    finally:
        d.close()


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("sample", ["int16", "float32"])
def test_decoder_layouts_stereo(dev, T, sample):
    api = _api()
    g = G16S
    word = api.PCM_FLOAT32 if sample == "float32" else 16
    frames, nbytes, bfi = _dec_case(g, T)
    want, _ = _decode_host(g, frames, nbytes, bfi, T, word)
    for lay in (0, api.PCM_INTERLEAVED, api.PCM_CHANNEL_MAJOR):
        got, tails = _decode_device(dev, g, frames, nbytes, bfi, T, word, lay)
        assert np.array_equal(got, want), lay
        for tail, sent in tails:
            assert np.array_equal(tail, sent), ("elements behind the buffer were written", lay)


def test_decode_packed_float_interleaved(dev):
    api = _api()
    g, T = G16S, 8
    fs, ms, hr, ch, rate = g
    frames, nbytes, bfi = _dec_case(g, T)
    want, wst = _decode_host(g, frames, nbytes, bfi, T, api.PCM_FLOAT32)
    d = _amd().DecBatch(B, fs, ch, ms, hr, nbytes, device=0)
    try:
        n = B * T * ch * d.N
        got, st = [], []
        for k in range(2):
            nb = np.repeat(np.asarray(nbytes, np.int32)[:, None], T, axis=1)
            offs = np.concatenate([[0], np.cumsum(nb.ravel())[:-1]]).reshape(B, T).astype(np.int64)
            buf = np.concatenate([frames[b, k * T + t, :nbytes[b]] for b in range(B) for t in range(T)])
            d_pcm, d_st = dev.zeros(n * 4), dev.zeros(B * T)
            d.decode_device_packed(dev.put(buf), buf.size, dev.put(offs), T, d_pcm, dev.put(nb), max(nbytes), dev.put(bfi[:, k * T:(k + 1) * T]), d_st,
                                   bps=api.PCM_FLOAT32 | api.PCM_INTERLEAVED, sync=True)
            got.append(_from_layout(dev.get(d_pcm, (n,), np.float32), api.PCM_INTERLEAVED, B, T, ch, d.N)); st.append(dev.get(d_st, (B, T), np.uint8))
        assert np.array_equal(np.concatenate(got, axis=1), want)
        assert np.array_equal(np.concatenate(st, axis=1) & 1, wst)
    finally:
        d.close()


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("g", [G16S, G48])
def test_round_trip_that_never_leaves_the_device(dev, g, T):
    """decode to float32 channel-major, encode from that very buffer at another bitrate on the same HIP stream with sync = 0: the bytes of the same round
    trip taken through the host in float32"""
    amd, api = _amd(), _api()
    fs, ms, hr, ch, rate = g
    rate2 = rate // 2 + 16000
    frames, nbytes, bfi = _dec_case(g, T)
    word = api.PCM_FLOAT32 | api.PCM_CHANNEL_MAJOR
    dec = amd.DecBatch(B, fs, ch, ms, hr, nbytes, device=0)
    enc = amd.Batch(B, fs, ch, ms, hr, [rate2] * B, device=0)
    s = dev.stream()
    try:
        stride, n = enc.stride, B * T * ch * dec.N
        nb = np.repeat(np.asarray(nbytes, np.int32)[:, None], T, axis=1)
        calls = [(dev.put(frames[:, k * T:(k + 1) * T]), dev.put(nb), dev.put(bfi[:, k * T:(k + 1) * T]), dev.zeros(n * 4), dev.zeros(B * T * stride)) for k in range(2)]
        for d_fr, d_nb, d_bfi, d_pcm, d_out in calls:
            dec.decode_device_sizes(d_fr, frames.shape[2], T, d_pcm, d_nb, d_bfi, None, bps=word, hip_stream=s, sync=False)
            enc.encode_device(d_pcm, word, T, d_out, stride, hip_stream=s, sync=False)
        dev.stream_sync(s)
        got = np.concatenate([dev.get(c[4], (B, T, stride), np.uint8) for c in calls], axis=1)
    finally:
        enc.close()
        dec.close()
    y, _ = _decode_host(g, frames, nbytes, bfi, T, api.PCM_FLOAT32)
    enc = amd.Batch(B, fs, ch, ms, hr, [rate2] * B, device=0)
    try:
        want = np.concatenate([enc.encode(np.ascontiguousarray(y[:, k * T:(k + 1) * T])) for k in range(2)], axis=1)
    finally:
        enc.close()
    _same(got, want, "device round trip against the host round trip")
