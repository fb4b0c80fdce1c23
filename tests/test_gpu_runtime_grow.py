"""GPU test of the host runtime's buffers (lc3_runtime.hip: grow_group, stage_words): on one batch - 16 kHz / 10 ms, mono, 2 streams - calls of 2, then 12,
then 3 frames.  Every buffer the entry point owns then grows once (2 -> 12) and is used once at a smaller size (3).  The fixed-rate cases (enc_host,
enc_device) run both encoder paths - 2 and 3 frames: the one-wave kernel; 12: the pipelined kernels, whose rows, records, hand-over and writer scratch
only they grow; the three cases with per-frame bitrates stay on the one-wave kernel at 12 frames too (it is the only kernel that takes them) and grow the
staging, plan and offset buffers.  One case per entry point that owns buffers; every call's bytes or PCM, sizes, flags and status are compared
exactly with the CPU oracle run over the same 17 frames in order.  The oracle's results are computed once (_case) and left unchanged."""
import functools

import numpy as np
import pytest

from lc3_harness import oracle_encode_streams
from test_gpu_dec_varsize import make_var_case, oracle_var
from test_gpu_dec_varsize_device import _Hip
from test_gpu_enc_varrate import make_pcm, oracle_frames, rate_plan

pytestmark = pytest.mark.gpu
FS, MS, HR, CH, B = 16000, 10.0, 0, 1, 2
CUTS = (0, 2, 14, 17)                       # calls of 2, 12 and 3 frames
T_ALL = CUTS[-1]
RATE, RATES = 32000, [24000, 32000, 64000]
STRIDE = 80                                 # bytes of the largest frame (64 kbit/s at 10 ms)
SENT, ST_SENT, ABSENT = 0x5A, 0xEE, 8


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


@functools.lru_cache(maxsize=None)
def _case():
    from audio_codec_amd.api import enc_plan_bitrates
    pcm = make_pcm(FS, MS, CH, B, T_ALL, seed=5)
    br = rate_plan(RATES, B, T_ALL, seed=6, change=(1, 3))
    frames, nb, bfi, _ = make_var_case(FS, MS, HR, CH, RATES, B, T_ALL, seed=7, p_zero=0.12, p_bfi=0.12)
    want_pcm, want_st = oracle_var(frames, nb, bfi, FS, MS, HR, CH)
    c = dict(pcm=pcm, br=br, fixed=oracle_encode_streams(pcm[:, :, 0], FS, MS, HR, [RATE] * B, portable_math=True), var=oracle_frames(pcm, FS, MS, HR, br),
             var_nb=enc_plan_bitrates(FS, CH, MS, HR, br)[0].astype(np.int32), frames=frames, nb=nb.astype(np.int32), bfi=bfi, want_pcm=want_pcm, want_st=want_st)
    assert frames.shape[2] <= STRIDE and nb.min() == 0 and bfi.max() == 1
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def _check_frames(out, nb, want, a):
    """out [B, T, stride] holds frames a ... a + T - 1 of want[stream][frame], each of its own size (nb, where the call reports sizes)"""
    for s in range(B):
        for t in range(out.shape[1]):
            w = want[s][a + t]
            assert nb is None or nb[s, t] == w.size, (s, a + t, int(nb[s, t]), w.size)
            assert np.array_equal(out[s, t, :w.size], w), (s, a + t)


def _enc_host(dev, bat, c, a, b):
    out = bat.encode(c["pcm"][:, a:b])
    _check_frames(out, None, c["fixed"], a)


def _enc_device(dev, bat, c, a, b):
    d_out = dev.put(np.zeros((B, b - a, STRIDE), np.uint8))
    bat.encode_device(dev.put(c["pcm"][:, a:b]), 16, b - a, d_out, STRIDE, sync=True)
    _check_frames(dev.get(d_out, (B, b - a, STRIDE), np.uint8), None, c["fixed"], a)


def _enc_host_rates(dev, bat, c, a, b):
    out = bat.encode(c["pcm"][:, a:b], bitrates=c["br"][:, a:b])
    _check_frames(out, bat.last_num_bytes, c["var"], a)


def _enc_device_rates(dev, bat, c, a, b):
    T = b - a
    d_out, d_nb, d_fl = dev.put(np.zeros((B, T, STRIDE), np.uint8)), dev.put(np.zeros((B, T), np.int32)), dev.put(np.full((B, T), ST_SENT, np.uint8))
    bat.encode_device_rates(dev.put(c["pcm"][:, a:b]), 16, T, d_out, STRIDE, dev.put(c["br"][:, a:b]), None, d_nb, d_fl, sync=True)
    _check_frames(dev.get(d_out, (B, T, STRIDE), np.uint8), dev.get(d_nb, (B, T), np.int32), c["var"], a)
    assert (dev.get(d_fl, (B, T), np.uint8) == 0).all()


def _enc_packed(dev, bat, c, a, b):
    from audio_codec_amd.api import plan_packed
    T = b - a
    d_out, d_off, d_tot = dev.put(np.full(B * T * STRIDE, SENT, np.uint8)), dev.put(np.full((B, T), -9, np.int64)), dev.put(np.full(1, -9, np.int64))
    d_nb, d_fl = dev.put(np.zeros((B, T), np.int32)), dev.put(np.full((B, T), ST_SENT, np.uint8))
    bat.encode_device_packed(dev.put(c["pcm"][:, a:b]), 16, T, d_out, B * T * STRIDE, 0, dev.put(c["br"][:, a:b]), None, d_off, d_tot, d_nb, d_fl, sync=True)
    nb, offs = dev.get(d_nb, (B, T), np.int32), dev.get(d_off, (B, T), np.int64)
    rc, want_offs, want_total, _ = plan_packed(c["var_nb"][:, a:b], 0)
    assert rc == 0 and np.array_equal(nb, c["var_nb"][:, a:b]) and np.array_equal(offs, want_offs) and int(dev.get(d_tot, (1,), np.int64)[0]) == want_total
    buf = dev.get(d_out, (B * T * STRIDE,), np.uint8)
    for s in range(B):
        for t in range(T):
            assert np.array_equal(buf[offs[s, t]:offs[s, t] + nb[s, t]], c["var"][s][a + t]), (s, a + t)
    assert (buf[want_total:] == SENT).all() and (dev.get(d_fl, (B, T), np.uint8) == 0).all()


def _cmp_pcm(got, st, c, a, b):
    bad = np.argwhere((got != c["want_pcm"][:, a:b]).any(axis=(2, 3)))
    assert len(bad) == 0, ("first differing (stream, frame of the call)", a, bad[:6].tolist())
    assert np.array_equal(st, c["want_st"][:, a:b]), (a, st.tolist())


def _dec_host(dev, d, c, a, b):
    got, st = d.decode(c["frames"][:, a:b], c["bfi"][:, a:b], num_bytes=c["nb"][:, a:b])
    _cmp_pcm(got, st, c, a, b)


def _dec_outputs(dev, T):
    return dev.put(np.full((B, T, CH, FS // 100), SENT * 0x101, np.int16)), dev.put(np.full((B, T), ST_SENT, np.uint8))


def _dec_device_sizes(dev, d, c, a, b):
    T = b - a
    d_pcm, d_st = _dec_outputs(dev, T)
    d.decode_device_sizes(dev.put(c["frames"][:, a:b]), c["frames"].shape[2], T, d_pcm, dev.put(c["nb"][:, a:b]), dev.put(c["bfi"][:, a:b]), d_st, sync=True)
    _cmp_pcm(dev.get(d_pcm, (B, T, CH, FS // 100), np.int16), dev.get(d_st, (B, T), np.uint8), c, a, b)


def _packed_frames(fr, nb):
    """the frames fr [B, T, stride] of sizes nb back to back -> (buffer, offsets [B, T], bytes)"""
    from audio_codec_amd.api import plan_packed
    rc, offs, total, _ = plan_packed(nb, 0)
    assert rc == 0
    buf = np.full(total + 16, 0xC3, np.uint8)
    for s in range(nb.shape[0]):
        for t in range(nb.shape[1]):
            buf[offs[s, t]:offs[s, t] + nb[s, t]] = fr[s, t, :nb[s, t]]
    return buf, offs.astype(np.int64), total


def _dec_packed(dev, d, c, a, b):
    T = b - a
    buf, offs, total = _packed_frames(c["frames"][:, a:b], c["nb"][:, a:b])
    d_pcm, d_st = _dec_outputs(dev, T)
    d.decode_device_packed(dev.put(buf), total, dev.put(offs), T, d_pcm, dev.put(c["nb"][:, a:b]), STRIDE, dev.put(c["bfi"][:, a:b]), d_st, sync=True)
    _cmp_pcm(dev.get(d_pcm, (B, T, CH, FS // 100), np.int16), dev.get(d_st, (B, T), np.uint8), c, a, b)


RAGGED = ((2, 1), (12, 7), (3, 3))          # frames of stream 0 and of stream 1 present in each call: stream 1 falls behind and stops at its frame 11


def _dec_ragged(dev, d, c, k, pos):
    """call k of RAGGED: stream s holds its frames pos[s] ... pos[s] + RAGGED[k][s] - 1; absent frames keep the sentinel and report ABSENT"""
    T, cnt = CUTS[k + 1] - CUTS[k], RAGGED[k]
    S = c["frames"].shape[2]
    fr, nb, bfi = np.full((B, T, S), 0xA5, np.uint8), np.full((B, T), -7, np.int32), np.full((B, T), 7, np.uint8)
    for s in range(B):
        p, n = pos[s], cnt[s]
        fr[s, :n], nb[s, :n], bfi[s, :n] = c["frames"][s, p:p + n], c["nb"][s, p:p + n], c["bfi"][s, p:p + n]
    d_pcm, d_st = _dec_outputs(dev, T)
    d.set_frame_counts(dev.put(np.array(cnt, np.int32)))
    d.decode_device_sizes(dev.put(fr), S, T, d_pcm, dev.put(nb), dev.put(bfi), d_st, sync=True)
    d.set_frame_counts(None)
    got, st = dev.get(d_pcm, (B, T, CH, FS // 100), np.int16), dev.get(d_st, (B, T), np.uint8)
    for s in range(B):
        p, n = pos[s], cnt[s]
        assert np.array_equal(got[s, :n], c["want_pcm"][s, p:p + n]) and np.array_equal(st[s, :n], c["want_st"][s, p:p + n]), (k, s)
        assert (got[s, n:] == SENT * 0x101).all() and (st[s, n:] == ABSENT).all(), ("absent frames", k, s)
        pos[s] += n


@pytest.mark.parametrize("call", [_enc_host, _enc_device, _enc_host_rates, _enc_device_rates, _enc_packed], ids=lambda f: f.__name__[1:])
def test_encoder_buffers_grow_and_are_reused(dev, call):
    c = _case()
    bat = _amd().Batch(B, FS, CH, MS, HR, [int(c["br"][s, 0]) if "rates" in call.__name__ or call is _enc_packed else RATE for s in range(B)], device=0)
    try:
        for a, b in zip(CUTS[:-1], CUTS[1:]):
            call(dev, bat, c, a, b)
            assert (bat.last_status(b - a) == 0).all(), (a, b)
    finally:
        bat.close()


@pytest.mark.parametrize("call", [_dec_host, _dec_device_sizes, _dec_packed], ids=lambda f: f.__name__[1:])
def test_decoder_buffers_grow_and_are_reused(dev, call):
    c = _case()
    d = _amd().DecBatch(B, FS, CH, MS, HR, None, device=0)
    try:
        for a, b in zip(CUTS[:-1], CUTS[1:]):
            call(dev, d, c, a, b)
    finally:
        d.close()


def test_decoder_ragged_buffers_grow_and_are_reused(dev):
    c = _case()
    d = _amd().DecBatch(B, FS, CH, MS, HR, None, device=0)
    try:
        pos = [0] * B
        for k in range(len(RAGGED)):
            _dec_ragged(dev, d, c, k, pos)
        assert pos == [17, 11]
    finally:
        d.close()
