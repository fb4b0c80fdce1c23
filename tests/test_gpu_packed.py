"""GPU tests of packed frames (lc3plus_enc_batch_encode_packed, lc3plus_dec_batch_decode_packed): the packed call against the slotted call of the same
batch configuration on the same input - bytes, offsets, sizes, flags and the stream state after the calls - on the one-wave kernel (T <= 8), the
pipelined writer (T = 64) and the large layout; the capacity rule with sentinel bytes; the decoder on frames at odd, reversed, gapped offsets against
decode_sizes_device on slots; and a round trip on one HIP stream with sync = 0.  Device buffers through ctypes (test_gpu_dec_varsize_device._Hip)."""
import numpy as np
import pytest

from lc3_harness import oracle_encode_streams
from test_gpu_dec_varsize_device import _Hip
from test_gpu_enc_varrate import make_pcm, rate_plan

pytestmark = pytest.mark.gpu
SENT = 0xA5
CAP = 8


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


# (fs, channels, ms, hr, start rate, rates switched per frame, bandwidths)
GEOMS = {
    "48k_mono": (48000, 1, 10.0, 0, 64000, [32000, 64000, 128000, 200000, 320000], [0, 8000, 16000, 20000]),
    "16k_stereo": (16000, 2, 10.0, 0, 64000, [32000, 48000, 64000, 96000], [0, 4000, 8000]),
    "48k_2p5": (48000, 1, 2.5, 0, 96000, [64000, 96000, 128000, 256000], [0, 8000, 16000]),
    "96k_hr": (96000, 1, 10.0, 1, 256000, [160000, 256000, 400000, 500000], None),
}


def _plans(fs, ch, ms, hr, rates, bws, B, T, mode, seed):
    br = bw = None
    if mode in ("rates", "both"):
        br = rate_plan(rates, B, T, seed=seed, change=(1, 1)).astype(np.int32)
        rng = np.random.default_rng(seed + 1)
        bad = rng.random((B, T)) < 0.08                                     # refused entries: the frame keeps the carried rate
        br[bad] = rng.choice([1, -64000, 10 ** 9], size=int(bad.sum()))
    if mode in ("bws", "both") and bws is not None:
        rng = np.random.default_rng(seed + 2)
        bw = rng.choice(bws, size=(B, T)).astype(np.int32)
    return br, bw


def _slotted(dev, bat, pcm, br, bw, stride):
    B, T = pcm.shape[:2]
    d_pcm = dev.put(pcm)
    d_out = dev.put(np.full((B, T, stride), SENT, np.uint8))
    if br is None and bw is None:
        bat.encode_device(d_pcm, 16, T, d_out, stride, sync=True)
        nb = np.array([[bat.num_bytes(b)] * T for b in range(B)], np.int32)
        fl = np.zeros((B, T), np.uint8)
    else:
        d_nb = dev.put(np.zeros((B, T), np.int32)); d_fl = dev.put(np.zeros((B, T), np.uint8))
        bat.encode_device_rates(d_pcm, 16, T, d_out, stride, dev.put(br) if br is not None else None, dev.put(bw) if bw is not None else None,
                                d_nb, d_fl, sync=True)
        nb = dev.get(d_nb, (B, T), np.int32); fl = dev.get(d_fl, (B, T), np.uint8)
    return dev.get(d_out, (B, T, stride), np.uint8), nb, fl


def _packed(dev, bat, pcm, br, bw, order, cap=None, extra=64, hip_stream=None, sync=True):
    B, T = pcm.shape[:2]
    size = (cap if cap is not None else B * T * 1300) + extra
    d_out = dev.put(np.full(size, SENT, np.uint8))
    d_off = dev.put(np.full((B, T), -9, np.int64)); d_tot = dev.put(np.full(1, -9, np.int64))
    d_nb = dev.put(np.zeros((B, T), np.int32)); d_fl = dev.put(np.full((B, T), 0xEE, np.uint8))
    bat.encode_device_packed(dev.put(pcm), 16, T, d_out, size - extra if cap is None else cap, order, dev.put(br) if br is not None else None,
                             dev.put(bw) if bw is not None else None, d_off, d_tot, d_nb, d_fl, hip_stream=hip_stream, sync=sync)
    if not sync:
        dev.sync()
    return (dev.get(d_out, (size,), np.uint8), dev.get(d_off, (B, T), np.int64), int(dev.get(d_tot, (1,), np.int64)[0]),
            dev.get(d_nb, (B, T), np.int32), dev.get(d_fl, (B, T), np.uint8))


def _concat(out_s, nb, order):
    B, T = nb.shape
    idx = [(s, t) for s in range(B) for t in range(T)] if order == 0 else [(s, t) for t in range(T) for s in range(B)]
    return np.concatenate([out_s[s, t, :nb[s, t]] for s, t in idx])


CASES = [(g, T, m) for g in GEOMS for T in (6, 64) for m in ("fixed", "rates", "bws", "both") if GEOMS[g][6] is not None or m in ("fixed", "rates")]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("geom,T,mode", CASES)
def test_packed_equals_slotted(dev, geom, T, mode, order):
    fs, ch, ms, hr, r0, rates, bws = GEOMS[geom]
    amd = _amd()
    from audio_codec_amd.api import plan_packed
    B, K = 12, 2
    stride = (625 if hr else 400) * ch
    slot = amd.Batch(B, fs, ch, ms, hr, [r0] * B, device=0)
    pack = amd.Batch(B, fs, ch, ms, hr, [r0] * B, device=0)
    try:
        for k in range(K):
            pcm = make_pcm(fs, ms, ch, B, T, seed=7 + k)
            br, bw = _plans(fs, ch, ms, hr, rates, bws, B, T, mode, seed=11 + k)
            out_s, nb_s, fl_s = _slotted(dev, slot, pcm, br, bw, stride)
            buf, offs, total, nb, fl = _packed(dev, pack, pcm, br, bw, order)
            assert (nb == nb_s).all() and (fl == fl_s).all()
            rc, want_offs, want_total, ovf = plan_packed(nb, order)
            assert rc == 0 and (offs == want_offs).all() and total == want_total and not ovf.any()
            want = _concat(out_s, nb, order)
            assert total == want.size
            assert np.array_equal(buf[:total], want), np.flatnonzero(buf[:total] != want)[:8]
            assert (buf[total:] == SENT).all()
        if T <= 8:
            # the one-wave kernel leaves every state word the same way; the pipelined path leaves some words the later frames do not read in an order
            # that varies from run to run (two slotted batches differ there too), and its equality shows in the second call's bytes above
            assert np.array_equal(slot.export_streams(range(B)), pack.export_streams(range(B)))
    finally:
        slot.close(); pack.close()


@pytest.mark.parametrize("T,mode", [(6, "fixed"), (64, "fixed"), (64, "rates")])
def test_capacity_cut(dev, T, mode):
    fs, ch, ms, hr, r0, rates, bws = GEOMS["48k_mono"]
    amd = _amd()
    B = 10
    slot = amd.Batch(B, fs, ch, ms, hr, [r0] * B, device=0)
    pack = amd.Batch(B, fs, ch, ms, hr, [r0] * B, device=0)
    try:
        pcm = make_pcm(fs, ms, ch, B, T, seed=3)
        br, bw = _plans(fs, ch, ms, hr, rates, bws, B, T, mode, seed=5)
        out_s, nb_s, fl_s = _slotted(dev, slot, pcm, br, bw, 400)
        total = int(nb_s.sum())
        cap = total // 2 + 3
        buf, offs, tot, nb, fl = _packed(dev, pack, pcm, br, bw, 0, cap=cap, extra=4096)
        assert tot == total and (nb == nb_s).all()
        fits = offs + nb <= cap
        assert ((fl & CAP) != 0).sum() > 0 and (((fl & CAP) != 0) == ~fits).all()
        assert ((fl & 7) == fl_s).all()
        for s in range(B):
            for t in range(T):
                if fits[s, t]:
                    assert np.array_equal(buf[offs[s, t]:offs[s, t] + nb[s, t]], out_s[s, t, :nb[s, t]]), (s, t)
        last = max(int(offs[s, t] + nb[s, t]) for s in range(B) for t in range(T) if fits[s, t])
        assert (buf[last:] == SENT).all()                                    # nothing past the last frame that fits, at or past cap included
        # the state advanced past the frames that were not written: the next call matches the slotted batch byte for byte
        pcm2 = make_pcm(fs, ms, ch, B, T, seed=4)
        br2, bw2 = _plans(fs, ch, ms, hr, rates, bws, B, T, mode, seed=6)
        out_s2, nb_s2, _ = _slotted(dev, slot, pcm2, br2, bw2, 400)
        buf2, _, tot2, _, _ = _packed(dev, pack, pcm2, br2, bw2, 0)
        assert np.array_equal(buf2[:tot2], _concat(out_s2, nb_s2, 0))
        if T <= 8:
            assert np.array_equal(slot.export_streams(range(B)), pack.export_streams(range(B)))
    finally:
        slot.close(); pack.close()


def _scatter(frames_s, nb, seed):
    """Frames of [B, T, stride] slots at odd offsets, in reverse stream order, with gaps -> (buffer, offsets [B, T])."""
    B, T = nb.shape
    rng = np.random.default_rng(seed)
    offs = np.zeros((B, T), np.int64)
    pos = 1
    for s in reversed(range(B)):
        for t in range(T):
            pos += int(rng.integers(0, 7)) | 1
            offs[s, t] = pos
            pos += max(int(nb[s, t]), 0)
    buf = np.full(pos + 16, 0x3C, np.uint8)
    for s in range(B):
        for t in range(T):
            if nb[s, t] > 0:
                buf[offs[s, t]:offs[s, t] + nb[s, t]] = frames_s[s, t, :nb[s, t]]
    return buf, offs


@pytest.mark.parametrize("geom", ["48k_mono", "16k_stereo"])
def test_decoder_packed_equals_slotted(dev, geom):
    fs, ch, ms, hr, r0, rates, bws = GEOMS[geom]
    amd = _amd()
    from audio_codec_amd.api import dec_plan_packed_lenient
    B, T = 8, 24
    stride = 400 * ch
    enc = amd.Batch(B, fs, ch, ms, hr, [r0] * B, device=0)
    pcm = make_pcm(fs, ms, ch, B, T, seed=21)
    br = rate_plan(rates, B, T, seed=22, change=(1, 2)).astype(np.int32)
    out_s, nb, _ = _slotted(dev, enc, pcm, br, None, stride)
    enc.close()
    nb = nb.copy(); bfi = np.zeros((B, T), np.uint8)
    nb[0, 3] = 0; bfi[1, 5] = 1                                              # lost frames
    buf, offs = _scatter(out_s, nb, seed=23)
    cap = buf.size - 16
    maxb = int(nb.max()) - 1
    offs[2, 4] = -3                                                           # a negative offset
    offs[3, 7] = cap - int(nb[3, 7]) + 1                                      # one byte past the capacity
    big = np.argwhere(nb > maxb)                                              # frames above max_frame_bytes
    start = np.full(B, r0 // 800, np.int32)                      # the sizes the streams start from (the rate's bytes at 10 ms)
    rc, eff, lost, inv, end, mx = dec_plan_packed_lenient(fs, ch, ms, hr, start, nb, offs, cap, maxb, bfi)
    assert rc == 0 and inv[2, 4] and inv[3, 7] and len(big) > 0 and all(inv[s, t] for s, t in big)
    d1 = amd.DecBatch(B, fs, ch, ms, hr, list(start), device=0)
    d2 = amd.DecBatch(B, fs, ch, ms, hr, list(start), device=0)
    try:
        shape = (B, T, ch, pcm.shape[3])
        # packed
        d_pcm1 = dev.put(np.zeros(shape, np.int16)); d_st1 = dev.put(np.full((B, T), 0xEE, np.uint8))
        d1.decode_device_packed(dev.put(buf), cap, dev.put(offs), T, d_pcm1, dev.put(nb), maxb, dev.put(bfi), d_st1, sync=True)
        # slotted, with the frames the packed rule refuses marked invalid by a bad flag (the same outcome: concealed, status bit 1, carry kept)
        bfi2 = bfi.copy(); bfi2[(inv != 0)] = 2
        d_pcm2 = dev.put(np.zeros(shape, np.int16)); d_st2 = dev.put(np.full((B, T), 0xEE, np.uint8))
        d2.decode_device_sizes(dev.put(out_s), stride, T, d_pcm2, dev.put(nb), dev.put(bfi2), d_st2, sync=True)
        p1, s1 = dev.get(d_pcm1, shape, np.int16), dev.get(d_st1, (B, T), np.uint8)
        p2, s2 = dev.get(d_pcm2, shape, np.int16), dev.get(d_st2, (B, T), np.uint8)
        assert np.array_equal(p1, p2), np.argwhere((p1 != p2).any(axis=(2, 3)))[:6].tolist()
        assert np.array_equal(s1, s2)
        assert np.array_equal((s1 & 2) != 0, inv != 0)
        assert [d1.num_bytes(s) for s in range(B)] == [int(x) for x in end]
    finally:
        d1.close(); d2.close()


@pytest.mark.parametrize("ready", [0, 1])
def test_round_trip_one_stream_sync0(dev, ready):
    fs, ch, ms, hr = 48000, 1, 10.0, 0
    amd = _amd()
    B, T, K = 16, 12, 3
    enc = amd.Batch(B, fs, ch, ms, hr, [64000] * B, device=0)
    dec = amd.DecBatch(B, fs, ch, ms, hr, [80] * B, device=0)
    ref = amd.DecBatch(B, fs, ch, ms, hr, [80] * B, device=0)
    s = dev.stream()
    try:
        if ready:
            enc.set_input_ready(1)
        pcm = make_pcm(fs, ms, ch, B, K * T, seed=31)
        shape = (B, T, ch, pcm.shape[3])
        calls = []
        for k in range(K):                                                   # inputs and outputs allocated up front: nothing waits in between
            calls.append((dev.put(pcm[:, k * T:(k + 1) * T]), dev.put(np.full(B * T * 400, SENT, np.uint8)), dev.put(np.zeros((B, T), np.int64)),
                          dev.put(np.zeros((B, T), np.int32)), dev.put(np.zeros(shape, np.int16))))
        for d_pcm, d_out, d_off, d_nb, d_dec in calls:
            enc.encode_device_packed(d_pcm, 16, T, d_out, B * T * 400, 1, d_offsets_ptr=d_off, d_num_bytes_ptr=d_nb, hip_stream=s, sync=False)
            dec.decode_device_packed(d_out, B * T * 400, d_off, T, d_dec, d_nb, 400, hip_stream=s, sync=False)
        dev.stream_sync(s)
        want = oracle_encode_streams(pcm[:, :, 0], fs, ms, hr, [64000] * B, portable_math=True)
        for k, (d_pcm, d_out, d_off, d_nb, d_dec) in enumerate(calls):
            buf = dev.get(d_out, (B * T * 400,), np.uint8); offs = dev.get(d_off, (B, T), np.int64); nb = dev.get(d_nb, (B, T), np.int32)
            for b in range(B):
                for t in range(T):
                    assert np.array_equal(buf[offs[b, t]:offs[b, t] + nb[b, t]], want[b][k * T + t]), (k, b, t)
            got = dev.get(d_dec, shape, np.int16)
            frames = np.zeros((B, T, 400), np.uint8)
            for b in range(B):
                for t in range(T):
                    frames[b, t, :nb[b, t]] = want[b][k * T + t]
            want_pcm, _ = ref.decode(frames)
            assert np.array_equal(got, want_pcm), k
    finally:
        enc.close(); dec.close(); ref.close()


def test_argument_errors(dev):
    amd = _amd()
    from audio_codec_amd.api import LC3Error
    bat = amd.Batch(2, 48000, 1, 10.0, 0, [64000] * 2, device=0)
    d = amd.DecBatch(2, 48000, 1, 10.0, 0, [160] * 2, device=0)
    try:
        p = dev.put(np.zeros((2, 1, 1, 480), np.int16)); o = dev.put(np.zeros(1024, np.uint8)); f = dev.put(np.zeros((2, 1), np.int64))
        for kw in (dict(order=2, out_capacity=100), dict(order=0, out_capacity=-1)):
            with pytest.raises(LC3Error):
                bat.encode_device_packed(p, 16, 1, o, kw["out_capacity"], kw["order"], sync=True)
        with pytest.raises(LC3Error):
            d.decode_device_packed(o, 100, f, 1, dev.put(np.zeros((2, 1, 1, 480), np.int16)), dev.put(np.zeros((2, 1), np.int32)), 0, sync=True)
    finally:
        bat.close(); d.close()
