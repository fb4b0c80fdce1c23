"""GPU tests of per-frame rates and bandwidths in device memory (lc3plus_enc_batch_encode_rates_device, Batch.encode_device_rates): every comparison
byte for byte against the CPU oracle given lc3_enc_set_bitrate and lc3_enc_set_bandwidth before every frame, skipping the values the rule refuses
(the reference after a refused setter).  Which values those are comes from the host hook of the same rule (test_enc_rates_device_cpu.py checks it
against the host-array forms).  Calls are queued with sync = 0 and synchronised once, unless a test says otherwise.  Device buffers through ctypes
(test_gpu_parity._Dev): the tests do not depend on torch."""
import os
import zlib

import numpy as np
import pytest

from lc3_harness import Oracle
from test_gpu_dec_varsize_device import _Hip
from test_gpu_enc_varbw import bw_values
from test_gpu_enc_varrate import make_pcm, rate_plan

pytestmark = pytest.mark.gpu
LC3_ERROR, LC3_NULL_ERROR, LC3_HRMODE_BW_ERROR, LC3_BW_WARNING = 1, 3, 14, 18
FL_RATE, FL_BW_REFUSED, FL_BW_RANGE = 1, 2, 4
SENT = 0xA5
HERE = os.path.dirname(os.path.abspath(__file__))


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


def nbytes_of(fs, ch, ms, hr, rate):
    from audio_codec_amd.api import enc_plan_bitrates
    return int(enc_plan_bitrates(fs, ch, ms, hr, [[rate]])[0][0, 0])


def expected(fs, ch, ms, hr, start_rates, start_bw, br, bw, out_stride):
    """The rule over the whole plan (its carries run across calls): num_bytes, bandwidth in force, flags, last rates."""
    from audio_codec_amd.api import enc_plan_rates_lenient
    rc, nb, inf, fl, end = enc_plan_rates_lenient(fs, ch, ms, hr, start_rates, start_bw, bitrates=br, bandwidths=bw, out_stride=out_stride)
    assert rc == 0
    return nb, inf, fl, end


class OracleStreams:
    """One CPU oracle encoder per stream, fed frame by frame with the setters the rule accepts."""
    def __init__(self, fs, ch, ms, hr, rates, bws=None):
        self.o = [Oracle(fs, ch, ms, hr, int(r), portable_math=True) for r in rates]
        self.fs, self.ch, self.ms, self.hr = fs, ch, ms, hr
        for o, r in zip(self.o, rates):
            o.nbytes = nbytes_of(fs, ch, ms, hr, int(r))
        if bws is not None:
            for o, w in zip(self.o, bws):
                assert o.set_bandwidth(int(w)) == 0

    def encode(self, pcm, br=None, bw=None, nb=None, fl=None):
        """pcm [B, T, ch, N]; br / bw None or [B, T]; nb / fl the rule's sizes and flags: list over streams of lists of frames."""
        B, T = pcm.shape[:2]
        out = []
        for b in range(B):
            row = []
            for t in range(T):
                o = self.o[b]
                if br is not None and not fl[b, t] & FL_RATE:
                    assert o.set_bitrate(int(br[b, t])) == 0
                if nb is not None:
                    o.nbytes = int(nb[b, t])                                 # the stream-frame's bytes: for an odd size not channels x the first channel's
                if bw is not None and not fl[b, t] & (FL_BW_REFUSED | FL_BW_RANGE):
                    assert o.set_bandwidth(int(bw[b, t])) in (0, LC3_BW_WARNING)
                row.append(o.encode(pcm[b, t]))
            out.append(row)
        return out

    def set_bitrate(self, b, rate):
        assert self.o[b].set_bitrate(int(rate)) == 0
        self.o[b].nbytes = nbytes_of(self.fs, self.ch, self.ms, self.hr, int(rate))


def run_calls(dev, bat, pcm, br, bw, cuts, out_stride, hip_stream=None, sync=False, bitdepth=16):
    """One encode_device_rates call per [cuts[k], cuts[k + 1]) frames, every input uploaded first; one synchronise at the end -> out [B, T, out_stride]
    (sentinel-filled before), num_bytes [B, T], flags [B, T]."""
    B = pcm.shape[0]
    calls = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        n = b - a
        d_pcm = dev.put(np.ascontiguousarray(pcm[:, a:b]))
        d_br = dev.put(np.ascontiguousarray(br[:, a:b]).astype(np.int32)) if br is not None else None
        d_bw = dev.put(np.ascontiguousarray(bw[:, a:b]).astype(np.int32)) if bw is not None else None
        d_out = dev.put(np.full((B, n, out_stride), SENT, np.uint8))
        d_nb = dev.put(np.full((B, n), -7, np.int32))
        d_fl = dev.put(np.full((B, n), 0xEE, np.uint8))
        calls.append((d_pcm, n, d_out, d_br, d_bw, d_nb, d_fl))
    for d_pcm, n, d_out, d_br, d_bw, d_nb, d_fl in calls:
        bat.encode_device_rates(d_pcm, bitdepth, n, d_out, out_stride, d_br, d_bw, d_nb, d_fl, hip_stream=hip_stream, sync=sync)
    dev.sync()
    out = np.concatenate([dev.get(c[2], (B, c[1], out_stride), np.uint8) for c in calls], axis=1)
    nb = np.concatenate([dev.get(c[5], (B, c[1]), np.int32) for c in calls], axis=1)
    fl = np.concatenate([dev.get(c[6], (B, c[1]), np.uint8) for c in calls], axis=1)
    return out, nb, fl


def check_frames(out, nb, want, t0=0):
    """Payloads against the oracle's frames, and every byte behind a payload still the sentinel."""
    bad = []
    for b in range(out.shape[0]):
        for t in range(out.shape[1]):
            w = want[b][t0 + t]
            if nb[b, t] != w.size or (out[b, t, :w.size] != w).any() or (out[b, t, w.size:] != SENT).any():
                bad.append((b, t0 + t))
    assert not bad, (len(bad), bad[:8])


def spoil_rates(br, fs, ch, ms, hr, seed, big):
    """About one entry in six replaced by a rate the rule refuses: outside the limits, 0, negative, INT32_MAX, or a valid rate (big) whose frame
    does not fit out_stride."""
    rng = np.random.default_rng(seed)
    from test_enc_rates_device_cpu import _limits
    lo, hi = _limits(fs, ch, ms, hr)
    bad = np.array([lo - 1, hi + 1, 0, -1, 2 ** 31 - 1, -2 ** 31, big], np.int64)
    br = br.astype(np.int64).copy()
    m = rng.random(br.shape) < 1 / 6
    br[m] = bad[rng.integers(len(bad), size=int(m.sum()))]
    return br.astype(np.int32)


def spoil_bws(bw, seed):
    rng = np.random.default_rng(seed)
    bw = bw.astype(np.int64).copy()
    m = rng.random(bw.shape) < 1 / 8
    bw[m] = np.array([-1, 7, 2 ** 31 - 1, -2 ** 31], np.int64)[rng.integers(4, size=int(m.sum()))]
    return bw.astype(np.int32)


# tag, fs, frame_ms, hrmode, channels, bitrates, mode: rates alone (r), bandwidths alone (b), both (rb)
POINTS = [
    ("fb48k_10_r", 48000, 10.0, 0, 1, [40000, 64000, 96000, 128000, 272000], "r"),
    ("fb48k_10_b", 48000, 10.0, 0, 1, [64000, 96000], "b"),
    ("fb48k_10_rb", 48000, 10.0, 0, 1, [48000, 64000, 96000, 128000], "rb"),
    ("fb48k_10_stereo_odd_rb", 48000, 10.0, 0, 2, [128800, 160800, 200800, 96000], "rb"),     # 161, 201, 251, 120 bytes
    ("cd44k_10_rb", 44100, 10.0, 0, 1, [44100, 73500, 128000], "rb"),
    ("swb32k_5_b", 32000, 5.0, 0, 1, [64000, 96000], "b"),
    ("wb16k_2p5_stereo_r", 16000, 2.5, 0, 2, [128000, 160000, 256000], "r"),
    ("nb8k_10_rb", 8000, 10.0, 0, 1, [16000, 24000, 32000], "rb"),
    ("fb48k_2p5_b", 48000, 2.5, 0, 1, [128000], "b"),
    ("hr48k_5_r", 48000, 5.0, 1, 1, [148800, 256000, 400000], "r"),
    ("hr96k_10_r", 96000, 10.0, 1, 1, [149600, 256000, 400000], "r"),                          # the large layout
]
CUTS = (0, 5, 25)        # a call of at most 8 frames and a longer one (the pipelined path for bandwidths alone)


@pytest.mark.parametrize("tag,fs,ms,hr,ch,rates,mode", POINTS, ids=[p[0] for p in POINTS])
def test_parity_with_oracle(dev, tag, fs, ms, hr, ch, rates, mode):
    B, T = 4, CUTS[-1]
    seed = zlib.crc32(tag.encode())
    pcm = make_pcm(fs, ms, ch, B, T, seed=17)
    start = [rates[b % len(rates)] for b in range(B)]
    stride = max(nbytes_of(fs, ch, ms, hr, r) for r in rates)
    from test_enc_rates_device_cpu import _limits
    big = _limits(fs, ch, ms, hr)[1]
    br = spoil_rates(rate_plan(rates, B, T, seed), fs, ch, ms, hr, seed + 1, big) if "r" in mode else None
    bw = spoil_bws(rate_plan(bw_values(fs), B, T, seed + 2), seed + 3) if "b" in mode else None
    nb, inf, fl, end = expected(fs, ch, ms, hr, start, [0] * B, br, bw, stride)
    want = OracleStreams(fs, ch, ms, hr, start).encode(pcm, br, bw, nb, fl)
    bat = _amd().Batch(B, fs, ch, ms, hr, start, device=0)
    out, got_nb, got_fl = run_calls(dev, bat, pcm, br, bw, CUTS, stride)
    check_frames(out, got_nb, want)
    assert (got_nb == nb).all() and (got_fl == fl).all()
    if br is not None:
        assert (fl & FL_RATE).any(), "no refused rate: the case does not exercise the carry"
    if bw is not None:
        assert (fl & FL_BW_REFUSED).any() and (fl & FL_BW_RANGE).any()
    # read back: the configuration the device left
    assert [bat.num_bytes(s) for s in range(B)] == nb[:, -1].tolist()
    if not hr:
        assert [bat.bandwidth(s) for s in range(B)] == inf[:, -1].tolist()
    bat.close()


@pytest.mark.parametrize("mode,T", [("r", 6), ("rb", 12), ("b", 4), ("b", 20)])
def test_same_as_host_arrays_on_valid_input(dev, mode, T):
    fs, ms, ch, B = 48000, 10.0, 1, 6
    rates = [64000, 96000, 128000, 160000]
    pcm = make_pcm(fs, ms, ch, B, T, seed=5)
    br = rate_plan(rates, B, T, seed=6) if "r" in mode else None
    bw = rate_plan([0, 4000, 8000, 12000, 20000], B, T, seed=7) if "b" in mode else None
    start = [rates[b % 4] for b in range(B)]
    amd = _amd()
    h, d = amd.Batch(B, fs, ch, ms, 0, start, device=0), amd.Batch(B, fs, ch, ms, 0, start, device=0)
    stride = max(nbytes_of(fs, ch, ms, 0, r) for r in rates)
    want = h.encode(pcm, bitrates=br, bandwidths=bw)
    want_nb, want_st = h.last_num_bytes.copy(), h.last_status(T)
    out, nb, fl = run_calls(dev, d, pcm, br, bw, (0, T), stride)
    assert (fl == 0).all() and (nb == want_nb).all()
    for b in range(B):
        for t in range(T):
            assert (out[b, t, :nb[b, t]] == want[b, t, :nb[b, t]]).all(), (b, t)
    assert (d.last_status(T) == want_st).all()
    assert [d.num_bytes(s) for s in range(B)] == [h.num_bytes(s) for s in range(B)]
    assert d.stride == h.stride
    assert [d.bandwidth(s) for s in range(B)] == [h.bandwidth(s) for s in range(B)]
    h.close(); d.close()


@pytest.mark.parametrize("ch", [1, 2])
def test_invalid_entries_of_every_kind_and_the_carry(dev, ch):
    """Every kind of refused entry beside valid ones, in two calls; the second call starts from the carry the first one left, and an encode()
    after them continues from the configuration the device holds."""
    fs, ms, B = 48000, 10.0, 3
    lo, hi = 20 * 8 * 100 * ch, 400 * 8 * 100 * ch
    ok = [64000 * ch, 96000 * ch, 128800 * ch]
    stride = nbytes_of(fs, ch, ms, 0, max(ok))
    row_r = [ok[0], lo - 1, hi + 1, 0, -5, 2 ** 31 - 1, hi, ok[1], -2 ** 31, ok[2], 1, ok[0]]
    row_b = [8000, 20001, -1, 49, 2 ** 31 - 1, 4000, 30000, 0, -2 ** 31, 16000, 8000, 8000]
    T = len(row_r)
    br = np.array([row_r, row_r[::-1], [0] * T], np.int32)
    bw = np.array([row_b, row_b[::-1], [-1] * T], np.int32)
    pcm = make_pcm(fs, ms, ch, B, T + 4, seed=9)
    start = [ok[1]] * B
    nb, inf, fl, end = expected(fs, ch, ms, 0, start, [0] * B, br, bw, stride)
    ora = OracleStreams(fs, ch, ms, 0, start)
    want = ora.encode(pcm[:, :T], br, bw, nb, fl)
    bat = _amd().Batch(B, fs, ch, ms, 0, start, device=0)
    out, got_nb, got_fl = run_calls(dev, bat, pcm[:, :T], br, bw, (0, 5, T), stride)
    check_frames(out, got_nb, want)
    assert (got_nb == nb).all() and (got_fl == fl).all()
    assert (fl[2] == FL_RATE | FL_BW_RANGE).all() and (nb[2] == nbytes_of(fs, ch, ms, 0, ok[1])).all()
    # encode() behind them, no read-back in between: the device's configuration carries on
    d_pcm = dev.put(np.ascontiguousarray(pcm[:, T:]))
    d_out = dev.put(np.full((B, 4, stride), SENT, np.uint8))
    bat.encode_device(d_pcm, 16, 4, d_out, stride)
    dev.sync()
    out2 = dev.get(d_out, (B, 4, stride), np.uint8)
    nb2 = np.repeat(nb[:, -1:], 4, axis=1)
    check_frames(out2, nb2, ora.encode(pcm[:, T:], nb=nb2))
    bat.close()


def test_call_does_not_wait(dev):
    """Rates, bandwidths and PCM are copied onto the call's stream behind queued encoder work; until the copy lands the device arrays hold invalid
    values.  The call returns while the stream is busy, and the result is right.  A first call of the same shape has sized the batch's buffers."""
    fs, ms, ch, B, T = 48000, 10.0, 1, 8, 16
    rates = [64000, 96000, 128000]
    pcm = make_pcm(fs, ms, ch, B, 2 * T, seed=21)
    br = rate_plan(rates, B, 2 * T, seed=22)
    bw = rate_plan([0, 4000, 12000, 20000], B, 2 * T, seed=23)
    start = [64000] * B
    stride = nbytes_of(fs, ch, ms, 0, 128000)
    nb, inf, fl, end = expected(fs, ch, ms, 0, start, [0] * B, br, bw, stride)
    assert (fl == 0).all()
    want = OracleStreams(fs, ch, ms, 0, start).encode(pcm, br, bw, nb, fl)
    amd = _amd()
    bat = amd.Batch(B, fs, ch, ms, 0, start, device=0)
    EB, ET = 4096, 64                                                        # the delay: encoder calls of 4096 streams x 64 frames
    enc = amd.Batch(EB, fs, 1, ms, 0, [64000] * EB, device=0)
    d_epcm = dev.put(np.random.default_rng(0).integers(-8000, 8000, size=(EB, ET, 1, 480)).astype(np.int16))
    d_eout = dev.zeros(EB * ET * enc.stride)
    s = dev.stream()
    first = [np.ascontiguousarray(x[:, :T]) for x in (pcm, br, bw)]
    d_pcm0, d_br0, d_bw0 = dev.put(first[0]), dev.put(first[1]), dev.put(first[2])
    d_out0 = dev.put(np.full((B, T, stride), SENT, np.uint8))
    bat.encode_device_rates(d_pcm0, 16, T, d_out0, stride, d_br0, d_bw0, hip_stream=s)
    enc.encode_device(d_epcm, 16, ET, d_eout, enc.stride, hip_stream=s)
    second = [np.ascontiguousarray(x[:, T:]) for x in (pcm, br, bw)]
    d_pcm = dev.zeros(second[0].nbytes)
    d_br = dev.put(np.full((B, T), -1, np.int32))                            # read before the copy: every rate and bandwidth refused
    d_bw = dev.put(np.full((B, T), -1, np.int32))
    d_out = dev.put(np.full((B, T, stride), SENT, np.uint8))
    d_nb, d_fl = dev.zeros(B * T * 4), dev.zeros(B * T)
    hs = [dev.pin(x) for x in second]
    dev.sync()
    for _ in range(8):
        enc.encode_device(d_epcm, 16, ET, d_eout, enc.stride, hip_stream=s)
    for dst, src in zip((d_pcm, d_br, d_bw), hs):
        dev.copy_async(dst, src, s)
    bat.encode_device_rates(d_pcm, 16, T, d_out, stride, d_br, d_bw, d_nb, d_fl, hip_stream=s)
    busy = dev.busy(s)
    dev.stream_sync(s)
    assert busy, "the call waited for its stream"
    out = np.concatenate([dev.get(d_out0, (B, T, stride), np.uint8), dev.get(d_out, (B, T, stride), np.uint8)], axis=1)
    got_nb = dev.get(d_nb, (B, T), np.int32)
    assert (dev.get(d_fl, (B, T), np.uint8) == 0).all() and (got_nb == nb[:, T:]).all()
    check_frames(out, nb, want)
    enc.close(); bat.close()


def test_read_back_and_mixing_with_host_calls(dev):
    """Device-rate calls, then encode() with no read-back (the stride bound), set_bitrate on one stream, encode_bitrates, a checkpoint, a reset /
    export / import round trip, and an out_stride below the bound that stride() makes acceptable."""
    fs, ms, ch, B = 48000, 10.0, 1, 4
    rates = [64000, 96000, 128000]
    amd = _amd()
    T = 40
    pcm = make_pcm(fs, ms, ch, B, T, seed=31)
    start = [64000] * B
    ora = OracleStreams(fs, ch, ms, 0, start)
    bat = amd.Batch(B, fs, ch, ms, 0, start, device=0)
    big = nbytes_of(fs, ch, ms, 0, 128000)
    # 1. device rates (out_stride 200 > every frame): the bound becomes 200
    br = rate_plan(rates, B, 6, seed=32)
    br[:, -1] = [64000, 96000, 128000, 64000]
    nb, inf, fl, end = expected(fs, ch, ms, 0, start, [0] * B, br, None, 200)
    out, got_nb, _ = run_calls(dev, bat, pcm[:, :6], br, None, (0, 6), 200)
    check_frames(out, got_nb, ora.encode(pcm[:, :6], br, None, nb, fl))
    # 2. encode() without a read-back: below the bound refused, at it accepted, and the streams keep the device's rates
    d_pcm = dev.put(np.ascontiguousarray(pcm[:, 6:9]))
    d_out = dev.put(np.full((B, 3, 200), SENT, np.uint8))
    with pytest.raises(amd.LC3Error) as e:
        bat.encode_device(d_pcm, 16, 3, d_out, big)
    assert e.value.code == LC3_ERROR
    bat.encode_device(d_pcm, 16, 3, d_out, 200)
    dev.sync()
    nb2 = np.repeat(nb[:, -1:], 3, axis=1)
    check_frames(dev.get(d_out, (B, 3, 200), np.uint8), nb2, ora.encode(pcm[:, 6:9], nb=nb2))
    # 3. stride() reads back; out_stride = stride() is accepted from then on
    assert bat.stride == big and [bat.num_bytes(s) for s in range(B)] == nb[:, -1].tolist()
    d_out = dev.put(np.full((B, 2, big), SENT, np.uint8))
    bat.encode_device(dev.put(np.ascontiguousarray(pcm[:, 9:11])), 16, 2, d_out, big)
    dev.sync()
    nb3 = np.repeat(nb[:, -1:], 2, axis=1)
    check_frames(dev.get(d_out, (B, 2, big), np.uint8), nb3, ora.encode(pcm[:, 9:11], nb=nb3))
    # 4. more device calls, then set_bitrate on stream 0 (a host writer: reads back first), encode(): the others keep the device's configuration
    br = rate_plan(rates, B, 5, seed=33)
    nb, inf, fl, end = expected(fs, ch, ms, 0, nb[:, -1] * 800, [0] * B, br, None, big)
    out, got_nb, _ = run_calls(dev, bat, pcm[:, 11:16], br, None, (0, 5), big)
    check_frames(out, got_nb, ora.encode(pcm[:, 11:16], br, None, nb, fl))
    assert bat.set_bitrate(0, 40000) == 0
    ora.set_bitrate(0, 40000)
    out = bat.encode(pcm[:, 16:19])
    sizes = [nbytes_of(fs, ch, ms, 0, 40000)] + nb[1:, -1].tolist()
    check_sizes = np.repeat(np.array(sizes)[:, None], 3, axis=1)
    want = ora.encode(pcm[:, 16:19], nb=check_sizes)
    for b in range(B):
        for t in range(3):
            assert (out[b, t, :sizes[b]] == want[b][t]).all(), (b, t)
    # 5. device calls, then encode_bitrates (reads back, then its own rates), a checkpoint round trip, and device calls again
    br = rate_plan(rates, B, 4, seed=34)
    cur = [int(r) for r in (np.array(sizes) * 800)]
    nb, inf, fl, end = expected(fs, ch, ms, 0, cur, [0] * B, br, None, big)
    out, got_nb, _ = run_calls(dev, bat, pcm[:, 19:23], br, None, (0, 4), big)
    check_frames(out, got_nb, ora.encode(pcm[:, 19:23], br, None, nb, fl))
    br2 = rate_plan(rates, B, 3, seed=35)
    out = bat.encode(pcm[:, 23:26], bitrates=br2)
    nb_h = bat.last_num_bytes.copy()
    want = ora.encode(pcm[:, 23:26], br2, None, nb_h, np.zeros((B, 3), np.uint8))
    for b in range(B):
        for t in range(3):
            assert (out[b, t, :nb_h[b, t]] == want[b][t]).all(), (b, t)
    st = bat.get_state()
    bat.set_state(st)
    # 6. reset_streams with rates after device calls (reads back), export / reset / import of another stream
    br = rate_plan(rates, B, 4, seed=36)
    nb, inf, fl, end = expected(fs, ch, ms, 0, br2[:, -1], [0] * B, br, None, big)
    out, got_nb, _ = run_calls(dev, bat, pcm[:, 26:30], br, None, (0, 4), big)
    check_frames(out, got_nb, ora.encode(pcm[:, 26:30], br, None, nb, fl))
    bat.reset_streams([2], bitrates=[96000])
    ora.o[2] = Oracle(fs, ch, ms, 0, 96000, portable_math=True); ora.o[2].nbytes = nbytes_of(fs, ch, ms, 0, 96000)
    blob = bat.export_streams([1])
    bat.reset_streams([1])
    bat.import_streams([1], blob)
    assert [bat.num_bytes(s) for s in range(B)] == [nb[0, -1], nb[1, -1], 120, nb[3, -1]]
    br = rate_plan(rates, B, 10, seed=37)
    cur = [int(x) * 800 for x in (nb[0, -1], nb[1, -1], 120, nb[3, -1])]
    nb, inf, fl, end = expected(fs, ch, ms, 0, cur, [0] * B, br, None, big)
    out, got_nb, _ = run_calls(dev, bat, pcm[:, 30:40], br, None, (0, 10), big)
    check_frames(out, got_nb, ora.encode(pcm[:, 30:40], br, None, nb, fl))
    bat.close()


def test_promised_calls_interleaved_and_two_streams(dev):
    """Under set_input_ready: bandwidths-alone calls on the pipelined path and rate calls, interleaved with promised encode() calls of the same length,
    then the same on two hip_streams in turn.  Everything is uploaded first; one synchronise at the end."""
    fs, ms, ch, B, n = 48000, 10.0, 1, 16, 12
    plan = ["b", "e", "b", "b", "e", "r", "e", "rb", "b", "e", "b"]
    K = len(plan)
    T = n * K * 2
    pcm = make_pcm(fs, ms, ch, B, T, seed=41)
    rates = [64000, 96000, 128000]
    br = spoil_rates(rate_plan(rates, B, T, seed=42), fs, ch, ms, 0, seed=43, big=320000)
    bw = spoil_bws(rate_plan(bw_values(fs), B, T, seed=44), seed=45)
    stride = nbytes_of(fs, ch, ms, 0, 128000)
    start = [64000] * B
    amd = _amd()
    bat = amd.Batch(B, fs, ch, ms, 0, start, device=0)
    bat.set_input_ready(True)
    s2 = [None, dev.stream()]
    # expected: the rule call by call (each call's start is the carry), frames of encode() calls at the carried configuration
    ora = OracleStreams(fs, ch, ms, 0, start)
    cur_r, cur_b = np.array(start, np.int32), np.zeros(B, np.int32)
    calls, want_all = [], []
    for k in range(2 * K):
        m = plan[k % K]
        a = k * n
        p = np.ascontiguousarray(pcm[:, a:a + n])
        if m == "e":
            nbk = np.repeat(np.array([nbytes_of(fs, ch, ms, 0, int(r)) for r in cur_r])[:, None], n, axis=1)
            want_all.append((ora.encode(p, nb=nbk), nbk))
            calls.append((m, dev.put(p), None, None, dev.put(np.full((B, n, stride), SENT, np.uint8)), k))
            continue
        r = np.ascontiguousarray(br[:, a:a + n]) if "r" in m else None
        w = np.ascontiguousarray(bw[:, a:a + n]) if "b" in m else None
        nbk, inf, fl, end = expected(fs, ch, ms, 0, cur_r, cur_b, r, w, stride)
        want_all.append((ora.encode(p, r, w, nbk, fl), nbk))
        cur_r = end
        if w is not None:
            cur_b = inf[:, -1].astype(np.int32)
        calls.append((m, dev.put(p), dev.put(r) if r is not None else None, dev.put(w) if w is not None else None,
                      dev.put(np.full((B, n, stride), SENT, np.uint8)), k))
    for m, d_pcm, d_r, d_w, d_out, k in calls:
        hs = s2[k % 2] if k >= K else None                                    # the second half alternates between the batch's stream and another
        if m == "e":
            bat.encode_device(d_pcm, 16, n, d_out, stride, hip_stream=hs)
        else:
            bat.encode_device_rates(d_pcm, 16, n, d_out, stride, d_r, d_w, hip_stream=hs)
    dev.sync()
    for (m, _, _, _, d_out, k), (want, nbk) in zip(calls, want_all):
        check_frames(dev.get(d_out, (B, n, stride), np.uint8), nbk, want)
    bat.close()


def test_reference_golden_with_device_rates(dev):
    """tests/golden/e2_variable_bitrates.npz (frames of the ETSI reference encoder with lc3_enc_set_bitrate before every frame), rates from device memory."""
    z = np.load(os.path.join(HERE, "golden", "e2_variable_bitrates.npz"))
    tags = sorted({k.split("/")[0] for k in z.files})
    assert len(tags) == 11
    bad = {}
    for tag in tags:
        fs, ms, hr, ch = (int(x) if i != 1 else float(x) for i, x in enumerate(z[tag + "/cfg"]))
        pcm, br, frames, sizes = z[tag + "/pcm"], z[tag + "/bitrates"], z[tag + "/frames"], z[tag + "/sizes"]
        B, T = br.shape
        b = _amd().Batch(B, fs, ch, ms, hr, [int(x) for x in br[:, 0]], device=0)
        stride = int(sizes.max())
        out, nb, fl = run_calls(dev, b, pcm, br.astype(np.int32), None, (0, 6, T), stride)
        assert (fl == 0).all() and (nb == sizes).all(), tag
        n = [(s, t) for s in range(B) for t in range(T) if (out[s, t, :sizes[s, t]] != frames[s, t, :sizes[s, t]]).any()]
        if n:
            bad[tag] = n[:6]
        b.close()
    assert not bad, bad


def test_argument_errors_leave_the_batch_unchanged(dev):
    fs, ms, ch, B, T = 48000, 10.0, 1, 3, 4
    amd = _amd()
    pcm = make_pcm(fs, ms, ch, B, T + 3, seed=51)
    a, twin = amd.Batch(B, fs, ch, ms, 0, [64000] * B, device=0), amd.Batch(B, fs, ch, ms, 0, [64000] * B, device=0)
    d_pcm = dev.put(np.ascontiguousarray(pcm[:, :T]))
    d_out = dev.zeros(B * T * 200)
    d_br = dev.put(np.full((B, T), 128000, np.int32))
    d_bw = dev.put(np.full((B, T), 8000, np.int32))
    lib = a.lib

    def call(bat, pcm_p, bitdepth, br_p, bw_p, n, stride):
        return lib.lc3plus_enc_batch_encode_rates_device(bat.h, pcm_p, bitdepth, br_p, bw_p, n, d_out, stride, None, None, None, 1)
    assert call(a, None, 16, d_br, d_bw, T, 200) == LC3_NULL_ERROR
    assert lib.lc3plus_enc_batch_encode_rates_device(a.h, d_pcm, 16, d_br, d_bw, T, None, 200, None, None, None, 1) == LC3_NULL_ERROR
    assert call(a, d_pcm, 16, None, None, T, 200) == LC3_NULL_ERROR
    assert lib.lc3plus_enc_batch_encode_rates_device(None, d_pcm, 16, d_br, None, T, d_out, 200, None, None, None, 1) == LC3_NULL_ERROR
    assert call(a, d_pcm, 8, d_br, d_bw, T, 200) == LC3_ERROR
    assert call(a, d_pcm, 16, d_br, d_bw, 0, 200) == LC3_ERROR
    assert call(a, d_pcm, 16, d_br, d_bw, -3, 200) == LC3_ERROR
    assert call(a, d_pcm, 16, d_br, d_bw, T, 79) == LC3_ERROR                       # below the stride bound (stride() = 80)
    for bat in (a, twin):                                                         # a bandwidth with a cut-off line below 1 in force
        assert bat.set_bandwidth(1, 30) == 0
    assert call(a, d_pcm, 16, None, d_bw, T, 200) == LC3_ERROR
    for bat in (a, twin):
        assert bat.set_bandwidth(1, 0) == 0
    hr = amd.Batch(1, 48000, 1, 5.0, 1, [256000], device=0)
    d1 = dev.put(np.zeros((1, 1, 1, hr.N), np.int16))
    assert lib.lc3plus_enc_batch_encode_rates_device(hr.h, d1, 16, None, d_bw, 1, d_out, 200, None, None, None, 1) == LC3_HRMODE_BW_ERROR
    hr.close()
    assert [a.num_bytes(s) for s in range(B)] == [80] * B and a.stride == 80
    got, want = a.encode(pcm[:, T:]), twin.encode(pcm[:, T:])
    assert (got == want).all()
    a.close(); twin.close()
