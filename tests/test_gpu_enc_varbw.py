"""GPU tests of per-frame bandwidths in the batched encoder (lc3plus_enc_batch_encode_bandwidths, Batch.encode(bandwidths=...)): streams whose
bandwidth changes every one to three frames, against the CPU oracle given lc3_enc_set_bandwidth (after lc3_enc_set_bitrate, when rates switch too)
before every frame, as the reference CLI applies its switching files (R/codec_exe.c:295-325).  Bar: bytes identical, frame for frame."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

from lc3_harness import Oracle, synth_pcm
from test_gpu_enc_varrate import _Dev, make_pcm, rate_plan

pytestmark = pytest.mark.gpu
LC3_ERROR, LC3_NULL_ERROR, LC3_HRMODE_BW_ERROR, LC3_BW_WARNING = 1, 3, 14, 18
FR_BWC = 74


def _amd():
    import audio_codec_amd
    return audio_codec_amd


def bw_values(fs):
    """Bandwidths worth switching between at fs: off, the largest accepted, values off the 4 kHz grid, the smallest line-1 value at 2.5 ms, and
    refused values (above min(fs, 40000) / 2) that keep the bandwidth in force."""
    top = min(fs, 40000) // 2
    return [0, top, top - 1, 200, 4000, 5000, 7999, 8000, top // 2 + 123, top + 1, 30000]


def bw_plan(values, B, T, seed, change=(1, 3)):
    return rate_plan(values, B, T, seed, change)


def oracle_frames(pcm, fs, ms, bws, rates=None, br=None, traced=False):
    """The oracle with (set_bitrate and) set_bandwidth before every frame: list over streams of lists of frames (and [B * ch, T] bw_idx when traced)."""
    from audio_codec_amd.api import enc_plan_bitrates
    B, T, ch, N = pcm.shape
    if br is None:
        br = np.repeat(np.asarray(rates, np.int32)[:, None], T, axis=1)
    nbytes = enc_plan_bitrates(fs, ch, ms, 0, br)[0]
    frames, bwi = [], np.zeros((B * ch, T), np.int32)
    for b in range(B):
        o = Oracle(fs, ch, ms, 0, int(br[b, 0]), portable_math=True)
        tr = o.enable_trace() if traced else None
        row = []
        for t in range(T):
            assert o.set_bitrate(int(br[b, t])) == 0
            o.nbytes = int(nbytes[b, t])                                    # the stream-frame's bytes: for an odd size not channels x the first channel's
            assert o.set_bandwidth(int(bws[b, t])) in (0, LC3_BW_WARNING)
            row.append(o.encode(pcm[b, t]))
            if traced:
                for c in range(ch):
                    bwi[b * ch + c, t] = tr[c].bw_idx
        frames.append(row)
    return (frames, bwi) if traced else frames


def mismatches(got, nb, want, t0=0):
    bad = []
    for b in range(got.shape[0]):
        for t in range(got.shape[1]):
            w = want[b][t0 + t]
            if nb[b, t] != w.size or (got[b, t, :w.size] != w).any():
                bad.append((b, t0 + t))
    return bad


def expected_result(fs, ms, start, bws):
    from audio_codec_amd.api import enc_plan_bandwidths
    return enc_plan_bandwidths(fs, ms, 0, start, bws)


# operating points: tag, fs, frame_ms, channels, bitrate per stream
POINTS = [
    ("wb16k_10", 16000, 10.0, 1, 32000),
    ("swb24k_5", 24000, 5.0, 1, 48000),
    ("swb32k_2p5", 32000, 2.5, 1, 96000),
    ("cd44k_10", 44100, 10.0, 1, 96000),
    ("fb48k_10", 48000, 10.0, 1, 64000),
    ("fb48k_5", 48000, 5.0, 1, 128000),
    ("fb48k_2p5", 48000, 2.5, 1, 128000),
    ("fb48k_10_stereo", 48000, 10.0, 2, 160800),
    ("swb32k_5_stereo", 32000, 5.0, 2, 96000),
    ("wb16k_2p5_stereo", 16000, 2.5, 2, 128000),
]
CALLS = (3, 14, 64)      # the one-wave kernel, the pipelined path of a short call, a long pipelined call


@pytest.mark.parametrize("tag,fs,ms,ch,rate", POINTS, ids=[p[0] for p in POINTS])
def test_parity_with_oracle(tag, fs, ms, ch, rate):
    B = 4
    T = sum(CALLS)
    pcm = make_pcm(fs, ms, ch, B, T, seed=13)
    bws = bw_plan(bw_values(fs), B, T, seed=zlib.crc32(tag.encode()))
    want = oracle_frames(pcm, fs, ms, bws, rates=[rate] * B)
    b = _amd().Batch(B, fs, ch, ms, 0, [rate] * B)
    bad, t0, warned = [], 0, 0
    for n in CALLS:
        start = [b.bandwidth(s) for s in range(B)]
        in_force, rc = expected_result(fs, ms, start, bws[:, t0:t0 + n])
        out = b.encode(pcm[:, t0:t0 + n], bandwidths=bws[:, t0:t0 + n])
        assert b.last_result == rc, (tag, n)
        warned += rc == LC3_BW_WARNING
        assert (b.last_num_bytes == np.array([[b.num_bytes(s)] for s in range(B)])).all()
        bad += mismatches(out, b.last_num_bytes, want, t0)
        assert [b.bandwidth(s) for s in range(B)] == in_force[:, -1].tolist()
        t0 += n
    assert not bad, (tag, len(bad), bad[:8])
    assert warned, "no refused value in any call: the case does not exercise the warning"


@pytest.mark.parametrize("fs,ms,ch,T", [(48000, 10.0, 1, 14), (32000, 5.0, 2, 64), (48000, 2.5, 1, 24)])
def test_pipelined_records_carry_the_capped_index(fs, ms, ch, T):
    B = 6
    pcm = make_pcm(fs, ms, ch, B, T, seed=3)
    bws = bw_plan(bw_values(fs), B, T, seed=T)
    want, bwi = oracle_frames(pcm, fs, ms, bws, rates=[64000 * ch] * B, traced=True)
    b = _amd().Batch(B, fs, ch, ms, 0, [64000 * ch] * B)
    out = b.encode(pcm, bandwidths=bws)
    assert not mismatches(out, b.last_num_bytes, want)
    rec = b.last_records(T).view(np.int32)
    assert (rec[:, :, FR_BWC] == bwi).all()


@pytest.mark.parametrize("switch", ["LC3PLUS_ENC_FUSED", "LC3PLUS_ENC_SHAPE_WAVE", "LC3PLUS_ENC_NO_SPLIT"])
def test_diagnostic_switches_give_the_same_bytes(switch):
    fs, ms, B, T = 48000, 10.0, 8, 40
    pcm = make_pcm(fs, ms, 1, B, T, seed=5)
    bws = bw_plan(bw_values(fs), B, T, seed=9)
    want = oracle_frames(pcm, fs, ms, bws, rates=[80000] * B)
    old = os.environ.get(switch)
    os.environ[switch] = "1"                                                 # read once, when the batch is created
    try:
        b = _amd().Batch(B, fs, 1, ms, 0, [80000] * B)
    finally:
        if old is None:
            del os.environ[switch]
        else:
            os.environ[switch] = old
    bad = []
    for t0, n in ((0, 4), (4, 36)):
        out = b.encode(pcm[:, t0:t0 + n], bandwidths=bws[:, t0:t0 + n])
        bad += mismatches(out, b.last_num_bytes, want, t0)
    assert not bad, (switch, bad[:8])


@pytest.mark.parametrize("T", [5, 24])
def test_constant_bandwidths_equal_set_bandwidth_and_encode(T):
    fs, ms, B = 48000, 10.0, 8
    per = [0, 4000, 8000, 12000, 16000, 20000, 9100, 300]
    pcm = make_pcm(fs, ms, 1, B, T, seed=7)
    a = _amd().Batch(B, fs, 1, ms, 0, [64000] * B)
    for s in range(B):
        assert a.set_bandwidth(s, per[s]) == 0
    v = _amd().Batch(B, fs, 1, ms, 0, [64000] * B)
    assert (v.encode(pcm, bandwidths=np.array(per)[:, None]) == a.encode(pcm)).all()
    assert v.last_result == 0 and [v.bandwidth(s) for s in range(B)] == per
    z = _amd().Batch(B, fs, 1, ms, 0, [64000] * B)
    assert (z.encode(pcm, bandwidths=0) == _amd().Batch(B, fs, 1, ms, 0, [64000] * B).encode(pcm)).all()


def test_with_bitrates_equals_oracle_rate_then_bandwidth():
    fs, ms, B, T = 48000, 10.0, 5, 30
    pcm = make_pcm(fs, ms, 1, B, T, seed=8)
    br = rate_plan([32000, 64000, 96000, 128000, 256000], B, T, seed=2)
    bws = bw_plan(bw_values(fs), B, T, seed=3)
    want = oracle_frames(pcm, fs, ms, bws, br=br)
    b = _amd().Batch(B, fs, 1, ms, 0, [int(x) for x in br[:, 0]])
    bad = []
    for t0, n in ((0, 3), (3, 27)):
        out = b.encode(pcm[:, t0:t0 + n], bitrates=br[:, t0:t0 + n], bandwidths=bws[:, t0:t0 + n])
        assert (b.last_num_bytes == br[:, t0:t0 + n] * 480 // 384000).all()
        bad += mismatches(out, b.last_num_bytes, want, t0)
    assert not bad, bad[:8]
    assert [b.num_bytes(s) for s in range(B)] == [int(x) * 480 // 384000 for x in br[:, -1]]


def test_carry_into_encode_and_checkpoint_resume():
    fs, ms, B = 32000, 10.0, 4
    pcm = make_pcm(fs, ms, 1, B, 48, seed=10)
    bws = bw_plan(bw_values(fs), B, 16, seed=11)
    last, _ = expected_result(fs, ms, [0] * B, bws)
    last = last[:, -1]
    full = np.concatenate([bws, np.repeat(last[:, None], 32, axis=1)], axis=1)
    want = oracle_frames(pcm, fs, ms, full, rates=[64000] * B)
    b = _amd().Batch(B, fs, 1, ms, 0, [64000] * B)
    out = b.encode(pcm[:, :16], bandwidths=bws)
    assert not mismatches(out, b.last_num_bytes, want)
    assert [b.bandwidth(s) for s in range(B)] == last.tolist()
    nb = np.full((B, 16), 80)
    assert not mismatches(b.encode(pcm[:, 16:32]), nb, want, 16)              # encode() continues with each stream's bandwidth
    st = b.get_state()
    c = _amd().Batch(B, fs, 1, ms, 0, [64000] * B)                              # resumed on a batch configured with those bandwidths
    for s in range(B):
        assert c.set_bandwidth(s, int(last[s])) == 0
    c.set_state(st)
    assert not mismatches(c.encode(pcm[:, 32:48], bandwidths=last[:, None]), nb, want, 32)


def test_refused_calls_leave_everything_untouched():
    from audio_codec_amd.api import LC3Error
    fs, ms, B, T = 48000, 5.0, 3, 12
    pcm = make_pcm(fs, ms, 1, B, 2 * T, seed=12)
    bws = bw_plan(bw_values(fs), B, T, seed=13)
    a = _amd().Batch(B, fs, 1, ms, 0, [64000] * B)
    ref = _amd().Batch(B, fs, 1, ms, 0, [64000] * B)
    for s, v in ((0, 8000), (2, 300)):
        a.set_bandwidth(s, v); ref.set_bandwidth(s, v)
    stride = a.stride
    for bad_value in (-1, -4000, 99, 1):                                        # at 5 ms the cut-off line is below 1 under 100 Hz
        bad = bws.copy(); bad[2, T - 1] = bad_value
        out = np.full((B, T, stride), 0xA5, np.uint8)
        rc = a.lib.lc3plus_enc_batch_encode_bandwidths(a.h, pcm.ctypes.data, 0, 16, np.ascontiguousarray(bad, np.int32).ctypes.data, None, T,
                                                       out.ctypes.data, stride, 0, None, None, 1)
        assert rc == LC3_ERROR and (out == 0xA5).all()
    bw32 = np.ascontiguousarray(bws, np.int32)
    out = np.full((B, T, stride), 0xA5, np.uint8)
    for args, code in (((0, 16, bw32.ctypes.data, None, T, None, stride), LC3_NULL_ERROR),           # no output
                       ((0, 16, None, None, T, out.ctypes.data, stride), LC3_NULL_ERROR),            # no bandwidths
                       ((0, 20, bw32.ctypes.data, None, T, out.ctypes.data, stride), LC3_ERROR),     # bitdepth
                       ((0, 16, bw32.ctypes.data, None, T, out.ctypes.data, stride - 1), LC3_ERROR)):  # out_stride
        rc = a.lib.lc3plus_enc_batch_encode_bandwidths(a.h, pcm.ctypes.data, *args, 0, None, None, 1)
        assert rc == code, (args, rc)
    br_bad = np.full((B, T), 15999, np.int32)                                  # a rate fails as in encode_bitrates
    rc = a.lib.lc3plus_enc_batch_encode_bandwidths(a.h, pcm.ctypes.data, 0, 16, bw32.ctypes.data, br_bad.ctypes.data, T, out.ctypes.data, stride, 0,
                                                   None, None, 1)
    assert rc == 6 and (out == 0xA5).all()
    assert [a.bandwidth(s) for s in range(B)] == [8000, 0, 300]
    g1 = a.encode(pcm[:, :T], bandwidths=bws)
    g2 = ref.encode(pcm[:, :T], bandwidths=bws)
    assert (g1 == g2).all() and a.last_result == ref.last_result
    assert (a.encode(pcm[:, T:]) == ref.encode(pcm[:, T:])).all()
    hr = _amd().Batch(2, 48000, 1, 10.0, 1, [160000] * 2)
    with pytest.raises(LC3Error) as e:
        hr.encode(make_pcm(48000, 10.0, 1, 2, 2, seed=1), bandwidths=0)
    assert e.value.code == LC3_HRMODE_BW_ERROR
    assert hr.bandwidth(0) == 0 and a.bandwidth(-1) == -1 and a.bandwidth(B) == -1


def test_device_pointers_sync0_promised_calls_with_overwritten_arrays():
    """Three promised device-pointer calls of equal length queued without a synchronisation (they overlap), each with its own bandwidth array that the
    host overwrites right after the call returns; then a call without the promise.  Bytes equal host calls that are given the same arrays."""
    fs, ms, B, T, K = 48000, 10.0, 256, 16, 3
    pcm = make_pcm(fs, ms, 1, B, (K + 1) * T, seed=14)
    plans = [bw_plan(bw_values(fs), B, T, seed=40 + k) for k in range(K + 1)]
    ref = _amd().Batch(B, fs, 1, ms, 0, [64000] * B)
    b = _amd().Batch(B, fs, 1, ms, 0, [64000] * B)
    d = _Dev()
    try:
        b.set_input_ready(True)
        outs = []
        arr = np.zeros((B, T), np.int32)
        for k in range(K + 1):
            if k == K:
                b.set_input_ready(False)
            dp = d.put(pcm[:, k * T:(k + 1) * T]); do = d.put(np.full((B, T, 96), 0xA5, np.uint8))
            arr[:] = plans[k]
            b.encode_device(dp, 16, T, do, 96, sync=False, bandwidths=arr)
            arr[:] = 0xFFFF                                                   # the call has copied what it needs
            outs.append(do)
        d.sync()
        for k, do in enumerate(outs):
            got = d.get(do, (B, T, 96), np.uint8)
            want = ref.encode(pcm[:, k * T:(k + 1) * T], bandwidths=plans[k])
            assert (got[:, :, :80] == want).all(), k
        assert [b.bandwidth(s) for s in range(B)] == [ref.bandwidth(s) for s in range(B)]
    finally:
        d.free()


def test_host_pointers_in_several_runs_equal_device_pointers():
    fs, ms, B, T = 48000, 10.0, 4096, 32                                     # 126 MB of PCM: the host call is cut into runs
    pcm = np.ascontiguousarray(np.tile(make_pcm(fs, ms, 1, 64, T, seed=17), (B // 64, 1, 1, 1)))
    bws = bw_plan(bw_values(fs), B, T, seed=31)
    h = _amd().Batch(B, fs, 1, ms, 0, [64000] * B)
    dv = _amd().Batch(B, fs, 1, ms, 0, [64000] * B)
    out_h = h.encode(pcm, bandwidths=bws)
    d = _Dev()
    try:
        dp = d.put(pcm); do = d.put(np.zeros((B, T, 80), np.uint8))
        dv.encode_device(dp, 16, T, do, 80, sync=True, bandwidths=bws)
        out_d = d.get(do, (B, T, 80), np.uint8)
    finally:
        d.free()
    assert h.last_result == dv.last_result == LC3_BW_WARNING
    bad = np.nonzero((out_h != out_d).any(axis=2))
    assert not bad[0].size, (bad[0][:8], bad[1][:8])
    want = oracle_frames(pcm[:3], fs, ms, bws[:3], rates=[64000] * 3)          # and a few streams against the oracle
    assert not mismatches(out_h[:3], np.full((3, T), 80), want)


def _g192_frames(data):
    """Payloads of a G.192 file (R/codec_exe.c:705-735: sync word, length in bits, one int16 per bit)."""
    v = np.frombuffer(data, "<u2")
    frames, i = [], 0
    while i < v.size:
        assert v[i] == 0x6B21
        nbits = int(v[i + 1])
        bits = (v[i + 2:i + 2 + nbits] == 0x0081).astype(np.uint8).reshape(-1, 8)
        frames.append(np.packbits(bits, axis=1, bitorder="little").reshape(-1))
        i += 2 + nbits
    return frames


@pytest.mark.parametrize("fs,ms,channels,g192", [(48000, 10.0, 1, 0), (32000, 5.0, 2, 1), (48000, 10.0, 1, 1)])
def test_cli_bandwidth_file_switching_every_frame(tmp_path, fs, ms, channels, g192):
    """tools/lc3plus_enc_cli -bandwidth FILE with a new value every frame (refused values included) over more than one block of 256 frames, with
    and without a rate switching file: against the oracle, and against the reference CLI (oracle/_ref/LC3plus) when it is built."""
    import subprocess
    from lc3_harness import ORACLE_DIR
    from test_gpu_parity import _container, _write_wav
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "tools", "lc3plus_enc_cli")
    subprocess.check_call(["make", "-s", "-C", root, "cli"])
    rng = np.random.default_rng(fs + channels + g192)
    N = int(fs * ms / 1000); T = 300
    pcm = synth_pcm(channels, T, N, fs, seed=48)
    wav = tmp_path / "in.wav"
    _write_wav(wav, pcm.reshape(channels, -1).T.reshape(-1), fs, channels, 16)
    vals = bw_values(fs)
    bw = np.array([vals[i] for i in rng.integers(len(vals), size=T - 7)], dtype="<i8")   # wraps around (R/codec_exe.c:858-866)
    bwf = tmp_path / "bw.bin"; bw.tofile(bwf)
    rate = 64000
    rates = np.array([32000, 48000, 64000, 96000])[rng.integers(4, size=T)].astype("<i8")
    swf = tmp_path / "rates.swf"; rates.tofile(swf)
    fmt = ["-formatG192"] if g192 else []
    for with_rates in (False, True):
        sw = ["-swf", str(swf)] if with_rates else []
        ours = tmp_path / ("ours%d.bit" % with_rates)
        subprocess.check_call([cli, "-E", "-q", "-frame_ms", str(ms), "-bandwidth", str(bwf)] + sw + fmt + [str(wav), str(ours), str(rate * channels)])
        got = open(ours, "rb").read()
        o = Oracle(fs, channels, ms, 0, rate * channels, portable_math=True)
        frames = []
        for t in range(T):
            if with_rates:
                assert o.set_bitrate(int(rates[t]) * channels) == 0
            o.set_bandwidth(int(bw[t % bw.size]))
            frames.append(o.encode(pcm[:, t], 16))
        if g192:
            gf = _g192_frames(got)
            assert len(gf) == T and all(f.size == w.size and (f == w).all() for f, w in zip(gf, frames))
        else:
            assert got == _container(frames, fs, rate * channels, channels, ms, T * N, 0)
        ref_cli = os.path.join(ORACLE_DIR, "_ref", "LC3plus")
        if os.path.exists(ref_cli):
            theirs = tmp_path / ("ref%d.bit" % with_rates)
            subprocess.check_call([ref_cli, "-E", "-q", "-frame_ms", str(ms), "-bandwidth", str(bwf)] + sw + fmt + [str(wav), str(theirs), str(rate * channels)],
                                  stdout=subprocess.DEVNULL)
            assert open(theirs, "rb").read() == got
