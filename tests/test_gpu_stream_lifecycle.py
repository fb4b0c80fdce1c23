"""GPU tests of the stream lifecycle (lc3plus_{enc,dec}_batch_{reset,export,import}_streams; Batch / DecBatch.reset_streams, export_streams,
import_streams and their _device forms): a reset stream continues exactly as a fresh CPU-oracle encoder or decoder fed the same input from there, the
streams around it as if nothing happened; a stream exported from one batch and imported into another continues there exactly as it would have in the
first.  Every comparison is byte- or sample-exact.  Device buffers through ctypes (test_gpu_parity._Dev, test_gpu_dec_varsize_device._Hip)."""
import ctypes as C

import numpy as np
import pytest

from lc3_harness import make_dec_case, oracle_decode_streams
from test_gpu_enc_varrate import make_pcm, oracle_frames
from test_gpu_dec_varsize_device import _Hip

pytestmark = pytest.mark.gpu
LC3_ERROR, LC3_NULL_ERROR, LC3_BITRATE_ERROR, LC3_NUMBYTES_ERROR = 1, 3, 6, 7


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


def _enc_want(pcm, fs, ms, hr, rates, t0=0):
    """The oracle from frame t0 on, one fixed rate per stream: list over streams of [T - t0, nbytes] arrays."""
    B, T = pcm.shape[:2]
    br = np.repeat(np.asarray(rates, np.int32)[:, None], T - t0, axis=1)
    return [np.stack(f) for f in oracle_frames(np.ascontiguousarray(pcm[:, t0:]), fs, ms, hr, br)]


def _enc_check(got, want, what=""):
    """got: list over streams of [T, >= nbytes] batch output; want: list of [T, nbytes]."""
    bad = [(s, t) for s in range(len(want)) for t in range(want[s].shape[0]) if (got[s][t, :want[s].shape[1]] != want[s][t]).any()]
    assert not bad, (what, "first differing (stream, frame)", bad[:6])


ENC_POINTS = [
    (48000, 10.0, 0, 1, [64000, 80000, 96000, 128000], [48000, 160000]),
    (48000, 10.0, 0, 2, [128800, 160800, 96000, 200000], [232800, 128000]),         # odd stream-frame sizes: 161, 201, 291 bytes
    (16000, 2.5, 0, 1, [64000, 96000, 128000], [160000, 80000]),
    (44100, 10.0, 0, 1, [64000, 96000, 73500], [44100, 128000]),
    (48000, 5.0, 1, 1, [160000, 256000, 200000], [300000, 180000]),
    (96000, 10.0, 1, 1, [256000, 300000, 400000], [200000, 350000]),              # the large kernel layout
]


@pytest.mark.parametrize("fs,ms,hr,ch,rates,new", ENC_POINTS)
def test_encoder_reset_mid_run(fs, ms, hr, ch, rates, new):
    """Encode T1 frames, reset streams 0, 3 (configuration kept) and 2, B - 1 (new bitrates), encode T2 more: the reset streams equal a fresh oracle
    fed pcm[s, T1:], the others the oracle over T1 + T2.  T2 = 12 frames: the pipelined path after the reset."""
    B, T1, T2 = 6, 10, 12
    pcm = make_pcm(fs, ms, ch, B, T1 + T2, seed=fs // 1000 + ch + hr)
    rates = [rates[s % len(rates)] for s in range(B)]
    b = _amd().Batch(B, fs, ch, ms, hr, rates, device=0)
    a = b.encode(pcm[:, :T1])
    b.reset_streams([3, 0])
    b.reset_streams([B - 1, 2], bitrates=new)
    after = list(rates); after[B - 1], after[2] = new
    assert [b.num_bytes(s) for s in range(B)] == [int(after[s] * (480 if fs == 44100 else int(fs * ms / 1000)) // (8 * fs)) for s in range(B)]
    z = b.encode(pcm[:, T1:])
    whole = _enc_want(pcm, fs, ms, hr, rates)
    fresh = _enc_want(pcm, fs, ms, hr, after, t0=T1)
    for s in range(B):
        if s in (0, 2, 3, B - 1):
            _enc_check([a[s]], [whole[s][:T1]], "before")
            _enc_check([z[s]], [fresh[s]], "reset stream %d" % s)
        else:
            _enc_check([np.concatenate([a[s][:, :whole[s].shape[1]], z[s][:, :whole[s].shape[1]]])], [whole[s]], "stream %d" % s)
    b.close()


def test_reset_then_per_frame_bitrates():
    """After a reset with a new rate, encode(bitrates=...) equals the oracle; stream 1's new rate (120 bytes) turns attack handling on, stream 3's plan
    switches it off and on again."""
    from test_gpu_enc_varrate import rate_plan
    fs, ms, B, T1, T2 = 48000, 10.0, 5, 9, 14
    N = 480
    rng = np.random.default_rng(9)
    pcm = (rng.standard_normal((B, T1 + T2, 1, N)) * 300).astype(np.int16)
    for s in range(B):
        for t in range(1, T1 + T2, 3):                                   # transients for the attack detector
            pcm[s, t, 0, (37 * s + 101 * t) % N:][:40] += 12000
    rates = [64000] * B
    b = _amd().Batch(B, fs, 1, ms, 0, rates, device=0)
    a = b.encode(pcm[:, :T1])
    b.reset_streams([1, 3], bitrates=[96000, 80000])
    plan = rate_plan([64000, 96000, 128000, 80000], B, T2, seed=4)
    plan[1, :] = 96000
    z = b.encode(pcm[:, T1:], bitrates=plan)
    nb = b.last_num_bytes
    want_a = _enc_want(pcm[:, :T1], fs, ms, 0, rates)
    _enc_check(list(a), want_a, "first call")
    # streams not reset: the oracle over the whole run with set_bitrate before every frame
    br = np.concatenate([np.full((B, T1), 64000, np.int32), plan], axis=1)
    whole = oracle_frames(pcm, fs, ms, 0, br)
    fresh = oracle_frames(np.ascontiguousarray(pcm[:, T1:]), fs, ms, 0, plan)
    for s in range(B):
        want = fresh[s] if s in (1, 3) else whole[s][T1:]
        for t in range(T2):
            assert nb[s, t] == want[t].size and (z[s, t, :want[t].size] == want[t]).all(), (s, t)
    b.close()


def test_reset_between_pipelined_device_calls(dev):
    """set_input_ready(1), device pointers, sync = 0 throughout and one synchronise: resets (one with new rates) queued between pipelined calls still give
    the oracle's bytes."""
    fs, ms, B, T, K = 48000, 10.0, 64, 12, 4
    rates = [[64000, 80000, 96000, 128000][s % 4] for s in range(B)]
    pcm = make_pcm(fs, ms, 1, B, T * K, seed=21)
    amd = _amd()
    b = amd.Batch(B, fs, 1, ms, 0, rates, device=0)
    stride = 400
    ins = [dev.put(np.ascontiguousarray(pcm[:, k * T:(k + 1) * T])) for k in range(K)]
    outs = [dev.zeros(B * T * stride) for _ in range(K)]
    dev.sync()
    b.set_input_ready(True)
    resets = {1: ([0, 17, 63], None), 2: ([5, 17], [160000, 48000])}      # before call k
    for k in range(K):
        if k in resets:
            st, br = resets[k]
            b.reset_streams(st, bitrates=br, sync=False)
        b.encode_device(ins[k], 16, T, outs[k], stride, sync=False)
    dev.sync()
    got = np.concatenate([dev.get(o, (B, T, stride), np.uint8) for o in outs], axis=1)
    # the oracle: per stream, one encoder per segment between its resets, each fresh
    for s in range(B):
        cuts, rate, segs = [0], rates[s], []
        for k in sorted(resets):
            st, br = resets[k]
            if s in st:
                segs.append((cuts[-1], k * T, rate)); cuts.append(k * T)
                if br is not None:
                    rate = br[st.index(s)]
        segs.append((cuts[-1], K * T, rate))
        for t0, t1, r in segs:
            _enc_check([got[s, t0:t1]], _enc_want(pcm[s:s + 1, t0:t1], fs, ms, 0, [r]), "stream %d frames %d .. %d" % (s, t0, t1))
    b.close()


# stereo: even stream-frame sizes (make_dec_case encodes with one stereo oracle encoder, whose frames split evenly)
DEC_POINTS = [p if p[3] == 1 else (48000, 10.0, 0, 2, [128000, 160000, 96000, 192000], [256000, 112000]) for p in ENC_POINTS]


def _dec_case(fs, ms, hr, ch, rates, new, B, T1, T2, seed):
    """Frames of B streams over T1 + T2 frames with lost frames; streams 2 and B - 1 change to the rates `new` at T1 (their frames from there on
    come from encoders started at T1).  -> frames [B, T, stride], bfi, sizes before [B], sizes after [B]."""
    rates = [rates[s % len(rates)] for s in range(B)]
    after = list(rates); after[2], after[B - 1] = new
    f1, nb1, bfi = make_dec_case(fs, ms, hr, ch, rates, T1 + T2, seed=seed)
    f2, nb2, _ = make_dec_case(fs, ms, hr, ch, after, T2, seed=seed + 1)
    frames = np.zeros((B, T1 + T2, max(f1.shape[2], f2.shape[2])), np.uint8)
    frames[:, :, :f1.shape[2]] = f1
    for s in (2, B - 1):
        frames[s, T1:] = 0; frames[s, T1:, :f2.shape[2]] = f2[s]
    return frames, bfi, nb1, [nb2[s] if s in (2, B - 1) else nb1[s] for s in range(B)]


def _dec_check(got, st, want, wst, what=""):
    bad = np.argwhere((got != want).any(axis=(-2, -1)))
    assert len(bad) == 0, (what, "first differing (stream, frame)", bad[:6].tolist())
    assert (st == wst).all(), (what, np.argwhere(st != wst)[:6].tolist())


@pytest.mark.parametrize("fs,ms,hr,ch,rates,new", DEC_POINTS)
def test_decoder_reset_mid_run(fs, ms, hr, ch, rates, new):
    """Decode T1 frames (lost ones among them), reset streams 0, 3 (sizes kept) and 2, B - 1 (new sizes), decode T2 more: PCM and concealment status of
    the reset streams equal a fresh oracle decoder's from T1 on, the others the oracle's over T1 + T2."""
    B, T1, T2 = 6, 10, 12
    frames, bfi, nb1, nb2 = _dec_case(fs, ms, hr, ch, rates, new, B, T1, T2, seed=fs // 1000 + ch)
    d = _amd().DecBatch(B, fs, ch, ms, hr, nb1, device=0)
    p1, s1 = d.decode(frames[:, :T1], bfi[:, :T1])
    d.reset_streams([0, 3])
    d.reset_streams([B - 1, 2], num_bytes=[nb2[B - 1], nb2[2]])
    assert [d.num_bytes(s) for s in range(B)] == nb2
    p2, s2 = d.decode(frames[:, T1:], bfi[:, T1:])
    whole, wst = oracle_decode_streams(frames, nb1, bfi, fs, ms, hr, ch)
    fresh, fst = oracle_decode_streams(np.ascontiguousarray(frames[:, T1:]), nb2, np.ascontiguousarray(bfi[:, T1:]), fs, ms, hr, ch)
    _dec_check(p1, s1, whole[:, :T1], wst[:, :T1], "before")
    for s in range(B):
        if s in (0, 2, 3, B - 1):
            _dec_check(p2[s], s2[s], fresh[s], fst[s], "reset stream %d" % s)
        else:
            _dec_check(p2[s], s2[s], whole[s, T1:], wst[s, T1:], "stream %d" % s)
    d.close()


def test_decoder_reset_after_device_sizes_call(dev):
    """A reset with a new size queued with sync = 0 right behind a decode_sizes_device call, on a stream kept busy by encoder calls: the reset returns
    while the stream is still busy (it does not wait to refresh the configuration the device call left), and num_bytes(stream) then reports the new
    size.  The decoding around it equals the oracle."""
    fs, ms, B, T1, T2 = 48000, 10.0, 6, 8, 10
    frames, bfi, nb1, nb2 = _dec_case(fs, ms, 0, 1, [64000, 80000, 96000], [128000, 48000], B, T1, T2, seed=77)
    stride = frames.shape[2]
    amd = _amd()
    d = amd.DecBatch(B, fs, 1, ms, 0, None, device=0)
    EB, ET = 4096, 64
    enc = amd.Batch(EB, fs, 1, ms, 0, [64000] * EB, device=0)
    d_epcm = dev.put(np.random.default_rng(0).integers(-8000, 8000, size=(EB, ET, 1, 480)).astype(np.int16))
    d_eout = dev.zeros(EB * ET * enc.stride)
    s = dev.stream()
    sizes1 = np.repeat(np.asarray(nb1, np.int32)[:, None], T1, axis=1)
    sizes1[bfi[:, :T1] == 1] = 0
    d_fr, d_nb, d_pcm = dev.put(np.ascontiguousarray(frames[:, :T1])), dev.put(sizes1), dev.zeros(B * T1 * d.N * 2)
    enc.encode_device(d_epcm, 16, ET, d_eout, enc.stride, hip_stream=s, sync=False)          # grows the encoder's buffers
    d_tmp = dev.zeros(d.stream_state_size)
    for _ in range(3):                                                   # the batch's staging slots: allocated before the timed call
        d.export_streams_device([0], d_tmp, hip_stream=s)
    dev.stream_sync(s)
    for _ in range(6):
        enc.encode_device(d_epcm, 16, ET, d_eout, enc.stride, hip_stream=s, sync=False)
    d.decode_device_sizes(d_fr, stride, T1, d_pcm, d_nb, hip_stream=s)
    d.reset_streams([2, B - 1], num_bytes=[nb2[2], nb2[B - 1]], hip_stream=s, sync=False)
    busy = dev.busy(s)
    assert [d.num_bytes(x) for x in range(B)] == nb2
    dev.stream_sync(s)
    assert busy, "the reset waited for its stream"
    p1 = dev.get(d_pcm, (B, T1, 1, d.N), np.int16)
    p2, s2 = d.decode(frames[:, T1:], bfi[:, T1:])
    whole, wst = oracle_decode_streams(frames, nb1, bfi, fs, ms, 0, 1)
    fresh, fst = oracle_decode_streams(np.ascontiguousarray(frames[:, T1:]), nb2, np.ascontiguousarray(bfi[:, T1:]), fs, ms, 0, 1)
    assert (p1 == whole[:, :T1]).all()
    for x in range(B):
        if x in (2, B - 1):
            _dec_check(p2[x], s2[x], fresh[x], fst[x], "reset stream %d" % x)
        else:
            _dec_check(p2[x], s2[x], whole[x, T1:], wst[x, T1:], "stream %d" % x)
    enc.close(); d.close()


def test_whole_batch_reset_equals_fresh_batch():
    """c1 (4096 streams, 48 kHz / 10 ms, 64 kbps) and d1: after some calls, a reset of every stream gives the state of a freshly created batch."""
    amd = _amd()
    B, T = 4096, 9
    pcm = make_pcm(48000, 10.0, 1, 16, T, seed=3)
    pcm = np.tile(pcm, (B // 16, 1, 1, 1))
    b = amd.Batch(B, 48000, 1, 10.0, 0, [64000] * B, device=0)
    fresh = amd.Batch(B, 48000, 1, 10.0, 0, [64000] * B, device=0)
    out = b.encode(pcm)
    st0 = fresh.get_state()
    assert (b.get_state() != st0).any()
    b.reset_streams(np.random.default_rng(1).permutation(B))
    assert (b.get_state() == st0).all()
    assert (b.encode(pcm) == out).all()                                  # and it encodes as the fresh batch did
    b.close(); fresh.close()
    d = amd.DecBatch(B, 48000, 1, 10.0, 0, [80] * B, device=0)
    dfresh = amd.DecBatch(B, 48000, 1, 10.0, 0, [80] * B, device=0)
    bfi = np.zeros((B, T), np.uint8); bfi[::7, 4] = 1
    pcm_out, _ = d.decode(out, bfi)
    dst0 = dfresh.get_state()
    assert (d.get_state() != dst0).any()
    d.reset_streams(list(range(B)))
    assert (d.get_state() == dst0).all()
    assert (d.decode(out, bfi)[0] == pcm_out).all()
    d.close(); dfresh.close()


def _slices(state, B, ch, row_words):
    return state.view(np.uint8).reshape(B, ch * row_words * 4)


@pytest.mark.parametrize("via", ["host", "device"])
def test_encoder_migration(dev, via):
    """Stream 2 of batch A (5 streams) moves to stream 6 of batch B (9 streams, other rates and state) after T1 frames; B's stream 6 then continues
    exactly as A's stream 2 does on the same input, and both equal the oracle.  The blob's rows are A's get_state() slice of that stream."""
    fs, ms, ch, T1, T2 = 48000, 10.0, 2, 11, 13
    amd = _amd()
    pcm = make_pcm(fs, ms, ch, 9, T1 + T2, seed=41)
    ra = [96000, 128000, 160800, 64000, 200000]
    rb = [64000] * 9
    A = amd.Batch(5, fs, ch, ms, 0, ra, device=0)
    Bb = amd.Batch(9, fs, ch, ms, 0, rb, device=0)
    A.encode(pcm[:5, :T1])
    Bb.encode(pcm[:, :T1][::-1].copy())
    size = A.stream_state_size
    assert size == Bb.stream_state_size == 16 + ch * 960 * 4
    if via == "host":
        blob = A.export_streams([2, 4])
        Bb.import_streams([6, 0], blob)
    else:
        d_blob = dev.zeros(2 * size)
        A.export_streams_device([2, 4], d_blob, sync=True)                # the importing batch runs on a stream of its own
        Bb.import_streams_device([6, 0], d_blob, sync=True)
        blob = dev.get(d_blob, (2, size), np.uint8)
    rows = _slices(A.get_state(), 5, ch, 960)
    assert (blob[0, 16:] == rows[2]).all() and (blob[1, 16:] == rows[4]).all()
    Bb.set_bitrate(6, ra[2]); Bb.set_bitrate(0, ra[4])
    za = A.encode(pcm[:5, T1:])
    zin = pcm[:, T1:][::-1].copy(); zin[6] = pcm[2, T1:]; zin[0] = pcm[4, T1:]
    zb = Bb.encode(zin)
    want = _enc_want(pcm[:5], fs, ms, 0, ra)
    for i, j in ((2, 6), (4, 0)):
        n = want[i].shape[1]
        assert (zb[j, :, :n] == za[i, :, :n]).all()
        _enc_check([za[i]], [want[i][T1:]], "A stream %d" % i)
    A.close(); Bb.close()


def test_encoder_migration_after_pipelined_call(dev):
    """The export right behind a pipelined call (device pointers, input_ready, sync = 0), whose MDCT memory went through the hand-over: the blob holds
    the complete state - the importing batch continues byte for byte."""
    fs, ms, B, T, K = 48000, 10.0, 32, 12, 3
    amd = _amd()
    pcm = make_pcm(fs, ms, 1, B, T * (K + 1), seed=51)
    A = amd.Batch(B, fs, 1, ms, 0, [64000] * B, device=0)
    Bb = amd.Batch(3, fs, 1, ms, 0, [96000] * 3, device=0)
    stride = A.stride
    ins = [dev.put(np.ascontiguousarray(pcm[:, k * T:(k + 1) * T])) for k in range(K)]
    outs = [dev.zeros(B * T * stride) for _ in range(K)]
    size = A.stream_state_size
    d_blob = dev.zeros(size)
    dev.sync()
    A.set_input_ready(True)
    for k in range(K):
        A.encode_device(ins[k], 16, T, outs[k], stride, sync=False)
    A.export_streams_device([13], d_blob, sync=False)
    dev.sync()                                                           # the importing batch runs on a stream of its own
    Bb.import_streams_device([1], d_blob, sync=True)
    Bb.set_bitrate(1, 64000)
    nxt = np.zeros((3, T, 1, 480), np.int16); nxt[1] = pcm[13, K * T:]
    zb = Bb.encode(nxt)
    want = _enc_want(pcm[13:14], fs, ms, 0, [64000])[0]
    got = np.concatenate([dev.get(o, (B, T, stride), np.uint8)[13] for o in outs])
    assert (got[:, :80] == want[:K * T]).all()
    assert (zb[1, :, :80] == want[K * T:]).all()
    A.close(); Bb.close()


@pytest.mark.parametrize("via", ["host", "device"])
def test_decoder_migration(dev, via):
    """Decoder stream 1 of A (4 streams) moves to stream 5 of B (7 streams): B continues exactly as A, both equal the oracle, PCM and status."""
    fs, ms, T1, T2 = 48000, 10.0, 9, 11
    amd = _amd()
    rates = [64000, 96000, 128000, 80000]
    frames, nb, bfi = make_dec_case(fs, ms, 0, 1, rates, T1 + T2, seed=61)
    A = amd.DecBatch(4, fs, 1, ms, 0, nb, device=0)
    Bb = amd.DecBatch(7, fs, 1, ms, 0, [80] * 7, device=0)
    A.decode(frames[:, :T1], bfi[:, :T1])
    other = np.zeros((7, T1, frames.shape[2]), np.uint8); other[:4] = frames[:, :T1][::-1]
    Bb.decode(other, np.zeros((7, T1), np.uint8))
    size = A.stream_state_size
    assert size == 16 + 2456 * 4
    if via == "host":
        blob = A.export_streams([1])
        Bb.import_streams([5], blob)
    else:
        d_blob = dev.zeros(size)
        A.export_streams_device([1], d_blob, sync=True)
        Bb.import_streams_device([5], d_blob, sync=True)
        blob = dev.get(d_blob, (1, size), np.uint8)
    assert (blob[0, 16:] == _slices(A.get_state(), 4, 1, 2456)[1]).all()
    Bb.set_num_bytes(5, nb[1])
    pa, sa = A.decode(frames[:, T1:], bfi[:, T1:])
    fin = np.zeros((7, T2, frames.shape[2]), np.uint8); fin[5] = frames[1, T1:]
    fb = np.zeros((7, T2), np.uint8); fb[5] = bfi[1, T1:]
    pb, sb = Bb.decode(fin, fb)
    want, wst = oracle_decode_streams(frames, nb, bfi, fs, ms, 0, 1)
    assert (pb[5] == pa[1]).all() and (sb[5] == sa[1]).all()
    _dec_check(pa, sa, want[:, T1:], wst[:, T1:], "A")
    A.close(); Bb.close()


def test_header_mismatch_device_and_host(dev):
    """A device buffer of exactly n x stream_state_size bytes of the importing decoder batch: slot 0 a good blob, slot 1 the blob of a 32 kHz decoder
    (same size, other header), slot 2 an encoder blob, slot 3 a good blob.  Status 1, 1 for slots 1 and 2, whose streams continue as in a twin batch
    without the import; 0 for the others, which are imported.  The same import from host memory returns LC3_ERROR and changes nothing."""
    fs, ms = 48000, 10.0
    amd = _amd()
    rates = [64000, 80000, 96000, 128000, 64000]
    frames, nb, bfi = make_dec_case(fs, ms, 0, 1, rates, 16, seed=71)
    D = amd.DecBatch(5, fs, 1, ms, 0, nb, device=0)
    twin = amd.DecBatch(5, fs, 1, ms, 0, nb, device=0)
    src = amd.DecBatch(5, fs, 1, ms, 0, nb, device=0)
    src.decode(frames[:, :8][::-1].copy(), bfi[:, :8])                  # other histories
    for x in (D, twin):
        x.decode(frames[:, :8], bfi[:, :8])
    d32 = amd.DecBatch(2, 32000, 1, ms, 0, [80, 80], device=0)
    enc = amd.Batch(2, fs, 1, ms, 0, [64000, 64000], device=0)
    size = D.stream_state_size
    good = src.export_streams([0, 3])
    mixed = np.zeros((4, size), np.uint8)
    mixed[0] = good[0]; mixed[3] = good[1]
    mixed[1] = d32.export_streams([1])[0]
    e = enc.export_streams([0])[0]; mixed[2, :e.size] = e
    streams = [4, 1, 2, 0]
    d_blob, d_st = dev.put(mixed), dev.put(np.full(4, 0xEE, np.uint8))
    before = D.get_state()
    with pytest.raises(amd.LC3Error) as err:
        D.import_streams(streams, mixed)
    assert err.value.code == LC3_ERROR and (D.get_state() == before).all()
    D.import_streams_device(streams, d_blob, d_st, sync=True)
    assert dev.get(d_st, 4, np.uint8).tolist() == [0, 1, 1, 0]
    twin.import_streams([4, 0], good)                                    # what the good slots do
    assert (D.get_state() == twin.get_state()).all()
    p1, s1 = D.decode(frames[:, 8:], bfi[:, 8:])
    p2, s2 = twin.decode(frames[:, 8:], bfi[:, 8:])
    assert (p1 == p2).all() and (s1 == s2).all()
    for x in (D, twin, src, d32):
        x.close()
    enc.close()


def test_argument_errors_change_nothing(dev):
    amd = _amd()
    fs, ms, B, T = 48000, 10.0, 4, 10
    pcm = make_pcm(fs, ms, 1, B, 2 * T, seed=81)
    b = amd.Batch(B, fs, 1, ms, 0, [64000] * B, device=0)
    twin = amd.Batch(B, fs, 1, ms, 0, [64000] * B, device=0)
    b.encode(pcm[:, :T]); twin.encode(pcm[:, :T])
    L, size = b.lib, b.stream_state_size
    st = np.array([0, 1], np.int32)
    d_blob = dev.zeros(2 * size + 16)
    blob = np.zeros((2, size), np.uint8)
    for call, code in ((lambda: L.lc3plus_enc_batch_reset_streams(b.h, None, 1, None, None, 1), LC3_NULL_ERROR),
                       (lambda: L.lc3plus_enc_batch_reset_streams(None, st.ctypes.data, 1, None, None, 1), LC3_NULL_ERROR),
                       (lambda: L.lc3plus_enc_batch_export_streams(b.h, st.ctypes.data, 2, None, 0, None, 1), LC3_NULL_ERROR),
                       (lambda: L.lc3plus_enc_batch_import_streams(b.h, None, 2, blob.ctypes.data, 0, None, None, 1), LC3_NULL_ERROR),
                       (lambda: L.lc3plus_enc_batch_reset_streams(b.h, st.ctypes.data, 0, None, None, 1), LC3_ERROR),
                       (lambda: L.lc3plus_enc_batch_reset_streams(b.h, st.ctypes.data, -2, None, None, 1), LC3_ERROR),
                       (lambda: L.lc3plus_enc_batch_import_streams(b.h, st.ctypes.data, 2, C.c_void_p(d_blob + 8), 1, None, None, 1), LC3_ERROR)):
        assert call() == code
    for streams, code in (([B], LC3_ERROR), ([-1], LC3_ERROR), ([1, 1], LC3_ERROR), ([0, 2, 0], LC3_ERROR)):
        with pytest.raises(amd.LC3Error) as e:
            b.reset_streams(streams)
        assert e.value.code == code
        with pytest.raises(amd.LC3Error) as e:
            b.export_streams_device(streams, d_blob)
        assert e.value.code == code
    for rates in ([64000, 0], [64000, 10 ** 7], [-5, 64000], [64000, 15000]):
        with pytest.raises(amd.LC3Error) as e:
            b.reset_streams([0, 1], bitrates=rates)
        assert e.value.code == LC3_BITRATE_ERROR
    with pytest.raises(amd.LC3Error) as e:
        b.import_streams([0, 1], blob)                                   # zero headers
    assert e.value.code == LC3_ERROR
    assert [b.num_bytes(s) for s in range(B)] == [80] * B
    assert (b.get_state() == twin.get_state()).all()
    assert (b.encode(pcm[:, T:]) == twin.encode(pcm[:, T:])).all()
    b.close(); twin.close()
    frames, nb, bfi = make_dec_case(fs, ms, 0, 1, [64000] * B, 2 * T, seed=82)
    d = amd.DecBatch(B, fs, 1, ms, 0, nb, device=0)
    dt = amd.DecBatch(B, fs, 1, ms, 0, nb, device=0)
    d.decode(frames[:, :T], bfi[:, :T]); dt.decode(frames[:, :T], bfi[:, :T])
    assert d.lib.lc3plus_dec_batch_reset_streams(d.h, None, 1, None, None, 1) == LC3_NULL_ERROR
    for streams, code in (([B], LC3_ERROR), ([2, 2], LC3_ERROR)):
        with pytest.raises(amd.LC3Error) as e:
            d.reset_streams(streams)
        assert e.value.code == code
    for sizes in ([80, 19], [401, 80], [0, 80]):
        with pytest.raises(amd.LC3Error) as e:
            d.reset_streams([0, 1], num_bytes=sizes)
        assert e.value.code == LC3_NUMBYTES_ERROR
    assert [d.num_bytes(s) for s in range(B)] == [80] * B
    assert (d.get_state() == dt.get_state()).all()
    p1, s1 = d.decode(frames[:, T:], bfi[:, T:]); p2, s2 = dt.decode(frames[:, T:], bfi[:, T:])
    assert (p1 == p2).all() and (s1 == s2).all()
    d.close(); dt.close()
