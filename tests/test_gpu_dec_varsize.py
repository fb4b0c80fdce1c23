"""GPU tests of per-frame frame sizes in the batched decoder (lc3plus_dec_batch_decode_sizes, DecBatch.decode(num_bytes=...)):
streams whose bitrate changes from frame to frame, lost frames given as size 0 or bfi, against the CPU oracle decoder fed one frame
at a time with the frame's own size (R/dec_lc3_fl.c:134-163).  Bar: PCM identical sample for sample, status identical."""
import numpy as np
import pytest

from lc3_harness import Oracle, OracleDecoder, synth_pcm, make_dec_case

pytestmark = pytest.mark.gpu
LC3_ERROR, LC3_NUMBYTES_ERROR = 1, 7


def _amd():
    import audio_codec_amd
    return audio_codec_amd


def make_var_case(fs, ms, hr, channels, rates, B, T, seed, change=(1, 4), p_zero=0.08, p_bfi=0.08, p_flip=0.08, lost_head=0, rate_plan=None):
    """B streams encoded by the CPU oracle with the bitrate drawn from `rates` anew every change[0]..change[1] frames.  Returns frames [B, T, stride],
    num_bytes [B, T] (0 = lost), bfi [B, T], sizes [B, T] (every frame's encoded size).  rate_plan [B, T]: the bitrate of every frame instead.  Flips bytes of good frames (mono, or stereo frames whose size equals the last good one: where an earlier
    channel is corrupt the reference skips the size update of the later one, which the batch does not reproduce - INTEGRATION.md)."""
    rng = np.random.default_rng(seed)
    N = int((48000 if fs == 44100 else fs) * ms / 1000)
    pcm = synth_pcm(B * channels, T, N, fs, seed=seed).reshape(B, channels, T, N).transpose(0, 2, 1, 3)
    per, sizes = [], np.zeros((B, T), np.int32)
    def per_channel(rate):                                   # the bitrate of each channel's encoder for a stream-frame of `rate`
        n = rate * int(ms * 10) // 80000
        return [(n // channels + (c < n % channels)) * 80000 // int(ms * 10) for c in range(channels)]
    for b in range(B):
        # one mono encoder per channel: a stereo encoder splits its bitrate evenly, the decoder's split of an odd size gives the first channel a byte more
        enc = [Oracle(fs, 1, ms, hr, 64000 if hr == 0 else 256000) for _ in range(channels)]
        row, left = [], 0
        for t in range(T):
            rate = None
            if rate_plan is not None:
                rate = int(rate_plan[b, t])
            elif left == 0:
                rate = int(rates[rng.integers(len(rates))])
                left = int(rng.integers(change[0], change[1] + 1))
            if rate is not None:
                for o, r in zip(enc, per_channel(rate)):
                    assert o.set_bitrate(r) == 0
            left -= 1
            row.append(np.concatenate([o.encode(pcm[b, t, c][None]) for c, o in enumerate(enc)]))
            sizes[b, t] = row[-1].size
        per.append(row)
    stride = int(sizes.max())
    frames = np.zeros((B, T, stride), np.uint8)
    for b in range(B):
        for t in range(T):
            frames[b, t, :sizes[b, t]] = per[b][t]
    num_bytes = sizes.copy()
    bfi = np.zeros((B, T), np.uint8)
    u = rng.random((B, T))
    num_bytes[u < p_zero] = 0
    bfi[(u >= p_zero) & (u < p_zero + p_bfi)] = 1
    num_bytes[:, :lost_head] = 0
    for b in range(B):
        last = 0
        for t in range(T):
            good = num_bytes[b, t] and not bfi[b, t]
            if good and rng.random() < p_flip and (channels == 1 or num_bytes[b, t] == last):
                k = rng.integers(0, num_bytes[b, t], size=3)
                frames[b, t, k] ^= rng.integers(1, 256, size=3).astype(np.uint8)
            if good:
                last = num_bytes[b, t]
    return frames, num_bytes, bfi, sizes


def oracle_var(frames, num_bytes, bfi, fs, ms, hr, channels):
    B, T = num_bytes.shape
    out, status = None, np.zeros((B, T), np.uint8)
    for b in range(B):
        o = OracleDecoder(fs, channels, ms, hr, portable_math=True)
        if out is None:
            out = np.zeros((B, T, channels, o.N), np.int16)
        for t in range(T):
            nb = int(num_bytes[b, t])
            rc, pcm = o.decode(frames[b, t, :max(nb, 1)], int(bfi[b, t]), 16, num_bytes=nb)
            assert rc in (0, 2), rc
            out[b, t] = pcm
            status[b, t] = rc == 2
    return out, status


def _cmp(got, st, want, wst):
    bad = np.argwhere((got != want).any(axis=(2, 3)))
    assert len(bad) == 0, ("first differing (stream, frame)", bad[:6].tolist())
    assert (st == wst).all(), np.argwhere(st != wst)[:6].tolist()


CASES = [
    # 48 kHz / 10 ms: 80 / 90 / 100 / 110 bytes are the LTPF beta thresholds, more than 128 bytes leaves the LDS-staged parse kernel
    (48000, 10.0, 0, 1, [56000, 64000, 68000, 72000, 76000, 80000, 84000, 88000, 96000, 102400, 104000, 160000]),
    (48000, 5.0, 0, 1, [32000, 64000, 96000, 128000, 256000]),
    (48000, 2.5, 0, 1, [64000, 96000, 128000, 320000]),
    (32000, 5.0, 0, 1, [32000, 64000, 96000, 192000]),
    (16000, 10.0, 0, 1, [16000, 24000, 32000, 64000, 128000]),
    (8000, 2.5, 0, 1, [64000, 96000, 128000, 160000]),
    (48000, 10.0, 1, 1, [128000, 256000, 400000, 500000]),
    (96000, 2.5, 1, 1, [198400, 256000, 320000, 672000]),
    (96000, 10.0, 1, 1, [149600, 256000, 400000, 500000]),
    (48000, 10.0, 0, 1, [56000, 64000, 68000, 72000, 76000, 80000, 84000, 88000, 96000, 102400]),   # at most 128 bytes: every call staged in LDS
    (48000, 10.0, 0, 2, [128000, 128800, 144000, 160800, 176000, 204800, 232800]),   # odd stream sizes (161, 201, 291 bytes): the first channel a byte more
    (48000, 5.0, 0, 2, [64000, 129600, 192000, 257600]),                             # 81 and 161 bytes
]


@pytest.mark.parametrize("fs,ms,hr,channels,rates", CASES)
def test_varsize_vs_oracle(fs, ms, hr, channels, rates):
    B, T = 12, 40
    frames, num_bytes, bfi, _ = make_var_case(fs, ms, hr, channels, rates, B, T, seed=fs // 1000 + int(ms * 10) + hr + channels, lost_head=2)
    want, wst = oracle_var(frames, num_bytes, bfi, fs, ms, hr, channels)
    d = _amd().DecBatch(B, fs, channels, ms, hr, None, device=0)      # no size before the first good frame
    a, sa = d.decode(frames[:, :17], bfi[:, :17], num_bytes=num_bytes[:, :17])   # two calls: the carry crosses them
    b, sb = d.decode(frames[:, 17:], bfi[:, 17:], num_bytes=num_bytes[:, 17:])
    _cmp(np.concatenate([a, b], axis=1), np.concatenate([sa, sb], axis=1), want, wst)
    d.close()


def test_continuity_and_checkpoint():
    """A per-frame-size call, then fixed-size decode() calls, equal the oracle over the whole sequence; num_bytes(stream) is the last good size;
    get_state / set_state into a batch created with those sizes continues identically."""
    fs, ms, B, T1, T2 = 48000, 10.0, 8, 24, 16
    rates = [64000, 80000, 96000, 120000, 160000]
    frames, num_bytes, bfi, sizes = make_var_case(fs, ms, 0, 1, rates, B, T1, seed=5)
    num_bytes[:, 0] = sizes[:, 0]; bfi[:, 0] = 0                  # the batch is created with a size the oracle does not know: start with a good frame
    # the fixed-size tail: every stream continues at the size of its last good frame of the first part
    last = np.array([[x for x, l in zip(num_bytes[b], bfi[b]) if x and not l][-1] for b in range(B)])
    pcm = synth_pcm(B, T1 + T2, 480, fs, seed=5)
    tail = np.zeros((B, T2, frames.shape[2] if frames.shape[2] >= last.max() else last.max()), np.uint8)
    for b in range(B):
        # an encoder at that size on other content is as good a bitstream as any: the decoder only has to agree with the oracle
        o = Oracle(fs, 1, ms, 0, int(last[b]) * 800)
        for t in range(T2):
            tail[b, t, :last[b]] = o.encode(pcm[b, T1 + t][None])
    all_nb = np.concatenate([num_bytes, np.repeat(last[:, None], T2, axis=1)], axis=1)
    all_bfi = np.concatenate([bfi, np.zeros((B, T2), np.uint8)], axis=1)
    stride = max(frames.shape[2], tail.shape[2])
    all_fr = np.zeros((B, T1 + T2, stride), np.uint8)
    all_fr[:, :T1, :frames.shape[2]] = frames; all_fr[:, T1:, :tail.shape[2]] = tail
    want, wst = oracle_var(all_fr, all_nb, all_bfi, fs, ms, 0, 1)
    amd = _amd()
    d = amd.DecBatch(B, fs, 1, ms, 0, [100] * B, device=0)
    a, sa = d.decode(frames, bfi, num_bytes=num_bytes)
    assert [d.num_bytes(b) for b in range(B)] == [int(x) for x in last]
    st = d.get_state()
    b1, sb1 = d.decode(tail)
    _cmp(np.concatenate([a, b1], axis=1), np.concatenate([sa, sb1], axis=1), want, wst)
    d2 = amd.DecBatch(B, fs, 1, ms, 0, [int(x) for x in last], device=0)
    d2.set_state(st)
    b2, sb2 = d2.decode(tail)
    assert (b2 == b1).all() and (sb2 == sb1).all()
    d.close(); d2.close()


@pytest.mark.parametrize("T", [1, 7, 64])
def test_equal_sizes_match_fixed_path(T):
    """All sizes equal to the configured ones, no zeros: byte-identical to lc3plus_dec_batch_decode on the same input."""
    rates = [32000, 64000, 96000, 128000, 160000, 256000]
    frames, nbytes, bfi = make_dec_case(48000, 10.0, 0, 1, rates, T, seed=T)
    amd = _amd()
    d1 = amd.DecBatch(len(rates), 48000, 1, 10.0, 0, nbytes, device=0)
    d2 = amd.DecBatch(len(rates), 48000, 1, 10.0, 0, nbytes, device=0)
    for k in range(2):
        p1, s1 = d1.decode(frames, bfi)
        p2, s2 = d2.decode(frames, bfi, num_bytes=np.repeat(np.array(nbytes)[:, None], T, axis=1))
        assert (p1 == p2).all() and (s1 == s2).all()
    d1.close(); d2.close()


def test_validation_leaves_sizes_unchanged():
    amd = _amd()
    B, T = 3, 4
    frames, nbytes, bfi = make_dec_case(48000, 10.0, 0, 1, [64000, 96000, 128000], T, seed=3)
    wide = np.zeros((B, T, 420), np.uint8); wide[:, :, :frames.shape[2]] = frames
    d = amd.DecBatch(B, 48000, 1, 10.0, 0, nbytes, device=0)
    nb = np.repeat(np.array(nbytes)[:, None], T, axis=1)
    # (frames, size put at stream 1 frame 2, flag put at stream 2 frame 1, expected error)
    for fr, bad_nb, bad_flag, code in ((frames, 19, 0, LC3_NUMBYTES_ERROR), (wide, 401, 0, LC3_NUMBYTES_ERROR),
                                        (frames, frames.shape[2] + 1, 0, LC3_NUMBYTES_ERROR), (frames, 80, 2, LC3_ERROR)):
        x = nb.copy(); f = np.zeros((B, T), np.uint8)
        x[1, 2] = bad_nb; f[2, 1] = bad_flag
        with pytest.raises(amd.LC3Error) as e:
            d.decode(fr, f, num_bytes=x)
        assert e.value.code == code
        assert [d.num_bytes(b) for b in range(B)] == list(nbytes)
    d.close()


def test_per_frame_sizes_between_ahead_calls():
    """Under the input-ready promise: asynchronous device-pointer calls without flags (ahead), a per-frame-size call, more ahead calls, then a call with
    bfi whose first frame is lost - against the oracle over the whole sequence (the ahead call after an ordered call waits for all of it)."""
    from test_gpu_parity import _Dev
    amd = _amd()
    d = _Dev()
    try:
        U, reps, T = 64, 32, 16                                          # 2048 streams: the calls overlap
        fs, ms = 48000, 10.0
        rng = np.random.default_rng(77)
        choice = np.array([64000, 80000, 96000, 104000, 128000])
        plan = choice[rng.integers(len(choice), size=(U, 6 * T))]
        plan[:, :2 * T] = plan[:, :1]                                    # calls 0 and 1: ahead, one size per stream
        plan[:, 3 * T:5 * T] = plan[:, 3 * T - 1:3 * T]                  # calls 3 and 4: ahead, at the last size of the per-frame-size call 2
        frames, num_bytes, bfi, _ = make_var_case(fs, ms, 0, 1, None, U, 6 * T, seed=77, p_zero=0, p_bfi=0, p_flip=0, rate_plan=plan)
        call5_bfi = np.zeros((U, T), np.uint8); call5_bfi[:, 0] = 1
        all_bfi = np.zeros((U, 6 * T), np.uint8); all_bfi[:, 5 * T:] = call5_bfi
        all_nb = num_bytes.copy()
        want, wst = oracle_var(frames, all_nb, all_bfi, fs, ms, 0, 1)
        B = U * reps
        fr = np.ascontiguousarray(np.tile(frames, (reps, 1, 1))); stride = fr.shape[2]
        dec = amd.DecBatch(B, fs, 1, ms, 0, [int(x) for x in np.tile(num_bytes[:, 0], reps)], device=0)
        N = dec.N
        ins = [d.put(fr[:, k * T:(k + 1) * T]) for k in range(6)]
        outs = [d.zeros(B * T * N * 2) for _ in range(6)]
        d.sync()
        dec.set_input_ready(True)
        for k in range(6):
            if k in (0, 1, 3, 4):
                dec.decode_device(ins[k], stride, T, outs[k], 16, sync=False)
            elif k == 2:
                dec.decode_device(ins[k], stride, T, outs[k], 16, sync=False, num_bytes=np.tile(num_bytes[:, 2 * T:3 * T], (reps, 1)))
            else:
                dec.decode_device(ins[k], stride, T, outs[k], 16, sync=False, num_bytes=np.tile(num_bytes[:, 5 * T:], (reps, 1)),
                                  bfi=np.tile(call5_bfi, (reps, 1)))
        d.sync()
        out = np.concatenate([d.get(outs[k], (B, T, 1, N), np.int16) for k in range(6)], axis=1)
        for r in range(reps):
            bad = np.argwhere((out[r * U:(r + 1) * U] != want).any(axis=(2, 3)))
            assert len(bad) == 0, ("copy", r, "first differing (stream, frame)", bad[:4].tolist())
    finally:
        d.free()


def test_golden_reference_variable_sizes():
    """tests/golden/d2_variable_frame_sizes.npz: streams the unmodified ETSI encoder made with its bitrate switched every one to three frames,
    damaged on purpose, and the PCM / status the unmodified ETSI decoder produced from them one frame at a time (make_golden_dec_var.py):
    one call per stream set, no size known before the first good frame."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "d2_variable_frame_sizes.npz"))
    for tag in g["tags"]:
        tag = str(tag)
        fs, dms, hr, ch = (int(v) for v in g[tag + "_cfg"])
        frames, num_bytes, bfi = g[tag + "_frames"], g[tag + "_num_bytes"], g[tag + "_bfi"]
        d = _amd().DecBatch(frames.shape[0], fs, ch, dms / 10.0, hr, None, device=0)
        got, status = d.decode(frames, bfi, num_bytes=num_bytes)
        assert (status == g[tag + "_status"]).all(), tag
        bad = np.argwhere((got != g[tag + "_pcm"]).any(axis=(2, 3)))
        assert len(bad) == 0, (tag, bad[:4].tolist())
        d.close()


@pytest.mark.parametrize("fs,ms,channels,rates,g192", [(48000, 10.0, 1, [32000, 64000, 80000, 96000, 128000], 0),
                                                        (48000, 10.0, 2, [40000, 64000, 96000], 1),
                                                        (32000, 5.0, 1, [32000, 64000, 96000], 1)])
def test_cli_bitrate_switching_file(tmp_path, fs, ms, channels, rates, g192):
    """tools/lc3plus_dec_cli on files the reference CLI encoded with a bitrate switching file (-swf, a new rate every 1-3 frames), in the
    .lc3plus container and in G.192, with frames lost through an error pattern file: the same WAV and error detection file as the reference CLI."""
    import os, subprocess
    from lc3_harness import ORACLE_DIR
    from test_gpu_parity import _write_wav
    ref_cli = os.path.join(ORACLE_DIR, "_ref", "LC3plus")
    if not os.path.exists(ref_cli):
        pytest.skip("the reference CLI (oracle/_ref/LC3plus) is not built")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "tools", "lc3plus_dec_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-s", "-C", root, "cli"])
    rng = np.random.default_rng(fs + channels + g192)
    N = int(fs * ms / 1000); T = 300                               # more than one block of 256 frames
    pcm = synth_pcm(channels, T, N, fs, seed=43)                   # [channels, T, N]
    wav = tmp_path / "in.wav"
    _write_wav(wav, pcm.reshape(channels, -1).T.reshape(-1), fs, channels, 16)
    plan, left = [], 0
    while len(plan) < T:
        r = int(rates[rng.integers(len(rates))]); plan += [r] * int(rng.integers(1, 4))
    swf = tmp_path / "rates.swf"; np.array(plan[:T], dtype="<i8").tofile(swf)    # per channel (R/codec_exe.c:296-302)
    bs = tmp_path / "in.lc3plus"
    fmt = ["-formatG192"] if g192 else []
    subprocess.check_call([ref_cli, "-E", "-q", "-frame_ms", str(ms), "-swf", str(swf)] + fmt + [str(wav), str(bs), str(rates[0])], stdout=subprocess.DEVNULL)
    epf = tmp_path / "loss.dat"; (rng.random(T) < 0.1).astype("<i2").tofile(epf)
    opts = ["-q", "-epf", str(epf)] + fmt
    ours, oedf, theirs, tedf = tmp_path / "ours.wav", tmp_path / "ours.edf", tmp_path / "ref.wav", tmp_path / "ref.edf"
    subprocess.check_call([cli, "-D"] + opts + ["-edf", str(oedf), str(bs), str(ours)])
    subprocess.check_call([ref_cli, "-D"] + opts + ["-edf", str(tedf), str(bs), str(theirs)], stdout=subprocess.DEVNULL)
    got, ref = open(ours, "rb").read(), open(theirs, "rb").read()
    assert open(oedf, "rb").read() == open(tedf, "rb").read()
    assert len(ref) == len(got) and ref[:44] == got[:44]
    # as test_cli_decoder_front_end: the reference's host powf() against the device's (float)pow((double)) may put a sample one LSB apart
    a, b = (np.frombuffer(x[44:], dtype="<i2").astype(np.int64) for x in (ref, got))
    assert (np.abs(a - b) <= 1).all() and (a == b).mean() > 0.999
