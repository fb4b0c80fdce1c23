"""GPU parity through long quiet (quiet_tails.py; test_quiet_tails_cpu.py shows on the CPU that the inputs reach what they are for).  Encoder: streams
whose 12.8 kHz signal decays for half a second through the subnormals to exactly zero - one that sticks in the subnormals for good, one that restarts on
a tiny normal state, one that gets +-1 samples on a subnormal one - on the pipelined kernels, the one-wave kernel, the traced kernel and under overlapped
calls, with call boundaries inside the subnormal window so that the state crosses HBM while it is subnormal; the exported blobs of the two paths.
Decoder: loss bursts up to and past the last audible concealed frame and one of 600 frames, whose float output ends subnormal and not zero, through every
entry point, the traced kernel and a checkpoint in the middle of the burst.  Every comparison is equality with the oracle (portable math): bytes, LTPF
words, samples, status; floats bit for bit with +0 equal to -0 and nothing else forgiven - a subnormal against 0 fails.

Where a subnormal shows.  Once a signal is that quiet the bitstream is that of silence and the PCM is zero: a library built to flush subnormals passes
every byte and sample comparison here.  What the kernels computed is in the traces - but a traced encode runs the one-wave kernel, a traced decode not
the four-frames-a-wave IMDCT - and in the state: the encoder's blob holds the last 384 samples of the HP50 output, the decoder's the last 861 samples
it put out.  So the product-path tests export the streams behind calls that end inside the subnormal window and compare those words with the oracle's
trace (_check_history, test_decoder_state_in_the_long_burst_holds_the_oracle_s_subnormals); a flushing build fails them in every family."""
import ctypes as C

import numpy as np
import pytest

import quiet_tails as qt
from lc3_harness import DecTrace, Trace, oracle_decode_streams
from test_gpu_dec_varsize_device import _Hip, _device_calls
from test_gpu_enc_ragged_pipe import _records_words

pytestmark = pytest.mark.gpu
SENT = 0xA5
FR_LTPF = 48                                                             # csrc/lc3_plan.h: 4 ints, LTPF flag, active, pitch index, side bits
S = len(qt.CLASSES)
F48_10, F48_2P5, F16_10 = qt.FAMILIES[0], qt.FAMILIES[2], qt.FAMILIES[3]
FAM = pytest.mark.parametrize("family", qt.FAMILIES, ids=qt.fam_id)


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


def _batch(family):
    fs, ms, hr, rate = family
    return _amd().Batch(S, fs, 1, ms, hr, [rate] * S, device=0)


def _cuts(T, n, pipelined=False, start=0):
    """call boundaries from start in steps of n up to T; pipelined: a last call of fewer than 9 frames is joined to the one before, so that every call
    runs the pipelined kernels"""
    c = list(range(start, T, n)) + [T]
    if pipelined and len(c) > 2 and c[-1] - c[-2] < 9:
        del c[-2]
    return c


def _same_bits(a, c):
    """the rule of test_stage_traces_match_oracle: floats bit for bit, +0 equal to -0"""
    a, c = np.asarray(a), np.asarray(c)
    if a.dtype.kind != "f":
        return a == c
    return (a.view(np.uint32) == c.view(np.uint32)) | ((a == 0) & (c == 0))


def _feed(dev, bat, r, cuts, ltpf=None, each=True, after=None):
    """encode_device over [cuts[k], cuts[k + 1]) -> uint8 [S, frames, stride].  ltpf: an int32 [S, T, 4] array that takes the LTPF words of the records
    of every call that leaves some.  each: wait and read the status behind every call, else queue all calls and wait once.  after(b): called behind
    the call that ends at frame b."""
    stride, outs = bat.stride, []
    ins = [(dev.put(np.ascontiguousarray(r["pcm"][:, a:b])), dev.put(np.full((S, b - a, stride), SENT, np.uint8)), a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    dev.sync()
    for d_pcm, d_out, a, b in ins:
        bat.encode_device(d_pcm, 16, b - a, d_out, stride)
        if each:
            dev.sync()
            assert not bat.last_status(b - a).any(), (a, b)
            if ltpf is not None and _records_words(bat, b - a)[0] > 0:
                ltpf[:, a:b] = bat.last_records(b - a).view(np.int32)[:, :, FR_LTPF:FR_LTPF + 4]
            if after is not None:
                after(b)
    dev.sync()
    return np.concatenate([dev.get(d_out, (S, b - a, stride), np.uint8) for _, d_out, a, b in ins], axis=1)


def _check_bytes(got, r, what, t0=0):
    want = r["frames"][:, t0:t0 + got.shape[1]]
    nb = want.shape[2]
    bad = np.argwhere((got[:, :, :nb] != want).any(axis=2) | (got[:, :, nb:] != SENT).any(axis=2))
    assert len(bad) == 0, (what, len(bad), "first differing (class, frame)", [(qt.CLASSES[s], t0 + t) for s, t in bad[:8].tolist()])


def _blob_rows(blob, family):
    """the state rows of exported blobs [n, 16-byte header + LC3D_STATE_WORDS words] with the one legitimate difference between the paths set to 0: words
    [LC3D_ST_XPREV, LC3D_ST_XPREV + slot - (N - la_zeros)), the part of the MDCT-memory slot in front of the memory itself (right-aligned in a slot of
    300 words, 600 in the large layout).  No kernel reads them, and a pipelined call hands them over from LDS its front kernel never wrote
    (test_gpu_pcm_placed._enc_state_rows).  At 48 kHz / 10 ms the memory fills the slot and nothing is masked.  Everything from LC3D_ST_H12 on - the
    12.8 kHz and 6.4 kHz histories, the HP50 state and the pitch and LTPF words among the scalars - is compared.  -> header, rows, slot"""
    fs, ms, hr, rate = family
    N = qt.frame_len(fs, ms)
    ml = N - {10.0: 3 * N // 8, 5.0: N // 4, 2.5: 0}[ms]
    mc = 600 if N > 480 or ml > 300 else 300
    rows = np.ascontiguousarray(blob[:, 16:]).view(np.uint32).copy()
    assert rows.shape[1] == mc + 660 and mc - ml >= 0
    rows[:, :mc - ml] = 0                                                # never reaches LC3D_ST_H12 = mc
    return blob[:, :16], rows, mc


def _check_history(rows, mc, family, at, what):
    """The 12.8 kHz history of blobs exported behind frame at - 1 (LC3D_ST_H12 = the slot's end, 384 words, the newest sample last) against the oracle.
    It is the HP50 output itself, which the oracle's s12k8 trace shows 24 samples late: frame t's s12k8[i] is sample t * len12 + i - 24 of that stream.
    So every word of the history is in the trace of the frames up to the export and of the one behind it (the newest 24 samples; behind the last frame
    there is none, and they are left out).  Bit for bit, +0 equal to -0; a subnormal against 0 fails.  -> the oracle's words, float32 [S, n]"""
    r = qt.enc_oracle(family)
    T, len12 = r["pcm"].shape[1], int(128 * family[1] / 10)
    stream12 = np.ascontiguousarray(r["s12k8"][:, :, :len12]).reshape(S, -1)
    first = max(0, 360 - at * len12)                                     # early in the stream the oldest words are older than the stream
    n = 384 if at < T else 360
    want = stream12[:, at * len12 - 360 + first:at * len12 - 360 + n]
    got = rows[:, mc + first:mc + n].view(np.float32)
    bad = np.argwhere(~_same_bits(got, want))
    assert len(bad) == 0, (what, at, len(bad), [(qt.CLASSES[s], first + i, got[s, i].item(), want[s, i].item()) for s, i in bad[:8].tolist()])
    return want


# ---- the encoder ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["calls_of_20", "cut_in_the_subnormal_window"])
@FAM
def test_product_path_bytes_and_ltpf_words(dev, family, run):
    """the pipelined kernels in calls of 20 frames, and in calls of the length quiet_tails.cut_length picks: a call boundary then falls inside the
    subnormal window of every tail class, and the HP50 state, the 12.8 kHz history and the pitch words cross HBM while they are subnormal.  Bytes of
    every frame of every stream, and the LTPF words of the records of every call that leaves records (all of them but in the large layout).  In the second
    run the streams are exported behind every call and the blobs' 12.8 kHz history is compared with the oracle's (_check_history): the bitstream of a
    frame that quiet no longer depends on the signal, the history is the signal."""
    r = qt.enc_oracle(family)
    T = r["pcm"].shape[1]
    n = 20 if run == "calls_of_20" else qt.cut_length(family)[0]
    cuts = _cuts(T, n, pipelined=True)
    ltpf = np.full((S, T, 4), -99, np.int32)
    bat = _batch(family)
    seen = []
    def history(b):                                                          # the 12.8 kHz history in the blobs behind the call, against the oracle
        _, rows, mc = _blob_rows(bat.export_streams(range(S)), family)
        w = np.abs(_check_history(rows, mc, family, b, run)[:, -int(128 * family[1] / 10):])
        seen.append(((w > 0) & (w < qt.FLT_MIN)).any(axis=1))
    got = _feed(dev, bat, r, cuts, ltpf=ltpf, after=history if run != "calls_of_20" else None)
    _check_bytes(got, r, run)
    if run != "calls_of_20":                                                 # some export of every tail class held subnormals
        assert len(seen) == len(cuts) - 1 and np.array(seen).any(axis=0)[[qt.CLASSES.index(k) for k in qt.TAILS]].all()
    if qt.frame_len(family[0], family[1]) <= 480:                       # LC3D_LAYOUT_BIG (96 kHz / 10 ms) hands over no records; a call that left none keeps -99
        bad = np.argwhere((ltpf != r["ltpf"]).any(axis=2))
        assert len(bad) == 0, (len(bad), [(qt.CLASSES[s], t, ltpf[s, t].tolist(), r["ltpf"][s, t].tolist()) for s, t in bad[:6].tolist()])
    bat.close()


@pytest.mark.parametrize("n", [8, 3, 1])
@pytest.mark.parametrize("family", [F48_10, F48_2P5], ids=qt.fam_id)
def test_short_path_bytes(family, n):
    """the one-wave kernel with its in-kernel HP50 and writer: calls of 8, 3 and 1 frames over the whole stream"""
    r = qt.enc_oracle(family)
    T = r["pcm"].shape[1]
    bat = _batch(family)
    got = np.concatenate([bat.encode(r["pcm"][:, a:b]) for a, b in zip(range(0, T, n), list(range(n, T, n)) + [T])], axis=1)
    assert _records_words(bat, T % n or n)[0] == 0
    nb = r["frames"].shape[2]
    bad = np.argwhere((got[:, :, :nb] != r["frames"]).any(axis=2))
    assert len(bad) == 0, (len(bad), [(qt.CLASSES[s], t) for s, t in bad[:8].tolist()])
    bat.close()


@pytest.mark.parametrize("family", [F48_10, F16_10], ids=qt.fam_id)
def test_traced_path_pitch_chain_bit_for_bit(family):
    """encode_traced, call after call of 21 frames over the whole stream: the 12.8 kHz signal, the pitch lag, the normalised correlation, the LTPF
    parameters and their bit count of every frame against the oracle's trace, floats bit for bit (+0 equals -0; a subnormal against 0 fails)"""
    r = qt.enc_oracle(family)
    T = r["pcm"].shape[1]
    bat = _batch(family)
    nb = r["frames"].shape[2]
    bad = []
    for a in range(0, T, 21):
        n = min(21, T - a)
        got, traces = bat.encode_traced(r["pcm"][:, a:a + n])
        if not np.array_equal(got[:, :, :nb], r["frames"][:, a:a + n]):
            bad.append(("bytes", [(qt.CLASSES[s], a + t) for s, t in np.argwhere((got[:, :, :nb] != r["frames"][:, a:a + n]).any(axis=2))[:4].tolist()]))
        for s in range(S):
            for t in range(n):
                g = Trace.from_buffer_copy(traces[s * n + t].tobytes()[:C.sizeof(Trace)])
                for f, want in (("s12k8", r["s12k8"][s, a + t]), ("T0", r["T0"][s, a + t]), ("normcorr", r["normcorr"][s, a + t]),
                                ("ltpf_param", r["ltpf"][s, a + t, :3]), ("ltpf_bits", r["ltpf"][s, a + t, 3])):
                    v = getattr(g, f)
                    v = np.ctypeslib.as_array(v) if hasattr(v, "__len__") else np.asarray([v], np.float32 if f == "normcorr" else np.int32)
                    same = _same_bits(v, np.atleast_1d(want))
                    if not same.all():
                        i = int(np.flatnonzero(~same)[0])
                        bad.append((qt.CLASSES[s], a + t, f, int((~same).sum()), "first", i, v[i].item(), np.atleast_1d(want)[i].item()))
    assert not bad, (len(bad), bad[:10])
    bat.close()


@pytest.mark.parametrize("family", [F48_10, F48_2P5], ids=qt.fam_id)
def test_blobs_of_the_two_paths_are_equal(dev, family):
    """Three batches on the same PCM: pipelined calls of 20, short calls of 8, and pipelined calls of 11, 37 and 23 frames in turn.  export_streams at a
    frame inside the subnormal window of all four plain tails, at one where their state is zero, and at the end: equal blobs, word for word, but for the
    words _blob_rows names.  And both against the oracle (_check_history): what the HP50 kernels computed while the signal was subnormal, which no byte
    of the bitstream shows any more."""
    r = qt.enc_oracle(family)
    T = r["pcm"].shape[1]
    win = qt.windows(family)
    lo, hi = max(win[k][0] for k in qt.PLAIN_TAILS), min(win[k][1] for k in qt.PLAIN_TAILS)
    p_sub, p_zero = (lo + 1 + hi) // 2, max(win[k][1] for k in qt.PLAIN_TAILS) + 9
    assert lo < p_sub <= hi and p_zero < T - 9
    for k in qt.PLAIN_TAILS:                                             # what crosses into the blob at p_sub is subnormal and not zero, at p_zero zero
        x = np.abs(r["s12k8"][qt.CLASSES.index(k)])
        assert 0 < x[p_sub - 1][x[p_sub - 1] > 0].max() < qt.FLT_MIN and not x[p_zero - 1].any()
    a, b, c = _batch(family), _batch(family), _batch(family)
    ragged = [0]
    while ragged[-1] < T:
        ragged.append(min(T, ragged[-1] + (11, 37, 23)[len(ragged) % 3]))
    if T - ragged[-2] < 9:
        del ragged[-2]
    for at, prev in ((p_sub, 0), (p_zero, p_sub), (T, p_zero)):
        _check_bytes(_feed(dev, a, r, _cuts(at, 20, pipelined=True, start=prev)), r, "pipelined", prev)
        _check_bytes(_feed(dev, b, r, _cuts(at, 8, start=prev)), r, "short", prev)
        ha, ra, mc = _blob_rows(a.export_streams(range(S)), family)
        hb, rb, _ = _blob_rows(b.export_streams(range(S)), family)
        assert np.array_equal(ha, hb)
        bad = np.argwhere(ra != rb)
        assert len(bad) == 0, (at, len(bad), [(qt.CLASSES[s], w) for s, w in bad[:12].tolist()])
        for name, rows in (("pipelined", ra), ("short", rb)):
            want = _check_history(rows, mc, family, at, name)
        if at == p_sub:                                                  # and what was compared there is subnormal and not zero in every plain tail
            for k in qt.PLAIN_TAILS:
                w = np.abs(want[qt.CLASSES.index(k), -128:])
                assert w.any() and w[w > 0].max() < qt.FLT_MIN, k
    _check_bytes(_feed(dev, c, r, ragged), r, "calls of 11, 37, 23")
    hc, rc, _ = _blob_rows(c.export_streams(range(S)), family)
    bad = np.argwhere(ra != rc)
    assert np.array_equal(ha, hc) and len(bad) == 0, (len(bad), [(qt.CLASSES[s], w) for s, w in bad[:12].tolist()])
    a.close(); b.close(); c.close()


def test_overlapped_calls_bytes(dev):
    """48 kHz / 10 ms in calls of 20 frames under set_input_ready(True): device pointers, every call queued behind the other, one wait at the end"""
    r = qt.enc_oracle(F48_10)
    bat = _batch(F48_10)
    bat.set_input_ready(True)
    cuts = _cuts(r["pcm"].shape[1], 20, pipelined=True)
    got = _feed(dev, bat, r, cuts, each=False)
    assert not bat.last_status(cuts[-1] - cuts[-2]).any()
    _check_bytes(got, r, "overlapped")
    bat.close()


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------------------
D48_10, D48_2P5 = qt.DEC_FAMILIES[0], qt.DEC_FAMILIES[1]
NP = len(qt.PATTERNS)


def _dec_batch(family, n=NP, nbytes=None):
    fs, ms, hr, ch, rate = family
    return _amd().DecBatch(n, fs, ch, ms, hr, [nbytes or qt.dec_case(family)["nbytes"]] * n, device=0)


def _dec_check(got, st, want, wst, t0=0, names=qt.PATTERNS):
    bad = np.argwhere((got != want).any(axis=(2, 3)))
    assert len(bad) == 0, (len(bad), "first differing (pattern, frame)", [(names[s], t0 + t) for s, t in bad[:8].tolist()])
    assert (st == wst).all(), [(names[s], t0 + t) for s, t in np.argwhere(st != wst)[:8].tolist()]


@pytest.mark.parametrize("family", qt.DEC_FAMILIES, ids=qt.dec_fam_id)
def test_decoder_bursts_in_every_family(family):
    """decode() with flags, cut so that a call boundary falls inside every burst and very_long is cut every 64 frames: the concealment words cross HBM
    between calls for the whole burst.  PCM sample for sample and the status."""
    r = qt.dec_case(family)
    d = _dec_batch(family)
    cuts = qt.dec_cuts()
    outs = [d.decode(r["frames"][:, a:b], r["bfi"][:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    _dec_check(np.concatenate([o[0] for o in outs], axis=1), np.concatenate([o[1] for o in outs], axis=1), r["pcm"], r["status"])
    d.close()


def test_decoder_state_in_the_long_burst_holds_the_oracle_s_subnormals():
    """48 kHz / 10 ms on the product kernels (decode() runs the four-frames-a-wave IMDCT, which a traced call does not): very_long's blob exported at
    frame 608, behind the last of its 600 lost frames.  Its LTPF output history (csrc/lc3_plan.h: DST_LY, of which the first 228 * 48000 / 12800 + 6 = 861 words are the
    last 861 samples the synthesis put out, the newest last) is the oracle's x_out over the last two frames, bit for bit (+0 equals -0; a subnormal
    against 0 fails), and two thirds of it are subnormals: the PCM of these frames has been all zero for 500 frames and shows nothing of it."""
    r = qt.dec_case(D48_10)
    i, at, ly = qt.PATTERNS.index("very_long"), qt.GOOD + qt.VERY_LONG, 861
    assert r["bfi"][i, qt.GOOD:at].all() and not r["bfi"][i, at]
    want = np.ascontiguousarray(r["x_out"][at - 2:at, 0]).reshape(-1)[-ly:]
    a = np.abs(want)
    assert ((a > 0) & (a < qt.FLT_MIN)).sum() > ly // 2 and not r["pcm"][i, at - 2:at].any()
    d = _dec_batch(D48_10)
    cuts = [c for c in qt.dec_cuts() if c < at] + [at]
    for x, y in zip(cuts[:-1], cuts[1:]):
        got, st = d.decode(r["frames"][:, x:y], r["bfi"][:, x:y])
        _dec_check(got, st, r["pcm"][:, x:y], r["status"][:, x:y], t0=x)
    blob = d.export_streams([i])
    DST_LY = 1560
    assert blob.shape == (1, 16 + 4 * (1560 + 864 + 16 + 16))
    got = np.ascontiguousarray(blob[0, 16:]).view(np.float32)[DST_LY:DST_LY + ly]
    bad = np.flatnonzero(~_same_bits(got, want))
    assert len(bad) == 0, (len(bad), [(int(j), got[j].item(), want[j].item()) for j in bad[:8]])
    d.close()


def test_decoder_device_flags_entry(dev):
    """sizes and loss flags in device memory, the calls queued behind each other and one wait"""
    r = qt.dec_case(D48_10)
    d = _dec_batch(D48_10)
    nb = np.full((NP, qt.DEC_T), r["nbytes"], np.int32)
    got, st = _device_calls(dev, d, r["frames"], nb, r["bfi"], qt.dec_cuts())
    _dec_check(got, st, r["pcm"], r["status"])
    d.close()


def test_decoder_flagged_and_parse_ahead_calls_alternate(dev):
    """Under set_input_ready(True), no host wait: parse-ahead calls without flags (8 good frames each) alternate with device-size calls that carry flags
    (81 frames each).  In the first flagged call every stream's burst starts at the call's first frame, in the second it ends at the call's last: the
    concealment words go from the parse-ahead call's bookkeeping on its own stream to the ordered call's on the caller's and back, every time in the
    middle of what the burst needs - the first lost frame behind a parse-ahead call, the first good frame behind a burst.  128 streams (the eight
    bursts 16 times), so that the calls have something to overlap with."""
    r = qt.dec_case(D48_10)
    K, L = qt.LAST_AUDIBLE[D48_10], qt.LAST_AUDIBLE[D48_10] + 10
    lens = (31, 45, K, K + 1, K + 10, 80, 40, 60)
    seg = [8, L, 8, L, 8]
    edges = np.cumsum([0] + seg)
    T = int(edges[-1])
    bfi = np.zeros((NP, T), np.uint8)
    for s, n in enumerate(lens):
        bfi[s, edges[1]:edges[1] + n] = 1
        bfi[s, edges[4] - n:edges[4]] = 1
    frames = np.ascontiguousarray(r["frames"][:, :T])
    want, wst = oracle_decode_streams(frames, [r["nbytes"]] * NP, bfi, 48000, 10.0, 0, 1)
    assert (wst == bfi).all() and want[2, edges[1] + K - 1].any() and not want[4, edges[1] + K:edges[1] + K + 10].any()
    reps = 16
    fr, fl = np.tile(frames, (reps, 1, 1)), np.tile(bfi, (reps, 1))
    B, N, stride = NP * reps, 480, frames.shape[2]
    d = _dec_batch(D48_10, n=B)
    ins = [dev.put(fr[:, a:b]) for a, b in zip(edges[:-1], edges[1:])]
    nbs = [dev.put(np.full((B, n), r["nbytes"], np.int32)) for n in seg]
    fls = [dev.put(fl[:, a:b]) for a, b in zip(edges[:-1], edges[1:])]
    sts = [dev.put(np.full((B, n), 0xEE, np.uint8)) for n in seg]
    outs = [dev.zeros(B * n * N * 2) for n in seg]
    dev.sync()
    d.set_input_ready(True)
    for k, n in enumerate(seg):
        if k % 2 == 0:
            d.decode_device(ins[k], stride, n, outs[k], 16, sync=False)
        else:
            d.decode_device_sizes(ins[k], stride, n, outs[k], nbs[k], fls[k], sts[k], sync=False)
    dev.sync()
    got = np.concatenate([dev.get(o, (B, n, 1, N), np.int16) for o, n in zip(outs, seg)], axis=1)
    for k in (1, 3):
        st = dev.get(sts[k], (B, seg[k]), np.uint8)
        assert (st == fl[:, edges[k]:edges[k + 1]]).all(), k
    for i in range(reps):
        bad = np.argwhere((got[i * NP:(i + 1) * NP] != want).any(axis=(2, 3)))
        assert len(bad) == 0, ("copy", i, len(bad), "first differing (stream, frame)", bad[:8].tolist())
    d.close()


def test_decoder_24_bit_output():
    """very_long and the bursts of K and K + 1 frames at 24 bits, where the concealment stays above zero for 35 frames longer"""
    r = qt.dec_case(D48_10)
    pick = [qt.PATTERNS.index(k) for k in ("burst_K", "burst_K1", "very_long")]
    d = _dec_batch(D48_10, n=len(pick))
    cuts = qt.dec_cuts()
    outs = [d.decode(r["frames"][pick, a:b], r["bfi"][pick, a:b], bps=24) for a, b in zip(cuts[:-1], cuts[1:])]
    got = np.concatenate([o[0] for o in outs], axis=1)
    assert got.dtype == np.int32
    _dec_check(got, np.concatenate([o[1] for o in outs], axis=1), r["pcm24"][pick], r["status"][pick], names=[qt.PATTERNS[i] for i in pick])
    d.close()


@pytest.mark.parametrize("family", [D48_10, D48_2P5], ids=qt.dec_fam_id)
def test_decoder_traced_long_burst_bit_for_bit(family):
    """decode_traced over very_long in calls of 64 frames: x_out bit for bit against the oracle's trace (+0 equals -0; a subnormal against 0 fails) for
    all 616 frames, the lost ones down to the subnormals; the integer fields on every good frame, and the loss flag on every frame"""
    r = qt.dec_case(family)
    i = qt.PATTERNS.index("very_long")
    N = r["pcm"].shape[3]
    d = _dec_batch(family, n=1)
    cuts = qt.dec_cuts()
    bad = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        got, st, traces = d.decode_traced(r["frames"][i:i + 1, a:b], r["bfi"][i:i + 1, a:b])
        _dec_check(got, st, r["pcm"][i:i + 1, a:b], r["status"][i:i + 1, a:b], t0=a, names=["very_long"])
        for t in range(a, b):
            g = DecTrace.from_buffer_copy(traces[t - a].tobytes()[:C.sizeof(DecTrace)])
            x = np.ctypeslib.as_array(g.x_out)[:N]
            same = _same_bits(x, r["x_out"][t, 0])
            if not same.all():
                j = int(np.flatnonzero(~same)[0])
                bad.append((t, "x_out", int((~same).sum()), "first", j, x[j].item(), r["x_out"][t, 0, j].item()))
            if not r["bfi"][i, t]:
                ints = qt.int_fields(g)
                if not np.array_equal(ints[1:], r["ints"][t, 0, 1:]):
                    bad.append((t, "integer fields", ints.tolist(), r["ints"][t, 0].tolist()))
    assert not bad, (len(bad), bad[:8])
    d.close()


def test_decoder_checkpoint_in_the_middle_of_the_long_burst():
    """get_state after 300 lost frames of very_long, set_state into a fresh batch, on to the end: the PCM, and a second get_state at the end, are those
    of the run that was never interrupted"""
    r = qt.dec_case(D48_10)
    at = qt.GOOD + 300
    cuts = [c for c in qt.dec_cuts() if c < at] + [at] + [c for c in qt.dec_cuts() if c > at]
    def run(d, a, b):
        cs = [c for c in cuts if a <= c <= b]
        outs = [d.decode(r["frames"][:, x:y], r["bfi"][:, x:y]) for x, y in zip(cs[:-1], cs[1:])]
        return np.concatenate([o[0] for o in outs], axis=1), np.concatenate([o[1] for o in outs], axis=1)
    whole = _dec_batch(D48_10)
    pw, sw = run(whole, 0, qt.DEC_T)
    _dec_check(pw, sw, r["pcm"], r["status"])
    first = _dec_batch(D48_10)
    p1, s1 = run(first, 0, at)
    state = first.get_state()
    first.close()
    second = _dec_batch(D48_10)
    second.set_state(state)
    p2, s2 = run(second, at, qt.DEC_T)
    _dec_check(np.concatenate([p1, p2], axis=1), np.concatenate([s1, s2], axis=1), r["pcm"], r["status"])
    assert second.get_state().tobytes() == whole.get_state().tobytes()
    whole.close(); second.close()
