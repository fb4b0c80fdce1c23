"""GPU: parity at every call shape (tests/call_shapes.py) - how many frames a call holds, how many channel-streams the batch has, which call came before it.

One test per sequence, parametrised by geometry.  The calls are made in order on one batch through the device-pointer API, each inside api.launch_census(): the
launches of the kernels that expose a shape rule equal call_shapes.expected_launches (a call that took another path cannot pass), every (stream, frame) of every call
equals the portable-math CPU oracle's continuous run - bytes and num_bytes, or samples and status - every output buffer starts as sentinels and what a call may not
write keeps them, last_status is clear, and the batch ends in the state of a twin batch that took the same frames in calls of 12.  tests/test_call_shapes_cpu.py
holds what the sequences reach.

What the API does not give is not compared: under the encoder's promise the calls are queued with no host wait, and last_status is the last call's only, so the
status words of the calls before it in a promised sequence are not read (the ordered sequences read them after every call); the decoder's call without flags
returns no status, so under its promise the samples alone are compared (a concealed frame's samples are the concealment's).

Every case prints its frames and wall time (pytest -s)."""
import time

import numpy as np
import pytest

import call_shapes as cs
from test_gpu_dec_varsize_device import _Hip
from test_gpu_enc_ragged_pipe import _ends_like

pytestmark = pytest.mark.gpu
SENT, GUARD, END_GUARD, PCM_SENT = 0xA5, 8, 256, 0x5A5A


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


def _report(what, name, frames, t0):
    print("call_shapes %-14s %-14s frames %6d wall %.2f s" % (what, name, frames, time.perf_counter() - t0))


def _launches(kind, ran, expect, where):
    got = {k: ran.get(k, 0) for k in expect}
    assert got == expect, (kind, where, {k: (got[k], expect[k]) for k in expect if got[k] != expect[k]})


# ---- encoder --------------------------------------------------------------------------------------------------------------------------------------------------
def _enc_ends_like(a, b, g):
    """test_gpu_enc_ragged_pipe._ends_like itself: state (every word but the ones in front of the MDCT memory in its slot, every byte at 48 kHz / 10 ms), sizes and,
    outside high resolution, bandwidths of the two batches"""
    _ends_like(a, b, dict(B=g["S"], fs=g["fs"], ms=g["ms"], hr=g["hr"], ch=g["ch"], N=g["N"], nb=np.array(g["nbytes"], np.int32)[:, None]))


def _enc_sequence(dev, name, seq, ready=False, run_frames=0, monkeypatch=None):
    amd, t0 = _amd(), time.perf_counter()
    g, lengths = cs.enc_geometry(name), cs.sequence(seq)
    pcm, want = cs.enc_pcm(name, seq), cs.oracle_encode(name, seq)
    S, stride, st = g["S"], max(g["nbytes"]) + GUARD, cs.starts(lengths)
    if run_frames:
        monkeypatch.setenv("LC3PLUS_ENC_RUN_FRAMES", str(run_frames))        # read while the batch is created
    bat = amd.Batch(S, g["fs"], g["ch"], g["ms"], g["hr"], list(g["rates"]), device=0)
    if run_frames:
        monkeypatch.delenv("LC3PLUS_ENC_RUN_FRAMES")
    twin = amd.Batch(S, g["fs"], g["ch"], g["ms"], g["hr"], list(g["rates"]), device=0)
    assert [bat.num_bytes(s) for s in range(S)] == g["nbytes"]
    ins = [dev.put(pcm[:, st[k]:st[k + 1]]) for k in range(len(lengths))]
    outs = [dev.put(np.full(S * n * stride + END_GUARD, SENT, np.uint8)) for n in lengths]       # sentinels behind every frame and behind the buffer's last frame
    dev.sync()                                                               # the promise: all PCM is on the device before the first call
    if ready:
        bat.set_input_ready(True)
    shapes = cs.enc_shapes(g, lengths, ready, run_frames)
    for k, n in enumerate(lengths):
        with amd.api.launch_census() as ran:
            bat.encode_device(ins[k], 16, n, outs[k], stride, sync=not ready)
        _launches("enc", ran, cs.expected_launches("enc", g, shapes[k]), (name, seq, k, n))
        if not ready:
            assert not bat.last_status(n).any(), (name, k, n, np.argwhere(bat.last_status(n))[:6].tolist())
    dev.sync()
    assert not bat.last_status(lengths[-1]).any()                            # (under the promise: the last call's, the only one the API keeps)
    bad, over = [], []
    for k, n in enumerate(lengths):
        raw = dev.get(outs[k], (S * n * stride + END_GUARD,), np.uint8)
        assert (raw[S * n * stride:] == SENT).all(), (name, seq, k, "bytes behind the call's last frame were written")
        got = raw[:S * n * stride].reshape(S, n, stride)
        for s in range(S):
            nb = g["nbytes"][s]
            bad += [(k, s, t) for t in np.nonzero((got[s, :, :nb] != want[s, st[k]:st[k + 1], :nb]).any(axis=1))[0].tolist()]
            over += [(k, s, t) for t in np.nonzero((got[s, :, nb:] != SENT).any(axis=1))[0].tolist()]
    assert not bad, (name, seq, "frames that differ from the oracle (call, stream, frame)", len(bad), bad[:10], [lengths[k] for k, _, _ in bad[:10]])
    assert not over, (name, seq, "bytes behind a frame were written", over[:10])
    for a, b in zip(cs.starts(cs.twin_lengths(int(st[-1])))[:-1], cs.starts(cs.twin_lengths(int(st[-1])))[1:]):
        twin.encode_device(dev.put(np.ascontiguousarray(pcm[:, a:b])), 16, int(b - a), dev.put(np.zeros((S, int(b - a), stride), np.uint8)), stride, sync=True)
    _enc_ends_like(bat, twin, g)
    bat.close()
    twin.close()
    _report(seq + (" rf%d" % run_frames if run_frames else ""), name, S * int(st[-1]), t0)


@pytest.mark.parametrize("name", list(cs.ENC_FAMILIES))
def test_encoder_ordered_calls(dev, name):
    """1 ... 273 frames in a fixed shuffled order on five streams, one batch per kernel family: both sides of the one-wave limit, of every run count, of the cap at
    16 runs, of the pre-kernels' pieces, of both rate-stream rules, of the shape kernel's stream and of the five-wave writer"""
    _enc_sequence(dev, name, "enc_ordered")


@pytest.mark.parametrize("name", list(cs.ENC_COUNT_BATCHES))
def test_encoder_stream_counts(dev, name):
    """1, 2, 63, 64 and 65 mono streams and 3 stereo ones at 1, 9, 17 and 48 frames: the tails of the grids that are cut by channel-streams"""
    _enc_sequence(dev, name, "enc_count")


@pytest.mark.parametrize("name", list(cs.ENC_READY_FAMILIES))
def test_encoder_under_the_promise(dev, name):
    """five equal calls each of 5 ... 257 frames queued with no host wait: the first of a block is ordered (the length changed), the others overlap it up to 256
    frames; runs of 64"""
    _enc_sequence(dev, name, "enc_ready", ready=True)


@pytest.mark.parametrize("name,run_frames", cs.ENC_SMALL_RUN_CASES, ids=["%s-rf%d" % c for c in cs.ENC_SMALL_RUN_CASES])
def test_encoder_runs_of_one_two_and_three_frames(dev, monkeypatch, name, run_frames):
    """LC3PLUS_ENC_RUN_FRAMES = 1 and 3 at 9, 18 and 35 frames: front groups cut inside every run, fewer frames in a run than a wave takes; with 63 streams a run
    of one frame is 63 (stream, frame) pairs, a wave of the lane kernels less one lane"""
    _enc_sequence(dev, name, "enc_small_runs", run_frames=run_frames, monkeypatch=monkeypatch)


@pytest.mark.parametrize("name", list(cs.ENC_TAIL_BATCHES))
def test_encoder_whole_writer_workgroups(dev, name):
    """one stream, calls of 255, 256 and 257 frames: a whole workgroup of the writer and one frame either side - at 100 bytes the five-wave writer, at 101
    lc3_enc_pack_kernel (the size limit at it and above it); and calls of 20, 24 and 25 frames, the upper end of the second rate-stream rule"""
    _enc_sequence(dev, name, "enc_tails")


# ---- decoder --------------------------------------------------------------------------------------------------------------------------------------------------
def _dec_call(dev, d, c, how, a, b, d_fr, d_pcm, d_st, sync):
    """frames a ... b - 1 of the case as one call; -> the status the call returned on the host (hostsizes) or None"""
    g = c["g"]
    S, n, stride = g["S"], int(b - a), c["frames"].shape[2]
    if how == "fixed":
        d.decode_device(d_fr, stride, n, d_pcm, sync=sync)
    elif how == "hostsizes":
        nb, bfi = np.ascontiguousarray(c["sizes"][:, a:b]), np.ascontiguousarray(c["bfi"][:, a:b])
        st = np.full((S, n), 0xEE, np.uint8)
        rc = d.lib.lc3plus_dec_batch_decode_sizes(d.h, d_fr, 1, stride, nb.ctypes.data, bfi.ctypes.data, n, d_pcm, 1, 16, st.ctypes.data, None, 1)
        assert rc == 0, rc
        return st
    else:
        d.decode_device_sizes(d_fr, stride, n, d_pcm, dev.put(np.ascontiguousarray(c["sizes"][:, a:b])), dev.put(np.ascontiguousarray(c["bfi"][:, a:b])), d_st, sync=sync)
    return None


def _dec_sequence(dev, name, seq, how, S=None, role0=0):
    amd, t0 = _amd(), time.perf_counter()
    ready = how == "fixed"
    c = cs.dec_case(name, seq, S, role0, ready)
    want, wst = cs.oracle_decode(name, seq, S, role0, ready)
    g, lengths = c["g"], c["lengths"]
    S, ch, N, stride, st = g["S"], g["ch"], g["N"], c["frames"].shape[2], cs.starts(lengths)
    mk = lambda: amd.DecBatch(S, g["fs"], ch, g["ms"], g["hr"], list(g["sizes"]) if how == "fixed" else None, device=0)
    d, twin = mk(), mk()
    ins = [dev.put(c["frames"][:, st[k]:st[k + 1]]) for k in range(len(lengths))]
    outs = [dev.put(np.full(S * n * ch * N + N, PCM_SENT, np.uint16)) for n in lengths]
    sts = [dev.put(np.full(S * n + GUARD, 0xEE, np.uint8)) for n in lengths]
    dev.sync()                                                               # the promise: all frames are on the device before the first call
    if ready:
        d.set_input_ready(True)
    host_st = []
    for k, n in enumerate(lengths):
        a, b = int(st[k]), int(st[k + 1])
        flagged = c["bfi"][:, a:b].astype(bool)
        chan = np.array(g["chan_bytes"]).reshape(S, ch).max(axis=1)
        max_nb = int(chan.max()) if how == "fixed" else -(-stride // ch) if how == "sizes" else int(np.where(flagged, 0, chan[:, None]).max())
        with amd.api.launch_census() as ran:
            host_st.append(_dec_call(dev, d, c, how, a, b, ins[k], outs[k], sts[k], sync=not ready))
        _launches("dec", ran, cs.expected_launches("dec", g, cs.dec_shape(g, n, how, max_nb)), (name, seq, how, k, n))
    dev.sync()
    bad = []
    for k, n in enumerate(lengths):
        a, b = int(st[k]), int(st[k + 1])
        raw = dev.get(outs[k], (S * n * ch * N + N,), np.int16)
        got = raw[:S * n * ch * N].reshape(S, n, ch, N)
        assert (raw[S * n * ch * N:].view(np.uint16) == PCM_SENT).all(), (name, k, "samples behind the call's frames were written")
        if how == "hostsizes":
            status = host_st[k]
        elif how == "sizes":
            rs = dev.get(sts[k], (S * n + GUARD,), np.uint8)
            assert (rs[S * n:] == 0xEE).all(), (name, k, "status bytes behind the call's frames were written")
            status = rs[:S * n].reshape(S, n)
        else:
            status = None                                                    # the call without flags returns no status: samples only
        differ = (got != want[:, a:b]).any(axis=(2, 3))
        if status is not None:
            differ |= status != wst[:, a:b]
        bad += [(k, s, t) for s, t in np.argwhere(differ).tolist()]
    assert not bad, (name, seq, how, "frames that differ from the oracle decoder (call, stream, frame)", len(bad), bad[:10], [lengths[k] for k, _, _ in bad[:10]])
    tw = cs.starts(cs.twin_lengths(int(st[-1])))
    for a, b in zip(tw[:-1], tw[1:]):
        n = int(b - a)
        _dec_call(dev, twin, c, how, int(a), int(b), dev.put(np.ascontiguousarray(c["frames"][:, a:b])), dev.zeros(S * n * ch * N * 2), dev.zeros(S * n), sync=True)
    dev.sync()
    sa, sb = d.get_state(), twin.get_state()
    assert np.array_equal(sa, sb), (name, seq, how, "state words that differ from the twin's", np.flatnonzero(sa.view(np.uint32) != sb.view(np.uint32))[:12].tolist())
    d.close()
    twin.close()
    _report(seq + " " + how, name if S == 5 else "%s x%d" % (name, S), S * int(st[-1]), t0)


@pytest.mark.parametrize("how", ["hostsizes", "sizes"])
@pytest.mark.parametrize("name", list(cs.DEC_FAMILIES))
def test_decoder_ordered_calls(dev, name, how):
    """1 ... 129 frames in a fixed shuffled order on five streams, one loss role per stream laid out against the call boundaries: through decode_device with host
    sizes and flags, and through decode_device_sizes"""
    _dec_sequence(dev, name, "dec_ordered", how)


def test_decoder_whole_workgroups(dev):
    """one stream, calls of 255, 256 and 257 frames: a whole parse, plan and tail workgroup and one frame either side; boundary losses"""
    _dec_sequence(dev, "48k_10_80B", "dec_whole", "sizes", S=1, role0=1)


@pytest.mark.parametrize("S", [63, 64, 65])
def test_decoder_stream_counts(dev, S):
    """63, 64 and 65 streams at 1, 5 and 9 frames: the concealment kernel's 64 streams per wave; the role-3 streams never have a good frame"""
    _dec_sequence(dev, "48k_10_80B", "dec_count", "sizes" if S == 64 else "hostsizes", S=S)


@pytest.mark.parametrize("name", cs.DEC_READY_FAMILIES)
def test_decoder_under_the_promise(dev, name):
    """six equal calls each of 1 ... 17 frames queued with no host wait: every set of hand-over buffers twice per block.  The call takes no flags: the lost frames
    are refused payloads, placed by the same five roles"""
    _dec_sequence(dev, name, "dec_ready", "fixed")
