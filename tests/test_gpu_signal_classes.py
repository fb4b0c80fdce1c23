"""GPU parity on the crafted signal classes of signal_classes.py: narrow bandwidths, silence <-> full scale inside a stream, magnitudes of twenty escape
levels, lsb_mode without residual bits, the three pitch-lag regions - the branches lc3_harness.synth_pcm never enters (test_signal_classes_cpu.py has the
census on the same shapes).  One batch per geometry, one stream per (class, rate) with the rate varying fastest, so that the lanes of a wave and the two
streams of a pitch pair differ in both.  Every comparison is equality: the encoder's bytes against liblc3_oracle_pm.so and against the compiled reference's
frames in tests/golden/s1_signal_classes.npz, the decoder's samples against the oracle decoder."""
import functools
import os

import numpy as np
import pytest

import signal_classes as sc
from lc3_harness import Oracle, compare_frames, oracle_decode_streams
from test_gpu_dec_varsize_device import _Hip, _cmp, _device_calls
from test_gpu_enc_ragged import _amd, _ragged, _same_frames
from test_gpu_enc_ragged_pipe import _ends_like, _records_words
from test_gpu_enc_rates_device import SENT, check_frames

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s1_signal_classes.npz")
T = sc.T


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


@functools.lru_cache(maxsize=None)
def _case(geom):
    """a geometry's batch, computed once and left unchanged: PCM, sizes, the oracle's frames and the reference's"""
    fs, ms, hr, ch, rates, depth = sc.GEOMS[geom]
    pcm, labels, rr = sc.streams(geom)
    sizes = np.array([sc.stream_bytes(geom, r) for r in rr], np.int32)
    frames = sc.encode(geom, Oracle, portable_math=True)
    with np.load(GOLDEN) as z:
        gold = z["frames/" + geom]
    c = dict(geom=geom, fs=fs, ms=ms, hr=hr, ch=ch, depth=depth, B=len(rr), N=pcm.shape[3], T=T, pcm=pcm, labels=labels, start=rr, sizes=sizes,
             nb=np.repeat(sizes[:, None], T, axis=1), stride=int(sizes.max()), frames=frames, br=None, bw=np.zeros((len(rr), T), np.int32),
             want=[frames[b, :, :sizes[b]] for b in range(len(rr))], gold=[gold[b, :, :sizes[b]] for b in range(len(rr))])
    for v in list(c.values()) + c["want"] + c["gold"]:
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def _batch(c):
    return _amd().Batch(c["B"], c["fs"], c["ch"], c["ms"], c["hr"], c["start"], device=0)


def _check(out, c, what):
    """payloads against the oracle's frames and the reference's, every byte behind a payload still the sentinel"""
    for name in ("want", "gold"):
        try:
            check_frames(out, c["nb"][:, :out.shape[1]], c[name])
        except AssertionError:
            diff, tot, mld = compare_frames(out, c[name], c["fs"], c["ms"], c["hr"], c["ch"])
            nb = c["nb"]
            bad = [(b, t) for b in range(out.shape[0]) for t in range(out.shape[1])
                   if (out[b, t, :nb[b, t]] != c[name][b][t]).any() or (out[b, t, nb[b, t]:] != SENT).any()][:8]
            raise AssertionError("%s %s against %s: %d of %d frames differ, worst MLD %s, first (class, rate, frame): %s" % (
                c["geom"], what, "the oracle" if name == "want" else "the reference's frames", diff, tot, mld, [c["labels"][b] + (t,) for b, t in bad])) from None


def _dense(dev, bat, c, cuts, each=True):
    """encode_device over [cuts[k], cuts[k + 1]); each: wait and read last_status behind every call, else queue all of them and wait once"""
    B, stride, outs = c["B"], c["stride"], []
    ins = [(dev.put(np.ascontiguousarray(c["pcm"][:, a:b])), dev.put(np.full((B, b - a, stride), SENT, np.uint8)), b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    for d_pcm, d_out, n in ins:
        bat.encode_device(d_pcm, c["depth"], n, d_out, stride)
        if each:
            dev.sync()
            assert not bat.last_status(n).any(), np.argwhere(bat.last_status(n))[:6].tolist()
    dev.sync()
    assert not bat.last_status(ins[-1][2]).any()
    return np.concatenate([dev.get(d_out, (B, n, stride), np.uint8) for _, d_out, n in ins], axis=1)


# ---- the encoder ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(sc.GEOMS))
def test_three_call_shapes_give_the_reference_s_bytes_and_one_state(dev, geom):
    """(a) one call of 24 frames - in the standard layout the pipelined kernels: the call leaves records; (b) three calls of 8 - the one-wave kernel with its
    in-kernel writer: no records; (c) under the input-ready promise two calls of 12 queued back to back, one wait.  Three batches, the same bytes, no status
    bit; (a) and (b) end in one state."""
    c = _case(geom)
    a, b, p = _batch(c), _batch(c), _batch(c)
    _check(_dense(dev, a, c, (0, T)), c, "one call of 24")
    if c["N"] <= 480:                                                        # LC3D_LAYOUT_BIG: 96 kHz / 10 ms has no records to leave
        assert _records_words(a, T)[0] > 0
    _check(_dense(dev, b, c, (0, 8, 16, T)), c, "three calls of 8")
    assert _records_words(b, 8)[0] == 0
    p.set_input_ready(True)
    _check(_dense(dev, p, c, (0, 12, T), each=False), c, "two promised calls of 12")
    _ends_like(a, b, c)
    a.close(); b.close(); p.close()


def test_ragged_pipelined_calls_cut_a_stream_at_the_last_silent_frame(dev):
    """48 kHz mono, ragged calls of 20 frames on the pipelined kernels.  blocks (silent 0-2, noise 3-5, ...) has 3 frames in the first call: its last present
    frame is the last silent one and its next call starts on the noise; impulses and fade_in have 1, their only all-zero frame at the start, and the next
    call starts on the pulse and the first coded frame.  The other streams take 20 + 0, 0 + 20, 9 + 11 or 14 + 10 and the rest in a third call."""
    c = _case("48k_mono")
    other = ((20, 0, 4), (0, 20, 4), (9, 11, 4), (14, 10, 0))
    sched = np.array([{"blocks": (3, 20, 1), "impulses": (1, 20, 3), "fade_in": (1, 20, 3)}.get(k, other[i % 4]) for i, (k, _) in enumerate(c["labels"])], np.int32).T
    assert (sched.sum(axis=0) == T).all() and sched.shape == (3, c["B"])
    pcm = c["pcm"]
    for i, (k, _) in enumerate(c["labels"]):                                # the cut is where the docstring says: all-zero PCM up to it, signal right behind it
        if k in ("blocks", "impulses", "fade_in"):
            n = int(sched[0, i])
            assert not pcm[i, :n].any() and pcm[i, n].any(), (k, n)
    bat = _batch(c)
    got, nb, fl = _ragged(dev, bat, c, sched=sched, n_frames=20)
    assert _records_words(bat, 20)[0] > 0 and not bat.last_status(20).any()
    _same_frames(got, c["want"]); _same_frames(got, c["gold"])
    assert (nb == c["nb"]).all() and not fl.any()
    twin = _batch(c)
    _check(_dense(dev, twin, c, (0, T)), c, "the dense twin")
    _ends_like(bat, twin, c)
    bat.close(); twin.close()


# ---- the decoder on the same streams ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dec_case(geom):
    """the oracle's frames damaged by signal_classes.damage - per class: frame 0 lost, the frame behind an all-zero frame, the first loud frame after silence,
    five from loud into silence, a loss behind a frame with the LTPF active, one corrupted frame that is not marked - and the oracle decoder's PCM and status"""
    c = _case(geom)
    frames, bfi = sc.damage(c["frames"], c["labels"], c["sizes"])
    want, wst = oracle_decode_streams(frames, c["sizes"], bfi, c["fs"], c["ms"], c["hr"], 1)
    assert wst[bfi == 1].all()
    for v in (frames, bfi, want, wst):
        v.flags.writeable = False
    return frames, bfi, want, wst


@pytest.mark.parametrize("cuts,promise,flags", [((0, T), False, True), ((0, T), False, False), ((0, 12, T), True, True), ((0, 12, T), True, False)],
                         ids=["one_call_bfi", "one_call_sizes", "promised_12_bfi", "promised_12_sizes"])
@pytest.mark.parametrize("geom", sc.DEC_GEOMS)
def test_decoder_on_damaged_class_streams(dev, geom, cuts, promise, flags):
    """one call of 24 frames, and under the promise two calls of 12 queued back to back, where the second call's parser runs beside the first call's
    concealment; a lost frame marked in a bfi array, or without one by a size of 0"""
    c = _case(geom)
    frames, bfi, want, wst = _dec_case(geom)
    nb = c["nb"].copy()
    if not flags:
        nb[bfi == 1] = 0
    d = _amd().DecBatch(c["B"], c["fs"], 1, c["ms"], c["hr"], [int(x) for x in c["sizes"]], device=0)
    if promise:
        d.set_input_ready(True)
    got, st = _device_calls(dev, d, frames, nb, bfi if flags else None, list(cuts))
    _cmp(got, st, want, wst)
    d.close()
