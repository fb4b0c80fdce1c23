"""GPU: the encoder and decoder kernels at EVERY frame size of every operating point (tests/size_sweep.py) against the portable-math CPU oracle, which
tests/test_size_sweep_cpu.py pins to the compiled reference on the same streams.  Bar: bytes, samples and status words identical - zero differing frames.

The other parity tests share rate lists that stop at 320 kbit/s; at 5 and 2.5 ms that is 200 and 100 of the 400 bytes a channel-frame may have.  Here every
size runs on the one-wave encoder, on the pipelined kernels, through the per-frame-bitrate table and through both decoder parsers; whole batches of one size
move the runtime's stream-placement rules (mean, smallest and largest frame of a batch) and its choice of parser at every family's frame length, not only at
N = 480.  Shapes are small on purpose: one stream per size, or one wave plus two lanes.

Every case prints its frames, wall time and the oracle's share of it (pytest -s)."""
import ctypes as C
import functools
import os
import time

import numpy as np
import pytest

import size_sweep as S
from lc3_harness import ORACLE_DIR, OracleDecoder, oracle_decode_streams, synth_pcm

pytestmark = pytest.mark.gpu
family = pytest.mark.parametrize("family", S.FAMILIES, ids=S.ids())
GUARD, SENT = 8, 0xA5
PARSE_LDS, PARSE_GLOBAL = "lc3_dec_parse_kernel", "lc3_dec_parse_kernel_g"       # frames staged in LDS (up to 128 bytes), frames read from global memory


def _amd():
    import audio_codec_amd
    return audio_codec_amd


class _Clock:
    """wall time of a case and the part of it spent in the CPU oracle"""
    def __init__(self):
        self.t0, self.oracle = time.perf_counter(), 0.0

    def cpu(self, f, *a, **kw):
        t = time.perf_counter()
        r = f(*a, **kw)
        self.oracle += time.perf_counter() - t
        return r

    def report(self, what, fam, frames, differ):
        print("size_sweep %-22s %-12s frames %6d differ %d wall %.2f s oracle %.2f s" % (what, S.key(fam), frames, differ, time.perf_counter() - self.t0,
                                                                                         self.oracle))


@functools.lru_cache(maxsize=None)
def _oracle_sweep(fam):
    """the portable-math oracle's frames of every stream of the family [B, T, max size] - shared by the encoder and the decoder case, left unchanged"""
    pcm, nbytes, _ = S.streams(fam)
    out = S.oracle_encode(fam, pcm, nbytes)
    out.flags.writeable = False
    return out


def _differing(got, want, nbytes):
    """[(stream, frame)] whose bytes differ inside the frame's size"""
    return [(b, t) for b in range(want.shape[0]) for t in np.nonzero((got[b, :, :nbytes[b]] != want[b, :, :nbytes[b]]).any(axis=1))[0].tolist()]


def _rates(fam, nbytes):
    return [int(r) for r in S.rates(fam, nbytes)]


@family
def test_encoder_every_size_in_one_batch(family):
    """One stream per size and five at every edge, device pointers: a call of 7 frames (the one-wave kernel), then 13 (pipelined, not a multiple of four).
    Every frame's bytes equal the oracle's, the bytes behind each frame inside its slot keep their fill, the status words are zero."""
    from test_gpu_parity import _Dev
    fs, ms, hr = family
    clk = _Clock()
    pcm, nbytes, labels = S.streams(family)
    want = clk.cpu(_oracle_sweep, family)
    B, N = len(nbytes), S.frame_len(family)
    b = _amd().Batch(B, fs, 1, ms, hr, _rates(family, nbytes), device=0)
    assert [b.num_bytes(i) for i in range(B)] == list(nbytes) and b.stride == nbytes.max() and b.N == N
    stride = b.stride + GUARD
    d = _Dev()
    try:
        got = []
        for t0, n in ((0, 7), (7, S.T - 7)):
            dp, do = d.put(pcm[:, t0:t0 + n]), d.put(np.full((B, n, stride), SENT, np.uint8))
            b.encode_device(dp, 16, n, do, stride, sync=True)
            got.append(d.get(do, (B, n, stride), np.uint8))
            assert not b.last_status(n).any(), (family, t0, np.argwhere(b.last_status(n))[:6].tolist())
        got = np.concatenate(got, axis=1)
    finally:
        d.free()
        b.close()
    bad = _differing(got, want, nbytes)
    clk.report("enc every size", family, B * S.T, len(bad))
    assert not bad, (family, len(bad), [(labels[s], t) for s, t in bad[:8]])
    over = [(labels[s], t) for s in range(B) for t in range(S.T) if (got[s, t, nbytes[s]:] != SENT).any()]
    assert not over, (family, "bytes behind a frame were written", over[:8])


def _uniform_sizes(fam, inner):
    ss = S.sizes(fam)
    return sorted({ss[0], ss[-1]} | {n for n in inner if ss[0] <= n <= ss[-1]})


@family
def test_encoder_uniform_batches(family):
    """66 streams (a wave and two lanes) of ONE size - the lowest, 119, 120, the highest: mean, smallest and largest frame of the batch move together across
    the runtime's stream-placement rules.  Two calls of 16 frames: the second runs on the state the pipelined kernels left."""
    fs, ms, hr = family
    clk = _Clock()
    B, Tc, N = 66, 16, S.frame_len(family)
    pcm = synth_pcm(B, 2 * Tc, N, fs, seed=9200 + S.FAMILIES.index(family))
    tot = 0
    for n in _uniform_sizes(family, (119, 120)):
        nb = np.full(B, n, np.int32)
        want = clk.cpu(S.oracle_encode, family, pcm, nb)
        b = _amd().Batch(B, fs, 1, ms, hr, _rates(family, nb), device=0)
        got = np.concatenate([b.encode(pcm[:, :Tc]), b.encode(pcm[:, Tc:])], axis=1)
        b.close()
        bad = _differing(got, want, nb)
        tot += B * 2 * Tc
        assert not bad, (family, n, len(bad), bad[:8])
    clk.report("enc uniform", family, tot, 0)


@functools.lru_cache(maxsize=None)
def _ramp(fam):
    """the size ramp: (sizes int32 [6, L], bitrates [6, L], pcm [6, L, 1, N], the oracle's frames - set_bitrate in front of every frame)"""
    from test_gpu_enc_varrate import oracle_frames
    fs, ms, hr = fam
    plan = S.ramp_sizes(fam)
    br = np.array([[S.rate_for(fam, int(n)) for n in row] for row in plan], np.int32)
    pcm = synth_pcm(plan.shape[0], plan.shape[1], S.frame_len(fam), fs, seed=9300 + S.FAMILIES.index(fam))[:, :, None, :].copy()
    return plan, br, pcm, oracle_frames(pcm, fs, ms, hr, br)


@family
def test_encoder_size_ramp_per_frame_bitrates(family):
    """Six streams whose size changes with every frame - up, down, two shuffles, lowest and highest in turn - through encode(bitrates=...): every entry of
    the per-size configuration table (enc_build_table) is read.  Against the oracle with set_bitrate in front of every frame."""
    from test_gpu_enc_varrate import mismatches
    fs, ms, hr = family
    clk = _Clock()
    plan, br, pcm, want = clk.cpu(_ramp, family)
    b = _amd().Batch(plan.shape[0], fs, 1, ms, hr, [int(x) for x in br[:, 0]], device=0)
    out = b.encode(pcm, bitrates=br)
    assert (b.last_num_bytes == plan).all()
    assert set(plan.reshape(-1).tolist()) == set(S.sizes(family))
    bad = mismatches(out, b.last_num_bytes, want)
    b.close()
    clk.report("enc size ramp", family, plan.size, len(bad))
    assert not bad, (family, len(bad), [(s, t, int(plan[s, t])) for s, t in bad[:8]])


def _cmp_dec(fam, got, st, want, wst, sizes_of=None):
    bad = np.argwhere((got != want).any(axis=(2, 3)) | (st != wst))
    assert len(bad) == 0, (fam, len(bad), "first differing (stream, frame" + (", size)" if sizes_of is not None else ")"),
                           [tuple(x) + ((int(sizes_of[tuple(x)]),) if sizes_of is not None else ()) for x in bad[:8].tolist()])


@family
def test_decoder_every_size_in_one_batch(family):
    """The frames of every stream of the sweep - one per size, five at every edge, where the pitched one keeps the LTPF running across each step of its gain
    table - lost and corrupted as make_dec_case does it, in one batch: a call of 9 frames, then the rest.  PCM and status equal the oracle decoder's."""
    fs, ms, hr = family
    clk = _Clock()
    _, nb, _ = S.streams(family)
    frames, bfi = S.damage(family, clk.cpu(_oracle_sweep, family), nb)
    want, wst = clk.cpu(S.decode_streams, family, OracleDecoder, frames, nb, bfi, portable_math=True)
    d = _amd().DecBatch(nb.size, fs, 1, ms, hr, nb, device=0)
    a, sa = d.decode(frames[:, :9], bfi[:, :9])
    b, sb = d.decode(frames[:, 9:], bfi[:, 9:])
    d.close()
    _cmp_dec(family, np.concatenate([a, b], axis=1), np.concatenate([sa, sb], axis=1), want, wst, sizes_of=np.repeat(nb[:, None], S.T, axis=1))
    clk.report("dec every size", family, nb.size * S.T, 0)


@family
def test_decoder_uniform_batches_take_the_parser_their_size_implies(family):
    """66 streams of ONE size - the lowest, 128, 129, the highest - damaged, T = 16 in calls of 7 and 9: up to 128 bytes the parser stages the frames in
    LDS at this family's frame length, from 129 it reads them from global memory.  The launch census says which parser ran, so that the case cannot pass
    on the other one."""
    amd = _amd()
    fs, ms, hr = family
    clk = _Clock()
    B, Tn, N = 66, 16, S.frame_len(family)
    pcm = synth_pcm(B, Tn, N, fs, seed=9400 + S.FAMILIES.index(family))
    tot = 0
    for n in _uniform_sizes(family, (128, 129)):
        nb = np.full(B, n, np.int32)
        frames, bfi = S.damage(family, clk.cpu(S.oracle_encode, family, pcm, nb), nb)
        want, wst = clk.cpu(S.decode_streams, family, OracleDecoder, frames, nb, bfi, portable_math=True)
        d = amd.DecBatch(B, fs, 1, ms, hr, nb, device=0)
        with amd.api.launch_census() as ran:
            a, sa = d.decode(frames[:, :7], bfi[:, :7])
            b, sb = d.decode(frames[:, 7:], bfi[:, 7:])
        d.close()
        expect, other = (PARSE_LDS, PARSE_GLOBAL) if n <= 128 else (PARSE_GLOBAL, PARSE_LDS)
        assert ran.get(expect, 0) >= 2 and other not in ran, (family, n, {k: v for k, v in ran.items() if "parse" in k})
        _cmp_dec(family, np.concatenate([a, b], axis=1), np.concatenate([sa, sb], axis=1), want, wst)
        tot += B * Tn
    clk.report("dec uniform", family, tot, 0)


@family
def test_decoder_size_ramp_per_frame_sizes(family):
    """The ramp streams' frames through decode(num_bytes=...), every eleventh frame lost (size 0), no size known before the first frame; against the oracle
    decoder fed each frame with its own size."""
    from test_gpu_dec_varsize import oracle_var
    fs, ms, hr = family
    clk = _Clock()
    plan, _, _, enc = clk.cpu(_ramp, family)
    B, L = plan.shape
    frames = np.zeros((B, L, int(plan.max())), np.uint8)
    for s in range(B):
        for t in range(L):
            frames[s, t, :plan[s, t]] = enc[s][t]
    num_bytes = plan.copy()
    num_bytes[:, 10::11] = 0
    bfi = np.zeros((B, L), np.uint8)
    want, wst = clk.cpu(oracle_var, frames, num_bytes, bfi, fs, ms, hr, 1)
    d = _amd().DecBatch(B, fs, 1, ms, hr, None, device=0)
    cut = L // 2 + 1
    a, sa = d.decode(frames[:, :cut], bfi[:, :cut], num_bytes=num_bytes[:, :cut])
    b, sb = d.decode(frames[:, cut:], bfi[:, cut:], num_bytes=num_bytes[:, cut:])
    d.close()
    _cmp_dec(family, np.concatenate([a, b], axis=1), np.concatenate([sa, sb], axis=1), want, wst, sizes_of=plan)
    clk.report("dec size ramp", family, B * L, 0)


def test_stereo_every_seventh_total_48k_2p5ms():
    """Stereo at 48 kHz / 2.5 ms: stream-frames of 40, 41, 799, 800 bytes and every seventh total between, 12 frames in one call, encoder and decoder.  An
    odd total gives the first channel a byte more and the second channel's payload an odd address."""
    fs, ms, hr, Tn = 48000, 2.5, 0, 12
    fam = (fs, ms, hr)
    clk = _Clock()
    totals = np.array(S.stereo_totals(), np.int32)
    B, N = totals.size, S.frame_len(fam)
    br = (totals * 8 * fs // N).astype(np.int32)                          # 3 200 bit/s per byte: exact
    assert (_amd().api.enc_plan_bitrates(fs, 2, ms, hr, br[:, None])[0][:, 0] == totals).all() and (totals % 2).any()
    pcm = np.ascontiguousarray(synth_pcm(2 * B, Tn, N, fs, seed=9500).reshape(B, 2, Tn, N).transpose(0, 2, 1, 3))
    L = C.CDLL(os.path.join(ORACLE_DIR, "liblc3_oracle_pm.so"))
    L.lc3o_encode_batch16_ch.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    b = _amd().Batch(B, fs, 2, ms, hr, [int(x) for x in br], device=0)
    assert [b.num_bytes(i) for i in range(B)] == totals.tolist() and b.stride == 800
    got = b.encode(pcm)
    assert not b.last_status(Tn).any()
    b.close()
    want = np.zeros_like(got)
    assert clk.cpu(L.lc3o_encode_batch16_ch, fs, ms, hr, 2, B, Tn, br.ctypes.data, pcm.ctypes.data, want.ctypes.data, want.shape[2]) == 0
    bad = _differing(got, want, totals)
    assert not bad, (len(bad), [(int(totals[s]), t) for s, t in bad[:8]])
    frames, bfi = S.damage(fam, want, totals)
    wpcm, wst = clk.cpu(oracle_decode_streams, frames, totals, bfi, fs, ms, hr, 2)
    d = _amd().DecBatch(B, fs, 2, ms, hr, totals, device=0)
    out, st = d.decode(frames, bfi)
    d.close()
    _cmp_dec(fam, out, st, wpcm, wst, sizes_of=np.repeat(totals[:, None], Tn, axis=1))
    clk.report("stereo enc + dec", fam, 2 * B * Tn, 0)
