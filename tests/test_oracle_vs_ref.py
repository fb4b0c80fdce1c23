"""CPU: the oracle restatement against the unmodified ETSI reference.  Where the compiled reference is built (oracle/_ref, from the
reference's sources by oracle/Makefile) every case runs it live and also checks that the committed digests still match it; everywhere
else the case compares the restatement's outputs with those digests (md5 of the reference's outputs, tests/golden/vs_ref_digests.json,
written from the live reference by tests/golden/make_golden_vs_ref.py)."""
import hashlib
import json
import os

import numpy as np
import pytest
from lc3_harness import Oracle, Ref, have_ref, oracle_encode_streams, ref_encode_streams, synth_pcm

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vs_ref_digests.json")
RATES = [16000, 24000, 32000, 48000, 64000, 80000, 96000, 128000, 160000, 192000, 256000, 320000]


def md5(*arrays):
    h = hashlib.md5()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(repr((a.dtype.str, a.shape)).encode()); h.update(a.tobytes())
    return h.hexdigest()


def reference(key, live):
    """The reference's result for `key`: the committed one, which `live()` (the same computation on the compiled reference) must
    reproduce wherever oracle/_ref is built."""
    with open(DIGESTS) as f:
        want = json.load(f)[key]
    if have_ref():
        assert live() == want, (key, "the compiled reference disagrees with tests/golden/vs_ref_digests.json (make_golden_vs_ref.py)")
    return want


# ----------------------------------------------------------------------------------------------------------------------------------
# encoder
# ----------------------------------------------------------------------------------------------------------------------------------
ALL_RATES_STREAMS = [list(range(12)), [1 + 4 * i for i in range(12)], [62, 63, 126, 127] * 3]


def _all_rates(encode, streams):
    pcm = synth_pcm(max(streams) + 1, 40, 480, 48000, seed=7)[streams]
    return [md5(o) for o in encode(pcm, 48000, 10.0, 0, RATES)]


@pytest.mark.parametrize("streams", ALL_RATES_STREAMS)
def test_48k_10ms_all_rates(streams):
    key = "48k_10ms_all_rates/" + ",".join(map(str, streams))
    assert _all_rates(oracle_encode_streams, streams) == reference(key, lambda: _all_rates(ref_encode_streams, streams))


def _96k_2p5ms_hr(encode):
    rates = [256000, 198400, 320000, 672000, 256000, 256000]
    pcm = synth_pcm(64, 80, 240, 96000, seed=3)[[0, 1, 2, 3, 62, 63]]
    return [md5(o) for o in encode(pcm, 96000, 2.5, 1, rates)]


def test_96k_2p5ms_hr():
    assert _96k_2p5ms_hr(oracle_encode_streams) == reference("96k_2p5ms_hr", lambda: _96k_2p5ms_hr(ref_encode_streams))


def _stereo_bitrate_switch_bandwidth_bitdepth(Enc):
    pcm = synth_pcm(4, 40, 480, 48000, seed=5)
    e, fr = Enc(48000, 2, 10.0, 0, 128000), []
    for t in range(40):
        fr.append(e.encode(pcm[0:2, t]))
        if t == 20:
            assert e.set_bitrate(192000) == 0
            e.nbytes = 240
    out = [md5(*fr)]
    e = Enc(48000, 1, 10.0, 0, 64000, bandwidth=8000)
    out.append(md5(*[e.encode(pcm[2:3, t]) for t in range(40)]))
    for depth, scale in ((24, 200), (32, 60000)):
        e = Enc(48000, 1, 10.0, 0, 96000)
        p32 = pcm[3].astype(np.int32) * scale + 77
        out.append(md5(*[e.encode(p32[t][None], depth) for t in range(40)]))
    return out


def test_stereo_bitrate_switch_bandwidth_bitdepth():
    got = _stereo_bitrate_switch_bandwidth_bitdepth(Oracle)
    assert got == reference("stereo_bitrate_switch_bandwidth_bitdepth", lambda: _stereo_bitrate_switch_bandwidth_bitdepth(Ref))


API_CASES = [(48000, 10.0, 0, 8000), (48000, 10.0, 0, 400000), (48000, 7.5, 0, 64000), (32000, 10.0, 1, 64000),
             (96000, 10.0, 0, 256000), (96000, 2.5, 1, 100000), (48000, 5.0, 1, 148800), (44100, 10.0, 0, 64000)]


def _ref_api_codes():
    import ctypes as C
    from lc3_harness import REF_SO
    L = C.CDLL(REF_SO)
    L.lc3_enc_set_frame_ms.argtypes = [C.c_void_p, C.c_float]
    out = []
    for fs, ms, hr, br in API_CASES:
        buf = C.create_string_buffer(L.lc3_enc_get_size(fs, 1) + 8)
        p = C.cast(buf, C.c_void_p)
        out.append([L.lc3_enc_init(p, fs, 1), L.lc3_enc_set_frame_ms(p, ms), L.lc3_enc_set_hrmode(p, hr), L.lc3_enc_set_bitrate(p, br),
                    L.lc3_enc_get_num_bytes(p), L.lc3_enc_get_input_samples(p), L.lc3_enc_get_delay(p)])
        L.lc3_free_encoder_structs(p)
    return out


def test_api_error_codes_match():
    import ctypes as C
    from lc3_harness import ORACLE_DIR
    o = C.CDLL(os.path.join(ORACLE_DIR, "liblc3_oracle.so"))
    o.lc3o_enc_set_frame_ms.argtypes = [C.c_void_p, C.c_float]
    want = reference("enc_api_codes", _ref_api_codes)
    for (fs, ms, hr, br), w in zip(API_CASES, want):
        ob = C.create_string_buffer(o.lc3o_enc_sizeof()); q = C.cast(ob, C.c_void_p)
        got = [o.lc3o_enc_init(q, fs, 1), o.lc3o_enc_set_frame_ms(q, ms), o.lc3o_enc_set_hrmode(q, hr), o.lc3o_enc_set_bitrate(q, br),
               o.lc3o_enc_get_num_bytes(q), o.lc3o_enc_get_input_samples(q), o.lc3o_enc_get_delay(q)]
        assert got == w, (fs, ms, hr, br, got, w)


GEOMETRIES = [
    (48000, 5.0, 0, 240, [32000, 64000, 96000, 128000, 256000]),
    (24000, 10.0, 0, 240, [16000, 32000, 64000, 128000]),
    (96000, 5.0, 1, 480, [256000, 400000]),
    (96000, 10.0, 1, 960, [149600, 256000, 500000]),
    (48000, 10.0, 1, 480, [128000, 256000, 400000]),
    (48000, 5.0, 1, 240, [160000, 320000]),
    (44100, 10.0, 0, 480, [32000, 64000, 128000]),
    (8000, 10.0, 0, 80, [16000, 32000, 64000]),
    (16000, 10.0, 0, 160, [16000, 32000, 64000, 128000]),
    (16000, 5.0, 0, 80, [32000, 64000, 128000]),
    (16000, 2.5, 0, 40, [64000, 96000, 192000]),
    (8000, 5.0, 0, 40, [32000, 64000, 96000]),
    (8000, 2.5, 0, 20, [64000, 96000, 160000]),
    (24000, 5.0, 0, 120, [32000, 64000, 160000]),
    (24000, 2.5, 0, 60, [64000, 96000, 256000]),
    (32000, 10.0, 0, 320, [32000, 64000, 96000, 192000, 320000]),
    (32000, 5.0, 0, 160, [32000, 64000, 192000]),
    (32000, 2.5, 0, 80, [64000, 96000, 256000]),
    (48000, 2.5, 0, 120, [64000, 128000, 320000]),
    (44100, 5.0, 0, 240, [64000, 128000]),
    (44100, 2.5, 0, 120, [96000]),
    (48000, 2.5, 1, 120, [172800, 256000, 400000]),
]


def _geometry(encode, fs, ms, hr, N, rates):
    pcm = synth_pcm(len(rates), 40, N, fs if fs != 44100 else 48000, seed=13)
    return [md5(o) for o in encode(pcm, fs, ms, hr, rates)]


def _geometry_key(fs, ms, hr, rates):
    return "geometry/%d/%g/%d/%s" % (fs, ms, hr, ",".join(map(str, rates)))


@pytest.mark.parametrize("fs,ms,hr,N,rates", GEOMETRIES)
def test_other_geometries(fs, ms, hr, N, rates):
    want = reference(_geometry_key(fs, ms, hr, rates), lambda: _geometry(ref_encode_streams, fs, ms, hr, N, rates))
    assert _geometry(oracle_encode_streams, fs, ms, hr, N, rates) == want


DFT_SIZES = [2, 3, 4, 5, 8, 15, 16, 32, 10, 20, 30, 40, 60, 80, 120, 160, 240, 480]


def _dft(apply, n):
    """100 seeded inputs of n complex values, each transformed in place by `apply`: the digest of the outputs' bits."""
    rng = np.random.default_rng(n)
    outs = []
    for _ in range(100):
        x = (rng.standard_normal(2 * n) * rng.choice([1, 1e3, 1e-3, 32768])).astype(np.float32)
        apply(x)
        outs.append(x.view(np.uint32))
    return md5(*outs)


def _ref_dft(n):
    import ctypes as C
    from lc3_harness import REF_SO
    ref = C.CDLL(REF_SO)
    ref.LC3_iisfft_plan.argtypes = [C.c_void_p, C.c_int, C.c_int]; ref.LC3_iisfft_apply.argtypes = [C.c_void_p, C.c_void_p]
    h = C.create_string_buffer(512)
    assert ref.LC3_iisfft_plan(h, n, -1) == 0
    return _dft(lambda x: ref.LC3_iisfft_apply(h, x.ctypes.data), n)


@pytest.mark.parametrize("n", DFT_SIZES)
def test_dft_kernels_match_the_reference_fft(n):
    """The restated DFT kernels (oracle/lc3_oracle_fft.inc) against LC3_iisfft_apply of the compiled reference, bit for bit."""
    import ctypes as C
    from lc3_harness import ORACLE_DIR
    orc = C.CDLL(os.path.join(ORACLE_DIR, "liblc3_oracle.so"))
    orc.lc3o_dft.argtypes = [C.c_void_p, C.c_int]

    def apply(x):
        assert orc.lc3o_dft(x.ctypes.data, n) == 1
    assert _dft(apply, n) == reference("dft/%d" % n, lambda: _ref_dft(n))


def _soak_every_operating_point_cfgs():
    def top(fs, ms):                                      # the family's largest bitrate: 400 bytes a frame (bitrate_limits in lc3_host.c, R/setup_enc_lc3.c:196-230)
        return 3200 * int(round(1000 / ms)) * (441 if fs == 44100 else 480) // 480
    cfg = []
    for fs in (8000, 16000, 24000, 32000, 44100, 48000):
        for ms in (10.0, 5.0, 2.5):
            lo = {10.0: 16000 if fs != 44100 else 32000, 5.0: 32000, 2.5: 64000}[ms]
            old = 320000 if fs != 44100 else 256000
            cfg.append((fs, ms, 0, [lo, 2 * lo, 3 * lo, 4 * lo, 6 * lo, old] + [top(fs, ms)] * (top(fs, ms) != old)))
    for ms, lo in ((10.0, 124800), (5.0, 148800), (2.5, 172800)):
        cfg.append((48000, ms, 1, [lo, 256000, 400000, 500000] + {10.0: [], 5.0: [600000], 2.5: [672000]}[ms]))
    for ms, lo in ((10.0, 149600), (5.0, 174400), (2.5, 198400)):
        cfg.append((96000, ms, 1, [lo, 256000, 400000, 500000] + {10.0: [], 5.0: [600000], 2.5: [672000]}[ms]))
    return cfg


def _soak(encode, fs, ms, hr, rates):
    N = int(round((48000 if fs == 44100 else fs) * ms / 1000))
    br = [rates[i % len(rates)] for i in range(12)]
    pcm = synth_pcm(64, 40, N, fs, seed=4000)[[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 62, 63]]     # 62 / 63: the silent and the full-scale stream
    return [md5(o) for o in encode(pcm, fs, ms, hr, br)]


def test_soak_every_operating_point_against_the_reference():
    """The 24 (sample rate, frame length, mode) families x mixed bitrates x 12 streams x 40 frames: restatement == compiled reference,
    byte for byte (same configuration list as the GPU soak, tools/soak.py)."""
    for fs, ms, hr, rates in _soak_every_operating_point_cfgs():
        want = reference("soak/%d/%g/%d" % (fs, ms, hr), lambda: _soak(ref_encode_streams, fs, ms, hr, rates))
        assert _soak(oracle_encode_streams, fs, ms, hr, rates) == want, (fs, ms, hr)


def _stereo_rates(fs, ms, rates):
    """a stereo stream's total bitrate for each of the first four mono rates: twice the rate, or the next lower one in steps of 800 bit/s whose stream-frame
    has an even number of bytes (the reference asserts on odd stereo sizes) - twice 500 kbit/s at 5 ms is 625 bytes, and at 44.1 kHz a frame lasts 480 / 441
    of its nominal length"""
    N = int(round(48000 * ms / 1000))
    out = []
    for r in rates[:4]:
        r *= 2
        while (r * N // ((44100 if fs == 44100 else 48000) * 8)) % 2:
            r -= 800
        out.append(r)
    return out


def _soak_stereo(Enc, fs, ms, hr, rates):
    N = int(round((48000 if fs == 44100 else fs) * ms / 1000))
    pcm = synth_pcm(8, 12, N, fs, seed=4100).reshape(4, 2, 12, N)
    out = []
    for s, br in enumerate(_stereo_rates(fs, ms, rates)):
        e = Enc(fs, 2, ms, hr, br)
        frames = [e.encode(pcm[s, :, t]) for t in range(12)]
        assert all(f.size == e.nbytes and f.size % 2 == 0 for f in frames), (fs, ms, hr, br, e.nbytes)
        out.append(md5(*frames))
    return out


def test_soak_every_operating_point_stereo_against_the_reference():
    """The restatement's stereo encoder in all 24 families x 4 streams x 12 frames: == the compiled reference, byte for byte.  Even stream-frame sizes only (the
    reference asserts on odd ones); the odd sizes are the restatement's own split, which the decoder pin above (dec_stereo_size_switch) reads back."""
    for fs, ms, hr, rates in _soak_every_operating_point_cfgs():
        want = reference("soak_stereo/%d/%g/%d" % (fs, ms, hr), lambda: _soak_stereo(Ref, fs, ms, hr, rates))
        assert _soak_stereo(Oracle, fs, ms, hr, rates) == want, (fs, ms, hr)


# ----------------------------------------------------------------------------------------------------------------------------------
# decoder: the chain encoder -> decoder; the restatement's (Oracle, OracleDecoder) against the reference's (Ref, RefDecoder).  The
# digests cover the frames that went in, the return codes and the PCM that came out.
# ----------------------------------------------------------------------------------------------------------------------------------
def _soak_cfgs():
    cfg = []
    for fs in (8000, 16000, 24000, 32000, 44100, 48000):
        for ms in (10.0, 5.0, 2.5):
            lo = {10.0: 16000 if fs != 44100 else 32000, 5.0: 32000, 2.5: 64000}[ms]
            cfg.append((fs, ms, 0, [lo, 2 * lo, 4 * lo, 320000 if fs != 44100 else 256000]))
    for ms, lo in ((10.0, 124800), (5.0, 148800), (2.5, 172800)):
        cfg.append((48000, ms, 1, [lo, 256000, 500000]))
    for ms, lo in ((10.0, 149600), (5.0, 174400), (2.5, 198400)):
        cfg.append((96000, ms, 1, [lo, 256000, 500000]))
    return cfg


def _dec_chain(Enc, Dec, fs, ms, hr, bi, br):
    N = int(round((48000 if fs == 44100 else fs) * ms / 1000))
    bps = 16 if bi % 2 == 0 else 24
    enc, dec = Enc(fs, 1, ms, hr, br), Dec(fs, 1, ms, hr)
    pcm = synth_pcm(64, 30, N, fs, seed=77)[[3, 5, 62, 63][bi % 4]]
    parts = []
    for t in range(30):
        fr = enc.encode(pcm[t:t + 1])
        bfi = 1 if t in (11, 12, 13, 22) else 0
        if t == 25: fr = fr[:0]                             # num_bytes = 0 -> bad frame (R/dec_lc3_fl.c:138-141)
        rc, a = dec.decode(fr, bfi, bps)
        parts += [fr, np.int32(rc), a]
    return md5(*parts)


def test_decoder_restatement_equals_the_reference_decoder():
    """oracle/lc3_oracle_dec.inc against lc3_dec_fl of the compiled reference: decoded PCM sample for sample on every operating-point
    family, with concealed frames (bfi = 1, and a frame of num_bytes = 0) in the stream, 16- and 24-bit output."""
    from lc3_harness import OracleDecoder, RefDecoder
    for fs, ms, hr, rates in _soak_cfgs():
        for bi, br in enumerate(rates):
            want = reference("dec_chain/%d/%g/%d/%d/%d" % (fs, ms, hr, bi, br), lambda: _dec_chain(Ref, RefDecoder, fs, ms, hr, bi, br))
            assert _dec_chain(Oracle, OracleDecoder, fs, ms, hr, bi, br) == want, (fs, ms, hr, br)


def _dec_stereo_size_switch(Enc, Dec):
    enc, dec = Enc(48000, 2, 10.0, 0, 128000), Dec(48000, 2, 10.0, 0)
    pcm = synth_pcm(2, 24, 480, 48000, seed=3)
    parts = []
    for t in range(24):
        if t == 12: assert enc.set_bitrate(96001) == 0              # odd total: 60 + 60 bytes; decoders re-derive from num_bytes
        fr = np.zeros(160, np.uint8)                                # the frame as the reference's binding returns it: in the
        e = enc.encode(pcm[:, t]); fr[:e.size] = e                  # 160-byte buffer of the encoder's first bitrate
        rc, a = dec.decode(fr)
        parts += [fr, np.int32(rc), a]
    return md5(*parts)


def test_decoder_restatement_stereo_and_size_switch():
    from lc3_harness import OracleDecoder, RefDecoder
    want = reference("dec_stereo_size_switch", lambda: _dec_stereo_size_switch(Ref, RefDecoder))
    assert _dec_stereo_size_switch(Oracle, OracleDecoder) == want


def _dec_api_codes(init, set_ms, set_hr, outs, free=None):
    out = []
    for fs in (8000, 16000, 24000, 32000, 44100, 48000, 96000, 22050):
        for ch in (0, 1, 2, 3):
            h, a = init(fs, ch)
            out.append([fs, ch, a])
            if a:
                continue
            for ms in (2.5, 5.0, 10.0, 7.5):
                for hr in (0, 1):
                    out.append([set_ms(h, ms), set_hr(h, hr), outs(h)])
            if free: free(h)
    return out


def _ref_dec_api_codes():
    import ctypes as C
    from lc3_harness import REF_SO
    R = C.CDLL(REF_SO)
    R.lc3_dec_set_frame_ms.argtypes = [C.c_void_p, C.c_float]
    keep = []

    def init(fs, ch):
        rb = C.create_string_buffer(max(R.lc3_dec_get_size(48000, 2), 64) + 8); keep.append(rb); r = C.cast(rb, C.c_void_p)
        return r, R.lc3_dec_init(r, fs, ch, 0)
    return _dec_api_codes(init, R.lc3_dec_set_frame_ms, R.lc3_dec_set_hrmode, R.lc3_dec_get_output_samples, R.lc3_free_decoder_structs)


def test_decoder_api_error_codes_match():
    """lc3_dec_init / set_frame_ms / set_hrmode / get_output_samples of the compiled reference (R/lc3.c:238-275,347-356) against the
    decoder restatement, over supported and unsupported arguments."""
    import ctypes as C
    from lc3_harness import ORACLE_DIR
    O = C.CDLL(os.path.join(ORACLE_DIR, "liblc3_oracle.so"))
    O.lc3o_dec_set_frame_ms.argtypes = [C.c_void_p, C.c_float]
    keep = []

    def init(fs, ch):
        ob = C.create_string_buffer(O.lc3o_dec_sizeof() + 8); keep.append(ob); o = C.cast(ob, C.c_void_p)
        return o, O.lc3o_dec_init(o, fs, ch)
    got = _dec_api_codes(init, O.lc3o_dec_set_frame_ms, O.lc3o_dec_set_hrmode, O.lc3o_dec_get_output_samples)
    want = reference("dec_api_codes", _ref_dec_api_codes)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (g, w)


PORTABLE_24_CASES = ((48000, 5.0, 2, 128000), (48000, 10.0, 1, 96000), (32000, 10.0, 1, 64000))


def _dec_portable_24(Enc, Dec, fs, ms, ch, br):
    """The chain (Enc, Dec) at 24-bit output beside the portable-math decoder restatement on the same frames: (digest of the chain's
    frames, codes and PCM; samples; samples equal).  The two decoders must agree on every code and be at most 1 LSB apart."""
    from lc3_harness import OracleDecoder
    N = int(fs * ms / 1000)
    enc, rd, od = Enc(fs, ch, ms, 0, br), Dec(fs, ch, ms, 0), OracleDecoder(fs, ch, ms, 0, portable_math=True)
    pcm = synth_pcm(ch, 40, N, fs, seed=41)
    parts, tot, same = [], 0, 0
    for t in range(40):
        fr = enc.encode(pcm[:, t])
        bfi = 1 if t % 11 in (3, 8, 9) else 0
        r1, a = rd.decode(fr, bfi, 24); r2, b = od.decode(fr, bfi, 24)
        assert r1 == r2
        assert np.abs(a.astype(np.int64) - b).max() <= 1, (fs, ms, t)
        parts += [fr, np.int32(r1), a]
        tot += a.size; same += int((a == b).sum())
    return md5(*parts), tot, same


def test_decoder_portable_math_boundary_at_24_bits():
    """The portable-math build of the decoder restatement (what the HIP kernels compute: libm calls as (float)f((double)x)) against the
    reference decoder with 24-bit output, where a different rounding of one powf() shows as one output LSB: at most 1 LSB apart,
    and identical in more than 99.9 % of the samples.  (With the glibc-math build the outputs are identical: tests above.)  Where the
    compiled reference is not built, the glibc-math restatement stands in for it, once its frames, codes and PCM have matched the
    reference's digest."""
    from lc3_harness import OracleDecoder, RefDecoder
    Enc, Dec = (Ref, RefDecoder) if have_ref() else (Oracle, OracleDecoder)
    tot = same = 0
    for fs, ms, ch, br in PORTABLE_24_CASES:
        digest, n, s = _dec_portable_24(Enc, Dec, fs, ms, ch, br)
        with open(DIGESTS) as f:
            assert digest == json.load(f)["dec_portable_24/%d/%g/%d/%d" % (fs, ms, ch, br)], (fs, ms, ch, br)
        tot += n; same += s
    assert same > 0.999 * tot, (same, tot)


def test_rms_and_energy_metrics_of_the_conformance_procedure():
    """The conformance script's default metric is not MLD but the ETSI `rms` tool at 14-bit resolution, and its low-pass cases use the
    energy difference (lc3_conformance.py:126-130, 542-556, 586-619).  oracle/_ref/rms is compiled from the reference's source (oracle/Makefile);
    this pins the harness around it: equal bitstreams -> no differing sample, -inf energy, gate holds; bitstreams of an input that was
    moved by one LSB -> the tool's figures parse, the thresholds are the script's (k = 14: -89.06 dB, 2^-11), and a lossy codec's
    answer to a changed input is correctly NOT inside a 14-bit gate, which is what the soaks would report next to the MLD if a frame ever differed."""
    import math
    from lc3_harness import rms_between, energy_diff_between, RMS_TOOL, ENG_THRESHOLD
    if not (have_ref() and os.path.exists(RMS_TOOL)):
        pytest.skip("oracle/_ref (compiled reference decoder + rms tool) not built (needs the reference's sources)")
    fs, ms, T = 48000, 10.0, 24
    pcm = synth_pcm(2, T, 480, fs, seed=41)
    pcm2 = pcm.copy(); pcm2[:, :, ::7] += 1
    pcm2 = np.clip(pcm2.astype(np.int32), -32768, 32767).astype(np.int16)
    a = oracle_encode_streams(pcm, fs, ms, 0, [64000, 128000])
    b = oracle_encode_streams(pcm2, fs, ms, 0, [64000, 128000])
    same = rms_between(a[0], a[0], fs, ms, 0)
    assert same["different_samples"] == 0 and same["ok"] and same["rms_db"] == float("-inf")
    assert energy_diff_between(a[0], a[0], fs, ms, 0) == float("-inf")
    for i in range(2):
        assert not (a[i] == b[i]).all()
        r = rms_between(a[i], b[i], fs, ms, 0)
        assert r["different_samples"] > 0 and math.isfinite(r["rms_db"]) and r["max_abs_diff"] > 0
        assert abs(r["rms_threshold_db"] - (-89.06)) < 0.01 and r["max_abs_diff_threshold"] == 2.0 ** -11
        assert not r["ok"]
        e = energy_diff_between(a[i], b[i], fs, ms, 0)
        assert 0 < e <= ENG_THRESHOLD


def reference_cases():
    """(key, the reference's result) for every committed digest: tests/golden/make_golden_vs_ref.py writes them from the live reference."""
    from lc3_harness import RefDecoder
    for streams in ALL_RATES_STREAMS:
        yield "48k_10ms_all_rates/" + ",".join(map(str, streams)), _all_rates(ref_encode_streams, streams)
    yield "96k_2p5ms_hr", _96k_2p5ms_hr(ref_encode_streams)
    yield "stereo_bitrate_switch_bandwidth_bitdepth", _stereo_bitrate_switch_bandwidth_bitdepth(Ref)
    yield "enc_api_codes", _ref_api_codes()
    for fs, ms, hr, N, rates in GEOMETRIES:
        yield _geometry_key(fs, ms, hr, rates), _geometry(ref_encode_streams, fs, ms, hr, N, rates)
    for n in DFT_SIZES:
        yield "dft/%d" % n, _ref_dft(n)
    for fs, ms, hr, rates in _soak_every_operating_point_cfgs():
        yield "soak/%d/%g/%d" % (fs, ms, hr), _soak(ref_encode_streams, fs, ms, hr, rates)
    for fs, ms, hr, rates in _soak_every_operating_point_cfgs():
        yield "soak_stereo/%d/%g/%d" % (fs, ms, hr), _soak_stereo(Ref, fs, ms, hr, rates)
    for fs, ms, hr, rates in _soak_cfgs():
        for bi, br in enumerate(rates):
            yield "dec_chain/%d/%g/%d/%d/%d" % (fs, ms, hr, bi, br), _dec_chain(Ref, RefDecoder, fs, ms, hr, bi, br)
    yield "dec_stereo_size_switch", _dec_stereo_size_switch(Ref, RefDecoder)
    yield "dec_api_codes", _ref_dec_api_codes()
    for fs, ms, ch, br in PORTABLE_24_CASES:
        yield "dec_portable_24/%d/%g/%d/%d" % (fs, ms, ch, br), _dec_portable_24(Ref, RefDecoder, fs, ms, ch, br)[0]
