"""Crafted test signals for the branches lc3_harness.synth_pcm never reaches (test infrastructure, a plain helper beside lc3_harness.py): narrow
bandwidths, silence <-> full scale inside a stream, escape-coded magnitudes, lsb_mode without residual bits, the three pitch-lag regions.

classes(fs, N, T, bitdepth) -> {name: [T, N]} in the order of ORDER.  The PCM is bit-reproducible: np.random.RandomState draws of integers and integer
arithmetic only - the sine is a table built with math.isqrt, the low-passes are integer FIRs whose taps come from that table - so
test_signal_classes_cpu.py can pin one SHA-256 per (class, fs, N, T).

Order.  A batch holds one stream per (class, rate) with the rate varying fastest (streams()).  With T = 24 a wave of the one-frame-per-lane kernels
holds 2.67 streams and the pitch kernel pairs streams 2k, 2k + 1, so ORDER keeps the extremes next to each other: the silence-heavy classes (dither,
blocks, impulses) sit between the DC and Nyquist classes whose high-resolution magnitudes need twenty escape levels, and every pitched class (square,
pulses, sine) lies beside an unpitched one (fade_in, clipped, low-passed noise)."""
import collections
import math

import numpy as np

FULL = 32767
ORDER = ("dither", "dc_min", "blocks", "dc_plus3", "impulses", "nyquist", "fade_in", "square_100", "clipped", "pulses_390", "lp3k", "pulses_57",
         "lp7k", "sine_1k", "lp11k", "sweep", "lp15k", "clicks")
ORDER_24 = ("dc_min24", "sine24")                  # bitdepth 24 only: behind dc_min and sine_1k
PITCHED = ("square_100", "pulses_390", "pulses_57", "sine_1k")

# ---- integer sine: a quarter-wave table in Q30, 4096 steps, built by half-angle square roots and rotation in Q60 -------------------------------------
_Q = 1 << 60


def _quarter_table():
    c, s = 0, _Q                                   # cos, sin of pi / 2
    for _ in range(12):                            # -> of pi / 2 / 4096
        c, s = math.isqrt((_Q + c) * _Q // 2), math.isqrt((_Q - c) * _Q // 2)
    t, ck, sk = [], _Q, 0
    for _ in range(4097):
        t.append((sk + (1 << 29)) >> 30)
        ck, sk = (ck * c - sk * s) >> 60, (sk * c + ck * s) >> 60
    t[4096] = 1 << 30
    return np.array(t + [1 << 30], np.int64)


_SIN = _quarter_table()


def isin(phase):
    """sin(2 pi phase / 2^32) in Q30 for an int64 array of phases (taken mod 2^32); linear interpolation in the table, error below 2^-25"""
    p = np.asarray(phase, np.int64) & 0xFFFFFFFF
    q, f = p >> 30, p & 0x3FFFFFFF
    f = np.where(q & 1, (1 << 30) - f, f)
    i, r = f >> 18, f & 0x3FFFF
    v = _SIN[i] + (((_SIN[i + 1] - _SIN[i]) * r) >> 18)
    return np.where(q >= 2, -v, v)


def icos(phase):
    return isin(np.asarray(phase, np.int64) + (1 << 30))


_PI_Q30 = 3373259426                               # pi in Q30


def lowpass_taps(fc, fs):
    """Q30 taps of a Blackman-windowed sinc with cutoff fc, 6 fs / 1000 + 1 taps (transition about 0.9 kHz, stop band about -74 dB)"""
    M = 3 * fs // 1000
    n = np.arange(-M, M + 1, dtype=np.int64)
    nz = np.where(n == 0, 1, n)
    sinc = (isin(n * ((fc << 32) // fs)) << 30) // (_PI_Q30 * nz)
    sinc = np.where(n == 0, (2 * fc << 30) // fs, sinc)
    w = (42 * (1 << 30) + 50 * icos(n * ((1 << 31) // M)) + 8 * icos(n * ((1 << 32) // M))) // 100
    return (sinc * w) >> 30


def _phase(n, num, den):
    """phase of sample n of a tone of num / den cycles per sample, mod 2^32 (int64 throughout: n * num stays below 2^53)"""
    return ((n * num % den) << 32) // den


def _gauss(rng, L, half):
    """about N(0, (2 half)^2): the sum of twelve uniform integers of [-half, half)"""
    return rng.randint(-half, half, size=(12, L)).astype(np.int64).sum(axis=0)


def _one(name, fs, N, T, seed):
    L = T * N
    n = np.arange(L, dtype=np.int64)
    fr = n // N
    rng = np.random.RandomState(seed)
    if name == "dither":
        return rng.randint(-1, 2, size=L)
    if name == "dc_min":
        return np.full(L, -32768, np.int64)
    if name == "dc_plus3":
        return np.full(L, 3, np.int64)
    if name == "impulses":                         # one full-scale sample in the middle of frames 1, 4, 7, ...: frame 0 is silent
        return np.where((fr % 3 == 1) & (n % N == N // 2), FULL, 0)
    if name == "nyquist":
        return np.where(n & 1, -FULL, FULL)
    if name == "blocks":                           # frames 0-2 silent, 3-5 full-scale noise, 6-8 silent, ...
        return np.where((fr // 3) & 1, rng.randint(-32768, 32768, size=L), 0)
    if name == "fade_in":                          # noise x (n / L)^4: exactly zero for about the first 7 % of the stream
        a = (n << 15) // L
        a4 = (((a * a) >> 15) ** 2) >> 15
        return (rng.randint(-32768, 32768, size=L) * a4) >> 15
    if name.startswith("lp"):
        fc = int(name[2:-1]) * 1000
        h = lowpass_taps(fc, fs)
        x = rng.randint(-8000, 8001, size=L + h.size - 1).astype(np.int64)
        return (np.convolve(x, h, mode="valid") + (1 << 29)) >> 30
    if name == "sweep":                            # the frequency rises linearly from 0 to 0.45 fs over the stream
        inc = (n * (45 * (1 << 32) // 100)) // L
        return (isin(np.cumsum(inc)) * 24000) >> 30
    if name == "square_100":                       # 100.3 Hz: a lag of 127.6 at 12.8 kHz, the half-sample region
        return np.where(_phase(n, 1003, 10 * fs) < (1 << 31), 12000, -12000)
    if name in ("pulses_390", "pulses_57"):        # lags of 32.8 (quarter-sample region) and 224.6 (integer region)
        f = int(name[7:])
        w = max(2, fs // 4000)                     # a triangle of 2 w - 1 samples, so that the 12.8 kHz signal sees every pulse
        start = (n * f) % fs < f
        tri = np.concatenate([np.arange(1, w + 1), np.arange(w - 1, 0, -1)]).astype(np.int64) * (28000 // w)
        return np.convolve(start.astype(np.int64), tri)[:L] + rng.randint(-8, 9, size=L)
    if name == "clicks":                           # quiet noise; eight full-scale samples in frames 2, 6, 10, ... at a place that moves
        x = rng.randint(-30, 31, size=L).astype(np.int64)
        at = (N // 3 + 7 * fr) % (N - 8)
        return np.where((fr % 4 == 2) & (n % N >= at) & (n % N < at + 8), FULL, x)
    if name == "sine_1k":
        return (isin(_phase(n, 1000, fs)) * FULL + (1 << 29)) >> 30
    if name == "clipped":                          # sigma of two full scales, clipped hard
        return np.clip(_gauss(rng, L, 32768), -32768, 32767)
    if name == "dc_min24":
        return np.full(L, -8388608, np.int64)
    if name == "sine24":
        return (isin(_phase(n, 1000, fs)) * 8388607 + (1 << 29)) >> 30
    raise KeyError(name)


def names(fs, bitdepth=16):
    out = []
    for k in ORDER:
        if k.startswith("lp") and int(k[2:-1]) * 2000 >= fs:
            continue
        out.append(k)
        if bitdepth == 24 and k == "dc_min":
            out.append("dc_min24")
        if bitdepth == 24 and k == "sine_1k":
            out.append("sine24")
    return out


def classes(fs, N, T, bitdepth=16):
    """{name: [T, N]} int16, or int32 for bitdepth 24: the 16-bit classes times 256 and the two of ORDER_24"""
    assert bitdepth in (16, 24)
    out = collections.OrderedDict()
    for k in names(fs, bitdepth):
        x = _one(k, fs, N, T, 1000 + (ORDER + ORDER_24).index(k))
        assert x.shape == (T * N,)
        if bitdepth == 24:
            x = x if k in ORDER_24 else x * 256
            assert x.min() >= -8388608 and x.max() <= 8388607
            out[k] = x.astype(np.int32).reshape(T, N)
        else:
            assert x.min() >= -32768 and x.max() <= 32767, k
            out[k] = x.astype(np.int16).reshape(T, N)
    return out


# ---- the geometries of the parity tests: fs, frame_ms, hrmode, channels, rates, bitdepth ----------------------------------------------------------------
T = 24
GEOMS = collections.OrderedDict([
    ("48k_mono", (48000, 10.0, 0, 1, (24000, 64000, 128000, 320000), 16)),
    ("48k_stereo", (48000, 10.0, 0, 2, (128800,), 16)),
    ("48k_24bit", (48000, 10.0, 0, 1, (96000,), 24)),
    ("32k_10", (32000, 10.0, 0, 1, (96000,), 16)),
    ("24k_5", (24000, 5.0, 0, 1, (48000,), 16)),
    ("16k_2p5", (16000, 2.5, 0, 1, (64000,), 16)),
    ("48k_hr", (48000, 10.0, 1, 1, (256000,), 16)),
    ("96k_hr", (96000, 10.0, 1, 1, (256000,), 16)),
    ("96k_2p5_hr", (96000, 2.5, 1, 1, (256000,), 16)),
])
DEC_GEOMS = ("48k_mono", "32k_10", "16k_2p5", "48k_hr", "96k_hr")
# the two channels of a stereo stream: (loud, silent), (pitched, clipped), ...; every class occurs
STEREO_PAIRS = (("clipped", "impulses"), ("square_100", "clipped"), ("blocks", "dc_min"), ("dither", "nyquist"), ("fade_in", "pulses_57"),
                ("lp3k", "sine_1k"), ("lp7k", "sweep"), ("pulses_390", "dc_plus3"), ("lp11k", "clicks"), ("blocks", "lp15k"))


def frame_len(fs, ms):
    return int(fs * ms / 1000)


def streams(geom, T=T):
    """-> pcm [B, T, channels, N], labels [B] of (class or class pair, rate), rates [B].  B = classes x rates, the rate varying fastest."""
    fs, ms, hr, ch, rates, depth = GEOMS[geom]
    N = frame_len(fs, ms)
    cl = classes(fs, N, T, depth)
    rows = [(a + "+" + b, np.stack([cl[a], cl[b]], axis=1)) for a, b in STEREO_PAIRS] if ch == 2 else [(k, v[:, None, :]) for k, v in cl.items()]
    pcm = np.stack([x for _, x in rows for _ in rates])
    labels = [(k, r) for k, _ in rows for r in rates]
    return np.ascontiguousarray(pcm), labels, [r for _, r in labels]


# ---- the decoder's damage, written out per class -----------------------------------------------------------------------------------------------------
# lost frames and the one corrupted frame (a flipped byte in the side information at the end of the frame).  Every class loses frame 0.
#   blocks (silent 0-2, loud 3-5, silent 6-8, loud 9-11, silent 12-14, ...): the first loud frame after silence, which is also the frame behind an all-zero
#     frame (3); a burst of five from loud into silence (10 .. 14); the frame behind that silence (15 stays) and a last silent frame before noise (20)
#   impulses (frames 1, 4, 7 hold one; its tail fills the next frame, the third is all zero): the pulse behind the zero frame (4), a zero frame (9)
#   fade_in (all zero for almost two frames): the frame behind the last all-zero one (2); a burst of five in the loud part
#   clicks: a click frame (6) and the burst of five from a click frame into the quiet (14 .. 18)
#   the pitched classes have the LTPF active from about the third frame on: single losses behind active frames (5, 13) and a burst (17 .. 21)
LOSS = {
    "blocks": ((0, 3, 10, 11, 12, 13, 14, 20), 17),
    "impulses": ((0, 4, 9, 13, 14, 15, 16, 17), 7),
    "fade_in": ((0, 2, 11, 12, 13, 14, 15), 20),
    "clicks": ((0, 6, 14, 15, 16, 17, 18), 10),
    "square_100": ((0, 5, 13, 17, 18, 19, 20, 21), 9),
    "pulses_390": ((0, 5, 13, 17, 18, 19, 20, 21), 9),
    "pulses_57": ((0, 5, 13, 17, 18, 19, 20, 21), 9),
    "sine_1k": ((0, 5, 13, 17, 18, 19, 20, 21), 9),
}
LOSS_DEFAULT = ((0, 7, 12, 13, 14, 15, 16), 20)


def damage(frames, labels, nbytes):
    """frames [B, T, stride] -> (damaged copy, bfi uint8 [B, T]) by LOSS; byte nbytes - 2 of the corrupted frame is inverted, the frame is not marked"""
    frames = frames.copy()
    bfi = np.zeros(frames.shape[:2], np.uint8)
    for b, (k, _) in enumerate(labels):
        lost, bad = LOSS.get(k, LOSS_DEFAULT)
        bfi[b, [t for t in lost if t < frames.shape[1]]] = 1
        if bad < frames.shape[1]:
            frames[b, bad, nbytes[b] - 2] ^= 0xFF
    return frames, bfi


# ---- CPU encodes shared by the fixture's generator and the tests ------------------------------------------------------------------------------------
def stream_bytes(geom, rate):
    """bytes of a stream-frame (all channels); none of the geometries is 44.1 kHz"""
    return int(rate * GEOMS[geom][1] / 8000)


def encode(geom, enc_cls, T=T, trace=None, dual_mono=False, **kw):
    """every stream of the geometry through one encoder of enc_cls (lc3_harness.Oracle or Ref) -> uint8 [B, T, stride], zero behind a frame.
    trace: called as trace(b, t, traces) behind every frame (Oracle only).  dual_mono: a stereo stream through one mono encoder per channel, the first
    with the larger half of an odd size, their frames joined - what a stereo encoder does (R/enc_lc3_fl.c:162-174, R/setup_enc_lc3.c: the channels share
    nothing), and the only way to the compiled reference's bytes at an odd size: its lc3_enc_fl asserts that the bytes it wrote are channels x the first
    channel's."""
    fs, ms, hr, ch, rates, depth = GEOMS[geom]
    pcm, labels, rr = streams(geom, T)
    out = np.zeros((len(rr), T, max(stream_bytes(geom, r) for r in rr)), np.uint8)
    for b, r in enumerate(rr):
        nb = stream_bytes(geom, r)
        if dual_mono and ch == 2:
            at = 0
            for c, n in enumerate((nb - nb // 2, nb // 2)):
                o = enc_cls(fs, 1, ms, hr, int(n * 8000 / ms), **kw)
                assert o.nbytes == n
                for t in range(T):
                    out[b, t, at:at + n] = o.encode(pcm[b, t, c:c + 1], depth)
                at += n
            continue
        o = enc_cls(fs, ch, ms, hr, r, **kw)
        if hasattr(o, "enable_trace"):                         # the oracle checks the size it wrote against nbytes, and its getter - like the reference's -
            o.nbytes = nb                                      # gives channels x the first channel's for an odd stereo size
        tr = o.enable_trace() if trace else None
        for t in range(T):
            out[b, t, :nb] = o.encode(pcm[b, t], depth)[:nb]
            if trace:
                trace(b, t, tr)
    return out


def decode(geom, dec_cls, frames, bfi, **kw):
    """mono streams [B, T, stride] through one decoder each -> (int16 [B, T, 1, N], status uint8 [B, T]: 1 where the frame was concealed)"""
    fs, ms, hr, ch, rates, depth = GEOMS[geom]
    assert ch == 1
    _, labels, rr = streams(geom, frames.shape[1])
    pcm = np.zeros(frames.shape[:2] + (1, frame_len(fs, ms)), np.int16)
    st = np.zeros(frames.shape[:2], np.uint8)
    for b, r in enumerate(rr):
        d = dec_cls(fs, 1, ms, hr, **kw)
        for t in range(frames.shape[1]):
            rc, x = d.decode(frames[b, t, :stream_bytes(geom, r)], int(bfi[b, t]))
            assert rc in (0, 2), rc
            pcm[b, t], st[b, t] = x, rc == 2
    return pcm, st
