"""Streams that go quiet and streams that drop out (test infrastructure, a plain helper beside signal_classes.py): what the codec does for the half
second after a loud signal stops, and over loss bursts far longer than the concealment's ramp.  No GPU and no reference tree: the PCM is integer
arithmetic (signal_classes' sine table, np.random.RandomState integer draws), everything else comes from the CPU oracle.

Encoder.  enc_streams(family) -> int16 [9, T, N] in the order of CLASSES, which is fixed: the pitch kernel pairs streams 2k and 2k + 1, so every
pair holds a decaying stream beside one that does something else.  Every stream starts with LOUD = 6 loud frames; Q is the number of frames in
640 ms (64, 128, 256 at 10, 5, 2.5 ms).  The 12.8 kHz HP50 biquad rounds its state to float at every step, so after the input stops its output
decays through about 45 decades - past FLT_MIN into the subnormals and then to exactly zero - within about half a second, and the pitch chain
(square roots, divisions, the LTPF decision) runs on those operands the whole time.
  0 sine_tail       200 Hz sine of amplitude 20000, then zeros
  1 control_loud    200 Hz and its harmonics with a little noise, never quiet
  2 square_tail     100 Hz square at full scale, then zeros
  3 noise_tail      full-scale noise, then zeros
  4 dc_tail         constant -32768, then zeros
  5 control_silent  zeros throughout
  6 restart         the sine, Q / 3 zero frames, the sine again for 6 frames, then zeros: the sine returns onto a state of about 1e-16 .. 1e-19
  7 lsb_on_tail     the sine, 3 Q / 4 zero frames, 8 frames that each hold one sample of +1 or -1 in the middle, then zeros: the first of
                    them arrives on a subnormal state (1e-42 .. 1e-44)
  8 noise_stuck     noise_tail with another seed.  At 48 kHz / 2.5 ms the biquad's rounding does not let this one reach zero: over the last Q frames
                    of the stream every sample of the 12.8 kHz signal is about 3e-44 (23 or 24 units of the smallest subnormal), and every call
                    boundary there crosses HBM with a subnormal state.  About half of all seeds do this in that family, none in the others, where the
                    stream is one more noise tail.  It is the ninth stream, so the pitch kernel's last wave runs it beside its own shadow.
Length.  Q silent frames are enough for a full-scale signal to reach zero.  restart and lsb_on_tail make sound again late in the stream, and from a
sample of +-1 the state needs almost as long to reach zero as from full scale (it falls by about one decade per 10 ms, and full scale is only five
decades above 1).  So that every tail class reaches zero at least 3 frames before the end, every family's streams are T = LOUD + 3 Q / 4 + 8 + Q
frames long (126, 238, 462): lsb_on_tail's last +-1 frame is followed by Q zero frames as the plain tails' last loud frame is, and the other tails
are lengthened with it (more zeros).

What the oracle (portable math) gives on these streams is in MEASURED below, per family and tail class: the first frame (counted from 0) whose 12.8 kHz
signal holds a subnormal, and the first all-zero frame behind it.  For sine_tail that is frame 46 and 58 at 10 ms (the 40th and 52nd silent frame),
87 and 106 at 5 ms, 173 and 204 at 2.5 ms.  tests/test_quiet_tails_cpu.py asserts the table against enc_oracle().

Decoder.  dec_case(family) encodes control_loud-like PCM with the oracle and lays loss flags over the frames, one stream per pattern (PATTERNS),
DEC_T = 616 frames each.  The concealment damps the last good spectrum frame by frame.  On this signal its 16-bit PCM is last non-zero in lost frame
K = 71 at 48 kHz / 10 ms (mono and stereo) and 16 kHz / 5 ms, 69 at 96 kHz / 5 ms and 66 at 48 kHz / 2.5 ms, and all zero from K + 1 on (at 48 kHz /
10 ms the 70th is all zero as well: the scrambled signs decide which of the last frames still round to +-1).  The issue measured 70 / 71 on its
own signal; as it asks, each family's three boundary bursts lie at that family's own K: K, K + 1 and K + 10 lost frames (LAST_AUDIBLE).  At 24 bits
the PCM stays non-zero for about 35 frames more.  The float output x_out first holds a subnormal in lost frame 548 .. 556 and has not reached zero
after 600: the smallest subnormals times the damping factor round back to themselves.  MEASURED_DEC has both figures per family, asserted by the
CPU test.  All of it is read from the oracle, never from the device."""
import collections
import functools

import numpy as np

import signal_classes as sc
from lc3_harness import Oracle, OracleDecoder

FLT_MIN = np.float32(1.17549435e-38)
LOUD = 6
CLASSES = ("sine_tail", "control_loud", "square_tail", "noise_tail", "dc_tail", "control_silent", "restart", "lsb_on_tail", "noise_stuck")
TAILS = ("sine_tail", "square_tail", "noise_tail", "dc_tail", "restart", "lsb_on_tail")
PLAIN_TAILS = TAILS[:4]
NOISE_SEED = {"noise_tail": 7007, "noise_stuck": 7003}
# fs, frame_ms, hrmode, bitrate
FAMILIES = ((48000, 10.0, 0, 64000), (48000, 5.0, 0, 96000), (48000, 2.5, 0, 128000), (16000, 10.0, 0, 32000), (44100, 10.0, 0, 64000),
            (96000, 10.0, 1, 256000))


def fam_id(f):
    return "%dk_%s%s" % (f[0] // 1000, str(f[1]).replace(".", "p").replace("p0", ""), "_hr" if f[2] else "")


def quiet_frames(ms):
    return int(round(640 / ms))


def frame_len(fs, ms):
    return int((48000 if fs == 44100 else fs) * ms / 1000)


def n_frames(ms):
    q = quiet_frames(ms)
    return LOUD + 3 * q // 4 + 8 + q


def _sine(n, fs, amp=20000):
    return (sc.isin(sc._phase(n, 200, fs)) * amp + (1 << 29)) >> 30


def _loud(n, fs, rng):
    """200 Hz with harmonics 2 .. 4 and +-8 of noise: pitched, and never quiet"""
    x = sum((sc.isin(sc._phase(n, 200 * h, fs)) * (12000 // h) + (1 << 29)) >> 30 for h in range(1, 5))
    return x + rng.randint(-8, 9, size=n.size)


def layout(ms):
    """per class the frame ranges [a, b) that hold sound, in order"""
    q, T = quiet_frames(ms), n_frames(ms)
    first = [(0, LOUD)]
    return collections.OrderedDict([
        ("sine_tail", first), ("control_loud", [(0, T)]), ("square_tail", first), ("noise_tail", first), ("dc_tail", first), ("control_silent", []),
        ("restart", first + [(LOUD + q // 3, LOUD + q // 3 + 6)]), ("lsb_on_tail", first + [(LOUD + 3 * q // 4, LOUD + 3 * q // 4 + 8)]),
        ("noise_stuck", first)])


def enc_streams(family):
    """-> int16 [9, T, N], CLASSES"""
    fs, ms, hr, rate = family
    N, T = frame_len(fs, ms), n_frames(ms)
    n = np.arange(T * N, dtype=np.int64)
    fr = n // N
    lay = layout(ms)
    out = []
    for i, k in enumerate(CLASSES):
        rng = np.random.RandomState(NOISE_SEED.get(k, 7000 + i))
        on = np.zeros(n.size, bool)
        for a, b in lay[k]:
            on |= (fr >= a) & (fr < b)
        if k == "control_loud":
            x = _loud(n, fs, rng)
        elif k == "square_tail":
            x = np.where(sc._phase(n, 100, fs) < (1 << 31), 32767, -32768)
        elif k in NOISE_SEED:
            x = rng.randint(-32768, 32768, size=n.size)
        elif k == "dc_tail":
            x = np.full(n.size, -32768, np.int64)
        else:
            x = _sine(n, fs)
        x = np.where(on, x, 0)
        if k == "lsb_on_tail":                                             # in place of the sine's second stretch: one sample, +1 and -1 in turn
            a, b = lay[k][1]
            late = (fr >= a) & (fr < b)
            x = np.where(late, np.where(n % N == N // 2, np.where((fr - a) & 1, -1, 1), 0), x)
        assert x.min() >= -32768 and x.max() <= 32767
        out.append(x.astype(np.int16).reshape(T, N))
    return np.stack(out), CLASSES


# ---- the oracle on the encoder streams ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def enc_oracle(family):
    """Oracle(portable_math=True) over every stream, computed once and left unchanged -> dict: pcm [9, T, N], frames uint8 [9, T, nbytes],
    s12k8 float32 [9, T, 129], T0 int32 [9, T], normcorr float32 [9, T], ltpf int32 [9, T, 4] (ltpf_param[0 .. 2], ltpf_bits)"""
    fs, ms, hr, rate = family
    pcm, _ = enc_streams(family)
    S, T, N = pcm.shape
    r = dict(pcm=pcm, s12k8=np.zeros((S, T, 129), np.float32), T0=np.zeros((S, T), np.int32), normcorr=np.zeros((S, T), np.float32),
             ltpf=np.zeros((S, T, 4), np.int32))
    for s in range(S):
        o = Oracle(fs, 1, ms, hr, rate, portable_math=True)
        assert o.N == N
        if s == 0:
            r["frames"] = np.zeros((S, T, o.nbytes), np.uint8)
        tr = o.enable_trace()
        for t in range(T):
            r["frames"][s, t] = o.encode(pcm[s, t][None])
            w = tr[0]
            r["s12k8"][s, t] = np.ctypeslib.as_array(w.s12k8)
            r["T0"][s, t], r["normcorr"][s, t] = w.T0, w.normcorr
            r["ltpf"][s, t] = (w.ltpf_param[0], w.ltpf_param[1], w.ltpf_param[2], w.ltpf_bits)
    for v in r.values():
        v.flags.writeable = False
    return r


def subnormal_frames(s12k8):
    """[..., T, 129] -> bool [..., T]: the frame's smallest non-zero magnitude is below FLT_MIN"""
    a = np.abs(s12k8)
    return (np.where(a > 0, a, np.float32(1)) < FLT_MIN).any(axis=-1)


def zero_frames(s12k8):
    return ~(s12k8 != 0).any(axis=-1)


def windows(family):
    """per class in TAILS: (first frame with a subnormal in s12k8, first all-zero frame behind it) of its last decay"""
    r = enc_oracle(family)
    sub, zero = subnormal_frames(r["s12k8"]), zero_frames(r["s12k8"])
    lay = layout(family[1])
    out = collections.OrderedDict()
    for k in TAILS:
        s, last = CLASSES.index(k), lay[k][-1][1]
        a = last + int(np.flatnonzero(sub[s, last:])[0])
        out[k] = (a, a + int(np.flatnonzero(zero[s, a:])[0]))
    return out


def cut_length(family, lo=9, hi=32):
    """The call length of the product path's second run: the n in [lo, hi] for which a call boundary - a multiple of n - falls inside the subnormal
    window of the most tail classes, the four plain tails among them (asserted); the smallest such n.  A boundary b counts where frame b - 1, the
    last of its call, holds a subnormal and is not all zero: the HP50 state and the 12.8 kHz history that cross HBM there are subnormal."""
    win = windows(family)
    def hit(n, k):
        a, z = win[k]
        return any(a < b <= z for b in range(n, n_frames(family[1]), n))
    best = max(range(lo, hi + 1), key=lambda n: (all(hit(n, k) for k in PLAIN_TAILS), sum(hit(n, k) for k in TAILS), -n))
    assert all(hit(best, k) for k in PLAIN_TAILS), (family, win)
    return best, [k for k in TAILS if hit(best, k)]


# first subnormal frame, first all-zero frame behind it (windows()), per family in the order of FAMILIES and per class in the order of TAILS
MEASURED = {
    (48000, 10.0, 0, 64000): ((46, 58), (47, 58), (46, 56), (49, 59), (73, 85), (96, 107)),
    (48000, 5.0, 0, 96000): ((87, 106), (89, 108), (87, 105), (92, 109), (135, 154), (179, 198)),
    (48000, 2.5, 0, 128000): ((173, 204), (173, 209), (161, 202), (178, 209), (264, 295), (350, 381)),
    (16000, 10.0, 0, 32000): ((46, 58), (49, 58), (46, 56), (47, 59), (73, 85), (97, 108)),
    (44100, 10.0, 0, 64000): ((47, 57), (47, 57), (46, 56), (49, 59), (75, 84), (96, 107)),
    (96000, 10.0, 1, 256000): ((46, 58), (47, 58), (46, 57), (49, 58), (73, 85), (96, 108)),
}
STUCK = (48000, 2.5, 0, 128000)                    # the family in which noise_stuck never reaches zero


# ---- the decoder --------------------------------------------------------------------------------------------------------------------------------------
DEC_T = 616
GOOD = 8
VERY_LONG = 600
# fs, frame_ms, hrmode, channels, bitrate
DEC_FAMILIES = ((48000, 10.0, 0, 1, 64000), (48000, 2.5, 0, 1, 128000), (16000, 5.0, 0, 1, 32000), (96000, 5.0, 1, 1, 256000), (48000, 10.0, 0, 2, 128000))
# per decoder family K, the last lost frame (counted from 1) whose concealed 16-bit PCM is not all zero: the oracle's, asserted by the CPU test
LAST_AUDIBLE = {DEC_FAMILIES[0]: 71, DEC_FAMILIES[1]: 66, DEC_FAMILIES[2]: 71, DEC_FAMILIES[3]: 69, DEC_FAMILIES[4]: 71}
PATTERNS = ("burst_31", "burst_45", "burst_K", "burst_K1", "burst_K10", "from_start", "two_bursts", "very_long")
DEC_INT_FIELDS = ("bfi", "bw_idx", "lastnz", "lsb_mode", "gg_idx", "fac_ns", "nfilt", "tns_order", "tns_idx", "scf_idx", "ltpf", "nf_seed", "zero_frame", "nres")


def dec_fam_id(f):
    return fam_id(f[:3]) + ("_stereo" if f[3] == 2 else "")


def loss_flags(family):
    """uint8 [8, DEC_T] in the order of PATTERNS, and per pattern its bursts [(first lost frame, length)]"""
    K = LAST_AUDIBLE[family]
    bursts = collections.OrderedDict([("burst_31", [(GOOD, 31)]), ("burst_45", [(GOOD, 45)]), ("burst_K", [(GOOD, K)]), ("burst_K1", [(GOOD, K + 1)]),
                                      ("burst_K10", [(GOOD, K + 10)]), ("from_start", [(0, 80)]), ("two_bursts", [(GOOD, 40), (GOOD + 41, 40)]),
                                      ("very_long", [(GOOD, VERY_LONG)])])
    assert tuple(bursts) == PATTERNS and DEC_T == GOOD + VERY_LONG + GOOD
    bfi = np.zeros((len(PATTERNS), DEC_T), np.uint8)
    for i, k in enumerate(PATTERNS):
        for a, n in bursts[k]:
            bfi[i, a:a + n] = 1
    return bfi, bursts


def dec_cuts():
    """call boundaries: every 64 frames, which cuts very_long nine times and falls inside two_bursts' second burst (frames 49 .. 88), and 24, which
    falls inside every other burst (each starts at frame 8 or 0 and is at least 31 frames long)"""
    return sorted(set(range(0, DEC_T, 64)) | {24, DEC_T})


def int_fields(tr):
    """the integer fields of a DecTrace but the quantised spectrum, in the order of DEC_INT_FIELDS, as one int32 row"""
    return np.concatenate([np.atleast_1d(np.ctypeslib.as_array(getattr(tr, f)) if hasattr(getattr(tr, f), "__len__") else getattr(tr, f)) for f in DEC_INT_FIELDS]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def dec_case(family):
    """-> dict: frames uint8 [8, DEC_T, nbytes] (every stream the same loud PCM, encoded by the oracle), nbytes, bfi [8, DEC_T], bursts, and the oracle
    decoder's (portable math): pcm int16 [8, DEC_T, ch, N], pcm24 int32 of the same shape (24-bit output), status [8, DEC_T]; for very_long its trace:
    x_out float32 [DEC_T, ch, N] and ints int32 [DEC_T, ch, 38] (int_fields).  Computed once and left unchanged."""
    fs, ms, hr, ch, rate = family
    N = frame_len(fs, ms)
    n = np.arange(DEC_T * N, dtype=np.int64)
    pcm = np.stack([_loud(n, fs, np.random.RandomState(7100 + c)) for c in range(ch)]).astype(np.int16).reshape(ch, DEC_T, N).transpose(1, 0, 2)
    enc = Oracle(fs, ch, ms, hr, rate, portable_math=True)
    one = np.stack([enc.encode(np.ascontiguousarray(pcm[t])) for t in range(DEC_T)])
    bfi, bursts = loss_flags(family)
    S = len(PATTERNS)
    r = dict(frames=np.ascontiguousarray(np.broadcast_to(one, (S,) + one.shape)), nbytes=enc.nbytes, bfi=bfi, bursts=bursts,
             pcm=np.zeros((S, DEC_T, ch, N), np.int16), pcm24=np.zeros((S, DEC_T, ch, N), np.int32), status=np.zeros((S, DEC_T), np.uint8),
             x_out=np.zeros((DEC_T, ch, N), np.float32), ints=np.zeros((DEC_T, ch, 38), np.int32))
    for s in range(S):
        for bps in (16, 24):
            d = OracleDecoder(fs, ch, ms, hr, portable_math=True)
            tr = d.enable_trace() if PATTERNS[s] == "very_long" and bps == 16 else None
            for t in range(DEC_T):
                rc, x = d.decode(one[t], int(bfi[s, t]), bps)
                assert rc in (0, 2), rc
                r["pcm" if bps == 16 else "pcm24"][s, t] = x
                if bps == 16:
                    r["status"][s, t] = rc == 2
                if tr is not None:
                    for c in range(ch):
                        r["x_out"][t, c] = np.ctypeslib.as_array(tr[c].x_out)[:N]
                        r["ints"][t, c] = int_fields(tr[c])
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return r


# per decoder family, counted from 1 over very_long's lost frames: (the last with non-zero 16-bit PCM, the first whose x_out holds a subnormal)
MEASURED_DEC = {
    (48000, 10.0, 0, 1, 64000): (71, 552),
    (48000, 2.5, 0, 1, 128000): (66, 548),
    (16000, 5.0, 0, 1, 32000): (71, 555),
    (96000, 5.0, 1, 1, 256000): (69, 556),
    (48000, 10.0, 0, 2, 128000): (71, 548),
}
