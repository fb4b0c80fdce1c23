"""CPU: the crafted signal classes of signal_classes.py - that their PCM is what it was (one SHA-256 per class and shape), that on the exact shapes the
GPU tests use they reach the branches they were made for (a census over the oracle's trace), and that the oracle restatement equals the compiled reference
on them, encoder and decoder.  tests/golden/s1_signal_classes.npz holds the reference's frames and the reference decoder's digests
(make_golden_signal_classes.py); where oracle/_ref is built the reference also runs live."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import signal_classes as sc
from lc3_harness import Oracle, OracleDecoder, Ref, RefDecoder, have_ref, synth_pcm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("bw", "nfilt", "maxq", "lastnz", "lsb", "nres", "ltpf_on", "ltpf_active", "pidx", "attack", "fac_ns", "weighted", "reg")
MIN_FRAMES = 3


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "s1_signal_classes.npz")))


def test_pcm_is_bit_reproducible():
    with open(os.path.join(GOLDEN, "signal_classes_sha256.json")) as f:
        want = json.load(f)
    got = {}
    for g, (fs, ms, hr, ch, rates, depth) in sc.GEOMS.items():
        N = sc.frame_len(fs, ms)
        for k, x in sc.classes(fs, N, sc.T, depth).items():
            assert x.shape == (sc.T, N) and x.dtype == (np.int16 if depth == 16 else np.int32)
            got["%s/%d/%d/%d/%d" % (k, fs, N, sc.T, depth)] = sha(x)
    assert got == want, sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))


def test_the_order_keeps_the_extremes_together():
    """what the module's docstring promises about neighbours, and that a low-pass at or above fs / 2 is left out"""
    o = sc.ORDER
    for k in sc.PITCHED:
        assert any(n not in sc.PITCHED for n in (o[o.index(k) - 1], o[(o.index(k) + 1) % len(o)])), k
    for k in ("blocks", "impulses"):
        assert {o[o.index(k) - 1], o[o.index(k) + 1]} <= {"dc_min", "dc_plus3", "nyquist"}, k
    assert [k for k in sc.names(16000) if k.startswith("lp")] == ["lp3k", "lp7k"] and "lp15k" in sc.names(32000) and "lp15k" not in sc.names(24000)
    assert sc.names(48000, 24)[1:3] == ["dc_min", "dc_min24"] and "sine24" in sc.names(48000, 24) and len(sc.names(48000)) == len(o)
    pcm, labels, rates = sc.streams("48k_mono")
    assert [r for _, r in labels[:5]] == [24000, 64000, 128000, 320000, 24000] and labels[0][0] == labels[3][0] != labels[4][0]
    assert {k for pair in sc.STEREO_PAIRS for k in pair} == set(o)


# ---- the census -------------------------------------------------------------------------------------------------------------------------------------
def _record(tr, N):
    xq = np.abs(np.ctypeslib.as_array(tr.xq)[:N])
    return (tr.bw_idx, tr.tns_nfilt, int(xq.max()), tr.lastnz, tr.lsb_mode, tr.n_res_bits, tr.ltpf_param[0], tr.ltpf_param[1], tr.ltpf_param[2], tr.attack,
            tr.fac_ns, tr.tns_lpc_weighted, tr.reg_nonzero)


def _census_of(pcm, fs, ms, hr, ch, rates, depth, sizes):
    """the oracle's trace over pcm [B, T, ch, N] -> {field: int [B * ch, T]}"""
    B, T = pcm.shape[:2]
    rec = np.zeros((B * ch, T, len(FIELDS)), np.int64)
    for b in range(B):
        o = Oracle(fs, ch, ms, hr, rates[b], portable_math=True)
        o.nbytes = sizes[b]
        tr = o.enable_trace()
        for t in range(T):
            o.encode(pcm[b, t], depth)
            for c in range(ch):
                rec[b * ch + c, t] = _record(tr[c], o.N)
    return {k: rec[:, :, i] for i, k in enumerate(FIELDS)}


@functools.lru_cache(maxsize=None)
def census(geom):
    """-> fields [channel-streams, T], and per channel-stream its class and rate"""
    fs, ms, hr, ch, rates, depth = sc.GEOMS[geom]
    pcm, labels, rr = sc.streams(geom)
    r = _census_of(pcm, fs, ms, hr, ch, rr, depth, [sc.stream_bytes(geom, x) for x in rr])
    r["cls"] = np.array([k for name, _ in labels for k in name.split("+")])
    r["rate"] = np.repeat(rr, ch)
    r["ylen"] = sc.frame_len(fs, ms) if hr else min(sc.frame_len(fs, ms), int(400 * ms / 10))     # the coded spectrum
    return r


def _zero(r):
    return r["maxq"] == 0


def _after_coded(r):
    z = _zero(r)
    return np.concatenate([np.zeros_like(z[:, :1]), z[:, 1:] & ~z[:, :-1]], axis=1)


def _before_coded(r):
    z = _zero(r)
    return np.concatenate([z[:, :-1] & ~z[:, 1:], np.zeros_like(z[:, :1])], axis=1)


def _pidx(lo, hi, active):
    return lambda r: (r["ltpf_on"] == 1) & (r["pidx"] >= lo) & (r["pidx"] <= hi) & ((r["ltpf_active"] == 1) | (not active))


ALL_GEOMS = tuple(sc.GEOMS)
NOISE = ("lp3k", "lp7k", "lp11k", "lp15k")
SILENT = ("blocks", "impulses", "fade_in")
# name, predicate over census(geom) -> bool [channel-streams, T], the geometries (a geometry, or a geometry and a rate) and the classes expected to meet it
# on at least MIN_FRAMES frames in each of them.  Frames of other classes do not count.
TARGETS = [
    ("bw 0 at 48 kHz", lambda r: r["bw"] == 0, ["48k_mono", "48k_stereo", "48k_24bit"], ("lp3k",)),
    ("bw 1 at 48 kHz", lambda r: r["bw"] == 1, ["48k_mono", "48k_stereo", "48k_24bit"], ("lp7k",)),
    ("bw 2 at 48 kHz", lambda r: r["bw"] == 2, ["48k_mono", "48k_stereo", "48k_24bit"], ("lp11k",)),
    ("bw 3 at 48 kHz", lambda r: r["bw"] == 3, ["48k_mono", "48k_stereo", "48k_24bit"], ("lp15k",)),
    ("bw 0 at 32 kHz", lambda r: r["bw"] == 0, ["32k_10"], ("lp3k",)),
    ("bw 1 at 32 kHz", lambda r: r["bw"] == 1, ["32k_10"], ("lp7k",)),
    ("bw 2 at 32 kHz", lambda r: r["bw"] == 2, ["32k_10"], ("lp11k",)),
    ("bw 0 at 24 and 16 kHz", lambda r: r["bw"] == 0, ["24k_5", "16k_2p5"], ("lp3k",)),
    ("one TNS filter at 48 kHz", lambda r: r["nfilt"] == 1, [("48k_mono", x) for x in sc.GEOMS["48k_mono"][4]], ("lp3k", "lp7k", "lp11k")),
    ("all-zero frame directly after a coded one", _after_coded, ALL_GEOMS, SILENT),
    ("all-zero frame directly before a coded one", _before_coded, ALL_GEOMS, SILENT),
    ("lastnz at the end of the coded spectrum", lambda r: r["lastnz"] == r["ylen"], [("48k_mono", 64000), "48k_hr", "96k_hr", "16k_2p5"],
     ("dither", "nyquist", "blocks")),
    ("lastnz at the very start beside coded frames", lambda r: (r["lastnz"] == 2) & (_after_coded(r) | _before_coded(r)), ALL_GEOMS, SILENT),
    ("lsb_mode 1 without residual bits", lambda r: (r["lsb"] == 1) & (r["nres"] == 0), [("48k_mono", 128000), ("48k_mono", 320000), "32k_10", "48k_hr"],
     ("clipped",)),
    ("max |xq| >= 2^20 in high resolution", lambda r: r["maxq"] >= 1 << 20, ["48k_hr", "96k_hr"], ("dc_min", "nyquist")),
    ("max |xq| >= 2^10 in normal mode", lambda r: r["maxq"] >= 1 << 10, [("48k_mono", 64000), ("48k_mono", 320000), "48k_24bit", "32k_10"],
     ("dc_min", "dc_plus3", "sine_1k")),
    ("pitch index 0 .. 379, LTPF active", _pidx(0, 379, True), [("48k_mono", 24000), ("48k_mono", 64000), "48k_stereo", "24k_5"], ("pulses_390", "sine_1k")),
    ("pitch index 380 .. 439, LTPF active", _pidx(380, 439, True), [("48k_mono", 24000), ("48k_mono", 64000), "48k_stereo", "24k_5"], ("square_100",)),
    ("pitch index 440 .. 511, LTPF active", _pidx(440, 511, True), [("48k_mono", 24000), ("48k_mono", 64000), "48k_stereo", "24k_5"], ("pulses_57",)),
    ("pitch index 380 .. 439 coded, LTPF inactive", lambda r: _pidx(380, 439, False)(r) & (r["ltpf_active"] == 0),
     [("48k_mono", 128000), "48k_hr", "96k_hr"], ("square_100",)),
    ("attack detected", lambda r: r["attack"] == 1, [("48k_mono", 128000), "48k_24bit", "32k_10"], ("impulses", "clicks", "blocks", "square_100")),
    ("TNS LPC weighting ran", lambda r: r["weighted"] > 0, [("48k_mono", 24000)], ("pulses_390", "sine_1k", "sweep")),
    ("high-resolution regulariser not zero", lambda r: r["reg"] == 1, ["48k_hr", "96k_hr", "96k_2p5_hr"], sc.ORDER),
] + [("fac_ns %d" % k, (lambda k: lambda r: (r["fac_ns"] == k) & ~_zero(r))(k), ["48k_mono"], sc.ORDER) for k in range(8)]
# Targets no class can meet stay here with the reason, (name, predicate, geometries, reason); test_every_target_is_reached asserts that they are still unmet,
# so that a class that starts to reach one moves it up.
UNREACHABLE = [
    ("a coded frame whose lastnz is 2", lambda r: (r["lastnz"] == 2) & ~_zero(r), ALL_GEOMS,
     "every class that is not silent has energy above the first pair of lines: a DC input leaks through the MDCT window into dozens of lines (lastnz >= 14 for "
     "dc_plus3 in every geometry), and the quantiser's offset of 0.375 only empties a frame whole"),
]
# rates of 48 kHz / 10 ms without attack handling (frames below 100 or from 340 bytes), and the geometries without it (not 10 ms, or high resolution)
NO_ATTACK = [("48k_mono", 24000), ("48k_mono", 64000), ("48k_mono", 320000), "24k_5", "16k_2p5", "48k_hr", "96k_hr", "96k_2p5_hr"]


def _count(pred, where, classes):
    geom, rate = where if isinstance(where, tuple) else (where, None)
    r = census(geom)
    m = pred(r) & np.isin(r["cls"], classes)[:, None]
    if rate is not None:
        m &= (r["rate"] == rate)[:, None]
    return int(m.sum())


def test_every_target_is_reached():
    short = [(name, where, n) for name, pred, wheres, classes in TARGETS for where in wheres for n in [_count(pred, where, classes)] if n < MIN_FRAMES]
    assert not short, short
    for name, pred, wheres, reason in UNREACHABLE:
        assert reason and all(_count(pred, w, sc.ORDER + sc.ORDER_24) == 0 for w in wheres), name
    for where in NO_ATTACK:
        assert _count(lambda r: r["attack"] == 1, where, sc.ORDER) == 0, where


def test_the_synthetic_pcm_reaches_none_of_the_bandwidth_and_transition_targets():
    """what justifies this file: on the suite's own generator, 64 streams x 40 frames at 48 kHz / 10 ms / 64 kbit/s, the detected bandwidth is the full
    band on every frame and no stream goes from coded to all-zero or back"""
    pcm = synth_pcm(64, 40, 480, 48000, seed=1717)[:, :, None, :]
    r = _census_of(pcm, 48000, 10.0, 0, 1, [64000] * 64, 16, [80] * 64)
    assert (r["bw"] == 4).all() and (r["nfilt"] == 2).all()
    assert not _after_coded(r).any() and not _before_coded(r).any() and _zero(r).all(axis=1).sum() == 1


# ---- the oracle's own pin ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ALL_GEOMS)
def test_oracle_equals_the_reference_s_frames_on_every_class(geom):
    """the fixture's half of the comparison, which needs no compiled reference: both builds of the oracle give the reference's bytes"""
    want = fixture()["frames/" + geom]
    for pm in (False, True):
        got = sc.encode(geom, Oracle, portable_math=pm)
        assert got.shape == want.shape
        bad = np.argwhere((got != want).any(axis=2))
        assert len(bad) == 0, (geom, pm, len(bad), [(sc.streams(geom)[1][b], t) for b, t in bad[:6].tolist()])


def test_oracle_equals_the_compiled_reference_on_every_class():
    """Oracle (glibc math) against Ref, Oracle(portable_math=True) against Oracle, byte for byte, over every geometry; the fixture is what Ref gives now"""
    if not have_ref():
        pytest.skip("oracle/_ref is not built")
    for geom in ALL_GEOMS:
        ref = sc.encode(geom, Ref, dual_mono=True)
        assert np.array_equal(ref, fixture()["frames/" + geom]), (geom, "make_golden_signal_classes.py")
        glibc, pm = sc.encode(geom, Oracle), sc.encode(geom, Oracle, portable_math=True)
        assert np.array_equal(glibc, ref), (geom, np.argwhere((glibc != ref).any(axis=2))[:6].tolist())
        assert np.array_equal(pm, glibc), (geom, np.argwhere((pm != glibc).any(axis=2))[:6].tolist())


def _damaged(geom):
    frames = fixture()["frames/" + geom]
    _, labels, rr = sc.streams(geom)
    return sc.damage(frames, labels, [sc.stream_bytes(geom, r) for r in rr])


def test_the_damage_is_what_the_module_says():
    """signal_classes.LOSS against the census of the encoder that made the frames: frame 0, the frame behind an all-zero frame, the first loud frame after
    silence, a burst of five from loud into silence, a loss directly behind a frame with the LTPF active, one corrupted frame that is not marked"""
    r = census("48k_mono")
    frames, bfi = _damaged("48k_mono")
    clean = fixture()["frames/48k_mono"]
    assert (bfi[:, 0] == 1).all()
    for b in range(bfi.shape[0]):
        changed = np.flatnonzero((frames[b] != clean[b]).any(axis=1))
        assert len(changed) == 1 and bfi[b, changed[0]] == 0 and (frames[b, changed[0]] != clean[b, changed[0]]).sum() == 1
    z, lost = _zero(r), bfi == 1
    k = r["cls"] == "blocks"
    assert (lost[k, 3] & z[k, 2] & ~z[k, 3]).all()                              # the first loud frame after silence: the frame behind an all-zero frame
    assert lost[k, 10:15].all() and not lost[k, 9].any() and not lost[k, 15].any() and (~z[k, 10] & z[k, 14]).all()      # five, from loud into silence
    k = r["cls"] == "impulses"
    assert (lost[k, 4] & z[k, 3]).all()
    k = r["cls"] == "fade_in"
    assert (lost[k, 2] & z[k, 0]).all()
    k = np.isin(r["cls"], sc.PITCHED) & (r["rate"] <= 64000)
    assert (lost[k, 5] & (r["ltpf_active"][k, 4] == 1)).all() and (lost[k, 13] & (r["ltpf_active"][k, 12] == 1)).all()


@pytest.mark.parametrize("geom", sc.DEC_GEOMS)
def test_decoder_restatement_on_every_class(geom):
    """OracleDecoder (glibc math) against the reference decoder's digests of the fixture, and sample for sample against RefDecoder where it is built.
    The portable-math build, which the GPU tests compare with, evaluates the SNS gains' and the global gain's powf as (float)pow((double)): the libm
    boundary of DESIGN section 4.  Against the reference that may move a sample by one LSB (test_oracle_vs_ref.test_decoder_portable_math_boundary_at_24_bits
    has the rule: at most 1 LSB, more than 99.9 % identical); on these classes it does so at 16 bits too - 4 of 829 440 samples at 48 kHz / 10 ms, in a
    concealed frame of blocks and fade_in and a decoded frame of lp15k, none in the other geometries - and never changes a status."""
    frames, bfi = _damaged(geom)
    want = fixture()["dec/" + geom]
    pcm, st = sc.decode(geom, OracleDecoder, frames, bfi)
    bad = [b for b in range(len(want)) if sha(pcm[b], st[b]) != want[b]]
    assert not bad, (geom, [sc.streams(geom)[1][b] for b in bad[:6]])
    assert (st[bfi == 1] == 1).all() and (st[:, 1:][bfi[:, 1:] == 0] == 0).mean() > 0.9          # the corrupted frame may or may not be noticed
    pm, pm_st = sc.decode(geom, OracleDecoder, frames, bfi, portable_math=True)
    d = np.abs(pm.astype(np.int32) - pcm)
    print(geom, "portable math against glibc: samples that differ", int((d != 0).sum()), "of", d.size)
    assert np.array_equal(pm_st, st) and d.max() <= 1 and (d != 0).mean() < 1e-3
    if have_ref():
        ref_pcm, ref_st = sc.decode(geom, RefDecoder, frames, bfi)
        assert [sha(ref_pcm[b], ref_st[b]) for b in range(len(want))] == want.tolist(), "make_golden_signal_classes.py"
        assert np.array_equal(pcm, ref_pcm) and np.array_equal(st, ref_st)
