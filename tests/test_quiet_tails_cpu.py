"""CPU: the streams of quiet_tails.py reach what they were made for, so that tests/test_gpu_quiet_tails.py cannot pass by missing it.  Everything here
is the oracle's (portable math): the 12.8 kHz signal of every tail class turns subnormal and then exactly zero, the LTPF is still switched on in
all-zero frames well behind the last loud one, the late +-1 samples and the restarted sine arrive on the state they were timed for, the loss bursts end
on either side of the last audible concealed frame, and the long burst's float output is subnormal and not zero at its end.  The figures in the helper's
docstring and tables are asserted against the oracle, and the PCM is pinned by one SHA-256 per (family, class)."""
import hashlib
import json
import os

import numpy as np
import pytest

import quiet_tails as qt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quiet_tails_sha256.json")
FAM = pytest.mark.parametrize("family", qt.FAMILIES, ids=qt.fam_id)
DEC_FAM = pytest.mark.parametrize("family", qt.DEC_FAMILIES, ids=qt.dec_fam_id)


def _nonzero_min(x):
    a = np.abs(np.asarray(x)).ravel()
    return a[a > 0].min() if (a > 0).any() else np.float32(0)


def test_pcm_is_bit_reproducible():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = {}
    for fam in qt.FAMILIES:
        pcm, names = qt.enc_streams(fam)
        assert pcm.dtype == np.int16 and pcm.shape == (len(qt.CLASSES), qt.n_frames(fam[1]), qt.frame_len(fam[0], fam[1])) and names == qt.CLASSES
        for k, x in zip(names, pcm):
            got["%s/%s" % (qt.fam_id(fam), k)] = hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()
    assert got == want, sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))


@FAM
def test_the_streams_are_laid_out_as_the_module_says(family):
    fs, ms, hr, rate = family
    pcm, names = qt.enc_streams(family)
    q, T = qt.quiet_frames(ms), pcm.shape[1]
    assert q == {10.0: 64, 5.0: 128, 2.5: 256}[ms] and T == qt.LOUD + 3 * q // 4 + 8 + q
    assert names[:8] == ("sine_tail", "control_loud", "square_tail", "noise_tail", "dc_tail", "control_silent", "restart", "lsb_on_tail")
    loud = pcm.astype(np.int64).__abs__().max(axis=2)                        # [stream, frame]
    lay = qt.layout(ms)
    for s, k in enumerate(names):
        on = np.zeros(T, bool)
        for a, b in lay[k]:
            on[a:b] = True
        assert ((loud[s] > 0) == on).all(), k
        if k != "control_silent":
            assert loud[s, :qt.LOUD].min() >= 12000, k
    assert lay["restart"] == [(0, 6), (6 + q // 3, 12 + q // 3)] and lay["lsb_on_tail"] == [(0, 6), (6 + 3 * q // 4, 14 + 3 * q // 4)]
    a, b = lay["lsb_on_tail"][1]
    late = pcm[names.index("lsb_on_tail"), a:b]
    assert (np.abs(late).sum(axis=1) == 1).all() and late[:, pcm.shape[2] // 2].tolist() == [1, -1] * 4
    assert (pcm[names.index("dc_tail"), :qt.LOUD] == -32768).all() and set(np.unique(pcm[names.index("square_tail"), :qt.LOUD])) == {-32768, 32767}


@FAM
def test_every_tail_turns_subnormal_and_then_zero(family):
    """in every family and every tail class the oracle's s12k8 has a frame whose smallest non-zero magnitude is below FLT_MIN and a later frame that is
    all zero, at least 3 frames before the end of the stream; the frames are the ones the helper's table gives"""
    r = qt.enc_oracle(family)
    T = r["pcm"].shape[1]
    win = qt.windows(family)
    for k in qt.TAILS:
        s = qt.CLASSES.index(k)
        a, z = win[k]
        m = _nonzero_min(r["s12k8"][s, a])
        print(qt.fam_id(family), k, "first subnormal frame", a, "smallest non-zero magnitude there", m, "first all-zero frame", z, "of", T)
        assert 0 < m < qt.FLT_MIN, k
        assert a < z <= T - 3 and not r["s12k8"][s, z].any(), k
        assert not r["s12k8"][s, z:].any(), k                                    # and it stays zero
    assert tuple(win.values()) == qt.MEASURED[family]
    s = qt.CLASSES.index("control_silent")
    assert not r["s12k8"][s].any() and not r["ltpf"][s, :, 0].any()
    s = qt.CLASSES.index("control_loud")
    assert not qt.subnormal_frames(r["s12k8"][s]).any() and _nonzero_min(r["s12k8"][s]) > 1e-6 and r["ltpf"][s, 3:, 0].all()


def test_the_stuck_noise_tail_never_reaches_zero_at_2p5_ms():
    """noise_stuck at 48 kHz / 2.5 ms: over the last Q frames every sample of the 12.8 kHz signal is a few dozen units of the smallest subnormal (3e-44) and no frame is all zero; in the other
    families the stream reaches zero like the other tails"""
    for fam in qt.FAMILIES:
        r = qt.enc_oracle(fam)
        x = r["s12k8"][qt.CLASSES.index("noise_stuck")]
        n12 = int(128 * fam[1] / 10)
        if fam == qt.STUCK:
            tail = np.abs(x[-qt.quiet_frames(fam[1]):, :n12])
            assert (tail > 0).all() and tail.max() < 1e-43 and not qt.zero_frames(x[qt.LOUD:]).any()
        else:
            assert qt.subnormal_frames(x).any() and qt.zero_frames(x)[-3:].all()


@FAM
def test_the_ltpf_is_on_in_all_zero_frames_of_the_tail(family):
    """at least one tail class has an all-zero input frame more than 3 frames behind the last loud one whose ltpf_param[0] is 1"""
    r = qt.enc_oracle(family)
    lay = qt.layout(family[1])
    found = {}
    for k in qt.TAILS:
        s = qt.CLASSES.index(k)
        last = lay[k][0][1] - 1                                                  # the last frame of the first loud stretch
        stop = lay[k][1][0] if len(lay[k]) > 1 else r["pcm"].shape[1]
        assert not r["pcm"][s, last + 1:stop].any()
        on = [t - last for t in range(last + 4, stop) if r["ltpf"][s, t, 0] == 1]
        if on:
            found[k] = on
    print(qt.fam_id(family), "silent frames behind the last loud one with the LTPF on:", found)
    assert found
    # lags and the normalised correlation keep moving far into the tail: the pitch chain is at work on the decaying operands
    s = qt.CLASSES.index("sine_tail")
    moves = np.flatnonzero(np.diff(r["T0"][s]))
    assert moves[-1] >= qt.LOUD + 20 * (10 / family[1]), moves[-1]
    nc = r["normcorr"][s, qt.LOUD:]
    assert ((nc > 0) & (nc < 1e-30)).any()


@FAM
def test_the_late_samples_arrive_on_the_state_they_were_timed_for(family):
    r = qt.enc_oracle(family)
    lay = qt.layout(family[1])
    s, a = qt.CLASSES.index("lsb_on_tail"), lay["lsb_on_tail"][1][0]
    prev = np.abs(r["s12k8"][s, a - 1])
    assert prev.any() and 0 < prev[prev > 0].max() < qt.FLT_MIN, "the first +-1 frame does not fall on a subnormal state"
    assert np.abs(r["pcm"][s, a]).sum() == 1
    s, a = qt.CLASSES.index("restart"), lay["restart"][1][0]
    prev = np.abs(r["s12k8"][s, a - 1])
    n12 = int(128 * family[1] / 10)
    assert (prev[:n12] >= qt.FLT_MIN).all() and prev.max() < 1e-6, "the sine does not return onto a small normal state"
    assert r["pcm"][s, a].any() and not r["pcm"][s, a - 1].any()


@FAM
def test_a_call_boundary_falls_into_every_subnormal_window(family):
    n, hit = qt.cut_length(family)
    r = qt.enc_oracle(family)
    assert n > 8 and set(qt.PLAIN_TAILS) <= set(hit)
    for k in hit:
        s = qt.CLASSES.index(k)
        ok = [b for b in range(n, r["pcm"].shape[1], n) if 0 < _nonzero_min(r["s12k8"][s, b - 1]) < qt.FLT_MIN]
        assert ok, k
    print(qt.fam_id(family), "call length", n, "boundaries inside the window of", hit)


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------------------
@DEC_FAM
def test_the_bursts_end_on_either_side_of_the_last_audible_frame(family):
    r = qt.dec_case(family)
    K = qt.LAST_AUDIBLE[family]
    pcm, bfi, P = r["pcm"], r["bfi"], qt.PATTERNS
    assert (r["status"] == bfi).all()                                           # every undamaged frame decodes, every lost one is concealed
    assert [int(bfi[i].sum()) for i in range(8)] == [31, 45, K, K + 1, K + 10, 80, 80, 600]
    for i, k in enumerate(P[:5]):
        a, n = r["bursts"][k][0]
        assert a == qt.GOOD and not bfi[i, :a].any() and bfi[i, a:a + n].all() and not bfi[i, a + n:].any()
    assert pcm[P.index("burst_K"), qt.GOOD + K - 1].any(), "the K-burst does not end on a frame with non-zero PCM"
    for k in ("burst_K1", "burst_K10", "very_long"):
        i = P.index(k)
        last = qt.GOOD + int(bfi[i].sum())
        assert not pcm[i, qt.GOOD + K:last].any(), k                             # all zero from the (K + 1)th lost frame to the end of the burst
        assert pcm[i, last:last + 8].any()                                       # and the stream comes back
    for k in ("burst_31", "burst_45"):
        i = P.index(k)
        assert pcm[i, qt.GOOD:qt.GOOD + int(k[6:])].any(axis=(1, 2)).all()       # audible concealment in every frame of the shorter bursts
    i = P.index("two_bursts")
    assert bfi[i, 8:48].all() and not bfi[i, 48] and bfi[i, 49:89].all() and not bfi[i, 89:].any() and pcm[i, 49:89].any(axis=(1, 2)).all()
    i = P.index("from_start")
    assert bfi[i, :80].all() and not bfi[i, 80:].any() and not pcm[i, :80].any() and pcm[i, 80].any()
    cuts = qt.dec_cuts()
    for i, k in enumerate(P):                                                    # a call boundary inside every burst, very_long cut every 64 frames
        for a, n in r["bursts"][k]:
            assert any(a < c < a + n for c in cuts), k
    assert set(range(64, qt.DEC_T, 64)) <= set(cuts)


@DEC_FAM
def test_the_long_burst_ends_subnormal_and_not_zero(family):
    r = qt.dec_case(family)
    i = qt.PATTERNS.index("very_long")
    lost = slice(qt.GOOD, qt.GOOD + qt.VERY_LONG)
    x = np.abs(r["x_out"][lost]).reshape(qt.VERY_LONG, -1)
    last = x[-1][x[-1] > 0]
    print(qt.dec_fam_id(family), "last lost frame: non-zero samples", last.size, "of", x.shape[1], "smallest", last.min(), "largest", last.max())
    assert last.size and 0 < last.min() < qt.FLT_MIN
    assert x.any(axis=1).all()                                                   # never zero within the burst
    mn = np.where(x > 0, x, np.float32(1)).min(axis=1)
    audible = np.flatnonzero(r["pcm"][i, lost].any(axis=(1, 2)))
    assert (int(audible[-1]) + 1, int(np.flatnonzero(mn < qt.FLT_MIN)[0]) + 1) == qt.MEASURED_DEC[family]
    assert qt.MEASURED_DEC[family][0] == qt.LAST_AUDIBLE[family]
    assert np.flatnonzero(r["pcm24"][i, lost].any(axis=(1, 2)))[-1] + 1 > qt.LAST_AUDIBLE[family] + 20          # 24 bits hear the concealment for longer
    assert (r["ints"][lost, :, 0] == 1).all() and not r["ints"][lost, :, 1:].any()                               # a lost frame's trace: bfi, nothing parsed
