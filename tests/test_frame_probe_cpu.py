"""The frame probe without a GPU (include/lc3plus_batch.h "Frame probe"): the exported symbols, the reason names against the oracle's, every refusal of
lc3plus_dec_batch_probe (its checks run before anything of the batch or the device is touched), and lc3plus_frame_info_side - the SIDE depth on the host, the
text the kernels run - word for word against the CPU oracle over every frame of hostile_frames.streams for all nine geometries and over the genuine frames of
tests/golden/d1_decoder_operating_points.npz."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

import audio_codec_amd
from audio_codec_amd import api
import frame_probe_ref as ref
import hostile_frames as hf
from lc3_harness import reject_names

NEW = ["lc3plus_dec_batch_probe", "lc3plus_frame_info_side", "lc3plus_reject_name"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "d1_decoder_operating_points.npz")


def test_symbols_are_exported():
    L = audio_codec_amd.load_library()
    for s in NEW:
        assert s in api.EXPORTS and hasattr(L, s), s
    assert (api.PROBE_SIDE, api.PROBE_FULL, api.FRAME_INFO_WORDS) == (0, 1, 48) == (ref.SIDE, ref.FULL, ref.WORDS)
    assert (api.FI_STATUS, api.FI_REASON, api.FI_NUM_BYTES, api.FI_BW_IDX, api.FI_TNS_ORDER, api.FI_TNS_IDX, api.FI_SCF_IDX, api.FI_LTPF, api.FI_NRES) == \
        (0, 1, 2, 3, 9, 11, 27, 34, 37)
    assert (api.FI_ST_CONCEALED, api.FI_ST_INVALID, api.FI_ST_LOST, api.FI_ST_SKIPPED) == (1, 2, 4, 8)


def test_reason_names_are_the_oracle_s():
    names = reject_names()
    assert api.reject_names() == names == hf.REJ_NAMES and len(names) == api.REJ_COUNT == 12
    L = audio_codec_amd.load_library()
    assert L.lc3plus_reject_name(-1) == b"" and L.lc3plus_reject_name(12) == b""
    for i, n in enumerate(names):
        assert getattr(api, "REJ_" + n.upper()) == i


def test_probe_refusals_need_no_device():
    """NULL arguments, then the value checks, in that order; the batch is never looked at before them (a block of zeros stands in for it)"""
    L = audio_codec_amd.load_library()
    fake = C.create_string_buffer(4096)
    b, p = C.cast(fake, C.c_void_p), C.cast(C.create_string_buffer(64), C.c_void_p)
    good = dict(b=b, frames=p, cap=64, offs=p, nb=p, mx=20, n=1, depth=0, info=p)

    def call(**kw):
        a = dict(good, **kw)
        return L.lc3plus_dec_batch_probe(a["b"], a["frames"], a["cap"], a["offs"], a["nb"], a["mx"], a["n"], a["depth"], a["info"], None, 1)
    LC3_ERROR, LC3_NULL_ERROR = 1, 3
    for k in ("b", "frames", "offs", "nb", "info"):
        assert call(**{k: None}) == LC3_NULL_ERROR, k
    for kw in (dict(n=0), dict(n=-5), dict(mx=0), dict(mx=-1), dict(cap=-1), dict(depth=2), dict(depth=-1)):
        assert call(**kw) == LC3_ERROR, kw
    assert call(b=None, n=0) == LC3_NULL_ERROR                          # NULL first
    assert fake.raw == bytes(4096)


def test_frame_info_side_refusals():
    L = audio_codec_amd.load_library()
    info = np.zeros((2, 48), np.int32)
    fr = np.zeros(40, np.uint8)
    assert L.lc3plus_frame_info_side(48000, 1, 10.0, 0, fr.ctypes.data, 40, None) == 3
    assert L.lc3plus_frame_info_side(48000, 1, 10.0, 0, None, 40, info.ctypes.data) == 3
    assert L.lc3plus_frame_info_side(12345, 1, 10.0, 0, fr.ctypes.data, 40, info.ctypes.data) != 0
    assert L.lc3plus_frame_info_side(48000, 3, 10.0, 0, fr.ctypes.data, 40, info.ctypes.data) != 0


def _compare_side(fs, ms, hr, ch, payload, want):
    got = api.frame_info_side(fs, ch, ms, hr, np.frombuffer(payload, np.uint8))
    assert got.shape == (ch, 48)
    assert np.array_equal(got, want), (fs, ms, hr, ch, len(payload), got.tolist(), want.tolist())


@pytest.mark.parametrize("geom", list(hf.GEOMS))
def test_side_records_on_hostile_streams(geom):
    """every stream-frame: words 0 - 2 are the oracle's verdict restricted to reasons 1 - 4, an empty payload is lost, a channel behind a refused channel 0 is
    skipped, and wherever the side information is accepted every word equals the oracle's trace (also on the frames a later check refuses)"""
    fs, ms, hr, ch, _ = hf.GEOMS[geom]
    pl, want = ref.geom_items(geom)
    full = want[ref.FULL]
    for i, p in enumerate(pl):
        w = want[ref.SIDE][i]
        _compare_side(fs, ms, hr, ch, p, w)
        for c in range(ch):                                              # the rule itself, against the FULL (= the decoder's) verdict
            if len(p) == 0:
                assert w[c, 0] == ref.ST_CONCEALED | ref.ST_LOST and not w[c, 1:].any()
            elif full[i, c, 0] == ref.ST_CONCEALED and full[i, c, 1] in ref.SIDE_REASONS:
                assert w[c, 0] == ref.ST_CONCEALED and w[c, 1] == full[i, c, 1] and not w[c, 3:].any()
                assert (w[c + 1:, 0] == (ref.ST_CONCEALED | ref.ST_SKIPPED)).all() and not w[c + 1:, 3:].any()
            elif full[i, c, 0] == 0:
                assert w[c, 0] == 0 and w[c, 1] == 0 and np.array_equal(w[c, 3:ref.TNS_ORDER], full[i, c, 3:ref.TNS_ORDER]) and np.array_equal(w[c, 27:37], full[i, c, 27:37])
    # a size the geometry refuses, and a negative one
    for nb in (19 * ch, 401 * ch if not hr else 626 * ch):
        got = api.frame_info_side(fs, ch, ms, hr, np.zeros(nb, np.uint8))
        assert np.array_equal(got, ref.invalid(ch)), nb


def test_side_records_on_genuine_frames():
    """the frames of the decoder's golden operating points (17 geometries, mono and stereo; the encoder's own frames, a few damaged on purpose): every word the
    oracle's, and most of them accepted"""
    z = np.load(GOLDEN)
    n = acc = 0
    for k in [str(t) for t in z["tags"]]:
        fs, dms, hr, ch = (int(v) for v in z[k + "_cfg"])
        frames, nbytes = z[k + "_frames"], z[k + "_nbytes"]
        for s in range(frames.shape[0]):
            for t in range(0, frames.shape[1], 3):
                p = frames[s, t, :int(nbytes[s])].tobytes()
                w = ref.records(fs, dms / 10.0, hr, ch, p)
                _compare_side(fs, dms / 10.0, hr, ch, p, w[ref.SIDE])
                n += 1; acc += int((w[ref.FULL][:, 0] == 0).all())
    assert n >= 200 and acc >= n * 3 // 4, (n, acc)


def test_every_side_reason_is_compared():
    """A condition on test_side_records_on_hostile_streams, which compares every record of frame_probe_ref.geom_items: over the nine geometries each of the
    reasons 1 - 4 is there at least three times (the hostile-frame census guarantees them per geometry), with lost and skipped channel-frames and accepted ones
    beside them - so that no reason can pass by being absent."""
    n = collections.Counter()
    for geom in hf.GEOMS:
        w = ref.geom_items(geom)[1][ref.SIDE]
        st, why = w[:, :, 0].reshape(-1), w[:, :, 1].reshape(-1)
        n.update(int(r) for r in why[st == ref.ST_CONCEALED])
        n["accepted"] += int((st == 0).sum()); n["lost"] += int((st & ref.ST_LOST != 0).sum()); n["skipped"] += int((st & ref.ST_SKIPPED != 0).sum())
    for r in ref.SIDE_REASONS:
        assert n[r] >= 3, (r, dict(n))
    assert set(n) - {"accepted", "lost", "skipped"} == set(ref.SIDE_REASONS), dict(n)         # nothing else refuses at this depth
    assert n["accepted"] >= 500 and n["lost"] >= 9 and n["skipped"] >= 3, dict(n)
