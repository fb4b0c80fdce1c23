"""CPU: the oracle restatement against the unmodified ETSI reference at EVERY frame size of every operating point (tests/size_sweep.py), encoder and decoder.
The scheme is test_oracle_vs_ref.py's: where the compiled reference is built (oracle/_ref) every case runs it live and checks that the committed digests still
match it; everywhere else the restatement's outputs are compared with those digests (md5 of the reference's outputs per family and block of 16 sizes,
tests/golden/size_sweep_digests.json, written from the live reference by tests/golden/make_golden_size_sweep.py).  The GPU comparison of
test_gpu_size_sweep.py means nothing until this pin holds."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

import size_sweep as S
from lc3_harness import OracleDecoder, Ref, RefDecoder, have_ref
from test_oracle_vs_ref import md5

HERE = os.path.dirname(os.path.abspath(__file__))
DIGESTS = os.path.join(HERE, "golden", "size_sweep_digests.json")
HEADER = "_header"
family = pytest.mark.parametrize("family", S.FAMILIES, ids=S.ids())


@functools.lru_cache(maxsize=None)
def _digests():
    with open(DIGESTS) as f:
        return json.load(f)


def reference(key, live):
    """The reference's result for `key`: the committed one, which `live()` (the same computation on the compiled reference) must reproduce wherever
    oracle/_ref is built."""
    want = _digests()[key]
    if have_ref():
        assert live() == want, (key, "the compiled reference disagrees with tests/golden/size_sweep_digests.json (make_golden_size_sweep.py)")
    return want


@functools.lru_cache(maxsize=None)
def oracle_sweep(fam):
    """(the exact-math oracle's frames of every stream [B, T, max size], the census) - one encode serves the four tests of a family"""
    out = []
    c = S.census(fam, frames_out=out)
    out[0].flags.writeable = False
    return out[0], c


def enc_digests(fam, frames):
    """{block tag: md5 of the frames of the streams whose size lies in the block, in stream order}"""
    _, nbytes, _ = S.streams(fam)
    return {tag: md5(*[frames[b, :, :n] for b, n in enumerate(nbytes) if n in ss]) for tag, ss in S.blocks(fam)}


def dec_case(fam, frames):
    """the frames of every stream of the sweep, damaged: (frames, nbytes, bfi).  The edge streams belong to it: the pitched one is what keeps the decoder's
    LTPF running on either side of each step of its gain table, which a one-per-size stream does only by chance."""
    _, nb, _ = S.streams(fam)
    fr, bfi = S.damage(fam, frames, nb)
    return fr, nb, bfi


def dec_digests(fam, dec_cls, frames, **kw):
    fr, nb, bfi = dec_case(fam, frames)
    pcm, st = S.decode_streams(fam, dec_cls, fr, nb, bfi, **kw)
    return {tag: md5(*[x for b, n in enumerate(nb) if n in ss for x in (fr[b, :, :n], bfi[b], st[b], pcm[b])]) for tag, ss in S.blocks(fam)}


def _differing_blocks(got, want):
    return sorted(k for k in want if got.get(k) != want[k])


def test_families_are_the_soak_configurations():
    spec = importlib.util.spec_from_file_location("soak", os.path.join(os.path.dirname(HERE), "tools", "soak.py"))
    soak = importlib.util.module_from_spec(spec); spec.loader.exec_module(soak)
    assert [(fs, ms, hr) for fs, ms, hr, _ in soak.configurations()] == list(S.FAMILIES)
    for (fs, ms, hr, rates), fam in zip(soak.configurations(), S.FAMILIES):
        assert max(rates) == S.rate_for(fam, S.sizes(fam)[-1]), fam            # the soak's top rate is the family's real maximum


@family
def test_sizes_rates_and_edges(family):
    """The range is the reference's (R/setup_enc_lc3.c:196-230: 20 ... 400 bytes, in high-resolution mode from the minimum bitrate to 210 / 375 / 625),
    every size has a bitrate that gives exactly it, one below and one above the range are refused, and edges() holds both sides of every threshold."""
    fs, ms, hr = family
    ss = S.sizes(family)
    assert (ss[0], ss[-1]) == ((20, 400) if not hr else ({(48000, 10.0): 156, (48000, 5.0): 93, (48000, 2.5): 54, (96000, 10.0): 187, (96000, 5.0): 109,
                                                           (96000, 2.5): 62}[(fs, ms)], {2.5: 210, 5.0: 375, 10.0: 625}[ms]))
    assert [S.rate_for(family, n) for n in ss] == sorted({S.rate_for(family, n) for n in ss})
    N = S.frame_len(family)
    for n in (ss[0] - 1, ss[-1] + 1):
        assert S._plan(family, -(-n * 8 * fs // N)) is None
    from audio_codec_amd.api import LC3Error, plan_chan
    for n in (ss[0] - 1, ss[-1] + 1):                                         # the decoder's range (derive_dchan) is the encoder's
        with pytest.raises(LC3Error) as err:
            plan_chan(fs, ms, hr, n)
        assert err.value.code == 7
    assert all(plan_chan(fs, ms, hr, n)["total_bits"] == 8 * n for n in (ss[0], ss[-1]))
    e = S.edges(family)
    assert set(e) <= set(ss) and {ss[0], ss[-1]} <= set(e)
    for n, words in S.thresholds(family):
        assert n in e and n - 1 in e, (n, words)
    assert {n for n in S.RUNTIME_EDGES if ss[0] <= n <= ss[-1]} <= set(e)
    names = {w for _, words in S.thresholds(family) for w in words}
    assert "budget_step" in names                                             # 1 280 or 2 560 total bits lie inside every family's range
    if not hr:
        assert {"ltpf_enable", "dec_ltpf_beta_idx"} <= names
    if ms == 10.0 and not hr and fs >= 32000:
        assert "attack_handling" in names
    pcm, nbytes, labels = S.streams(family)
    more = sum(len(nn) for _, nn in S.FAMILY_EXTRA.get(family, ()))
    assert pcm.shape == (len(ss) + 4 * len(e) + more, S.T, N) and [n for n, k in labels if k == "silence"] == list(e)
    assert not pcm[[i for i, (_, k) in enumerate(labels) if k == "silence"]].any()
    assert (pcm[[i for i, (_, k) in enumerate(labels) if k == "dc_min"]] == -32768).all()


@family
def test_encoder_oracle_equals_reference(family):
    """Every stream of the sweep - one per size, five at the edges - through the exact-math oracle: byte for byte the compiled reference's frames."""
    frames, _ = oracle_sweep(family)
    want = reference("enc/" + S.key(family), lambda: enc_digests(family, S.encode_streams(family, Ref)))
    bad = _differing_blocks(enc_digests(family, frames), want)
    assert not bad, (family, "blocks of sizes that differ", bad)


@family
def test_decoder_oracle_equals_reference(family):
    """The frames of every stream of the sweep, lost (0.15) and corrupted (0.1) as make_dec_case does it: PCM and status of the exact-math decoder
    restatement equal lc3_dec_fl of the compiled reference."""
    frames, _ = oracle_sweep(family)
    want = reference("dec/" + S.key(family), lambda: dec_digests(family, RefDecoder, frames))
    bad = _differing_blocks(dec_digests(family, OracleDecoder, frames, portable_math=False), want)
    assert not bad, (family, "blocks of sizes that differ", bad)


def portable_math_count(fam, frames):
    """(frames the portable-math build of the oracle encodes differently from the exact-math build, frames)"""
    pcm, nbytes, _ = S.streams(fam)
    pm = S.oracle_encode(fam, pcm, nbytes, portable_math=True)
    return int((pm != frames).any(axis=2).sum()), int(pm.shape[0] * pm.shape[1])


@family
def test_portable_math_boundary(family):
    """liblc3_oracle_pm.so - libm calls as (float)f((double)x), what the HIP kernels compute - against the exact-math oracle over the sweep: the project's
    existing condition (at least 97 % of the frames equal, test_mono_golden[portable]).  The count recorded when the digests were written is printed beside
    today's, so that a change of the host's libm is visible."""
    frames, _ = oracle_sweep(family)
    differ, total = portable_math_count(family, frames)
    print("portable math %s: %d of %d frames differ (recorded: %s)" % (S.key(family), differ, total,
                                                                       _digests()[HEADER]["portable_math_differing_frames"][S.key(family)]))
    assert total - differ >= 0.97 * total, (family, differ, total)


def census_row(fam, c):
    return "%-12s %6d %6d %6d %6d %6d %6d %6d" % ((S.key(fam),) + tuple(c[w] for w in S.CENSUS_WORDS))


CENSUS_HEAD = "%-12s %6s %6s %6s %6s %6s %6s %6s" % ("family", "frames", "above", ">1024", "lsb", "ltpf", "attack", "lsb all")


def lsb_mode_possible(fam):
    """R/quantize_spec.c: the quantiser's mode flag, without which no frame is in LSB mode, is set from the total bits for fs < 48000 and fs == 48000 only -
    at 96 kHz no size sets it"""
    return fam[0] != 96000


@family
def test_census_reach(family):
    """What the sweep reaches beyond the earlier rate lists (top: 320 kbit/s): every family of 2.5 and 5 ms without the high-resolution mode has at least ten
    frames above that top that leave more than 1 024 bits between the writer's cursors; every family has an LSB-mode frame - except at 96 kHz, where the
    reference's rule cannot set the mode at any size, and the count must then be zero."""
    fs, ms, hr = family
    _, c = oracle_sweep(family)
    print(CENSUS_HEAD); print(census_row(family, c))
    assert c["frames"] == len(S.streams(family)[1]) * S.T
    if not hr and ms in (2.5, 5.0):
        assert c["unused_gt_1024"] >= 10, c
    if lsb_mode_possible(family):
        assert c["lsb_mode_all_sizes"] >= 1, c
    else:
        assert c["lsb_mode_all_sizes"] == 0, c


def reference_cases():
    """(key, the reference's result) for every committed digest, and the header: tests/golden/make_golden_size_sweep.py writes them."""
    header = {"what": "md5 of the compiled reference's outputs per family and block of 16 sizes (tests/test_size_sweep_cpu.py); portable_math_differing_frames: "
                      "[frames liblc3_oracle_pm.so encodes differently from liblc3_oracle.so, frames] on the machine that wrote this file",
              "portable_math_differing_frames": {}}
    for fam in S.FAMILIES:
        frames = S.encode_streams(fam, Ref)
        yield "enc/" + S.key(fam), enc_digests(fam, frames)
        yield "dec/" + S.key(fam), dec_digests(fam, RefDecoder, frames)
        header["portable_math_differing_frames"][S.key(fam)] = list(portable_math_count(fam, oracle_sweep(fam)[0]))
    yield HEADER, header
