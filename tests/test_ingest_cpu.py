"""Packet ingest without a GPU (include/lc3plus_batch.h "Packet ingest"): the exported symbols and constants, every refusal of lc3plus_dec_batch_ingest in the
header's order (its checks run before anything of the batch or the device is touched), and lc3plus_plan_ingest - the text the kernels run - against the numpy
restatement of the rule (ingest_ref.rule) on every output array over the generated lists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audio_codec_amd
from audio_codec_amd import api
import ingest_ref as ref

NEW = ["lc3plus_dec_batch_ingest", "lc3plus_plan_ingest"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LC3_ERROR, LC3_NULL_ERROR = 1, 3
REQUIRED = ("stream", "seq", "offsets", "num_bytes", "base", "out_offsets", "out_num_bytes", "cell_item", "counts")
ARGS = ("stream", "seq", "offsets", "num_bytes", "info", "base", "floor", "seq_bits", "n_frames", "out_offsets", "out_num_bytes", "cell_item", "counts", "next_base",
        "stats", "item_status")


def test_symbols_are_exported():
    L = audio_codec_amd.load_library()
    for s in NEW:
        assert s in api.EXPORTS and hasattr(L, s), s


def test_status_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define\s+LC3PLUS_ING_(\w+)\s+(\d+)", text)}
    want = dict(USED=1, DUPLICATE=2, LATE=4, EARLY=8, BAD_STREAM=16, EMPTY=32, REFUSED=64, INVALID=128, STATS_WORDS=4)
    assert header == want
    for k, v in want.items():
        assert getattr(api, "ING_" + k) == v == getattr(ref, k, v), k
    assert (api.FI_ST_INVALID, api.FI_ST_LOST, api.FRAME_INFO_WORDS) == (ref.FI_INVALID, ref.FI_LOST, ref.WORDS)


def _refusals(call):
    """call(**overrides) -> the return code; the arguments are good unless overridden"""
    for k in REQUIRED:
        assert call(**{k: None}) == LC3_NULL_ERROR, k
    for k in ("info", "floor", "next_base", "stats", "item_status"):
        for kw in (dict(n=0), dict(seq_bits=8)):
            assert call(**dict(kw, **{k: None})) == LC3_ERROR, (k, kw)                # an optional NULL is no refusal: the value check behind it answers
    for kw in (dict(n=0), dict(n=-5), dict(n=1 << 29), dict(n=1 << 40), dict(n_frames=0), dict(n_frames=-3), dict(seq_bits=0), dict(seq_bits=15), dict(seq_bits=17),
               dict(seq_bits=24), dict(seq_bits=64)):
        assert call(**kw) == LC3_ERROR, kw
    for k in REQUIRED:                                                                 # NULL first
        assert call(n=0, seq_bits=3, n_frames=0, **{k: None}) == LC3_NULL_ERROR, k


def test_ingest_refusals_need_no_device():
    """a zero-filled block stands in for the batch: no refusal looks at it, and none writes to it or to an array"""
    L = audio_codec_amd.load_library()
    fake = C.create_string_buffer(4096)
    arr = C.create_string_buffer(256)
    p = C.cast(arr, C.c_void_p)
    good = dict({k: p for k in ARGS}, b=C.cast(fake, C.c_void_p), n=1, seq_bits=16, n_frames=1)

    def call(**kw):
        a = dict(good, **kw)
        return L.lc3plus_dec_batch_ingest(a["b"], a["n"], *[a[k] for k in ARGS], None, 1)
    assert call(b=None) == LC3_NULL_ERROR and call(b=None, n=0) == LC3_NULL_ERROR and call(b=None, stream=None, seq_bits=1) == LC3_NULL_ERROR
    _refusals(call)
    assert fake.raw == bytes(4096) and arr.raw == bytes(256)


def test_plan_refusals():
    L = audio_codec_amd.load_library()
    arr = C.create_string_buffer(256)
    p = C.cast(arr, C.c_void_p)
    good = dict({k: p for k in ARGS}, S=1, ch=1, n=1, seq_bits=16, n_frames=1)

    def call(**kw):
        a = dict(good, **kw)
        return L.lc3plus_plan_ingest(a["S"], a["ch"], a["n"], *[a[k] for k in ARGS])
    _refusals(call)
    for kw in (dict(S=0), dict(S=-1), dict(ch=0)):
        assert call(**kw) == LC3_ERROR, kw
    assert call(S=0, stream=None) == LC3_NULL_ERROR
    assert arr.raw == bytes(256)
    with pytest.raises(api.LC3Error):
        api.plan_ingest(2, 1, [0], [0], [0], [20], [0, 0], 4, seq_bits=12)


def _plan(c, optional=api.ING_OPTIONAL):
    return api.plan_ingest(c["n_streams"], c["channels"], c["stream"], c["seq"], c["offsets"], c["num_bytes"], c["base"], c["n_frames"], c["seq_bits"], c["info"],
                           c["floor"], optional)


def same(got, want, name, keys=ref.KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (name, k, got[k].dtype, got[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (name, k, "first differences at", bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


@pytest.mark.parametrize("name", list(ref.cpu_lists()))
def test_plan_equals_the_rule(name):
    c = ref.cpu_lists()[name]
    want = ref.rule(c)
    same(_plan(c), want, name)
    for optional in ((), ("stats",), ("item_status",), ("next_base",)):                  # the optional outputs NULL: the others are what they were
        got = _plan(c, optional)
        assert all(got[k] is None for k in api.ING_OPTIONAL if k not in optional)
        same(got, want, (name, optional), ref.KEYS[:4] + optional)


def test_rule_on_a_list_by_hand():
    """the restatement itself, on one stream of four frames written out: base 65534, so the frames are 65534, 65535, 0, 1"""
    V = ref.VERDICTS
    seq = [0, 65535, 0, 65533, 2, 65534, 1, 65535, 1]
    stream = [0, 0, 0, 0, 0, 0, 3, 0, 0]
    verdicts = ["refused0", "invalid", "ok", "ok", "ok", "lost", "ok", "refused0", "ok"]
    nb = [30, 31, 32, 33, 34, 35, 36, 37, 0]
    info = np.zeros((9, 1, ref.WORDS), np.int32)
    info[:, 0, 0] = [V[v][0] for v in verdicts]
    c = dict(n_streams=1, channels=1, n_frames=4, seq_bits=16, stream=stream, seq=seq, offsets=np.arange(9) * 100 + 7, num_bytes=nb, base=[65534], info=info,
             floor=None)
    r = ref.rule(c)
    assert r["cell_item"].tolist() == [[-1, 7, 2, -1]] and r["offsets"].tolist() == [[0, 707, 207, 0]] and r["num_bytes"].tolist() == [[0, 37, 32, 0]]
    assert r["counts"].tolist() == [3] and r["next_base"].tolist() == [1] and r["stats"].tolist() == [[3, 1, 1, 1]]
    assert r["item_status"].tolist() == [2 | 64, 2 | 128, 1, 4, 8, 32, 16, 1 | 64, 32]
    same(_plan(c), r, "by hand")
    c.update(floor=[9])
    r = ref.rule(c)
    assert r["counts"].tolist() == [4] and r["next_base"].tolist() == [2] and r["stats"].tolist() == [[4, 2, 1, 1]]
    same(_plan(c), r, "by hand, floor")
