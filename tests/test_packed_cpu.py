"""Packed frames on the host alone: the offsets of lc3plus_enc_batch_encode_packed (test hook lc3plus_plan_packed, the scan and capacity rule the device
runs) and the frame rule of lc3plus_dec_batch_decode_packed (test hook lc3plus_dec_plan_packed_lenient, lc3d_dec_frame_class_packed)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lc3plus_enc_batch_encode_packed", "lc3plus_plan_packed", "lc3plus_dec_batch_decode_packed", "lc3plus_dec_plan_packed_lenient"]


def _api():
    from audio_codec_amd import api
    return api


def test_symbols_exported():
    api = _api()
    out = subprocess.run(["nm", "-D", "--defined-only", api.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in NEW:
        assert s in names, s
        assert s in api.EXPORTS, s


def _want(sizes, order, cap):
    S, T = sizes.shape
    flat = sizes.reshape(-1) if order == 0 else sizes.T.reshape(-1)
    ex = np.concatenate([[0], np.cumsum(flat.astype(np.int64))[:-1]])
    offs = ex.reshape(S, T) if order == 0 else ex.reshape(T, S).T
    ovf = np.where(offs + sizes > cap, 8, 0).astype(np.uint8)
    return offs, int(sizes.astype(np.int64).sum()), ovf


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("S,T", [(1, 1), (3, 7), (64, 64), (257, 9)])
def test_plan_packed_is_cumsum(order, S, T):
    api = _api()
    rng = np.random.default_rng(S * 31 + T + order)
    sizes = rng.integers(20, 401, size=(S, T)).astype(np.int32)
    rc, offs, total, ovf = api.plan_packed(sizes, order)
    want_offs, want_total, want_ovf = _want(sizes, order, 1 << 62)
    assert rc == 0
    assert (offs == want_offs).all() and total == want_total and not ovf.any()


@pytest.mark.parametrize("order", [0, 1])
def test_plan_packed_overflow_bits(order):
    api = _api()
    rng = np.random.default_rng(5 + order)
    sizes = rng.integers(20, 401, size=(40, 16)).astype(np.int32)
    for cap in (0, 1, 19, int(sizes.sum()) // 3, int(sizes.sum()) - 1, int(sizes.sum())):
        rc, offs, total, ovf = api.plan_packed(sizes, order, cap)
        want_offs, want_total, want_ovf = _want(sizes, order, cap)
        assert rc == 0
        assert (offs == want_offs).all() and total == want_total
        assert (ovf == want_ovf).all(), cap


def test_plan_packed_refusals():
    api = _api()
    sizes = np.full((2, 2), 40, np.int32)
    assert api.plan_packed(sizes, 2)[0] != 0
    assert api.plan_packed(sizes, 0, -1)[0] != 0
    assert api.plan_packed(sizes, -1)[0] != 0


GEOMS = [(48000, 1, 10.0, 0), (48000, 2, 10.0, 0), (16000, 2, 10.0, 0), (48000, 1, 2.5, 0), (96000, 1, 10.0, 1)]


@pytest.mark.parametrize("fs,channels,ms,hr", GEOMS)
def test_packed_rule_equals_slotted_rule_on_slots(fs, channels, ms, hr):
    api = _api()
    rng = np.random.default_rng(fs + channels + int(ms * 10) + hr)
    S, T, stride = 24, 16, 160 * channels
    nb = rng.integers(-3, stride + 40, size=(S, T)).astype(np.int32)
    nb[rng.random((S, T)) < 0.1] = 0
    bfi = rng.integers(0, 3, size=(S, T)).astype(np.uint8) * (rng.random((S, T)) < 0.1)
    start = rng.integers(20 * channels, 100 * channels, size=S).astype(np.int32)
    offs = (np.arange(S * T, dtype=np.int64) * stride).reshape(S, T)
    a = api.dec_plan_sizes_lenient(fs, channels, ms, hr, start, nb, bfi, stride)
    b = api.dec_plan_packed_lenient(fs, channels, ms, hr, start, nb, offs, S * T * stride, stride, bfi)
    assert a[0] == 0 and b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_packed_rule_offsets_capacity_and_size():
    api = _api()
    S, T = 3, 6
    nb = np.full((S, T), 80, np.int32)
    offs = (np.arange(S * T, dtype=np.int64) * 83 + 1).reshape(S, T)[::-1].copy()          # odd, out of order, with gaps
    cap = int(offs.max()) + 80
    start = np.full(S, 60, np.int32)
    nb[0, 1] = 100                                                                         # good: a new size the carry takes
    offs[0, 2] = -1                                                                        # negative offset
    offs[1, 3] = cap - 79                                                                  # one byte past the capacity
    nb[2, 4] = 121                                                                         # above max_frame_bytes
    nb[2, 5] = 0                                                                           # lost, its offset not looked at
    offs[2, 5] = -5
    rc, eff, lost, inv, end, mx = api.dec_plan_packed_lenient(48000, 1, 10.0, 0, start, nb, offs, cap, 120)
    assert rc == 0
    want_inv = np.zeros((S, T), np.uint8); want_inv[0, 2] = want_inv[1, 3] = want_inv[2, 4] = 1
    assert (inv == want_inv).all()
    want_lost = want_inv.copy(); want_lost[2, 5] = 1
    assert (lost == want_lost).all()
    assert list(eff[0]) == [80, 100, 100, 80, 80, 80]                                    # the invalid frame keeps the carry
    assert list(eff[1]) == [80, 80, 80, 80, 80, 80] and list(eff[2]) == [80, 80, 80, 80, 80, 80]
    assert list(end) == [80, 80, 80]
    # the exact capacity fits
    offs2 = offs.copy(); offs2[1, 3] = cap - 80
    assert api.dec_plan_packed_lenient(48000, 1, 10.0, 0, start, nb, offs2, cap, 120)[3][1, 3] == 0
    assert api.dec_plan_packed_lenient(48000, 1, 10.0, 0, start, nb, offs, cap, 0)[0] != 0
