"""The frame probe on the GPU (lc3plus_dec_batch_probe; kernels lc3_probe_side_kernel, lc3_probe_full_kernel, lc3_probe_full_kernel_g of
liblc3plus_probe_hip.so).  Every record is held to equality: FULL depth against the CPU oracle's verdict, reason and trace (frame_probe_ref), SIDE depth against
api.frame_info_side of the same payloads; the items are the stream-frames of hostile_frames.streams for all nine geometries, flattened in shuffled order at
odd offsets with gaps and duplicates.  Then the edge items, the bytes around info, statelessness against a twin batch, and the sibling library's own launch
counts.  Device buffers through ctypes (test_gpu_dec_varsize_device._Hip)."""
import collections
import functools
import os
import sys

import numpy as np
import pytest

import frame_probe_ref as ref
import hostile_frames as hf
from lc3_harness import sibling_launches
from test_gpu_dec_varsize_device import _Hip

pytestmark = pytest.mark.gpu
ALL_GEOMS = tuple(hf.GEOMS)
COUNTS = (1, 63, 64, 65, 255, 256, 257)           # lane, wave and workgroup edges (a FULL workgroup is up to four waves, a SIDE one 256 lanes)
W = ref.WORDS
SENT = 0x5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


@functools.lru_cache(maxsize=None)
def _layout(geom):
    """The geometry's items in one buffer: a shuffled order with every seventh item twice, each copy at its own place, one to three bytes of 0xC3 between
    neighbours so that the offsets take every alignment, the last item ending with the buffer (whose length is a multiple of four: no word of the buffer's
    lies outside it) -> (buf, offsets [n], sizes [n], item index [n])"""
    pl, _ = ref.geom_items(geom)
    rng = np.random.RandomState(len(pl) * 31 + len(geom))
    order = list(rng.permutation(len(pl)))
    order = [j for k, i in enumerate(order) for j in ([i, i] if k % 7 == 3 else [i])]
    offs, at = [], 1
    for k, i in enumerate(order):
        offs.append(at)
        at += len(pl[i]) + (0 if k == len(order) - 1 else 1 + k % 3)
    pad = -at % 4                                                  # move everything up so that the last item ends on the buffer's last byte
    buf = np.full(at + pad, 0xC3, np.uint8)
    offs = np.array(offs, np.int64) + pad
    for o, i in zip(offs, order):
        buf[o:o + len(pl[i])] = np.frombuffer(pl[i], np.uint8)
    sizes = np.array([len(pl[i]) for i in order], np.int32)
    assert offs[-1] + sizes[-1] == buf.size and buf.size % 4 == 0 and len({int(o) % 4 for o in offs}) == 4
    for a in (buf, offs, sizes):
        a.flags.writeable = False
    return buf, offs, sizes, np.array(order)


def _batch(geom, B=1):
    fs, ms, hr, ch, _ = hf.GEOMS[geom]
    return _amd().DecBatch(B, fs, ch, ms, hr, None, device=0)


def _probe(dev, d, d_buf, cap, offs, sizes, max_bytes, depth, hip_stream=None):
    """one call with sync -> records [n, channels, W]; the record behind the last one must come back untouched"""
    n = len(offs)
    d_info = dev.put(np.full((n + 1, d.channels, W), SENT, np.uint32))
    d.probe_device(d_buf, cap, dev.put(np.asarray(offs, np.int64)), dev.put(np.asarray(sizes, np.int32)), max_bytes, n, d_info, depth, hip_stream, sync=True)
    got = dev.get(d_info, (n + 1, d.channels, W), np.int32)
    assert (got[n].view(np.uint32) == SENT).all(), "a word behind the last record was written"
    return got[:n]


def _same(got, want, what):
    bad = np.argwhere((got != want).any(axis=(1, 2)))
    assert len(bad) == 0, (what, "first differing items", bad[:4].ravel().tolist(), got[bad[0, 0]].tolist(), want[bad[0, 0]].tolist())


@pytest.mark.parametrize("geom", ALL_GEOMS)
def test_records_equal_the_oracle(dev, geom):
    """All items of the geometry, then 1 ... 257 of them (the list repeated): FULL equals the oracle on every word of every item - status, reason, byte counts,
    and on the accepted ones the side information, the TNS orders and indices and nres; SIDE equals api.frame_info_side of the same payloads"""
    fs, ms, hr, ch, _ = hf.GEOMS[geom]
    pl, want = ref.geom_items(geom)
    buf, offs, sizes, item = _layout(geom)
    side = np.stack([_amd().api.frame_info_side(fs, ch, ms, hr, np.frombuffer(p, np.uint8)) for p in pl])
    _same(side, want[ref.SIDE], "frame_info_side against the oracle")
    d = _batch(geom)
    d_buf = dev.put(buf)
    mx = int(sizes.max())
    for n in (len(item),) + COUNTS:
        idx = np.arange(n) % len(item)
        if n < len(item):
            idx = (idx * 5 + n) % len(item)                          # not always the same first items
        for depth, w in ((ref.FULL, want[ref.FULL]), (ref.SIDE, side)):
            got = _probe(dev, d, d_buf, buf.size, offs[idx], sizes[idx], mx, depth)
            _same(got, w[item[idx]], (geom, n, depth))
    d.close()


def test_every_reason_is_compared():
    """A condition on test_records_equal_the_oracle, which compares every item of frame_probe_ref.geom_items at FULL depth: over the nine geometries each of the
    eleven reasons is there on at least three channel-frames, beside accepted, lost and skipped ones."""
    n = collections.Counter()
    for geom in ALL_GEOMS:
        w = ref.geom_items(geom)[1][ref.FULL]
        st, why = w[:, :, 0].reshape(-1), w[:, :, 1].reshape(-1)
        n.update(int(r) for r in why[st == ref.ST_CONCEALED])
        n["accepted"] += int((st == 0).sum()); n["lost"] += int((st & ref.ST_LOST != 0).sum()); n["skipped"] += int((st & ref.ST_SKIPPED != 0).sum())
    for r in hf.REASONS:
        assert n[r] >= 3, (hf.REJ_NAMES[r], dict(n))
    assert n["accepted"] >= 500 and n["lost"] >= 9 and n["skipped"] >= 3, dict(n)


@pytest.mark.parametrize("geom", ["48k_10_20B", "48k_10_mixed", "48k_10_stereo_161B", "96k_10_hr_625B"])
def test_edge_items(dev, geom):
    """Items the rule refuses, between good ones: offset -1, an end one byte past the capacity, a size above max_frame_bytes, a size the geometry refuses,
    size 0 (with a wild offset: it is not looked at).  Each gives its status bits and nothing else; the good items around them are unharmed.  The capacity ends
    inside the buffer, on the last good item's last byte."""
    fs, ms, hr, ch, _ = hf.GEOMS[geom]
    pl, want = ref.geom_items(geom)
    buf, offs, sizes, item = _layout(geom)
    good = [int(k) for k in np.flatnonzero(sizes > 0)[:6]]
    z = int(min(sizes[k] for k in good))
    cap = int(max(offs[k] + sizes[k] for k in good))
    ok_max = int(max(sizes[k] for k in good))
    small = int(min(sizes[k] for k in good))
    edge = [(-1, z, 2), (cap - z + 1, z, 2), (int(offs[good[0]]), 19 * ch, 2), (1 << 40, 0, 4), (-(1 << 40), 0, 4)]
    if ok_max > small:
        edge.append((int(offs[[k for k in good if sizes[k] == ok_max][0]]), ok_max, 2))       # a good size above max_frame_bytes
        mx = ok_max - 1
        good = [k for k in good if sizes[k] <= mx]
    else:
        edge.append((int(offs[good[0]]), z + ch, 2))                                          # the next size the geometry takes: above max_frame_bytes
        mx = ok_max
    o = [int(offs[k]) for k in good[:3]] + [e[0] for e in edge] + [int(offs[k]) for k in good[3:]]
    s = [int(sizes[k]) for k in good[:3]] + [e[1] for e in edge] + [int(sizes[k]) for k in good[3:]]
    first = len(good[:3])
    d = _batch(geom)
    d_buf = dev.put(buf)
    for depth in (ref.FULL, ref.SIDE):
        got = _probe(dev, d, d_buf, cap, o, s, mx, depth)
        for k, (_, _, bit) in enumerate(edge):
            r = got[first + k]
            assert (r[:, 0] == (ref.ST_CONCEALED | bit)).all() and not r[:, 1:].any(), (depth, k, r[:, :4].tolist())
        rest = np.concatenate([got[:first], got[first + len(edge):]])
        _same(rest, want[depth][item[good]], (geom, depth, "good items beside the edge items"))
    d.close()


@pytest.mark.parametrize("geom", ["48k_10_mixed", "48k_10_stereo_161B"])
def test_probe_is_stateless(dev, geom):
    """decode_packed 13 frames, probe (both depths, the hostile items; then one more queued with sync = 0 on a second stream), decode_packed the rest: PCM,
    status, get_state() and num_bytes() equal those of a fresh batch that makes the same two decode calls and no probe"""
    fs, ms, hr, ch, zs = hf.GEOMS[geom]
    frames, sizes, bfi, kind, reason = hf.streams(geom)
    B, T, N = sizes.shape[0], hf.T, hf.frame_len(fs, ms)
    nb, _ = hf.as_empty(sizes, bfi)
    stride = frames.shape[2]
    buf, offs, isz, item = _layout(geom)
    _, want = ref.geom_items(geom)

    def run(with_probe):
        d = _batch(geom, B)
        outs = []
        d_buf = dev.put(buf)
        for a, b in ((0, hf.CUT), (hf.CUT, T)):
            n = b - a
            fr = np.ascontiguousarray(frames[:, a:b])
            po = (np.arange(B * n, dtype=np.int64) * stride).reshape(B, n)
            pcm, st = dev.put(np.zeros((B, n, ch, N), np.int16)), dev.put(np.full((B, n), 0xEE, np.uint8))
            d.decode_device_packed(dev.put(fr), fr.size, dev.put(po), n, pcm, dev.put(np.ascontiguousarray(nb[:, a:b], np.int32)), stride, None, st, sync=True)
            outs.append((dev.get(pcm, (B, n, ch, N), np.int16), dev.get(st, (B, n), np.uint8)))
            if with_probe and a == 0:
                for depth in (ref.FULL, ref.SIDE):
                    _same(_probe(dev, d, d_buf, buf.size, offs, isz, int(isz.max()), depth), want[depth][item], (geom, depth))
                s2 = dev.stream()
                d_info = dev.put(np.full((len(offs), ch, W), SENT, np.uint32))
                d.probe_device(d_buf, buf.size, dev.put(offs), dev.put(isz), int(isz.max()), len(offs), d_info, ref.FULL, s2, sync=False)
                pending = (s2, d_info)
        if with_probe:
            dev.stream_sync(pending[0])
            _same(dev.get(pending[1], (len(offs), ch, W), np.int32), want[ref.FULL][item], (geom, "second stream"))
        out = (np.concatenate([x[0] for x in outs], axis=1), np.concatenate([x[1] for x in outs], axis=1), d.get_state(), [d.num_bytes(s) for s in range(B)])
        d.close()
        return out
    a, b = run(True), run(False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    o = hf.decode(geom, frames, sizes, bfi)
    assert np.array_equal(a[0], o["pcm"]) and np.array_equal(a[1] & 1, o["status"])


def test_host_convenience_call():
    geom = "24k_5_30B"
    pl, want = ref.geom_items(geom)
    d = _batch(geom)
    for depth in (ref.FULL, ref.SIDE):
        _same(d.probe(pl[:70], depth), want[depth][:70], (geom, depth))
    d.close()


def test_every_probe_kernel_ran_under_a_comparison(dev):
    """the sibling library counts its launches: every kernel its code object holds (tools/kernel_resources.py) has run - here, once more, each under a
    comparison, so that the test stands alone - and a name it does not hold is answered with -1"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels
    lib = os.path.join(ROOT, "audio_codec_amd", "liblc3plus_probe_hip.so")
    names = sorted(kernels(lib, "gfx950"))
    assert names == ["lc3_probe_full_kernel", "lc3_probe_full_kernel_g", "lc3_probe_side_kernel"]
    for geom in ("48k_10_20B", "48k_hr_156B"):                          # staged in LDS; read from global memory
        pl, want = ref.geom_items(geom)
        buf, offs, sizes, item = _layout(geom)
        d = _batch(geom)
        d_buf = dev.put(buf)
        for depth in (ref.FULL, ref.SIDE):
            _same(_probe(dev, d, d_buf, buf.size, offs, sizes, int(sizes.max()), depth), want[depth][item], (geom, depth))
        d.close()
    for n in names:
        assert sibling_launches("probe", n) > 0, n
    assert sibling_launches("probe", "lc3_dec_parse_kernel") == -1
