"""GPU tests on the hostile payloads of hostile_frames.py: frames refused for every reason the reference has, next to accepted random payloads and genuine
frames, through every variant of the bitstream parser (lc3_dec_parse.inc) and on through concealment and synthesis.  Every comparison is an equality with
the portable-math CPU oracle, PCM sample for sample and status byte for byte; tests/test_hostile_frames_cpu.py counts, on the same arrays, which refusal
each frame is.  Device buffers through ctypes (test_gpu_dec_varsize_device._Hip)."""
import ctypes as C
import functools

import numpy as np
import pytest

import hostile_frames as hf
from lc3_harness import DecTrace, OracleDecoder
from test_gpu_dec_varsize_device import _Hip, _cmp, _device_calls

pytestmark = pytest.mark.gpu
ALL_GEOMS = tuple(hf.GEOMS)
ABSENT = 8
SENT, ST_SENT = 0x5A, 0xEE


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


@functools.lru_cache(maxsize=None)
def _case(geom):
    """the geometry's streams and the oracle's result, computed once and left unchanged"""
    fs, ms, hr, ch, zs = hf.GEOMS[geom]
    frames, sizes, bfi, kind, reason = hf.streams(geom)
    o = hf.decode(geom, frames, sizes, bfi)
    c = dict(fs=fs, ms=ms, hr=hr, ch=ch, B=len(zs), N=hf.frame_len(fs, ms), frames=frames, sizes=sizes, bfi=bfi, kind=kind, reason=reason,
             full=hf.stream_sizes(geom), want=o["pcm"], wst=o["status"], stride=frames.shape[2], pats=hf.patterns(geom))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def _batch(c, sizes=None, B=None):
    return _amd().DecBatch(B or c["B"], c["fs"], c["ch"], c["ms"], c["hr"], sizes, device=0)


# ---- the fixed-size parser: lc3_dec_parse_kernel, lc3_dec_parse_kernel_g ----------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ALL_GEOMS)
def test_fixed_size_parser(geom):
    """decode() in two launches of 13 + 11 frames, an empty frame given as flagged; the stream that changes its size does so between the launches"""
    c = _case(geom)
    _, fl = hf.as_flags(c["sizes"], c["bfi"], c["full"])
    d = _batch(c, [int(x) for x in c["full"][:, 0]])
    a, sa = d.decode(c["frames"][:, :hf.CUT], fl[:, :hf.CUT])
    for s in np.flatnonzero(c["full"][:, hf.CUT] != c["full"][:, 0]):
        assert d.set_num_bytes(int(s), int(c["full"][s, hf.CUT])) == 0
    b, sb = d.decode(c["frames"][:, hf.CUT:], fl[:, hf.CUT:])
    _cmp(np.concatenate([a, b], axis=1), np.concatenate([sa, sb], axis=1), c["want"], c["wst"])
    d.close()


# ---- per-frame sizes: lc3_dec_parse_kernel_var, lc3_dec_parse_kernel_g_var ------------------------------------------------------------------------------
@pytest.mark.parametrize("losses", ["flags", "empty"])
@pytest.mark.parametrize("geom", ALL_GEOMS)
def test_per_frame_sizes(dev, geom, losses):
    """decode_device_sizes under the input-ready promise, two calls of 12 queued back to back; every loss given through bfi, then every loss as size 0"""
    c = _case(geom)
    nb, fl = hf.as_flags(c["sizes"], c["bfi"], c["full"]) if losses == "flags" else hf.as_empty(c["sizes"], c["bfi"])
    d = _batch(c)
    d.set_input_ready(True)
    got, st = _device_calls(dev, d, c["frames"], nb, fl, [0, 12, hf.T])
    _cmp(got, st, c["want"], c["wst"])
    d.close()


# ---- packed frames: lc3_dec_parse_kernel_var_pk, lc3_dec_parse_kernel_g_var_pk ----------------------------------------------------------------------------
def _packed(dev, d, c, order):
    """the present frames back to back in `order` behind one shift byte, no gap between them -> (pcm, status)"""
    B, T = c["B"], hf.T
    nb, fl = hf.as_empty(c["sizes"], c["bfi"])
    offs = np.zeros((B, T), np.int64)
    total = int(nb.sum())
    buf = np.full(1 + total + 8, 0xC3, np.uint8)
    at = 0
    for s, t in order:
        if nb[s, t]:
            offs[s, t] = at
            buf[1 + at:1 + at + nb[s, t]] = c["frames"][s, t, :nb[s, t]]
            at += int(nb[s, t])
    assert at == total
    pcm, st = dev.put(np.full(B * T * c["ch"] * c["N"] * 2, SENT, np.uint8)), dev.put(np.full((B, T), ST_SENT, np.uint8))
    d.decode_device_packed(dev.put(buf) + 1, total, dev.put(offs), T, pcm, dev.put(nb.astype(np.int32)), c["stride"], None, st, sync=True)
    return dev.get(pcm, (B, T, c["ch"], c["N"]), np.int16), dev.get(st, (B, T), np.uint8)


@pytest.mark.parametrize("geom", ["48k_10_20B", "48k_10_mixed", "48k_hr_156B", "48k_10_stereo_161B"])
def test_packed_frames(dev, geom):
    """Frames back to back from an odd address (the unaligned staging loop), so that a frame's neighbours are other hostile frames; then the same frames in
    another order in the arena: a reader that strays past its frame changes the result."""
    c = _case(geom)
    order = [(s, t) for s in range(c["B"]) for t in range(hf.T)]
    d = _batch(c)
    got, st = _packed(dev, d, c, order)
    d.close()
    _cmp(got, st, c["want"], c["wst"])
    rng = np.random.RandomState(3)
    other = [order[i] for i in rng.permutation(len(order))]
    d = _batch(c)
    got2, st2 = _packed(dev, d, c, other)
    d.close()
    assert np.array_equal(got2, got) and np.array_equal(st2, st)


# ---- slot padding -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,stride", [("48k_10_20B", 64), ("48k_hr_156B", 256)])
def test_slot_padding(dev, geom, stride):
    """a stride larger than the frames, the bytes behind each payload 0x00, 0xFF and random: identical PCM and status, from the fixed-size kernels (decode) and
    from the per-frame-size ones (decode_device_sizes; the stride keeps the parser family of the geometry)"""
    c = _case(geom)
    B, T, z = c["B"], hf.T, c["stride"]
    nb, fl = hf.as_flags(c["sizes"], c["bfi"], c["full"])
    rng = np.random.RandomState(11)
    outs = []
    for fill in (0x00, 0xFF, None):
        fr = rng.randint(0, 256, size=(B, T, stride)).astype(np.uint8) if fill is None else np.full((B, T, stride), fill, np.uint8)
        fr[:, :, :z] = c["frames"]
        d = _batch(c, [z] * B)
        outs.append(d.decode(fr, fl))
        d.close()
        d = _batch(c)
        outs.append(_device_calls(dev, d, fr, nb, fl, [0, T]))
        d.close()
    for got, st in outs:
        _cmp(got, st, c["want"], c["wst"])


# ---- ragged calls -----------------------------------------------------------------------------------------------------------------------------------------
def _ragged_counts(c):
    """counts [3, B]: a stream's first two calls end on a refused frame or on the frame before one, in turn; the burst stream's calls end at frames 10 and 13,
    so that the second and the third call start inside the burst"""
    B, T = c["B"], hf.T
    counts = np.zeros((3, B), np.int64)
    for s in range(B):
        refused = np.flatnonzero(c["kind"][s] == hf.R)
        if c["pats"][s] == "burst":
            ends = [10, hf.CUT]
        elif len(refused) == 0:
            ends = [7, 15]
        else:
            r1 = int(refused[refused >= 4][0])
            r2 = int(refused[refused >= r1 + 3][0])
            ends = [r1 + 1 - s % 2, r2 + s % 2]                   # (+1: the refused frame is the last present one)
        counts[:, s] = [ends[0], ends[1] - ends[0], T - ends[1]]
    return counts


def test_ragged_calls_end_on_refused_frames(dev):
    c = _case("48k_10_mixed")
    B, T, S, ch, N = c["B"], hf.T, c["stride"], c["ch"], c["N"]
    nb_all, fl_all = c["sizes"].astype(np.int32), c["bfi"]
    counts = _ragged_counts(c)
    last = np.cumsum(counts, axis=0)[:2] - 1
    for k in range(2):                                             # calls that end on a refused frame, and on the frame before one
        assert (c["kind"][np.arange(B), last[k]] == hf.R).sum() >= 2 and (c["kind"][np.arange(B), last[k] + 1] == hf.R).sum() >= 2
    d = _batch(c)
    d_cnt = dev.put(np.zeros(B, np.int32))
    d.set_frame_counts(d_cnt)
    got, gst = np.zeros((B, T, ch, N), np.int16), np.zeros((B, T), np.uint8)
    for k in range(3):
        pos, cnt = counts[:k].sum(axis=0), counts[k]
        NF = int(cnt.max())
        fr = np.full((B, NF, S), 0xA5, np.uint8)
        nb = np.where((np.arange(B)[:, None] + np.arange(NF)[None, :]) % 2 == 0, -7, 100000).astype(np.int32)     # absent entries: garbage
        fl = np.full((B, NF), 7, np.uint8)
        for s in range(B):
            p, n = int(pos[s]), int(cnt[s])
            fr[s, :n] = c["frames"][s, p:p + n]; nb[s, :n] = nb_all[s, p:p + n]; fl[s, :n] = fl_all[s, p:p + n]
        up = np.ascontiguousarray(cnt, np.int32)
        assert dev.hip.hipMemcpy(C.c_void_p(d_cnt), C.c_void_p(up.ctypes.data), C.c_size_t(up.nbytes), C.c_int(1)) == 0
        d_pcm, d_st = dev.put(np.full((B, NF, ch, N), SENT | SENT << 8, np.int16)), dev.put(np.full((B, NF), ST_SENT, np.uint8))
        d.decode_device_sizes(dev.put(fr), S, NF, d_pcm, dev.put(nb), dev.put(fl), d_st, sync=True)
        pcm, st = dev.get(d_pcm, (B, NF, ch, N), np.int16), dev.get(d_st, (B, NF), np.uint8)
        for s in range(B):
            p, n = int(pos[s]), int(cnt[s])
            assert (pcm[s, n:] == (SENT | SENT << 8)).all(), ("absent PCM written", k, s)
            assert (st[s, n:] == ABSENT).all(), ("absent status", k, s, st[s].tolist())
            got[s, p:p + n] = pcm[s, :n]; gst[s, p:p + n] = st[s, :n]
    d.set_frame_counts(None)
    _cmp(got, gst, c["want"], c["wst"])
    twin = _batch(c)
    tp, ts = _device_calls(dev, twin, c["frames"], nb_all, fl_all, [0, T])
    assert np.array_equal(tp, got) and np.array_equal(ts, gst)
    assert (d.get_state() == twin.get_state()).all() and [d.num_bytes(s) for s in range(B)] == [twin.num_bytes(s) for s in range(B)]
    d.close(); twin.close()


# ---- a refused frame is a lost frame ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ALL_GEOMS)
def test_a_refused_frame_is_a_lost_frame(geom):
    """One batch decodes the streams as they are, a second one with bfi set to the oracle's status: the same PCM and status, and the same again over four
    further genuine frames - the state a refusal leaves is the state a loss leaves.  The streams of hostile_frames.lost_equivalent: every mono stream that
    keeps its size, the stereo streams whose refusals are in channel 0."""
    c = _case(geom)
    rows, _ = hf.lost_equivalent(geom)
    fr, nb = c["frames"][rows], c["sizes"][rows].astype(np.int32)
    tail = hf.tail(geom)[rows]
    tnb = np.repeat(c["full"][rows, -1:], tail.shape[1], axis=1).astype(np.int32)
    more = hf.decode(geom, np.concatenate([fr, tail], axis=1), np.concatenate([nb, tnb], axis=1),
                     np.concatenate([c["bfi"][rows], np.zeros(tnb.shape, np.uint8)], axis=1))
    assert np.array_equal(more["pcm"][:, :hf.T], c["want"][rows]) and (more["status"][:, hf.T:] == 0).all()
    outs = []
    for flags in (c["bfi"][rows], c["wst"][rows]):
        d = _batch(c, B=len(rows))
        a, sa = d.decode(fr, flags, num_bytes=nb)
        b, sb = d.decode(tail, None, num_bytes=tnb)
        outs.append((np.concatenate([a, b], axis=1), np.concatenate([sa, sb], axis=1), d.get_state()))
        d.close()
    for got, st, _ in outs:
        _cmp(got, st, more["pcm"], more["status"])
    assert (outs[0][2] == outs[1][2]).all()


# ---- stage traces -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["48k_10_128B", "96k_2p5_hr_62B"])
def test_stage_traces_on_accepted_random_payloads(geom):
    """the field-by-field comparison of test_gpu_dec_parity.test_stage_traces_match_oracle, with the same skipped fields, on the 24 accepted random payloads of
    the all-H stream"""
    c = _case(geom)
    s = c["pats"].index("all_h")
    z = int(c["full"][s, 0])
    fr = c["frames"][s:s + 1]
    db = _batch(c, [z], B=1)
    got, status, traces = db.decode_traced(fr, None)
    o = OracleDecoder(c["fs"], 1, c["ms"], c["hr"], portable_math=True)
    tr = o.enable_trace()
    bad = []
    for t in range(hf.T):
        rc, want = o.decode(fr[0, t, :z])
        assert rc == 0 and (got[0, t] == want).all() and status[0, t] == 0, t
        g = DecTrace.from_buffer_copy(traces[t].tobytes()[:C.sizeof(DecTrace)])
        for f, _ in DecTrace._fields_:
            if f in ("bfi", "xq", "q_gain", "scf_q"):
                continue
            ga, ca = getattr(g, f), getattr(tr[0], f)
            if hasattr(ga, "__len__"):
                n = c["N"] if len(ga) == 960 else len(ga)
                a, b = np.ctypeslib.as_array(ga)[:n], np.ctypeslib.as_array(ca)[:n]
            else:
                a, b = np.asarray([ga]), np.asarray([ca])
            same = (a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0)) if a.dtype.kind == "f" else (a == b)
            if not same.all():
                bad.append((t, f, int((~same).sum())))
    assert not bad, bad[:10]
    db.close()


# ---- output depths ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bps", [24, 32])
@pytest.mark.parametrize("geom", ALL_GEOMS)
def test_output_depths(geom, bps):
    """on the streams whose wide output is defined (hostile_frames.depth_streams; test_hostile_frames_cpu.py asserts the bound and that every geometry has
    such streams at both depths)"""
    c = _case(geom)
    rows = hf.depth_streams(geom, bps)
    assert rows
    nb = c["sizes"][rows].astype(np.int32)
    want = hf.decode(geom, c["frames"], c["sizes"], c["bfi"], bps=bps, rows=rows)
    d = _batch(c, B=len(rows))
    got, st = d.decode(c["frames"][rows], c["bfi"][rows], bps, num_bytes=nb)
    _cmp(got, st, want["pcm"], want["status"])
    d.close()
