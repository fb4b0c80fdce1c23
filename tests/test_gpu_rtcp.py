"""Reception reports on the GPU (lc3plus_dec_batch_rtcp_stats; the six kernels of liblc3plus_rtcp_hip.so).  Every output array is held to equality with the plain
Python restatement of the rule (rtcp_ref.stats, itself held to hand-worked values in test_rtcp_cpu.py), with guard elements behind every output: one item; one
stream of 1, 63, 64, 65 and 129 items and of one item more than each tier of the walk's sort holds (64 in registers, 1 024 in LDS, more placed in order in
global memory); 1, 2, 65 and 4 097 streams with streams that receive nothing; items of no stream scattered through; the sequence patterns, transits and crafted
states of rtcp_ref; make_report 0 and 1, lsr and dlsr NULL, each optional output NULL; state_in == state_out; two calls with the state carried; the chain
rtp_parse_device -> rtcp_stats_device on one HIP stream with a single wait; statelessness and the sibling library's own launch counts; a workspace one byte
short.  Device buffers through ctypes (test_gpu_dec_varsize_device._Hip)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import rtcp_ref as ref
import rtp_ref
from lc3_harness import sibling_launches
from test_gpu_dec_varsize_device import _Hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "audio_codec_amd", "liblc3plus_rtcp_hip.so")
GUARD = 16                                             # elements behind every output array
KERNELS = ["lc3_rtcp_count_kernel", "lc3_rtcp_fill_kernel", "lc3_rtcp_place_kernel", "lc3_rtcp_scan_kernel", "lc3_rtcp_scatter_kernel", "lc3_rtcp_walk_kernel"]
SENTINEL = {np.int32: 0x5A5A5A5A, np.uint8: 0x5A}
WAVE_ITEMS, LDS_ITEMS = 64, 1024                       # the tiers of the walk's sort


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


@pytest.fixture(scope="module")
def bat():
    d = _amd().DecBatch(3, 48000, 1, 10.0, 0, None, device=0)
    yield d
    d.close()


def _launches(name):
    return sibling_launches("rtcp", name)


def _u32(a):
    return (np.asarray(a).astype(np.int64).reshape(-1) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _same(got, want, name, keys=None):
    for k in keys or want:
        g, w = got[k], want[k]
        if w is None:
            assert g is None, (name, k)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (name, k, "first differences at", bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _shapes(n, S):
    return dict(state=((S, ref.STATE_WORDS), np.int32), blocks=((S, ref.BLOCK_BYTES), np.uint8), ext_seq=((n,), np.int32), item_status=((n,), np.uint8),
                stream_stats=((S, ref.STATS_WORDS), np.int32))


def _stats(dev, bat, c, make_report=True, optional=None, in_place=False, hip_stream=None, sync=True, shift=0, d_items=None, work_shift=0):
    """one stats call over case c -> dict as rtcp_ref.stats gives, the guards behind every output checked.  in_place: state_in is state_out; shift: blocks start
    that many bytes behind a 4-aligned address; d_items: (stream, seq, timestamp) already on the device"""
    api = _amd().api
    optional = api.RR_OPTIONAL if optional is None else optional
    n, S = len(c["stream"]), np.asarray(c["state"]).reshape(-1, ref.STATE_WORDS).shape[0]
    shapes = _shapes(n, S)
    want = [k for k in ref.KEYS if k == "state" or (k == "blocks" and make_report) or k in optional]
    ptr, size = {}, {}
    for k, (shape, dt) in shapes.items():
        size[k] = int(np.prod(shape))
        ptr[k] = dev.put(np.full(shift * (k == "blocks") + size[k] + GUARD, SENTINEL[dt], dt)) if k in want else None
    state = _u32(c["state"])
    if in_place:
        assert dev.hip.hipMemcpy(C.c_void_p(ptr["state"]), C.c_void_p(state.ctypes.data), C.c_size_t(state.nbytes), C.c_int(1)) == 0
    d_in = ptr["state"] if in_place else dev.put(state)
    d_stream, d_seq, d_ts = d_items if d_items else (dev.put(np.asarray(c["stream"], np.int32)), dev.put(_u32(c["seq"])), dev.put(_u32(c["timestamp"])))
    wb = api.rtcp_workspace_bytes(n, S)
    d_work = dev.put(np.full(wb + work_shift + GUARD, 0x5A, np.uint8))
    opt = lambda k: dev.put(_u32(c[k])) if c.get(k) is not None else None
    bat.rtcp_stats_device(n, d_stream, d_seq, d_ts, dev.put(_u32(c["arrival"])), S, d_in, ptr["state"], d_work + work_shift, wb, make_report,
                          dev.put(_u32(c["ssrc"])) if make_report else None, opt("lsr"), opt("dlsr"), ptr["blocks"] + shift if ptr["blocks"] else None,
                          ptr["ext_seq"], ptr["item_status"], ptr["stream_stats"], hip_stream, sync=sync)
    if not sync:
        dev.stream_sync(hip_stream) if hip_stream else dev.sync()
    out = {}
    for k, (shape, dt) in shapes.items():
        if ptr[k] is None:
            out[k] = None
            continue
        lead = shift * (k == "blocks")
        got = dev.get(ptr[k], (lead + size[k] + GUARD,), dt)
        assert (got[:lead] == SENTINEL[dt]).all() and (got[lead + size[k]:] == SENTINEL[dt]).all(), ("an element outside the output was written", k)
        out[k] = got[lead:lead + size[k]].reshape(shape)
    assert (dev.get(d_work + work_shift + wb, (GUARD,), np.uint8) == 0x5A).all(), "a byte behind the workspace was written"
    return out


def _mixed():
    """streams of every tier in one list: 5, 70, 1 100 and 2 100 items and one stream that receives nothing, with items of no stream scattered through"""
    rng = np.random.RandomState(5)
    lens = [5, 70, 0, 1100, 2100]
    stream = np.concatenate([np.full(k, s) for s, k in enumerate(lens)] + [np.array([-1, 5, 9, -3] * 10)])
    rng.shuffle(stream)
    n = stream.size
    seq = np.zeros(n, np.int64)
    for s, k in enumerate(lens):
        q = 65000 + np.cumsum(rng.choice([1, 1, 1, 2, 0], size=k))
        for j in np.flatnonzero(rng.rand(max(k - 1, 0)) < 0.05):
            q[j], q[j + 1] = q[j + 1], q[j]
        seq[stream == s] = q
    ts = 480 * seq + 1000 * stream
    return ref.case(stream, seq, ts, ts + 777 + rng.randint(-300, 300, size=n), len(lens))


def _sets():
    out = {"one_item": ref.case([0], [7], [100], [350]), "patterns": ref.patterns()[0], "transits": ref.transits(), "crafted_states": ref.crafted_states()[0],
           "all_dropped": ref.case([-1, 5, 2], [1, 2, 3], [0, 0, 0], [0, 0, 0], 2), "mixed_tiers": _mixed()}
    for n in (1, 63, 64, 65, 129, WAVE_ITEMS + 1, LDS_ITEMS, LDS_ITEMS + 1, 2 * LDS_ITEMS + 1):
        out["one_stream_%d" % n] = ref.one_stream(n, seed=n)
    out["streams_1"] = ref.traffic(21, 1, 40)
    out["streams_2_one_silent"] = ref.traffic(22, 2, 40, silent=(0,))
    out["streams_65"] = ref.traffic(23, 65, 12, silent=(0, 33, 64))
    out["streams_4097"] = ref.traffic(24, 4097, 3, silent=(0, 1, 1023, 1024, 4096) + tuple(range(2000, 2100)), bad_items=0.05)
    out["one_of_300"] = ref.one_stream(200, seed=9, n_streams=300, stream=299)
    return out


SETS = _sets()
WANT = {}


def _want(name, make_report=True):
    """a set's reference, computed once"""
    if (name, make_report) not in WANT:
        WANT[name, make_report] = ref.stats(SETS[name], make_report)
    return WANT[name, make_report]


@pytest.mark.parametrize("name", list(SETS))
def test_stats_equal_the_rule(dev, bat, name):
    """every output with make_report 1, then make_report 0 (blocks NULL), every optional output NULL with lsr and dlsr NULL"""
    c = SETS[name]
    _same(_stats(dev, bat, c), _want(name), name)
    got = _stats(dev, bat, c, make_report=False)
    assert got["blocks"] is None
    _same(got, _want(name, False), (name, "no report"))
    bare = dict(c, lsr=None, dlsr=None)
    got = _stats(dev, bat, bare, optional=())
    assert all(got[k] is None for k in _amd().api.RR_OPTIONAL)
    _same(got, ref.stats(bare), (name, "bare"), ("state", "blocks"))


def test_sets_reach_what_they_are_for():
    api = _amd().api
    assert set(_want("patterns")["item_status"].tolist()) == {api.RR_COUNTED, api.RR_JUMP, api.RR_RESTART, api.RR_REORDERED}
    assert set(_want("mixed_tiers")["item_status"].tolist()) >= {api.RR_DROPPED, api.RR_COUNTED, api.RR_REORDERED}
    counts = np.bincount(SETS["mixed_tiers"]["stream"][(SETS["mixed_tiers"]["stream"] >= 0) & (SETS["mixed_tiers"]["stream"] < 5)], minlength=5)
    assert counts[0] <= WAVE_ITEMS < counts[1] <= LDS_ITEMS < counts[3] and counts[2] == 0 and counts[4] > 2 * LDS_ITEMS
    w = _want("streams_4097")
    assert not w["state"][[0, 1, 1023, 1024, 4096, 2050]].any() and w["state"][4095].any() and (w["item_status"] == 0).sum() > 100
    f = ref.block_fields(_want("crafted_states")["blocks"][3])
    assert f["fraction"] == 255


@pytest.mark.parametrize("name", ["patterns", "mixed_tiers", "streams_65"])
def test_in_place_and_unaligned(dev, bat, name):
    """state_in == state_out; blocks at every misalignment (byte stores); a workspace at an odd address"""
    c = SETS[name]
    _same(_stats(dev, bat, c, in_place=True), _want(name), (name, "in place"))
    for shift in (1, 2, 3):
        _same(_stats(dev, bat, c, shift=shift, work_shift=shift, optional=()), _want(name), (name, shift), ("state", "blocks"))


@pytest.mark.parametrize("name,cut", [("patterns", 17), ("mixed_tiers", 1500), ("streams_65", 300), ("one_stream_1025", 1024), ("crafted_states", 1)])
def test_two_calls_equal_one(dev, bat, name, cut):
    """the set cut in two, the state carried on the device and in place, a report only in the second call"""
    c = SETS[name]
    a, b = ref.split(c, cut)
    first = _stats(dev, bat, a, make_report=False)
    second = _stats(dev, bat, dict(b, state=first["state"]), in_place=True)
    want = _want(name)
    _same(second, want, name, ("state", "blocks"))
    assert np.array_equal(np.concatenate([first["ext_seq"], second["ext_seq"]]), want["ext_seq"])
    assert np.array_equal(np.concatenate([first["item_status"], second["item_status"]]), want["item_status"])
    assert np.array_equal(first["stream_stats"] + second["stream_stats"], want["stream_stats"])


def test_host_convenience_call(bat):
    c = SETS["streams_65"]
    got = bat.rtcp_stats(c["stream"], c["seq"], c["timestamp"], c["arrival"], c["state"], True, c["ssrc"], c["lsr"], c["dlsr"])
    _same(got, _want("streams_65"), "rtcp_stats()")
    got = bat.rtcp_stats(c["stream"], c["seq"], c["timestamp"], c["arrival"], c["state"])
    _same(got, _want("streams_65", False), "rtcp_stats() without a report")


def test_parse_then_stats_on_one_stream(dev, bat):
    """datagrams -> rtp_parse_device -> rtcp_stats_device on one HIP stream, both with sync = 0: the stats call reads the parse's stream, seq and timestamp where
    the parse wrote them; one wait at the end; against the rule over the host plan's arrays"""
    api = _amd().api
    pc = rtp_ref.subset(rtp_ref.random_set(table=5), np.arange(3000))
    n, S = 3000, 3                                    # the batch's three streams: senders of streams 3 and 9 are unknown to it
    rng = np.random.RandomState(3)
    arrival = rng.randint(0, 2 ** 32, size=n, dtype=np.int64)
    plan = api.plan_rtp_parse(S, pc["ring"], pc["dg_offsets"], pc["dg_sizes"], pc["ssrc_key"], pc["ssrc_stream"], None, 0, ring_capacity=pc["ring_capacity"])
    assert (plan["stream"] >= 0).sum() > 100 and (plan["stream"] < 0).sum() > 100
    c = ref.case(plan["stream"], plan["seq"], plan["timestamp"], arrival, S)
    want = ref.stats(c)
    hs = dev.stream()
    d_stream, d_seq, d_ts = (dev.put(np.full(n, 0x5A5A5A5A, np.int32)) for _ in range(3))
    key = (np.asarray(pc["ssrc_key"], np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    bat.rtp_parse_device(n, dev.put(np.concatenate([pc["ring"], np.zeros(8, np.uint8)])), pc["ring_capacity"], dev.put(pc["dg_offsets"]), dev.put(pc["dg_sizes"]),
                         len(key), dev.put(key), dev.put(np.asarray(pc["ssrc_stream"], np.int32)), d_stream, d_seq, dev.put(np.zeros(n, np.int64)),
                         dev.put(np.zeros(n, np.int32)), None, 0, d_ts, None, None, None, hs, sync=False)
    got = _stats(dev, bat, c, hip_stream=hs, sync=False, d_items=(d_stream, d_seq, d_ts))
    _same(got, want, "parse -> stats")
    assert np.array_equal(dev.get(d_stream, (n,), np.int32), plan["stream"]) and np.array_equal(dev.get(d_ts, (n,), np.int32), plan["timestamp"])


def test_stateless_and_launch_counts(dev):
    """a decoder batch with state behind it: get_state() and the configuration are bit for bit what they were after stats calls, a later decode gives what a
    twin batch gives that never saw them, and every kernel's launch count moves by what DESIGN 10j states: one launch each per call, the place kernel only in
    a call of more than 1 024 items"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels
    from lc3_harness import synth_pcm
    assert sorted(kernels(LIB, "gfx950")) == KERNELS
    S, T = 3, 6
    enc = _amd().Batch(S, 48000, 1, 10.0, 0, [64000] * S, device=0)
    first, second = enc.encode(synth_pcm(S, T, 480, 48000, seed=5)), enc.encode(synth_pcm(S, T, 480, 48000, seed=6))
    dec, twin = (_amd().DecBatch(S, 48000, 1, 10.0, 0, [80] * S, device=0) for _ in range(2))
    dec.decode(first)
    twin.decode(first)
    before = (dec.get_state(), [dec.num_bytes(s) for s in range(S)])
    for name, place in (("patterns", 0), ("one_stream_1024", 0), ("one_stream_1025", 1), ("streams_65", 0), ("mixed_tiers", 1)):
        count = {k: _launches(k) for k in KERNELS}
        _same(_stats(dev, dec, SETS[name], hip_stream=dev.stream(), sync=False), _want(name), name)
        for k in KERNELS:
            assert _launches(k) == count[k] + (place if k == "lc3_rtcp_place_kernel" else 1), (name, k)
    after = (dec.get_state(), [dec.num_bytes(s) for s in range(S)])
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    a, b = dec.decode(second), twin.decode(second)
    for x, y in zip(a, b) if isinstance(a, tuple) else ((a, b),):
        assert np.array_equal(x, y)
    assert _launches("lc3_rtp_parse_kernel") == -1 and _launches("lc3_encode_kernel") == -1
    for x in (enc, dec, twin):
        x.close()


def test_short_workspace_is_refused(dev, bat):
    """a workspace one byte short: LC3Error, and no array is written"""
    api = _amd().api
    c = SETS["streams_65"]
    n, S = len(c["stream"]), 65
    wb = api.rtcp_workspace_bytes(n, S)
    outs = {k: dev.put(np.full(int(np.prod(shape)), SENTINEL[dt], dt)) for k, (shape, dt) in _shapes(n, S).items()}
    d_work = dev.put(np.full(wb, 0x5A, np.uint8))
    args = (n, dev.put(np.asarray(c["stream"], np.int32)), dev.put(_u32(c["seq"])), dev.put(_u32(c["timestamp"])), dev.put(_u32(c["arrival"])), S,
            dev.put(_u32(c["state"])), outs["state"], d_work)
    rest = (True, dev.put(_u32(c["ssrc"])), None, None, outs["blocks"], outs["ext_seq"], outs["item_status"], outs["stream_stats"])
    for short in (wb - 1, 0):
        with pytest.raises(api.LC3Error):
            bat.rtcp_stats_device(*args, short, *rest, sync=True)
    dev.sync()
    for k, (shape, dt) in _shapes(n, S).items():
        assert (dev.get(outs[k], shape, dt) == SENTINEL[dt]).all(), k
    assert (dev.get(d_work, (wb,), np.uint8) == 0x5A).all()
    bat.rtcp_stats_device(*args, wb, *rest, sync=True)                # the same call with the whole workspace runs
    assert np.array_equal(dev.get(outs["blocks"], (S, ref.BLOCK_BYTES), np.uint8), ref.stats(dict(c, lsr=None, dlsr=None))["blocks"])
