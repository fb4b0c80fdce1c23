"""RTP framing on the GPU (lc3plus_dec_batch_rtp_parse, lc3plus_enc_batch_rtp_stamp, lc3plus_dec_batch_rtp_stamp; the four kernels of liblc3plus_rtp_hip.so).
Every output is held to equality: the kernels against the host plans (api.plan_rtp_parse, api.plan_rtp_stamp, themselves held to the numpy rules in
test_rtp_cpu.py) on item counts that fill neither waves nor workgroups, with an SSRC table of one sender, of five, and of one more than LDS holds, with guard
elements behind every output and the whole wire buffer compared byte for byte; the chain encode_packed -> egress -> stamp -> parse -> probe -> ingest ->
set_frame_counts + decode_packed on one HIP stream with a single wait at the end, against the CPU oracle; statelessness; offsets past 4 GiB; and the sibling
library's own launch counts.  Device buffers through ctypes (test_gpu_dec_varsize_device._Hip)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import hostile_frames as hf
import rtp_ref as ref
from lc3_harness import sibling_launches, synth_pcm
from test_gpu_dec_varsize_device import _Hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "audio_codec_amd", "liblc3plus_rtp_hip.so")
GUARD = 16                                             # elements behind every output array
E2E_GEOMS = ("48k_10_128B", "48k_10_stereo_161B")      # the geometries of test_gpu_egress.py: one mono, one stereo
KERNELS = ["lc3_rtp_fill_kernel", "lc3_rtp_parse_kernel", "lc3_rtp_route_kernel", "lc3_rtp_stamp_kernel"]
SENTINEL = {np.int64: 0x5A5A5A5A5A5A5A5A, np.int32: 0x5A5A5A5A, np.uint8: 0x5A}
COUNTS = (1, 63, 64, 65, 257, 1000)
PARSE_TYPES = dict(stream=np.int32, seq=np.int32, offsets=np.int64, num_bytes=np.int32, timestamp=np.int32, marker=np.uint8, status=np.uint8, stats=np.int32)


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


def _launches(name):
    return sibling_launches("rtp", name)


def _dec(S, ch=1):
    return _amd().DecBatch(S, 48000, ch, 10.0, 0, None, device=0)


def _enc(S):
    return _amd().Batch(S, 48000, 1, 10.0, 0, [64000] * S, device=0)


def _outputs(dev, shapes, optional, always):
    """a device array per output, the sentinel in every element and GUARD elements behind; None for an optional output that is not asked for"""
    return {k: dev.put(np.full(n + GUARD, SENTINEL[dt], dt)) if k in always or k in optional else None for k, (n, dt) in shapes.items()}


def _collect(dev, ptr, shapes):
    out = {}
    for k, (n, dt) in shapes.items():
        if ptr[k] is None:
            out[k] = None
            continue
        got = dev.get(ptr[k], (n + GUARD,), dt)
        assert (got[n:] == SENTINEL[dt]).all(), ("an element behind the output was written", k)
        out[k] = got[:n]
    return out


def _same(got, want, name, keys=None):
    for k in keys or want:
        g, w = got[k], want[k]
        if w is None:
            assert g is None, (name, k)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (name, k, "first differences at", bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _plan_parse(c, optional=None):
    api = _amd().api
    return api.plan_rtp_parse(c["n_streams"], c["ring"], c["dg_offsets"], c["dg_sizes"], c["ssrc_key"], c["ssrc_stream"], c["payload_type"], c["payload_room"],
                              api.RTP_PARSE_OPTIONAL if optional is None else optional, c["ring_capacity"])


def _parse(dev, bat, c, d_ring, d_key, d_stream, optional=None, hip_stream=None, sync=True):
    """one parse call on decoder batch bat over the ring and the table already on the device -> dict as api.plan_rtp_parse gives"""
    api = _amd().api
    optional = api.RTP_PARSE_OPTIONAL if optional is None else optional
    n = len(c["dg_offsets"])
    shapes = {k: (api.RTP_STATS_WORDS if k == "stats" else n, dt) for k, dt in PARSE_TYPES.items()}
    ptr = _outputs(dev, shapes, optional, ref.PARSE_KEYS[:4])
    bat.rtp_parse_device(n, d_ring, c["ring_capacity"], dev.put(c["dg_offsets"]), dev.put(c["dg_sizes"]), len(c["ssrc_key"]), d_key, d_stream, ptr["stream"],
                         ptr["seq"], ptr["offsets"], ptr["num_bytes"], dev.put(c["payload_type"]) if c["payload_type"] is not None else None, c["payload_room"],
                         ptr["timestamp"], ptr["marker"], ptr["status"], ptr["stats"], hip_stream, sync=sync)
    if not sync:
        dev.stream_sync(hip_stream) if hip_stream else dev.sync()
    return _collect(dev, ptr, shapes)


def _table(dev, c):
    key = (np.asarray(c["ssrc_key"], np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return dev.put(key), dev.put(np.asarray(c["ssrc_stream"], np.int32))


@pytest.mark.parametrize("table", [5, 1, 4097])
@pytest.mark.parametrize("which", ["crafted0", "crafted2", "random"])
def test_parse_equals_the_host_plan(dev, which, table):
    """the crafted set (payload_room 0 and 2) and the random set of test_rtp_cpu.py at 1, 63, 64, 65, 257 and 1 000 items - the crafted set's 113 items repeated,
    the random set's 20 000 cut at changing places - over a table of 5 senders, of one, and of 4 097, one more than LDS holds, so that both searches run:
    every output and stats, the guards behind them, and the ring unchanged"""
    api = _amd().api
    assert table <= 4096 or table == 4097
    if which == "random":
        c = ref.random_set(table=table)
    else:
        c = dict(ref.crafted(int(which[-1]))[0])
        if table != 5:
            t = ref.random_set(table=table)
            c["ssrc_key"], c["ssrc_stream"] = t["ssrc_key"], t["ssrc_stream"]
    total = len(c["dg_offsets"])
    d = _dec(c["n_streams"])
    d_ring = dev.put(np.concatenate([c["ring"], np.zeros(8, np.uint8)]))
    d_key, d_stream = _table(dev, c)
    for k, n in enumerate(COUNTS):
        idx = (np.arange(n) + k * (which == "random")) % total
        part = ref.subset(c, idx)
        want = _plan_parse(part)
        assert want["stats"].sum() == n
        _same(_parse(dev, d, part, d_ring, d_key, d_stream), want, (which, table, n))
    part = ref.subset(c, np.arange(257) % total)                      # every optional output NULL (no fill kernel), on a second HIP stream, sync = 0
    got = _parse(dev, d, part, d_ring, d_key, d_stream, optional=(), hip_stream=dev.stream(), sync=False)
    assert all(got[k] is None for k in api.RTP_PARSE_OPTIONAL)
    _same(got, _plan_parse(part), (which, table, "optional outputs NULL"), ref.PARSE_KEYS[:4])
    assert np.array_equal(dev.get(d_ring, c["ring"].shape, np.uint8), c["ring"]), "the ring was written"
    d.close()


def _plan_stamp(c, optional):
    api = _amd().api
    return api.plan_rtp_stamp(c["pkt_route"], c["pkt_seq"], c["pkt_frame"], c["pkt_offset"], c["pkt_size"], c["ssrc"], c["ts_base"], c["payload_type"], c["ts_step"],
                              c["n_frames"], c["wire"], c["header_room"], c["payload_room"], c["pkt_flags"], c["n_packets"], c["marker_mode"], c["cell_status"],
                              c["resume"], c["route_stats"], c["wire_capacity"], optional)


def _u32(a):
    return (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _stamp(dev, bat, c, optional, hip_stream=None, sync=True):
    """one stamp call on batch bat (an encoder's or a decoder's) -> dict as api.plan_rtp_stamp gives; pkt_status whole, its tail behind n_packets the sentinel"""
    m, R = len(c["pkt_route"]), len(c["ssrc"])
    shapes = dict(pkt_status=(m, np.uint8), next_ts=(R, np.int32), next_resume=(R, np.uint8))
    ptr = _outputs(dev, shapes, optional, ())
    put = lambda a, dt: dev.put(np.ascontiguousarray(a, dtype=dt)) if a is not None else None
    d_wire = dev.put(c["wire"])
    bat.rtp_stamp_device(m, dev.put(np.array([c["n_packets"]], np.int64)), put(c["pkt_route"], np.int32), dev.put(_u32(c["pkt_seq"])), put(c["pkt_frame"], np.int32),
                         put(c["pkt_offset"], np.int64), put(c["pkt_size"], np.int32), R, c["n_frames"], dev.put(_u32(c["ssrc"])), dev.put(_u32(c["ts_base"])),
                         put(c["payload_type"], np.int32), c["ts_step"], d_wire, c["wire_capacity"], c["header_room"], c["payload_room"], put(c["pkt_flags"], np.uint8),
                         c["marker_mode"], put(c["cell_status"], np.uint8), put(c["resume"], np.uint8), put(c["route_stats"], np.int32), ptr["pkt_status"],
                         ptr["next_ts"], ptr["next_resume"], hip_stream, sync=sync)
    if not sync:
        dev.stream_sync(hip_stream) if hip_stream else dev.sync()
    out = _collect(dev, ptr, shapes)
    out["wire"] = dev.get(d_wire, c["wire"].shape, np.uint8)
    return out


STAMP_SHAPES = ((12, 0, 0, 0), (12, 0, 1, 1), (15, 3, 0, 2), (17, 2, 3, 3))      # header_room, payload_room, slack, shift


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_stamp_equals_the_host_plan(dev, n):
    """the packet lists of test_rtp_cpu.py at 1, 63, 64, 65 and 257 packets with three more entries behind *n_packets, on an encoder batch and on a decoder
    batch: the whole wire buffer byte for byte, the bytes at and past wire_capacity included, pkt_status with its tail untouched, next_ts and next_resume.
    Over the four shapes the header address takes each of the four alignments, so both store paths run"""
    api = _amd().api
    seen = set()
    for k, (hr, pr, slack, shift) in enumerate(STAMP_SHAPES):
        c = ref.stamp_case(n, 100 * n + k, hr, pr, marker_mode=k % 2 if k else 1, resume=k != 2, route_stats=k != 1, flags=k != 3, slack=slack, spare=3, shift=shift)
        optional = tuple(x for x in api.RTP_STAMP_OPTIONAL if x != "next_resume" or c["cell_status"] is not None)
        want = _plan_stamp(c, optional)
        bat = _enc(5) if k % 2 else _dec(5)
        got = _stamp(dev, bat, c, optional)
        stamped = want["pkt_status"][:n] == ref.STAMPED
        assert stamped.any() and (got["pkt_status"][n:] == SENTINEL[np.uint8]).all(), "entries behind *n_packets were written"
        want["pkt_status"][n:] = SENTINEL[np.uint8]
        _same(got, want, (n, k))
        assert (got["wire"][c["wire_capacity"]:] == ref.WIRE_FILL).all()
        seen |= set(((c["pkt_offset"][:n][stamped] + hr - pr - 12) % 4).tolist())
        bat.close()
    assert n < 63 or seen == {0, 1, 2, 3}
    c = ref.stamp_case(n, 7, spare=3)                                 # every optional input and output NULL (no route kernel), a second stream, sync = 0
    c.update(pkt_flags=None, cell_status=None, resume=None, route_stats=None, marker_mode=ref.MARKER_NEVER)
    bat = _enc(5)
    got = _stamp(dev, bat, c, (), hip_stream=dev.stream(), sync=False)
    assert all(got[k] is None for k in api.RTP_STAMP_OPTIONAL)
    _same(got, _plan_stamp(c, ()), (n, "optional NULL"), ("wire",))
    bat.close()


@pytest.mark.parametrize("geom", E2E_GEOMS)
def test_sender_to_receiver_without_a_host_wait(dev, geom):
    """set_frame_counts + encode_device_packed (frame-major, a capacity five frames and a few bytes short), egress into a wire buffer with header_room
    12 + payload_room, stamp, parse of the wire buffer with the list's offsets and sizes as the datagrams, probe, ingest with the probe's records,
    set_frame_counts + decode_device_packed from the wire buffer: all queued on one HIP stream with sync = 0 and one wait at the end.  The headers are the host
    plan's on the egress's list; the parsed items point at the oracle encoder's frames; PCM and status equal the oracle decoder's over those frames with
    exactly the frames that were not SENT lost; frames behind the ingest's count are absent"""
    from test_gpu_egress import _sender
    api = _amd().api
    fs, ms, hr, ch, _ = hf.GEOMS[geom]
    sc = _sender(geom)
    S, T, N, size = sc["S"], sc["T"], sc["N"], sc["size"]
    proom = 3 if ch == 1 else 0
    room, align = 12 + proom, 4
    present = int(np.clip(sc["counts"], 0, T).sum())
    cap = (present - 5) * size + 9
    buf = present * size + 64
    n = S * T
    wire_bytes = n * (room + size + align)
    enc = _amd().Batch(S, fs, ch, ms, hr, [sc["rate"]] * S, device=0)
    dec = _amd().DecBatch(S, fs, ch, ms, hr, None, device=0)
    i32, i64, u8 = (lambda k, v=-7: dev.put(np.full(k, v, np.int32))), (lambda k, v=-7: dev.put(np.full(k, v, np.int64))), (lambda k, v=0xEE: dev.put(np.full(k, v, np.uint8)))
    d_pcm_in, d_cnt, d_out = dev.put(sc["pcm"]), dev.put(sc["counts"]), u8(buf, 0xC3)
    d_off, d_tot, d_nb, d_fl = i64((S, T)), i64(1), i32((S, T)), u8((S, T))
    seq_base = (65530 + np.arange(S)).astype(np.int32)
    ssrc = 0x7FFFFFF0 + 7 * np.arange(S)                              # ascending as uint32, on both sides of 2^31
    ts_base = 0xFFFFF000 + 100000 * np.arange(S)
    d_base, d_ssrc, d_tsb, d_pt = dev.put(seq_base), dev.put(_u32(ssrc)), dev.put(_u32(ts_base)), dev.put(np.full(S, 96, np.int32))
    d_sid = dev.put(np.arange(S, dtype=np.int32))
    d_wire = u8(wire_bytes, ref.WIRE_FILL)
    p_route, p_seq, p_frame, p_off, p_size, p_flags = i32(n), i32(n), i32(n), i64(n, -1), i32(n, 0), u8(n)      # offset -1: the parse refuses what lies behind n_packets
    d_np, d_wt, d_next, d_stats, d_cs = i64(1), i64(1), i32(S), i32((S, 4)), u8((S, T))
    work = dev.put(np.zeros(api.egress_work_bytes(S, T) // 8 + 1, np.int64))
    d_pst, d_nts, d_nres = u8(n), i32(S), u8(S)
    i_stream, i_seq, i_off, i_nb, i_ts, i_m, i_st, i_stats = i32(n), i32(n), i64(n), i32(n), i32(n), u8(n), u8(n), i32(16)
    d_info = dev.put(np.zeros((n, ch, api.FRAME_INFO_WORDS), np.int32))
    d_oo, d_onb, d_ci, d_cnt2, d_nb2 = i64((S, T)), i32((S, T)), i32((S, T)), i32(S), i32(S)
    d_pcm, d_st = dev.put(np.full((S, T, ch, N), 0x5555, np.int16)), u8((S, T))
    dev.sync()
    s1 = dev.stream()
    enc.set_frame_counts(d_cnt)
    enc.encode_device_packed(d_pcm_in, 16, T, d_out, cap, api.PACK_FRAME_MAJOR, None, None, d_off, d_tot, d_nb, d_fl, s1, sync=False)
    enc.egress_device(T, d_out, buf, d_off, d_nb, size, S, d_base, p_route, p_seq, p_frame, p_off, p_size, d_np, work, d_fl, api.ENC_FL_PACK_CAP, d_cnt, None, 16,
                      api.PACK_FRAME_MAJOR, d_wire, wire_bytes, room, align, p_flags, d_wt, d_next, d_stats, d_cs, s1, sync=False)
    enc.rtp_stamp_device(n, d_np, p_route, p_seq, p_frame, p_off, p_size, S, T, d_ssrc, d_tsb, d_pt, N, d_wire, wire_bytes, room, proom, p_flags,
                         api.RTP_MARKER_AFTER_HOLE, d_cs, None, d_stats, d_pst, d_nts, d_nres, s1, sync=False)
    dec.rtp_parse_device(n, d_wire, wire_bytes, p_off, p_size, S, d_ssrc, d_sid, i_stream, i_seq, i_off, i_nb, d_pt, proom, i_ts, i_m, i_st, i_stats, s1, sync=False)
    dec.probe_device(d_wire, wire_bytes, i_off, i_nb, size, n, d_info, api.PROBE_FULL, s1, sync=False)
    dec.ingest_device(n, i_stream, i_seq, i_off, i_nb, d_base, T, d_oo, d_onb, d_ci, d_cnt2, 16, d_info, None, d_nb2, None, None, s1, sync=False)
    dec.set_frame_counts(d_cnt2)
    dec.decode_device_packed(d_wire, wire_bytes, d_oo, T, d_pcm, d_onb, size, None, d_st, 16, s1, sync=False)
    dev.stream_sync(s1)
    enc.set_frame_counts(None)
    # the egress's list, and the headers the host plan stamps on it
    k = int(dev.get(d_np, (1,), np.int64)[0])
    lst = {x: dev.get(p, (n,), dt) for x, p, dt in (("route", p_route, np.int32), ("seq", p_seq, np.int32), ("frame", p_frame, np.int32), ("off", p_off, np.int64),
                                                     ("size", p_size, np.int32), ("flags", p_flags, np.uint8))}
    cs, stats = dev.get(d_cs, (S, T), np.uint8), dev.get(d_stats, (S, 4), np.int32)
    sent = cs == api.EGR_SENT
    assert k == present - 5 == sent.sum() and not lst["flags"][:k].any()
    wire = dev.get(d_wire, (wire_bytes,), np.uint8)
    blank = wire.copy()
    for p in range(k):
        a = int(lst["off"][p]) + room - proom - 12
        blank[a:a + 12] = ref.WIRE_FILL
    want = api.plan_rtp_stamp(lst["route"], lst["seq"], lst["frame"], lst["off"], lst["size"], ssrc, ts_base, np.full(S, 96), N, T, blank, room, proom, lst["flags"], k,
                              api.RTP_MARKER_AFTER_HOLE, cs, None, stats)
    assert np.array_equal(wire, want["wire"]) and np.array_equal(dev.get(d_pst, (n,), np.uint8)[:k], want["pkt_status"][:k]) and (want["pkt_status"][:k] == 1).all()
    assert np.array_equal(dev.get(d_nts, (S,), np.int32), want["next_ts"]) and np.array_equal(dev.get(d_nres, (S,), np.uint8), want["next_resume"])
    assert np.array_equal(want["next_ts"], _u32(ts_base + np.clip(sc["counts"], 0, T) * N))
    for p in range(k):                                                # the payload_room bytes between header and frame were left alone
        a = int(lst["off"][p]) + room
        assert (wire[a - proom:a] == ref.WIRE_FILL).all() and np.array_equal(wire[a:a + size], sc["frames"][lst["route"][p], lst["frame"][p]]), p
    # the parse of the wire: the plan's, and the list's own routes, numbers and places
    got = dict(stream=dev.get(i_stream, (n,), np.int32), seq=dev.get(i_seq, (n,), np.int32), offsets=dev.get(i_off, (n,), np.int64), num_bytes=dev.get(i_nb, (n,), np.int32),
               timestamp=dev.get(i_ts, (n,), np.int32), marker=dev.get(i_m, (n,), np.uint8), status=dev.get(i_st, (n,), np.uint8), stats=dev.get(i_stats, (16,), np.int32))
    _same(got, api.plan_rtp_parse(S, wire, lst["off"], lst["size"], ssrc, np.arange(S), np.full(S, 96), proom), geom)
    assert (got["status"][:k] == 0).all() and (got["status"][k:] == api.RTP_RANGE).all() and (got["stream"][k:] == -1).all()
    assert np.array_equal(got["stream"][:k], lst["route"][:k]) and np.array_equal(got["seq"][:k], lst["seq"][:k])
    assert np.array_equal(got["offsets"][:k], lst["off"][:k] + room) and (got["num_bytes"][:k] == size).all()
    assert np.array_equal(got["timestamp"][:k], _u32(ts_base[lst["route"][:k]] + lst["frame"][:k] * N))
    tt, rr = lst["frame"][:k], lst["route"][:k]
    assert np.array_equal(got["marker"][:k], np.where(tt > 0, ~sent[rr, np.maximum(tt - 1, 0)], False).astype(np.uint8))
    # the receiver's tables and the decoder's output
    counts2 = dev.get(d_cnt2, (S,), np.int32)
    last = np.where(sent.any(axis=1), T - np.argmax(sent[:, ::-1], axis=1), 0)
    assert np.array_equal(counts2, last) and np.array_equal(dev.get(d_onb, (S, T), np.int32), np.where(sent, size, 0))
    pcm, st = dev.get(d_pcm, (S, T, ch, N), np.int16), dev.get(d_st, (S, T), np.uint8)
    o = hf.decode(geom, sc["frames"], np.where(sent, size, 0), np.zeros((S, T), np.uint8))
    for s in range(S):
        c = int(counts2[s])
        assert np.array_equal(st[s, :c], o["status"][s, :c]), (s, st[s].tolist())
        bad = np.argwhere((pcm[s, :c] != o["pcm"][s, :c]).any(axis=(1, 2)))
        assert len(bad) == 0, (s, "first differing frames", bad[:4].ravel().tolist())
        assert (st[s, c:] == api.DEC_ST_ABSENT).all() and (pcm[s, c:] == 0x5555).all(), s
    enc.close()
    dec.close()


def test_rtp_calls_are_stateless(dev):
    """an encoder batch and a decoder batch, each with state behind it: get_state() and the configuration are bit for bit what they were after parse and stamp
    calls - the host convenience calls and calls with sync = 0 on a second stream - every result is the plan's, and a later decode call gives what a twin
    batch gives that never saw them"""
    api = _amd().api
    S, T = 5, 12
    pc = ref.subset(ref.random_set(table=5), np.arange(300))
    pc = dict(pc, n_streams=S, payload_type=pc["payload_type"][:S])
    sc = ref.stamp_case(100, 3, 15, 3, spare=2)
    enc = _enc(S)
    pcm = synth_pcm(S, T, 480, 48000, seed=5)
    first = enc.encode(pcm)
    second = enc.encode(synth_pcm(S, T, 480, 48000, seed=6))
    dec, twin = (_amd().DecBatch(S, 48000, 1, 10.0, 0, [80] * S, device=0) for _ in range(2))
    dec.decode(first)
    twin.decode(first)
    want_parse, want_stamp = _plan_parse(pc), _plan_stamp(sc, api.RTP_STAMP_OPTIONAL)
    d_ring = dev.put(np.concatenate([pc["ring"], np.zeros(8, np.uint8)]))
    d_key, d_stream = _table(dev, pc)
    for bat in (enc, dec):
        before = (bat.get_state(), [bat.num_bytes(s) for s in range(S)])
        r = bat.rtp_stamp(sc["pkt_route"], sc["pkt_seq"], sc["pkt_frame"], sc["pkt_offset"], sc["pkt_size"], sc["ssrc"], sc["ts_base"], sc["payload_type"],
                          sc["ts_step"], sc["n_frames"], sc["wire"], sc["header_room"], sc["payload_room"], sc["pkt_flags"], sc["n_packets"], sc["marker_mode"],
                          sc["cell_status"], sc["resume"], sc["route_stats"], sc["wire_capacity"])
        _same(r, want_stamp, "rtp_stamp()")
        got = _stamp(dev, bat, sc, api.RTP_STAMP_OPTIONAL, hip_stream=dev.stream(), sync=False)
        got["pkt_status"][sc["n_packets"]:] = 0
        _same(got, want_stamp, "second stream")
        if bat is dec:
            r = bat.rtp_parse(pc["ring"], pc["dg_offsets"], pc["dg_sizes"], pc["ssrc_key"], pc["ssrc_stream"], pc["payload_type"], pc["payload_room"],
                              ring_capacity=pc["ring_capacity"])
            _same(r, want_parse, "rtp_parse()")
            _same(_parse(dev, bat, pc, d_ring, d_key, d_stream, hip_stream=dev.stream(), sync=False), want_parse, "second stream")
        after = (bat.get_state(), [bat.num_bytes(s) for s in range(S)])
        assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    a, b = dec.decode(second), twin.decode(second)
    for x, y in zip(a, b) if isinstance(a, tuple) else ((a, b),):
        assert np.array_equal(x, y)
    for x in (enc, dec, twin):
        x.close()


def test_offsets_past_4g(dev):
    """one arena of 4 GiB + 1 MiB serves as wire buffer and then as ring.  Packets and datagrams lie on both sides of byte 2^32 - one unaligned header is
    stamped across it, one datagram's header is read across it - and one ends at the capacity: results equal the plan's on a compact copy, and the windows a
    narrowed offset would write or read - the same offsets mod 2^32 - hold sentinels that stay and decoy datagrams that are not parsed.  The arena is
    allocated, not filled: only the windows looked at are written beforehand"""
    api = _amd().api
    hip = dev.hip
    G, arena = 2 ** 32, 2 ** 32 + 2 ** 20
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    assert free.value > arena + 2 ** 28, "the device has no room for an arena of 4 GiB + 1 MiB"
    base = C.c_void_p()
    assert hip.hipMalloc(C.byref(base), C.c_size_t(arena)) == 0
    dev.ptrs.append(base)

    def write(at, a):
        assert 0 <= at and at + a.size <= arena
        assert hip.hipMemcpy(C.c_void_p(base.value + at), C.c_void_p(a.ctypes.data), C.c_size_t(a.size), C.c_int(1)) == 0

    def read(at, k):
        out = np.zeros(k, np.uint8)
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(base.value + at), C.c_size_t(k), C.c_int(2)) == 0
        return out
    d = _dec(2)
    # ---- stamp: packets of 12 + 40 bytes; header_room 12, so the header lies at the packet's offset ----
    size, pad = 52, 32
    places = [5000, G - 6, G + 4096, G + 8193, arena - size]          # low; an unaligned header across 2^32; aligned above it; unaligned above it; at the capacity
    windows = sorted({a % G for a in places if a >= G} - set(places))
    assert windows == [4096, 8193, 2 ** 20 - size]
    fill = np.full(size + 2 * pad, ref.WIRE_FILL, np.uint8)
    for a in places[:-1] + windows:
        write(a - pad, fill)
    write(places[-1] - pad, fill[:pad + size])
    n = len(places)
    c = dict(pkt_route=np.array([0, 1, 0, 1, 1], np.int32), pkt_seq=np.array([65535, 0, 1, 2, 3]), pkt_frame=np.array([0, 1, 2, 0, 1], np.int32),
             pkt_offset=np.array(places, np.int64), pkt_size=np.full(n, size, np.int32), ssrc=np.array([0x80000001, 0x7FFFFFFF]), ts_base=np.array([0xFFFFFF00, 5]),
             payload_type=np.array([96, 97], np.int32), cell_status=np.array([[1, 2, 1], [2, 1, 1]], np.uint8), resume=np.array([1, 0], np.uint8))
    # the plan on a compact wire buffer: packet p at p * 128 + (its place mod 4)
    compact = np.array([p * 128 + a % 4 for p, a in enumerate(places)], np.int64)
    want = api.plan_rtp_stamp(c["pkt_route"], c["pkt_seq"], c["pkt_frame"], compact, c["pkt_size"], c["ssrc"], c["ts_base"], c["payload_type"], 480, 3,
                              np.full(n * 128, ref.WIRE_FILL, np.uint8), 12, 0, None, n, api.RTP_MARKER_AFTER_HOLE, c["cell_status"], c["resume"], None)
    assert (want["pkt_status"] == ref.STAMPED).all()
    d_status = dev.put(np.full(n + GUARD, SENTINEL[np.uint8], np.uint8))
    d.rtp_stamp_device(n, dev.put(np.array([n], np.int64)), dev.put(c["pkt_route"]), dev.put(_u32(c["pkt_seq"])), dev.put(c["pkt_frame"]), dev.put(c["pkt_offset"]),
                       dev.put(c["pkt_size"]), 2, 3, dev.put(_u32(c["ssrc"])), dev.put(_u32(c["ts_base"])), dev.put(c["payload_type"]), 480, base.value, arena, 12, 0, None,
                       api.RTP_MARKER_AFTER_HOLE, dev.put(c["cell_status"]), dev.put(c["resume"]), None, d_status, None, None, None, sync=True)
    st = dev.get(d_status, (n + GUARD,), np.uint8)
    assert (st[:n] == ref.STAMPED).all() and (st[n:] == SENTINEL[np.uint8]).all()
    for p, a in enumerate(places):
        tail = pad if p < n - 1 else 0
        got = read(a - pad, pad + size + tail)
        assert np.array_equal(got[pad:pad + 12], want["wire"][compact[p]:compact[p] + 12]), (p, a)
        assert (got[:pad] == ref.WIRE_FILL).all() and (got[pad + 12:] == ref.WIRE_FILL).all(), (p, a)
    for a in windows:
        assert (read(a - pad, size + 2 * pad) == ref.WIRE_FILL).all(), a
    # ---- parse: datagrams of 61 bytes with CSRCs, an extension and padding, so that bytes all along them are read ----
    def dgram(seq, ssrc):
        return np.frombuffer(ref.datagram(seq=seq, ts=seq * 1000, ssrc=ssrc, marker=seq & 1, csrc=(1, 2, 3), ext=(7, bytes(8)), pad=5, payload=bytes(range(20))), np.uint8)
    z = dgram(0, 0).size
    places = [1000, G - 5, G + 20011, arena - z]                      # low; the fixed header across 2^32; above it; at the capacity
    decoys = [a % G for a in places if a >= G]
    assert decoys == [20011, 2 ** 20 - z]
    for k, a in enumerate(decoys):
        write(a, dgram(100 + k, 0x80000001))                          # a valid datagram of a known sender, another number
    m = len(places)
    ring = np.zeros(m * 128, np.uint8)                                # the compact copy: datagram p at p * 128 + (its place mod 4)
    compact = np.array([p * 128 + a % 4 for p, a in enumerate(places)], np.int64)
    for p, a in enumerate(places):
        ring[compact[p]:compact[p] + z] = dgram(10 + p, (0x80000001, 0x7FFFFFFF, 0x12345678)[p % 3])
        write(a, ring[compact[p]:compact[p] + z])
    key, strm = np.array([0x7FFFFFFF, 0x80000001]), np.array([1, 0], np.int32)
    sizes = np.full(m, z, np.int32)
    want = api.plan_rtp_parse(2, ring, compact, sizes, key, strm, None, 2, ring_capacity=ring.size)
    assert want["status"].tolist() == [0, 0, ref.UNKNOWN_SSRC, 0] and want["stream"].tolist() == [0, 1, -1, 0]
    shapes = {k: (api.RTP_STATS_WORDS if k == "stats" else m, dt) for k, dt in PARSE_TYPES.items()}
    ptr = _outputs(dev, shapes, api.RTP_PARSE_OPTIONAL, ref.PARSE_KEYS[:4])
    d.rtp_parse_device(m, base.value, arena, dev.put(np.array(places, np.int64)), dev.put(sizes), 2, dev.put(_u32(key)), dev.put(strm), ptr["stream"], ptr["seq"],
                       ptr["offsets"], ptr["num_bytes"], None, 2, ptr["timestamp"], ptr["marker"], ptr["status"], ptr["stats"], None, sync=True)
    got = _collect(dev, ptr, shapes)
    _same(got, want, "past 4 GiB", ("stream", "seq", "num_bytes", "timestamp", "marker", "status", "stats"))
    ok = want["status"] == 0
    assert np.array_equal(got["offsets"], np.where(ok, want["offsets"] + np.array(places, np.int64) - compact, 0)), got["offsets"].tolist()
    assert got["offsets"][3] == arena - z + 12 + 12 + 12 + 2 > G
    for k, a in enumerate(decoys):                                    # reading leaves the decoys what they are
        assert np.array_equal(read(a, z), dgram(100 + k, 0x80000001))
    d.close()


def test_every_rtp_kernel_ran_under_a_comparison(dev):
    """the sibling library counts its launches: every kernel its code object holds (tools/kernel_resources.py) has run - here, once more, under a comparison, so
    that the test stands alone - and a name it does not hold is answered with -1"""
    api = _amd().api
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels
    names = sorted(kernels(LIB, "gfx950"))
    assert names == KERNELS
    before = {k: _launches(k) for k in names}
    c = ref.subset(ref.random_set(table=5), np.arange(65))
    d = _dec(c["n_streams"])
    d_key, d_stream = _table(dev, c)
    _same(_parse(dev, d, c, dev.put(np.concatenate([c["ring"], np.zeros(8, np.uint8)])), d_key, d_stream), _plan_parse(c), "parse")
    sc = ref.stamp_case(65, 1, spare=1)
    got = _stamp(dev, d, sc, api.RTP_STAMP_OPTIONAL)
    got["pkt_status"][65:] = 0
    _same(got, _plan_stamp(sc, api.RTP_STAMP_OPTIONAL), "stamp")
    d.close()
    for k in names:
        assert _launches(k) == before[k] + 1, k
    assert _launches("lc3_egress_copy_kernel") == -1 and _launches("lc3_encode_kernel") == -1
