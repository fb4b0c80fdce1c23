"""Redundant audio on the GPU (lc3plus_enc_batch_red_pack, lc3plus_dec_batch_red_pack, lc3plus_dec_batch_red_unpack; the eight kernels of
liblc3plus_red_hip.so).  Every output is held to equality: the kernels against the host plans (api.plan_red_pack, api.plan_red_unpack, themselves held to the
restatement of the rules in test_red_cpu.py) with guard elements behind every output, the whole wire buffer and both tail buffers compared byte for byte, over
three consecutive calls through the tails and packet counts on both sides of the scan's wave and tile edges; the chain encode_packed -> egress -> red_pack ->
stamp -> (a dropped burst) -> parse -> red_unpack -> probe -> ingest -> set_frame_counts + decode_packed on one HIP stream with a single wait at the end, against
the CPU oracle's decode of the loss-free frames; statelessness; and the sibling library's own launch counts.  Device buffers through ctypes
(test_gpu_dec_varsize_device._Hip)."""
import os
import sys

import numpy as np
import pytest

import hostile_frames as hf
import red_ref as ref
from lc3_harness import sibling_launches, synth_pcm
from test_gpu_dec_varsize_device import _Hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "audio_codec_amd", "liblc3plus_red_hip.so")
GUARD = 16                                             # elements behind every output array
KERNELS = ["lc3_red_base_kernel", "lc3_red_copy_kernel", "lc3_red_fill_kernel", "lc3_red_scatter_kernel", "lc3_red_size_kernel", "lc3_red_sums_kernel",
           "lc3_red_tail_kernel", "lc3_red_unpack_kernel"]
SENTINEL = {np.int64: 0x5A5A5A5A5A5A5A5A, np.int32: 0x5A5A5A5A, np.uint8: 0x5A}
PACK_TYPES = dict(red_offset=np.int64, red_size=np.int32, red_flags=np.uint8, red_blocks=np.uint8, wire_total=np.int64, route_stats=np.int32)
UNPACK_TYPES = dict(stream=np.int32, seq=np.int32, offsets=np.int64, num_bytes=np.int32, timestamp=np.int32, gen=np.uint8, status=np.uint8, stats=np.int32)
COUNTS = (1, 63, 64, 65, 257, 1000)


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


def _launches(name):
    return sibling_launches("red", name)


def _dec(S):
    return _amd().DecBatch(S, 48000, 1, 10.0, 0, None, device=0)


def _enc(S):
    return _amd().Batch(S, 48000, 1, 10.0, 0, [64000] * S, device=0)


def _u32(a):
    return (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


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


def _plan_pack(c, optional=None):
    api = _amd().api
    return api.plan_red_pack(c["n_streams"], c["frames"], c["offsets"], c["num_bytes"], c["max_frame_bytes"], c["pkt_route"], c["pkt_frame"], c["block_pt"], c["ts_step"],
                             c["wire"], c["max_depth"], c["depth"], c["max_packet_bytes"], c["n_packets"], c["flags"], c["skip_mask"], c["counts"], c["route_src"],
                             c["tail_bytes"], c["tail_sizes"], c["tail_stride"], c["wire_capacity"], c["header_room"], c["align"],
                             api.RED_PACK_OPTIONAL if optional is None else optional, c["frames_capacity"])


def _want_pack(c, optional=None):
    """the host plan's outputs as the device arrays must come out: entries behind n_packets and tail bytes behind an entry's size keep their fill"""
    want = _plan_pack(c, optional)
    n = c["n_packets"]
    for k in ("red_offset", "red_size", "red_flags", "red_blocks"):
        if want[k] is not None:
            want[k][n:] = SENTINEL[PACK_TYPES[k]]
    if want["tail_sizes"] is not None:
        tb = np.full_like(want["tail_bytes"], ref.TAIL_FILL)
        for s, g in np.ndindex(*want["tail_sizes"].shape):
            z = int(want["tail_sizes"][s, g])
            tb[s, g, :z] = want["tail_bytes"][s, g, :z]
        want["tail_bytes"] = tb
    if want["wire_total"] is not None:
        want["wire_total"] = np.array([want["wire_total"]], np.int64)
    return want


def _pack(dev, bat, c, d_tails_in=None, optional=None, hip_stream=None, sync=True):
    """one pack call on batch bat (an encoder's or a decoder's) -> dict as _want_pack gives, and the device pointers of the tails it wrote"""
    api = _amd().api
    optional = api.RED_PACK_OPTIONAL if optional is None else optional
    m, R, S, D = len(c["pkt_route"]), len(c["block_pt"]), c["n_streams"], c["max_depth"]
    shapes = {k: ({"wire_total": 1, "route_stats": R * api.RED_STATS_WORDS}.get(k, m), dt) for k, dt in PACK_TYPES.items()}
    ptr = _outputs(dev, shapes, optional, ("red_offset", "red_size"))
    put = lambda a, dt: dev.put(np.ascontiguousarray(a, dtype=dt)) if a is not None else None
    tail = "tail" in optional
    d_tb = dev.put(np.full(S * D * c["tail_stride"] + GUARD, ref.TAIL_FILL, np.uint8)) if tail else None
    d_tz = dev.put(np.full(S * D + GUARD, SENTINEL[np.int32], np.int32)) if tail else None
    if d_tails_in is None and c["tail_sizes"] is not None:
        d_tails_in = (dev.put(c["tail_bytes"]), dev.put(c["tail_sizes"]))
    d_in = d_tails_in if c["tail_sizes"] is not None else (None, None)
    d_wire = dev.put(np.concatenate([c["wire"], np.zeros(8, np.uint8)]))
    d_frames = dev.put(np.concatenate([c["frames"], np.zeros(8, np.uint8)]))
    work_bytes = api.red_work_bytes(m)
    d_work = dev.put(np.full(work_bytes // 8 + GUARD, SENTINEL[np.int64], np.int64))
    bat.red_pack_device(c["offsets"].shape[1], d_frames, c["frames_capacity"], put(c["offsets"], np.int64), put(c["num_bytes"], np.int32), c["max_frame_bytes"], R, m,
                        dev.put(np.array([c["n_packets"]], np.int64)), put(c["pkt_route"], np.int32), put(c["pkt_frame"], np.int32), D, put(c["block_pt"], np.int32),
                        c["ts_step"], c["max_packet_bytes"], d_wire, c["wire_capacity"], ptr["red_offset"], ptr["red_size"], d_work, c["header_room"], c["align"],
                        put(c["flags"], np.uint8), c["skip_mask"], put(c["counts"], np.int32), put(c["route_src"], np.int32), put(c["depth"], np.int32), d_in[0], d_in[1],
                        c["tail_stride"], d_tb, d_tz, ptr["red_flags"], ptr["red_blocks"], ptr["wire_total"], ptr["route_stats"], hip_stream, sync=sync)
    if not sync:
        dev.stream_sync(hip_stream) if hip_stream else dev.sync()
    out = _collect(dev, ptr, shapes)
    if out["route_stats"] is not None:
        out["route_stats"] = out["route_stats"].reshape(R, api.RED_STATS_WORDS)
    assert (dev.get(d_work, (work_bytes // 8 + GUARD,), np.int64)[work_bytes // 8:] == SENTINEL[np.int64]).all(), "the workspace was overrun"
    out["wire"] = dev.get(d_wire, c["wire"].shape, np.uint8)
    assert np.array_equal(dev.get(d_frames, c["frames"].shape, np.uint8), c["frames"]), "the frames were written"
    out["tail_bytes"] = out["tail_sizes"] = None
    if tail:
        tb, tz = dev.get(d_tb, (S * D * c["tail_stride"] + GUARD,), np.uint8), dev.get(d_tz, (S * D + GUARD,), np.int32)
        assert (tb[-GUARD:] == ref.TAIL_FILL).all() and (tz[-GUARD:] == SENTINEL[np.int32]).all(), "an element behind the tails was written"
        out["tail_bytes"], out["tail_sizes"] = tb[:-GUARD].reshape(S, D, c["tail_stride"]), tz[:-GUARD].reshape(S, D)
    return out, (d_tb, d_tz)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_pack_equals_the_host_plan(dev, n):
    """the tables of red_ref.pack_tables - 3 streams, 5 routes with fan-out and a bad route, depth 0 ... 4 per route and values the call clamps, 7 frames of 1, 20,
    1023 and 1024 bytes at every source residue, LOST, INVALID and SKIPPED frames, counts 0, 2, 3 and 7, a max_packet_bytes that cuts generations, a wire
    capacity the last packets overflow, BAD list entries - through three consecutive calls, each call reading the tails the call before wrote on the device, on
    an encoder batch and a decoder batch in turn, at 1, 63, 64, 65, 257 and 1 025 packets (one more than a tile of the scan) with three more entries behind
    *n_packets: every record, the whole wire buffer byte for byte with the bytes at and past wire_capacity, both tail buffers, and the guards"""
    api = _amd().api
    d_tails, tails = None, None
    dst_residues, blocks = set(), set()
    for call in range(3):
        c = ref.pack_case(call, n, tails)
        want = _want_pack(c)
        bat = _enc(3) if call % 2 else _dec(3)
        got, d_tails = _pack(dev, bat, c, d_tails)
        _same(got, want, (n, call))
        assert (got["wire"][c["wire_capacity"]:] == ref.WIRE_FILL).all()
        ok = (want["red_size"][:n] > 0) & (want["red_flags"][:n] == 0)
        dst_residues |= set(((want["red_offset"][:n][ok] + c["header_room"]) % 16).tolist())
        blocks |= set(want["red_blocks"][:n].tolist())
        tails = (got["tail_bytes"], got["tail_sizes"])
        bat.close()
    if n >= 63:
        assert {0, 1, 3, 7, 15} <= blocks and len(dst_residues) >= 8 and {r % 4 for r in dst_residues} == {0, 1, 2, 3}
    c = ref.pack_case(1, n, tails)                                    # every optional input and output NULL (no tail kernel), a second stream, sync = 0
    c.update(flags=None, counts=None, depth=None, tail_bytes=None, tail_sizes=None)
    bat = _enc(3)
    got, _ = _pack(dev, bat, c, None, (), hip_stream=dev.stream(), sync=False)
    assert all(got[k] is None for k in ("red_flags", "red_blocks", "wire_total", "route_stats", "tail_sizes"))
    _same(got, _want_pack(c, ()), (n, "optional NULL"), ("red_offset", "red_size", "wire"))
    bat.close()


def _plan_unpack(c, optional=None):
    api = _amd().api
    return api.plan_red_unpack(c["n_streams"], c["stream"], c["seq"], c["offsets"], c["num_bytes"], c["ring"], c["ts_step"], c["max_red"], c["timestamp"], c["block_pt"],
                               api.RED_UNPACK_OPTIONAL if optional is None else optional, c["ring_capacity"])


def _unpack(dev, bat, c, d_ring, optional=None, hip_stream=None, sync=True):
    """one unpack call on decoder batch bat over the ring already on the device -> dict as api.plan_red_unpack gives"""
    api = _amd().api
    optional = api.RED_UNPACK_OPTIONAL if optional is None else optional
    n = len(c["stream"])
    m = n * (c["max_red"] + 1)
    shapes = {k: ({"status": n, "stats": api.RED_UNPACK_STATS_WORDS}.get(k, m), dt) for k, dt in UNPACK_TYPES.items()}
    ptr = _outputs(dev, shapes, optional, ref.UNPACK_KEYS[:4])
    bat.red_unpack_device(n, dev.put(np.asarray(c["stream"], np.int32)), dev.put(_u32(c["seq"])), dev.put(np.asarray(c["offsets"], np.int64)),
                          dev.put(np.asarray(c["num_bytes"], np.int32)), d_ring, c["ring_capacity"], c["max_red"], c["ts_step"], ptr["stream"], ptr["seq"], ptr["offsets"],
                          ptr["num_bytes"], dev.put(_u32(c["timestamp"])) if c["timestamp"] is not None else None,
                          dev.put(np.asarray(c["block_pt"], np.int32)) if c["block_pt"] is not None else None, ptr["timestamp"], ptr["gen"], ptr["status"], ptr["stats"],
                          hip_stream, sync=sync)
    if not sync:
        dev.stream_sync(hip_stream) if hip_stream else dev.sync()
    return _collect(dev, ptr, shapes)


@pytest.mark.parametrize("which", ["crafted4", "crafted2", "crafted0", "random4", "random1"])
def test_unpack_equals_the_host_plan(dev, which):
    """the crafted set of test_red_cpu.py - valid packets of 0 ... 4 blocks at every alignment, a header list truncated at every byte, lengths past the payload, five
    and six headers, every per-block drop, the payload-type refusal, dropped and out-of-range items - under max_red 4, 2 and 0, and 1 000 items of seeded random
    bytes under max_red 4 and 1, at item counts that fill neither waves nor workgroups: every output and stats, the guards behind them, and the ring unchanged"""
    api = _amd().api
    max_red = int(which[-1])
    c = ref.crafted_unpack(max_red)[0] if which.startswith("crafted") else ref.random_unpack(1000, max_red=max_red)
    total = len(c["stream"])
    d = _dec(c["n_streams"])
    d_ring = dev.put(np.concatenate([c["ring"], np.zeros(8, np.uint8)]))
    for k, n in enumerate(COUNTS):
        part = ref.subset(c, (np.arange(n) + 7 * k) % total)
        want = _plan_unpack(part)
        assert want["stats"][:8].sum() == n
        _same(_unpack(dev, d, part, d_ring), want, (which, n))
    part = ref.subset(c, np.arange(257) % total)                      # every optional input and output NULL (no fill kernel), on a second HIP stream, sync = 0
    part.update(timestamp=None, block_pt=None)
    got = _unpack(dev, d, part, d_ring, optional=(), hip_stream=dev.stream(), sync=False)
    assert all(got[k] is None for k in api.RED_UNPACK_OPTIONAL)
    _same(got, _plan_unpack(part), (which, "optional NULL"), ref.UNPACK_KEYS[:4])
    assert np.array_equal(dev.get(d_ring, c["ring"].shape, np.uint8), c["ring"]), "the ring was written"
    d.close()


@pytest.mark.parametrize("depth", [1, 2, 4])
def test_sender_to_receiver_through_a_dropped_burst(dev, depth):
    """encode_device_packed, egress in place (stream-major), red_pack, stamp with red_offset / red_size / red_flags as the list, the sizes of a burst of `depth`
    packets of one stream and of the first packets of another overwritten with -1 by an asynchronous copy (the parse refuses them: never arrived), parse,
    red_unpack, probe, ingest with the probe's records, set_frame_counts + decode_device_packed from the wire buffer: 48k_10_128B, 4 streams x 16 frames, all
    queued on one HIP stream with sync = 0 and one wait at the end.  No cell is a gap, and PCM and status equal the oracle decoder's over the frames the encoder
    wrote, none of them lost"""
    api = _amd().api
    geom = "48k_10_128B"
    fs, ms, hr, ch, sizes = hf.GEOMS[geom]
    S, T, N, size = 4, 16, hf.frame_len(fs, ms), int(sizes[0])
    room, align, K = 12, 4, depth + 1
    n = S * T
    pcm_in = synth_pcm(S, T, N, fs, seed=41).reshape(S, T, ch, N)
    buf = n * size + 64
    wire_bytes = n * (room + 17 + K * size + align)
    stride = api.red_tail_stride(size)
    enc = _amd().Batch(S, fs, ch, ms, hr, [size * 800] * S, device=0)
    dec = _amd().DecBatch(S, fs, ch, ms, hr, None, device=0)
    i32, i64, u8 = (lambda k, v=-7: dev.put(np.full(k, v, np.int32))), (lambda k, v=-7: dev.put(np.full(k, v, np.int64))), (lambda k, v=0xEE: dev.put(np.full(k, v, np.uint8)))
    d_pcm_in, d_out = dev.put(pcm_in), u8(buf, 0xC3)
    d_off, d_tot, d_nb, d_fl = i64((S, T)), i64(1), i32((S, T)), u8((S, T))
    seq_base = (65530 + np.arange(S)).astype(np.int32)
    ssrc, ts_base = 0x7FFFFFF0 + 7 * np.arange(S), 0xFFFFF000 + 100000 * np.arange(S)
    d_base, d_ssrc, d_tsb = dev.put(seq_base), dev.put(_u32(ssrc)), dev.put(_u32(ts_base))
    d_red_pt, d_blk_pt, d_sid = dev.put(np.full(S, 97, np.int32)), dev.put(np.full(S, 96, np.int32)), dev.put(np.arange(S, dtype=np.int32))
    d_wire = u8(wire_bytes, ref.WIRE_FILL)
    p_route, p_seq, p_frame, p_off, p_size = i32(n), i32(n), i32(n), i64(n, -1), i32(n, 0)
    d_np, d_next, d_stats, d_cs = i64(1), i32(S), i32((S, 4)), u8((S, T))
    e_work = dev.put(np.zeros(api.egress_work_bytes(S, T) // 8 + 1, np.int64))
    r_off, r_size, r_flags, r_blocks, r_total, r_stats = i64(n, -1), i32(n, 0), u8(n), u8(n), i64(1), i32((S, 4))
    r_work = dev.put(np.zeros(api.red_work_bytes(n) // 8 + 1, np.int64))
    d_tb, d_tz = u8(S * depth * stride), i32(S * depth)
    d_pst, d_nts = u8(n), i32(S)
    i_stream, i_seq, i_off, i_nb, i_ts, i_st = i32(n), i32(n), i64(n), i32(n), i32(n), u8(n)
    m = n * K
    o_stream, o_seq, o_off, o_nb, o_ts, o_gen, o_st, o_stats = i32(m), i32(m), i64(m), i32(m), i32(m), u8(m), u8(n), i32(16)
    d_info = dev.put(np.zeros((m, ch, api.FRAME_INFO_WORDS), np.int32))
    d_oo, d_onb, d_ci, d_cnt2, d_nb2, d_ist = i64((S, T)), i32((S, T)), i32((S, T)), i32(S), i32(S), i32((S, 4))
    d_pcm, d_st = dev.put(np.full((S, T, ch, N), 0x5555, np.int16)), u8((S, T))
    bursts = [(1, 5, depth), (3, 0, depth), (2, T - 2 * depth, depth)]              # (stream, first frame, length): each ends at least `depth` packets before the last
    gone = dev.pin(np.full(depth, -1, np.int32))
    dev.sync()
    s1 = dev.stream()
    enc.encode_device_packed(d_pcm_in, 16, T, d_out, buf, api.PACK_STREAM_MAJOR, None, None, d_off, d_tot, d_nb, d_fl, s1, sync=False)
    enc.egress_device(T, d_out, buf, d_off, d_nb, size, S, d_base, p_route, p_seq, p_frame, p_off, p_size, d_np, e_work, d_fl, api.ENC_FL_PACK_CAP, None, None, 16,
                      api.PACK_STREAM_MAJOR, None, 0, 0, 1, None, None, d_next, d_stats, d_cs, s1, sync=False)
    enc.red_pack_device(T, d_out, buf, d_off, d_nb, size, S, n, d_np, p_route, p_frame, depth, d_blk_pt, N, 1 << 20, d_wire, wire_bytes, r_off, r_size, r_work, room, align,
                        d_fl, api.ENC_FL_PACK_CAP, None, None, None, None, None, stride, d_tb, d_tz, r_flags, r_blocks, r_total, r_stats, s1, sync=False)
    enc.rtp_stamp_device(n, d_np, p_route, p_seq, p_frame, r_off, r_size, S, T, d_ssrc, d_tsb, d_red_pt, N, d_wire, wire_bytes, room, 0, r_flags, api.RTP_MARKER_NEVER, None,
                         None, d_stats, d_pst, d_nts, None, s1, sync=False)
    for s, a, k in bursts:                                            # stream-major, every cell SENT: packet s * T + t is frame t of stream s
        dev.copy_async(r_size + 4 * (s * T + a), gone, s1)
    dec.rtp_parse_device(n, d_wire, wire_bytes, r_off, r_size, S, d_ssrc, d_sid, i_stream, i_seq, i_off, i_nb, d_red_pt, 0, i_ts, None, i_st, None, s1, sync=False)
    dec.red_unpack_device(n, i_stream, i_seq, i_off, i_nb, d_wire, wire_bytes, depth, N, o_stream, o_seq, o_off, o_nb, i_ts, d_blk_pt, o_ts, o_gen, o_st, o_stats, s1,
                          sync=False)
    dec.probe_device(d_wire, wire_bytes, o_off, o_nb, size, m, d_info, api.PROBE_FULL, s1, sync=False)
    dec.ingest_device(m, o_stream, o_seq, o_off, o_nb, d_base, T, d_oo, d_onb, d_ci, d_cnt2, 16, d_info, None, d_nb2, d_ist, None, s1, sync=False)
    dec.set_frame_counts(d_cnt2)
    dec.decode_device_packed(d_wire, wire_bytes, d_oo, T, d_pcm, d_onb, size, None, d_st, 16, s1, sync=False)
    dev.stream_sync(s1)
    # the sender: the plan's packets over the encoder's tables, stamped as RED
    assert int(dev.get(d_np, (1,), np.int64)[0]) == n and (dev.get(d_cs, (S, T), np.uint8) == api.EGR_SENT).all()
    frames, off, nb = dev.get(d_out, (buf,), np.uint8), dev.get(d_off, (S, T), np.int64), dev.get(d_nb, (S, T), np.int32)
    route, frame = dev.get(p_route, (n,), np.int32), dev.get(p_frame, (n,), np.int32)
    assert (nb == size).all() and np.array_equal(route, np.repeat(np.arange(S), T)) and np.array_equal(frame, np.tile(np.arange(T), S))
    want = api.plan_red_pack(S, frames, off, nb, size, route, frame, np.full(S, 96), N, np.full(wire_bytes, ref.WIRE_FILL, np.uint8), depth, None, 1 << 20, n,
                             dev.get(d_fl, (S, T), np.uint8), api.ENC_FL_PACK_CAP, header_room=room, align=align, tail_stride=stride)
    sizes_sent = want["red_size"].copy()
    wire = dev.get(d_wire, (wire_bytes,), np.uint8)
    blank = wire.copy()
    for p in range(n):
        blank[want["red_offset"][p]:want["red_offset"][p] + 12] = ref.WIRE_FILL
    assert np.array_equal(blank, want["wire"]) and np.array_equal(dev.get(r_off, (n,), np.int64), want["red_offset"]) and not dev.get(r_flags, (n,), np.uint8).any()
    assert np.array_equal(dev.get(r_blocks, (n,), np.uint8), want["red_blocks"]) and np.array_equal(dev.get(r_stats, (S, 4), np.int32), want["route_stats"])
    assert np.array_equal(dev.get(d_tz, (S, depth), np.int32), want["tail_sizes"]) and (want["tail_sizes"] == size).all() and (dev.get(d_pst, (n,), np.uint8) == 1).all()
    assert np.array_equal(dev.get(d_tb, (S, depth, stride), np.uint8)[:, :, :size], want["tail_bytes"][:, :, :size])
    lost = np.zeros(n, bool)
    for s, a, k in bursts:
        lost[s * T + a:s * T + a + k] = True
    assert np.array_equal(dev.get(r_size, (n,), np.int32), np.where(lost, -1, sizes_sent))
    # the receiver: the parse's refusals are the burst, the unpack is the plan's, the ingest has no gap
    st = dev.get(i_st, (n,), np.uint8)
    assert np.array_equal(st != 0, lost) and (st[lost] == api.RTP_RANGE).all()
    items = [dev.get(p, (n,), dt) for p, dt in ((i_stream, np.int32), (i_seq, np.int32), (i_off, np.int64), (i_nb, np.int32), (i_ts, np.int32))]
    u = api.plan_red_unpack(S, items[0], items[1], items[2], items[3], wire, N, depth, items[4], np.full(S, 96))
    got = dict(stream=dev.get(o_stream, (m,), np.int32), seq=dev.get(o_seq, (m,), np.int32), offsets=dev.get(o_off, (m,), np.int64), num_bytes=dev.get(o_nb, (m,), np.int32),
               timestamp=dev.get(o_ts, (m,), np.int32), gen=dev.get(o_gen, (m,), np.uint8), status=dev.get(o_st, (n,), np.uint8), stats=dev.get(o_stats, (16,), np.int32))
    _same(got, u, depth)
    assert np.array_equal(got["status"] != 0, lost) and (got["status"][lost] == api.RED_DROPPED).all() and not got["stats"][8:11].any()
    ist, counts2 = dev.get(d_ist, (S, 4), np.int32), dev.get(d_cnt2, (S,), np.int32)
    assert (counts2 == T).all() and (ist[:, 1] == 0).all() and (dev.get(d_onb, (S, T), np.int32) == size).all()
    oo = dev.get(d_oo, (S, T), np.int64)
    for s in range(S):
        for t in range(T):
            assert np.array_equal(wire[oo[s, t]:oo[s, t] + size], frames[off[s, t]:off[s, t] + size]), (s, t)
    fr = np.stack([[frames[off[s, t]:off[s, t] + size] for t in range(T)] for s in range(S)])
    o = hf.decode(geom, fr, np.full((S, T), size), np.zeros((S, T), np.uint8))
    pcm, dst = dev.get(d_pcm, (S, T, ch, N), np.int16), dev.get(d_st, (S, T), np.uint8)
    assert np.array_equal(dst, o["status"]) and not dst.any()
    bad = np.argwhere((pcm != o["pcm"]).any(axis=(2, 3)))
    assert len(bad) == 0, ("first differing (stream, frame)", bad[:4].tolist())
    enc.close()
    dec.close()


def test_red_calls_are_stateless(dev):
    """an encoder batch and a decoder batch, each with state behind it: get_state() and the configuration are bit for bit what they were after pack and unpack
    calls - the host convenience calls and calls with sync = 0 on a second stream, beside an encode call on the batch's own - every result is the plan's, and a
    later decode call gives what a twin batch gives that never saw them"""
    api = _amd().api
    S, T = 3, 12
    pc = ref.pack_case(0, 100, None)
    uc = ref.subset(ref.random_unpack(1000), np.arange(300))
    enc = _enc(S)
    first = enc.encode(synth_pcm(S, T, 480, 48000, seed=5))
    second = enc.encode(synth_pcm(S, T, 480, 48000, seed=6))
    dec, twin = (_amd().DecBatch(S, 48000, 1, 10.0, 0, [80] * S, device=0) for _ in range(2))
    dec.decode(first)
    twin.decode(first)
    want_pack, want_unpack = _want_pack(pc), _plan_unpack(uc)
    plain = _plan_pack(pc)
    d_ring = dev.put(np.concatenate([uc["ring"], np.zeros(8, np.uint8)]))
    for bat in (enc, dec):
        before = (bat.get_state(), [bat.num_bytes(s) for s in range(S)])
        r = bat.red_pack(pc["frames"], pc["offsets"], pc["num_bytes"], pc["max_frame_bytes"], pc["pkt_route"], pc["pkt_frame"], pc["block_pt"], pc["ts_step"], pc["wire"],
                         pc["max_depth"], pc["depth"], pc["max_packet_bytes"], pc["n_packets"], pc["flags"], pc["skip_mask"], pc["counts"], pc["route_src"], None, None,
                         pc["tail_stride"], pc["wire_capacity"], pc["header_room"], pc["align"], frames_capacity=pc["frames_capacity"])
        _same(r, plain, "red_pack()", [k for k in plain if k != "wire_total"])
        assert r["wire_total"] == plain["wire_total"]
        got, _ = _pack(dev, bat, pc, None, hip_stream=dev.stream(), sync=False)
        _same(got, want_pack, "second stream")
        got, _ = _pack(dev, bat, pc, None)
        _same(got, want_pack, "the batch's own stream")
        if bat is dec:
            r = bat.red_unpack(uc["stream"], uc["seq"], uc["offsets"], uc["num_bytes"], uc["ring"], uc["ts_step"], uc["max_red"], uc["timestamp"], uc["block_pt"],
                               ring_capacity=uc["ring_capacity"])
            _same(r, want_unpack, "red_unpack()")
            _same(_unpack(dev, bat, uc, d_ring, hip_stream=dev.stream(), sync=False), want_unpack, "second stream")
        after = (bat.get_state(), [bat.num_bytes(s) for s in range(S)])
        assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    # beside an encode call of the same batch: the encode on the batch's own stream, the pack on another, neither waited for in between
    third = synth_pcm(S, T, 480, 48000, seed=7)
    twin_enc = _enc(S)
    for seed in (5, 6):
        twin_enc.encode(synth_pcm(S, T, 480, 48000, seed=seed))
    d_pcm, d_bits = dev.put(third), dev.put(np.zeros((S, T, enc.stride), np.uint8))
    enc.encode_device(d_pcm, 16, T, d_bits, enc.stride, sync=False)
    got, _ = _pack(dev, enc, pc, None, hip_stream=dev.stream(), sync=False)
    dev.sync()
    _same(got, want_pack, "beside an encode call")
    assert np.array_equal(dev.get(d_bits, (S, T, enc.stride), np.uint8), twin_enc.encode(third)) and np.array_equal(enc.get_state(), twin_enc.get_state())
    twin_enc.close()
    a, b = dec.decode(second), twin.decode(second)
    for x, y in zip(a, b) if isinstance(a, tuple) else ((a, b),):
        assert np.array_equal(x, y)
    for x in (enc, dec, twin):
        x.close()


def test_every_red_kernel_ran_under_a_comparison(dev):
    """the sibling library counts its launches: every kernel its code object holds (tools/kernel_resources.py) has run - here, once more, under a comparison, so
    that the test stands alone - and a name it does not hold is answered with -1"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels
    names = sorted(kernels(LIB, "gfx950"))
    assert names == KERNELS
    before = {k: _launches(k) for k in names}
    d = _dec(3)
    c = ref.pack_case(2, 65, None)
    got, _ = _pack(dev, d, c)
    _same(got, _want_pack(c), "pack")
    u = ref.subset(ref.random_unpack(1000), np.arange(65))
    _same(_unpack(dev, d, u, dev.put(np.concatenate([u["ring"], np.zeros(8, np.uint8)]))), _plan_unpack(u), "unpack")
    d.close()
    for k in names:
        assert _launches(k) == before[k] + 1, k
    assert _launches("lc3_egress_copy_kernel") == -1 and _launches("lc3_encode_kernel") == -1
