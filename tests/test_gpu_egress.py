"""Packet egress on the GPU (lc3plus_enc_batch_egress, lc3plus_dec_batch_egress; the six kernels of liblc3plus_egress_hip.so).  Every output is held to
equality: the kernels against the host plan (api.plan_egress, itself held to the numpy rule in test_egress_cpu.py) on shapes that fill neither waves nor
workgroups nor tiles, with guard elements behind every output and the sentinel in every byte of the wire buffer no packet owns; the copy at every pair of source
and destination alignment; the sender chain set_frame_counts + encode_packed -> egress -> ingest -> set_frame_counts + decode_packed on one HIP stream with a
single wait at the end, against the CPU oracle; the forwarder chain probe -> ingest -> egress -> ingest; statelessness; offsets past 4 GiB; and the sibling
library's own launch counts.  Device buffers through ctypes (test_gpu_dec_varsize_device._Hip)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import egress_ref as ref
import hostile_frames as hf
from lc3_harness import Oracle, sibling_launches, synth_pcm
from test_gpu_dec_varsize_device import _Hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "audio_codec_amd", "liblc3plus_egress_hip.so")
GUARD = 16                                             # elements behind every output array
E2E_GEOMS = ("48k_10_128B", "48k_10_stereo_161B")      # one mono, one stereo geometry
KERNELS = ["lc3_egress_base_kernel", "lc3_egress_classify_kernel", "lc3_egress_copy_kernel", "lc3_egress_route_kernel", "lc3_egress_scatter_kernel",
           "lc3_egress_sums_kernel"]
SENTINEL = {np.int64: 0x5A5A5A5A5A5A5A5A, np.int32: 0x5A5A5A5A, np.uint8: 0x5A}


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


def _launches(name):
    return sibling_launches("egress", name)


def _shapes(c):
    R, T = len(c["seq_base"]), c["n_frames"]
    n = R * T
    return dict(pkt_route=((n,), np.int32), pkt_seq=((n,), np.int32), pkt_frame=((n,), np.int32), pkt_offset=((n,), np.int64), pkt_size=((n,), np.int32),
                pkt_flags=((n,), np.uint8), n_packets=((1,), np.int64), wire_total=((1,), np.int64), next_seq=((R,), np.int32),
                stats=((R, ref.STATS_WORDS), np.int32), cell_status=((R, T), np.uint8))


def _run(dev, bat, c, optional=None, hip_stream=None, sync=True):
    """one egress call on batch bat (an encoder's or a decoder's) -> dict as api.plan_egress gives, the list arrays cut at n_packets.  Every output lies in front
    of GUARD sentinel elements and holds the sentinel beforehand: the guards and the list's tail behind n_packets must come back untouched.  The wire buffer is
    the case's (every byte the sentinel), the bytes at and past wire_capacity included."""
    api = _amd().api
    optional = api.EGR_OPTIONAL if optional is None else optional
    shapes = _shapes(c)
    R, T = len(c["seq_base"]), c["n_frames"]
    ptr = {}
    for k, (shape, dt) in shapes.items():
        ptr[k] = dev.put(np.full(int(np.prod(shape)) + GUARD, SENTINEL[dt], dt)) if k not in api.EGR_OPTIONAL or k in optional else None
    put = lambda a: dev.put(a) if a is not None else None
    d_frames = dev.put(np.concatenate([c["frames"], np.zeros(8, np.uint8)]))
    d_wire = put(c["wire"])
    seq_base = (np.asarray(c["seq_base"], np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    work = dev.put(np.full(api.egress_work_bytes(R, T) // 8 + 1, -1, np.int64))
    bat.egress_device(T, d_frames, c["frames_capacity"], dev.put(c["offsets"]), dev.put(c["num_bytes"]), c["max_frame_bytes"], R, dev.put(seq_base), ptr["pkt_route"],
                      ptr["pkt_seq"], ptr["pkt_frame"], ptr["pkt_offset"], ptr["pkt_size"], ptr["n_packets"], work, put(c["flags"]), c["skip_mask"], put(c["counts"]),
                      put(c["route_src"]), c["seq_bits"], c["order"], d_wire, c["wire_capacity"], c["header_room"], c["align"], ptr["pkt_flags"], ptr["wire_total"],
                      ptr["next_seq"], ptr["stats"], ptr["cell_status"], hip_stream, sync=sync)
    if not sync:
        dev.stream_sync(hip_stream) if hip_stream else dev.sync()
    out = {}
    for k, (shape, dt) in shapes.items():
        if ptr[k] is None:
            out[k] = None
            continue
        size = int(np.prod(shape))
        got = dev.get(ptr[k], (size + GUARD,), dt)
        assert (got[size:] == SENTINEL[dt]).all(), ("an element behind the output was written", k)
        out[k] = got[:size].reshape(shape)
    n = int(out["n_packets"][0])
    assert 0 <= n <= R * T
    for k in ref.LIST:
        if out[k] is not None:
            assert (out[k][n:] == SENTINEL[shapes[k][1]]).all(), ("the list's tail was written", k)
    out["n_packets"] = n
    out["wire_total"] = int(out["wire_total"][0]) if out["wire_total"] is not None else None
    out["wire"] = dev.get(d_wire, c["wire"].shape, np.uint8) if c["wire"] is not None else None
    assert np.array_equal(dev.get(d_frames, c["frames"].shape, np.uint8), c["frames"]), "the source frames were written"
    return out


def _plan(c, optional=None):
    api = _amd().api
    return api.plan_egress(c["n_streams"], c["frames"], c["offsets"], c["num_bytes"], c["seq_base"], c["max_frame_bytes"], c["flags"], c["skip_mask"], c["counts"],
                           c["route_src"], c["seq_bits"], c["order"], c["wire"], c["wire_capacity"], c["header_room"], c["align"],
                           api.EGR_OPTIONAL if optional is None else optional, c["frames_capacity"])


def _same(got, want, name, keys=ref.KEYS):
    """equality; the list arrays over their first n_packets entries (the device's tails hold the sentinel, checked in _run)"""
    n = want["n_packets"]
    for k in keys + ("wire",):
        g, w = got[k], want[k]
        if isinstance(w, int) or w is None:
            assert g == w, (name, k, g, w)
            continue
        if k in ref.LIST:
            g, w = g[:n], w[:n]
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (name, k, "first differences at", bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _enc(S):
    return _amd().Batch(S, 48000, 1, 10.0, 0, [64000] * S, device=0)


def _dec(S, ch=1):
    return _amd().DecBatch(S, 48000, ch, 10.0, 0, None, device=0)


@pytest.mark.parametrize("name", list(ref.gpu_cases()))
def test_kernels_equal_the_host_plan(dev, name):
    """every output of the kernels against lc3plus_plan_egress and against the numpy rule, on an encoder batch; once more with every optional output NULL (no
    route kernel, no status), on a decoder batch and a second HIP stream"""
    c = ref.gpu_cases()[name]
    want = _plan(c)
    _same(want, ref.rule(c), (name, "plan against the rule"))
    b = _enc(c["n_streams"])
    _same(_run(dev, b, c), want, name)
    b.close()
    d = _dec(c["n_streams"])
    got = _run(dev, d, c, optional=(), hip_stream=dev.stream())
    assert all(got[k] is None for k in _amd().api.EGR_OPTIONAL)
    _same(got, want, (name, "optional outputs NULL"), ref.LIST[:5] + ("n_packets",))
    d.close()


@pytest.mark.parametrize("cut", [None, "inside", "end", "zero", "short"])
@pytest.mark.parametrize("wire", ref.WIRES)
def test_copy_at_every_alignment(dev, wire, cut):
    """frames of every size 1 ... 40, 63, 64, 65, 255, 256, 257, 400, 625 and 1250 from every source address mod 16 to the destinations this header room and
    alignment give: wire is byte for byte the numpy gather, the sentinel wherever no fitting packet's payload lies - header rooms, padding, the packets cut by
    wire_capacity, and every byte at and past wire_capacity"""
    c = ref.copy_case(wire, cut, seed=wire[0])
    want = ref.rule(c)
    n = want["n_packets"]
    assert n == 16 * len(ref.COPY_SIZES)
    src = c["offsets"].reshape(-1) % 16
    assert set(src.tolist()) == set(range(16))
    fits = want["pkt_flags"][:n] == 0
    assert {None: fits.all(), "inside": fits.any() and not fits.all(), "end": fits.any() and not fits.all(), "zero": not fits.any(), "short": not fits.any()}[cut]
    d = _dec(c["n_streams"])
    got = _run(dev, d, c)
    _same(got, want, (wire, cut))
    assert (got["wire"][c["wire_capacity"]:] == ref.WIRE_FILL).all()
    d.close()


def test_copy_covers_all_relative_alignments():
    """over the five destinations of WIRES, every (source mod 16, destination mod 16) pair occurs (pure bookkeeping of the cases above, no device)"""
    seen = set()
    for w in ref.WIRES:
        c = ref.copy_case(w, None, seed=w[0])
        r = ref.rule(c)
        n = r["n_packets"]
        src = c["offsets"][r["pkt_route"][:n], r["pkt_frame"][:n]] % 16
        seen |= set(zip(src.tolist(), ((r["pkt_offset"][:n] + c["header_room"]) % 16).tolist()))
    assert len(seen) == 256


def test_in_place_mode_copies_nothing(dev):
    """wire NULL: the offsets are the source's, nothing but the list is written (the frames are compared in _run), and the copy kernel is not launched"""
    c = ref.gpu_cases()["70x67_fan_inplace"]
    b = _enc(c["n_streams"])
    before = _launches("lc3_egress_copy_kernel")
    got = _run(dev, b, c)
    assert _launches("lc3_egress_copy_kernel") == before
    _same(got, _plan(c), "in place")
    n = got["n_packets"]
    src = np.asarray(c["route_src"])[got["pkt_route"][:n]]
    assert n > 0 and np.array_equal(got["pkt_offset"][:n], c["offsets"][src, got["pkt_frame"][:n]])
    assert np.array_equal(got["pkt_size"][:n], c["num_bytes"][src, got["pkt_frame"][:n]]) and not got["pkt_flags"][:n].any()
    assert got["wire_total"] == int(got["pkt_size"][:n].sum())
    b.close()


@functools.lru_cache(maxsize=None)
def _sender(geom):
    """6 streams x 9 frames of a geometry at the bitrate of its frame size: PCM, the oracle encoder's frames, ragged counts"""
    fs, ms, hr, ch, sizes = hf.GEOMS[geom]
    S, T, N, size = 6, 9, hf.frame_len(fs, ms), int(sizes[0])
    rate = size * 800
    pcm = synth_pcm(S * ch, T, N, fs, seed=31 + ch).reshape(S, ch, T, N).transpose(0, 2, 1, 3).copy()
    frames = np.zeros((S, T, size), np.uint8)
    for s in range(S):
        o = Oracle(fs, ch, ms, hr, rate, portable_math=True)
        for t in range(T):                                           # (Oracle.encode expects channels of equal bytes: 161 bytes are 81 + 80)
            planar, nb = np.ascontiguousarray(pcm[s, t]), C.c_int(0)
            ptrs = (C.c_void_p * ch)(*[planar[c].ctypes.data for c in range(ch)])
            assert o.lib.lc3o_enc_frame(o.p, ptrs, 16, frames[s, t].ctypes.data, C.byref(nb)) == 0 and nb.value == size
    out = dict(S=S, T=T, N=N, size=size, rate=rate, pcm=pcm, frames=frames, counts=np.array([9, 7, 0, 9, 4, 11], np.int32))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return out


@pytest.mark.parametrize("geom", E2E_GEOMS)
def test_sender_without_a_host_wait(dev, geom):
    """set_frame_counts + encode_device_packed (frame-major, a capacity five frames and a few bytes short), egress in place with identity routes, ingest with
    base = seq_base, set_frame_counts + decode_device_packed, all queued on one HIP stream with sync = 0 and one wait at the end.  The list is the host plan's on
    the encoder's tables; PCM and status equal the oracle decoder over the oracle encoder's frames with exactly the frames that were not SENT lost; frames
    behind the ingest's count are absent"""
    api = _amd().api
    fs, ms, hr, ch, _ = hf.GEOMS[geom]
    sc = _sender(geom)
    S, T, N, size = sc["S"], sc["T"], sc["N"], sc["size"]
    present = int(np.clip(sc["counts"], 0, T).sum())
    cap = (present - 5) * size + 9
    room = present * size + 64                                     # the buffer itself: a frame cut by cap is SKIPPED by its flag, not INVALID by its place
    enc = _amd().Batch(S, fs, ch, ms, hr, [sc["rate"]] * S, device=0)
    dec = _amd().DecBatch(S, fs, ch, ms, hr, None, device=0)
    i32, i64, u8 = (lambda n, v=-7: dev.put(np.full(n, v, np.int32))), (lambda n, v=-7: dev.put(np.full(n, v, np.int64))), (lambda n, v=0xEE: dev.put(np.full(n, v, np.uint8)))
    d_pcm_in, d_cnt, d_out = dev.put(sc["pcm"]), dev.put(sc["counts"]), u8(present * size + 64, 0xC3)
    d_off, d_tot, d_nb, d_fl = i64((S, T)), i64(1), i32((S, T)), u8((S, T))
    seq_base = (65530 + np.arange(S)).astype(np.int32)
    d_base = dev.put(seq_base)
    n = S * T
    p_route, p_seq, p_frame, p_off, p_size, p_flags = i32(n, -1), i32(n), i32(n), i64(n), i32(n, 0), u8(n)      # route -1: the ingest drops what lies behind n_packets
    d_np, d_wt, d_next, d_stats, d_cs = i64(1), i64(1), i32(S), i32((S, 4)), u8((S, T))
    work = dev.put(np.zeros(api.egress_work_bytes(S, T) // 8 + 1, np.int64))
    d_oo, d_onb, d_ci, d_cnt2, d_nb2 = i64((S, T)), i32((S, T)), i32((S, T)), i32(S), i32(S)
    d_pcm, d_st = dev.put(np.full((S, T, ch, N), 0x5555, np.int16)), u8((S, T))
    dev.sync()
    s1 = dev.stream()
    enc.set_frame_counts(d_cnt)
    enc.encode_device_packed(d_pcm_in, 16, T, d_out, cap, api.PACK_FRAME_MAJOR, None, None, d_off, d_tot, d_nb, d_fl, s1, sync=False)
    enc.egress_device(T, d_out, room, d_off, d_nb, size, S, d_base, p_route, p_seq, p_frame, p_off, p_size, d_np, work, d_fl, api.ENC_FL_PACK_CAP, d_cnt, None, 16,
                      api.PACK_FRAME_MAJOR, None, 0, 0, 1, p_flags, d_wt, d_next, d_stats, d_cs, s1, sync=False)
    dec.ingest_device(n, p_route, p_seq, p_off, p_size, d_base, T, d_oo, d_onb, d_ci, d_cnt2, 16, None, None, d_nb2, None, None, s1, sync=False)
    dec.set_frame_counts(d_cnt2)
    dec.decode_device_packed(d_out, room, d_oo, T, d_pcm, d_onb, size, None, d_st, 16, s1, sync=False)
    dev.stream_sync(s1)
    enc.set_frame_counts(None)
    # the encoder's tables, and the list the host plan makes of them
    off, nb, fl = dev.get(d_off, (S, T), np.int64), dev.get(d_nb, (S, T), np.int32), dev.get(d_fl, (S, T), np.uint8)
    out = dev.get(d_out, (present * size + 64,), np.uint8)
    want = api.plan_egress(S, out, off, nb, seq_base, size, fl, api.ENC_FL_PACK_CAP, sc["counts"], None, 16, api.PACK_FRAME_MAJOR, frames_capacity=room)
    got = dict(pkt_route=dev.get(p_route, (n,), np.int32), pkt_seq=dev.get(p_seq, (n,), np.int32), pkt_frame=dev.get(p_frame, (n,), np.int32),
               pkt_offset=dev.get(p_off, (n,), np.int64), pkt_size=dev.get(p_size, (n,), np.int32), pkt_flags=dev.get(p_flags, (n,), np.uint8),
               n_packets=int(dev.get(d_np, (1,), np.int64)[0]), wire_total=int(dev.get(d_wt, (1,), np.int64)[0]), next_seq=dev.get(d_next, (S,), np.int32),
               stats=dev.get(d_stats, (S, 4), np.int32), cell_status=dev.get(d_cs, (S, T), np.uint8), wire=None)
    _same(got, want, geom)
    k = got["n_packets"]
    assert k == present - 5 and (got["pkt_route"][k:] == -1).all() and (got["pkt_size"][k:] == 0).all()
    sent = got["cell_status"] == api.EGR_SENT
    skipped = got["cell_status"] == api.EGR_SKIPPED
    assert skipped.sum() == 5 and np.array_equal(skipped, (fl & api.ENC_FL_PACK_CAP) != 0) and sent.sum() == k
    assert np.array_equal(got["next_seq"], (seq_base + np.clip(sc["counts"], 0, T)) & 0xFFFF)
    for p in range(k):                                               # each packet is the oracle encoder's frame, where it lies
        r, t, o = int(got["pkt_route"][p]), int(got["pkt_frame"][p]), int(got["pkt_offset"][p])
        assert np.array_equal(out[o:o + size], sc["frames"][r, t]), (r, t)
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


def test_forwarder_fans_out_what_the_ingest_ordered(dev):
    """probe -> ingest -> egress with three routes per stream into a wire buffer with 12 bytes of header room, queued on one HIP stream; then each receiver's
    packets, read from the wire, are ingested again: the receiver's tables are the first ingest's tables of its source stream, and the wire payloads are byte
    for byte the winners' frames"""
    from test_gpu_ingest import _scenario
    api = _amd().api
    geom = E2E_GEOMS[0]
    fs, ms, hr, ch, _ = hf.GEOMS[geom]
    sc = _scenario(geom)
    S, T, n, size = len(sc["counts"]), hf.T, len(sc["stream"]), sc["size"]
    room, align, fan = 12, 4, 3
    route_src = np.repeat(np.arange(S), fan).astype(np.int32)[::-1].copy()
    R = route_src.size
    seq_base = (65500 + 11 * np.arange(R)).astype(np.int32)
    d = _amd().DecBatch(S, fs, ch, ms, hr, None, device=0)
    i32, i64, u8 = (lambda k, v=-7: dev.put(np.full(k, v, np.int32))), (lambda k, v=-7: dev.put(np.full(k, v, np.int64))), (lambda k, v=0xEE: dev.put(np.full(k, v, np.uint8)))
    d_buf, d_stream, d_seq, d_off, d_nb, d_base = (dev.put(sc[k]) for k in ("buf", "stream", "seq", "offsets", "num_bytes", "base"))
    d_info = dev.put(np.zeros((n, ch, api.FRAME_INFO_WORDS), np.int32))
    d_oo, d_onb, d_ci, d_counts = i64((S, T)), i32((S, T)), i32((S, T)), i32(S)
    cells = R * T
    wire_bytes = cells * (room + size + align)
    d_wire = u8(wire_bytes, ref.WIRE_FILL)
    p_route, p_seq, p_frame, p_off, p_size, p_flags = i32(cells), i32(cells), i32(cells), i64(cells), i32(cells), u8(cells)
    d_np, d_wt, d_next, d_cs = i64(1), i64(1), i32(R), u8((R, T))
    work = dev.put(np.zeros(api.egress_work_bytes(R, T) // 8 + 1, np.int64))
    dev.sync()
    s1 = dev.stream()
    d.probe_device(d_buf, sc["buf"].size, d_off, d_nb, size, n, d_info, api.PROBE_FULL, s1, sync=False)
    d.ingest_device(n, d_stream, d_seq, d_off, d_nb, d_base, T, d_oo, d_onb, d_ci, d_counts, 16, d_info, None, None, None, None, s1, sync=False)
    d.egress_device(T, d_buf, sc["buf"].size, d_oo, d_onb, size, R, dev.put(seq_base), p_route, p_seq, p_frame, p_off, p_size, d_np, work, None, 0, d_counts,
                    dev.put(route_src), 16, api.PACK_FRAME_MAJOR, d_wire, wire_bytes, room, align, p_flags, d_wt, d_next, None, d_cs, s1, sync=False)
    dev.stream_sync(s1)
    oo, onb, counts = dev.get(d_oo, (S, T), np.int64), dev.get(d_onb, (S, T), np.int32), dev.get(d_counts, (S,), np.int32)
    k = int(dev.get(d_np, (1,), np.int64)[0])
    assert k == fan * int((onb > 0).sum()) > 0
    want = api.plan_egress(S, sc["buf"], oo, onb, seq_base, size, None, 0, counts, route_src, 16, api.PACK_FRAME_MAJOR, np.full(wire_bytes, ref.WIRE_FILL, np.uint8),
                           wire_bytes, room, align, frames_capacity=sc["buf"].size)
    got = dict(pkt_route=dev.get(p_route, (cells,), np.int32), pkt_seq=dev.get(p_seq, (cells,), np.int32), pkt_frame=dev.get(p_frame, (cells,), np.int32),
               pkt_offset=dev.get(p_off, (cells,), np.int64), pkt_size=dev.get(p_size, (cells,), np.int32), pkt_flags=dev.get(p_flags, (cells,), np.uint8), n_packets=k,
               wire_total=int(dev.get(d_wt, (1,), np.int64)[0]), next_seq=dev.get(d_next, (R,), np.int32), stats=None, cell_status=dev.get(d_cs, (R, T), np.uint8),
               wire=dev.get(d_wire, (wire_bytes,), np.uint8))
    _same(got, want, "forwarder", tuple(x for x in ref.KEYS if x != "stats"))
    assert not got["pkt_flags"][:k].any()
    # every receiver ingests its packets from the wire
    rx = _amd().DecBatch(R, fs, ch, ms, hr, None, device=0)
    again = rx.ingest(got["pkt_route"][:k], got["pkt_seq"][:k], got["pkt_offset"][:k] + room, got["pkt_size"][:k] - room, seq_base, T, 16)
    assert (again["item_status"] == api.ING_USED).all()
    for r in range(R):
        s = int(route_src[r])
        assert again["counts"][r] == counts[s] and np.array_equal(again["num_bytes"][r], onb[s]), (r, s)
        assert again["next_base"][r] == got["next_seq"][r] == (int(seq_base[r]) + int(counts[s])) & 0xFFFF
        for t in range(T):
            z, a, b = int(onb[s, t]), int(again["offsets"][r, t]), int(oo[s, t])
            assert np.array_equal(got["wire"][a:a + z], sc["buf"][b:b + z]) and (z == 0 or np.array_equal(sc["buf"][b:b + z], sc["frames"][s, t, :z])), (r, t)
    rx.close()
    d.close()


def test_egress_is_stateless(dev):
    """an encoder batch and a decoder batch, each with state behind it: get_state() and the configuration are bit for bit what they were after egress calls - the
    host convenience call, a call with sync = 0 on a second stream, and one queued beside an encode call that is still in flight - and every result is the
    plan's"""
    api = _amd().api
    c = ref.gpu_cases()["70x67_identity_wire32"]
    S, T = c["n_streams"], 12
    want = _plan(c)
    enc = _enc(S)
    pcm = synth_pcm(S, T, 480, 48000, seed=5)
    first = enc.encode(pcm)
    dec = _amd().DecBatch(S, 48000, 1, 10.0, 0, [80] * S, device=0)
    dec.decode(first)
    for bat in (enc, dec):
        before = (bat.get_state(), [bat.num_bytes(s) for s in range(S)])
        r = bat.egress(c["frames"], c["offsets"], c["num_bytes"], c["seq_base"], c["max_frame_bytes"], c["flags"], c["skip_mask"], c["counts"], c["route_src"],
                       c["seq_bits"], c["order"], c["wire"], c["wire_capacity"], c["header_room"], c["align"], frames_capacity=c["frames_capacity"])
        _same(r, want, "egress()")
        _same(_run(dev, bat, c, hip_stream=dev.stream(), sync=False), want, "second stream")
        after = (bat.get_state(), [bat.num_bytes(s) for s in range(S)])
        assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    # beside an encode call: the encode is queued on one stream, the egress on another, nothing waited for in between
    twin = _enc(S)
    twin.encode(pcm)
    d_pcm, d_out = dev.put(pcm), dev.put(np.zeros((S, T, 80), np.uint8))
    sa, sb = dev.stream(), dev.stream()
    enc.encode_device(d_pcm, 16, T, d_out, 80, hip_stream=sa, sync=False)
    got = _run(dev, enc, c, hip_stream=sb, sync=False)
    dev.stream_sync(sa)
    _same(got, want, "beside an encode call")
    assert np.array_equal(dev.get(d_out, (S, T, 80), np.uint8), twin.encode(pcm))
    for b in (enc, dec, twin):
        b.close()


def test_offsets_past_4g(dev):
    """source frames on both sides of byte 2^32 of an arena of 4 GiB + 64 KiB, and a wire buffer of the same size whose packets' running offset crosses 2^32 by
    way of a header room of 2^30 + 4096 bytes: list and bytes exact, and the windows a narrowed offset would read or write - the same offsets mod 2^32 - hold
    decoys and sentinels that stay what they are.  The arenas are allocated, not filled: only the windows looked at are written beforehand"""
    api = _amd().api
    hip = dev.hip
    arena = 2 ** 32 + 2 ** 16
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    assert free.value > 2 * arena + 2 ** 28, "the device has no room for two arenas of 4 GiB + 64 KiB"
    src, wire = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(src), C.c_size_t(arena)) == 0
    dev.ptrs.append(src)
    assert hip.hipMalloc(C.byref(wire), C.c_size_t(arena)) == 0
    dev.ptrs.append(wire)

    def write(base, at, a):
        assert 0 <= at and at + a.size <= arena
        assert hip.hipMemcpy(C.c_void_p(base.value + at), C.c_void_p(a.ctypes.data), C.c_size_t(a.size), C.c_int(1)) == 0

    def read(base, at, k):
        out = np.zeros(k, np.uint8)
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(base.value + at), C.c_size_t(k), C.c_int(2)) == 0
        return out
    rng = np.random.RandomState(4)
    S, T, size = 2, 2, 700
    room, align = 2 ** 30 + 4096, 4096
    offsets = np.array([[1000, 2 ** 32 - 333], [2 ** 32 + 20011, arena - size]], np.int64)           # low; astride 2^32; above it; ending at the capacity
    nb = np.full((S, T), size, np.int32)
    body = rng.randint(0, 256, size=(S, T, size)).astype(np.uint8)
    decoy = np.full(size + 32, 0xD7, np.uint8)
    for o in offsets.reshape(-1):
        if o >= 2 ** 32 - size:
            write(src, int(o) % 2 ** 32 if o >= 2 ** 32 else int(o) - 2 ** 31, decoy)                  # where the offset lands once narrowed
    for s in range(S):
        for t in range(T):
            write(src, int(offsets[s, t]), body[s, t])
    adv = (room + size + align - 1) // align * align
    assert adv == 2 ** 30 + 8192 and 3 * adv + room > 2 ** 32 and 4 * adv <= arena
    fill = np.full(size + 64, ref.WIRE_FILL, np.uint8)
    places = [p * adv + room for p in range(4)]
    narrowed = sorted({a % m for a in places for m in (2 ** 32, 2 ** 31)} - set(places))               # where a payload lands once its offset is narrowed
    assert narrowed == [12288, 28672, 2 ** 30 + 20480]                                               # all inside header rooms
    for a in places + narrowed:
        write(wire, a - 32, fill)
    seq_base = np.array([65535, 7], np.int32)
    n = S * T
    out = {k: dev.put(np.full(n + GUARD, SENTINEL[dt], dt)) for k, dt in (("route", np.int32), ("seq", np.int32), ("frame", np.int32), ("offset", np.int64),
                                                                            ("size", np.int32), ("flags", np.uint8))}
    d_np, d_wt, d_cs = dev.put(np.full(1, -7, np.int64)), dev.put(np.full(1, -7, np.int64)), dev.put(np.full((S, T), 0xEE, np.uint8))
    work = dev.put(np.zeros(api.egress_work_bytes(S, T) // 8 + 1, np.int64))
    d_off, d_nb, d_base = dev.put(offsets), dev.put(nb), dev.put(seq_base)
    d = _dec(S)
    for mode in ("wire", "in place"):
        w = mode == "wire"
        d.egress_device(T, src.value, arena, d_off, d_nb, size, S, d_base, out["route"], out["seq"], out["frame"], out["offset"], out["size"], d_np, work, None, 0,
                        None, None, 16, api.PACK_FRAME_MAJOR, wire.value if w else None, arena if w else 0, room if w else 0, align if w else 1, out["flags"], d_wt,
                        None, None, d_cs, None, sync=True)
        assert int(dev.get(d_np, (1,), np.int64)[0]) == n and (dev.get(d_cs, (S, T), np.uint8) == api.EGR_SENT).all()
        assert dev.get(out["route"], (n + GUARD,), np.int32)[:n].tolist() == [0, 1, 0, 1] and dev.get(out["frame"], (n + GUARD,), np.int32)[:n].tolist() == [0, 0, 1, 1]
        assert dev.get(out["seq"], (n + GUARD,), np.int32)[:n].tolist() == [65535, 7, 0, 8]
        po = dev.get(out["offset"], (n + GUARD,), np.int64)
        assert (po[n:] == SENTINEL[np.int64]).all() and not dev.get(out["flags"], (n + GUARD,), np.uint8)[:n].any()
        if w:
            assert po[:n].tolist() == [p * adv for p in range(n)] and int(dev.get(d_wt, (1,), np.int64)[0]) == n * adv
            assert dev.get(out["size"], (n + GUARD,), np.int32)[:n].tolist() == [room + size] * n
        else:
            assert po[:n].tolist() == [int(offsets[s, t]) for t in range(T) for s in range(S)] and int(dev.get(d_wt, (1,), np.int64)[0]) == n * size
    for p, (s, t) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):
        got = read(wire, p * adv + room - 32, size + 64)
        assert (got[:32] == ref.WIRE_FILL).all() and (got[32 + size:] == ref.WIRE_FILL).all() and np.array_equal(got[32:32 + size], body[s, t]), (p, s, t)
    for a in narrowed:
        assert (read(wire, a - 32, size + 64) == ref.WIRE_FILL).all(), a
    for s in range(S):
        for t in range(T):
            assert np.array_equal(read(src, int(offsets[s, t]), size), body[s, t])
    d.close()


def test_every_egress_kernel_ran_under_a_comparison(dev):
    """the sibling library counts its launches: every kernel its code object holds (tools/kernel_resources.py) has run - here, once more, under a comparison, so
    that the test stands alone - and a name it does not hold is answered with -1"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels
    names = sorted(kernels(LIB, "gfx950"))
    assert names == KERNELS
    c = ref.gpu_cases()["3x5_fm"]
    assert c["wire"] is not None
    b = _enc(c["n_streams"])
    _same(_run(dev, b, c), _plan(c), "3x5_fm")
    b.close()
    for n in names:
        assert _launches(n) > 0, n
    assert _launches("lc3_ingest_item_kernel") == -1 and _launches("lc3_encode_kernel") == -1
