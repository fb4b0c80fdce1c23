"""Generic FEC on the GPU (lc3plus_enc_batch_fec_encode, lc3plus_dec_batch_fec_encode, lc3plus_dec_batch_fec_recover; the nine kernels of
liblc3plus_fec_hip.so).  Every output is held to equality: the kernels against the host plans (api.plan_fec_encode, api.plan_fec_recover, themselves held to the
restatement of the rules in test_fec_cpu.py) with guard elements behind every output, the whole fec_wire, both accumulators and the recovery region compared
byte for byte, the workspace filled with 0xA5 before every call; packet counts on both sides of the wave and tile edges, groups of 1, 5 and 16, a chain of twenty
one-frame calls through the state buffers; and encode_packed -> egress -> stamp -> fec_encode -> stamp -> (dropped packets) -> parse x 2 -> fec_recover -> parse
-> probe -> ingest -> decode_packed on one HIP stream with a single wait at the end, against the CPU oracle's decode.  Device buffers through ctypes
(test_gpu_dec_varsize_device._Hip)."""
import os
import sys

import numpy as np
import pytest

import fec_ref as ref
import hostile_frames as hf
from lc3_harness import sibling_launches, synth_pcm
from test_gpu_dec_varsize_device import _Hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "audio_codec_amd", "liblc3plus_fec_hip.so")
GUARD = 16                                             # elements behind every output array
POISON = 0xA5
KERNELS = ["lc3_fec_enc_base_kernel", "lc3_fec_enc_qbase_kernel", "lc3_fec_enc_scatter_kernel", "lc3_fec_enc_sums_kernel", "lc3_fec_enc_xor_kernel",
           "lc3_fec_fill_kernel", "lc3_fec_rec_bytes_kernel", "lc3_fec_rec_scatter_kernel", "lc3_fec_rec_verdict_kernel"]
SENTINEL = {np.int64: 0x5A5A5A5A5A5A5A5A, np.int32: 0x5A5A5A5A, np.uint8: 0x5A}
# packets -> (routes, frames per call)
SHAPES = {1: (1, 1), 63: (7, 9), 64: (4, 16), 65: (5, 13), 257: (257, 1), 1025: (41, 25)}


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


@pytest.fixture(scope="module")
def decs():
    """decoder batches by their number of streams (the recover call reads it), made once"""
    made = {}

    def get(S):
        if S not in made:
            made[S] = _amd().DecBatch(S, 48000, 1, 10.0, 0, None, device=0)
        return made[S]
    yield get
    for d in made.values():
        d.close()


@pytest.fixture
def dec(decs):
    return decs(4)


def _u32(a):
    return (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _same(got, want, name, keys=None):
    for k in keys or want:
        g, w = got[k], want[k]
        if w is None or np.isscalar(w):
            assert g == w, (name, k, g, w)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (name, k, "first differences at", bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _out(dev, n, dt):
    return dev.put(np.full(n + GUARD, SENTINEL[dt], dt))


def _back(dev, ptr, shape, dt, name):
    n = int(np.prod(shape))
    got = dev.get(ptr, (n + GUARD,), dt)
    assert (got[n:] == SENTINEL[dt]).all(), ("an element behind the output was written", name)
    return got[:n].reshape(shape)


def _plan_encode(c):
    return _amd().api.plan_fec_encode(c["pkt_route"], c["pkt_frame"], c["pkt_offset"], c["pkt_size"], c["wire"], c["n_frames"], c["seq_base"], c["group"],
                                      c["fec_seq_base"], c["fec_wire"], c["fec_stride"], c["header_room"], c["payload_room"], c["fec_header_room"], c["pkt_status"],
                                      c["n_packets"], c["route_stats"], c["flush"], c["state"], c["acc"], c["acc_stride"], c["max_fec_packets"], c["wire_capacity"],
                                      c["fec_capacity"])


def _encode(dev, bat, c, hip_stream=None, sync=True, seq_in_place=False):
    """the encode call on device buffers of its own: every output starts as the sentinel with GUARD elements behind it, the workspace as POISON -> the plan's dict,
    the records behind n_fec zero as the binding leaves them (on the device they must still hold the sentinel).  seq_in_place: the device array fec_seq_base is
    given as next_fec_seq too"""
    api = _amd().api
    R, T, Q = len(c["seq_base"]), c["n_frames"], c["max_fec_packets"]
    carry = c["state"] is not None
    A = c["acc_stride"] if carry else 0
    opt = lambda a, dt: None if a is None else dev.put(np.ascontiguousarray(a, dtype=dt))
    d = dict(n_packets=dev.put(np.array([c["n_packets"]], np.int64)), pkt_route=dev.put(c["pkt_route"]), pkt_frame=dev.put(c["pkt_frame"]),
             pkt_offset=dev.put(c["pkt_offset"]), pkt_size=dev.put(c["pkt_size"]), pkt_status=opt(c["pkt_status"], np.uint8),
             wire=dev.put(np.concatenate([c["wire"], np.zeros(8, np.uint8)])), seq_base=dev.put(_u32(c["seq_base"])), route_stats=opt(c["route_stats"], np.int32),
             group=dev.put(c["group"]), flush=opt(c["flush"], np.uint8), fec_seq_base=dev.put(_u32(c["fec_seq_base"])), state_in=opt(c["state"], np.int32),
             acc_in=opt(c["acc"], np.uint8), fec_wire=dev.put(np.concatenate([c["fec_wire"], np.full(8, ref.FILL, np.uint8)])))
    types = dict(n_fec=((1,), np.int64), fec_route=((Q,), np.int32), fec_seq=((Q,), np.int32), fec_frame=((Q,), np.int32), fec_offset=((Q,), np.int64),
                 fec_size=((Q,), np.int32), fec_flags=((Q,), np.uint8), fec_mask=((Q,), np.int32), next_fec_seq=((R,), np.int32), route_stats=((R, 4), np.int32))
    if carry:
        types.update(state=((R, 8), np.int32), acc=((R, A), np.uint8))
    o = {k: _out(dev, int(np.prod(s)), dt) for k, (s, dt) in types.items()}
    work = dev.put(np.full(api.fec_work_bytes(R, T) + 8, POISON, np.uint8))
    bat.fec_encode_device(len(c["pkt_route"]), d["n_packets"], d["pkt_route"], d["pkt_frame"], d["pkt_offset"], d["pkt_size"], d["wire"], c["wire_capacity"], R, T,
                          d["seq_base"], d["group"], d["fec_seq_base"], d["fec_wire"], c["fec_capacity"], c["fec_stride"], Q, o["n_fec"], o["fec_route"], o["fec_seq"],
                          o["fec_frame"], o["fec_offset"], o["fec_size"], work, c["header_room"], c["payload_room"], c["fec_header_room"], d["pkt_status"],
                          d["route_stats"], d["flush"], d["state_in"], d["acc_in"], o.get("state"), o.get("acc"), A, o["fec_flags"], o["fec_mask"],
                          d["fec_seq_base"] if seq_in_place else o["next_fec_seq"], o["route_stats"], hip_stream, sync)
    if not sync:
        dev.sync()
    got = {k: _back(dev, o[k], s, dt, k) for k, (s, dt) in types.items()}
    got["n_fec"] = int(got["n_fec"][0])
    if seq_in_place:
        assert (got["next_fec_seq"] == SENTINEL[np.int32]).all()
        got["next_fec_seq"] = dev.get(d["fec_seq_base"], (R,), np.int32)
    nq = min(got["n_fec"], Q)
    for k in ("fec_route", "fec_seq", "fec_frame", "fec_offset", "fec_size", "fec_flags", "fec_mask"):
        assert (got[k][nq:] == SENTINEL[types[k][1]]).all(), ("a record behind n_fec was written", k)
        got[k][nq:] = 0
    fw = dev.get(d["fec_wire"], (len(c["fec_wire"]) + 8,), np.uint8)
    assert (fw[len(c["fec_wire"]):] == ref.FILL).all()
    got["fec_wire"] = fw[:len(c["fec_wire"])]
    got.setdefault("state", None), got.setdefault("acc", None)
    assert np.array_equal(dev.get(d["wire"], (len(c["wire"]),), np.uint8), c["wire"]), "the wire buffer was modified"
    if carry:
        assert np.array_equal(dev.get(d["acc_in"], (R, A), np.uint8), c["acc"]) and np.array_equal(dev.get(d["state_in"], (R, 8), np.int32), c["state"]), "an input was modified"
    return got


def _case(n, group, call=0, **kw):
    R, T = SHAPES[n]
    g = [(1, 5, 16, 0, 3)[r % 5] for r in range(R)] if group == "mixed" else group
    c = ref.encode_case(1000 * n + call, R, T, g, align=(1, 4)[call & 1], holes=0.0, **kw)
    assert len(c["pkt_route"]) - 3 >= n
    return dict(c, n_packets=n)                                       # exactly n list entries: with the doubles and the refused ones among them, the last cells are holes


@pytest.mark.parametrize("n", sorted(SHAPES))
@pytest.mark.parametrize("group", [1, 5, 16, "mixed"])
def test_encode_equals_the_host_plan(dev, dec, n, group):
    """two consecutive calls through the state buffers, the second with counts and a flush, then one call without state: every output, the whole FEC buffer, state
    and accumulator; nothing of fec_wire outside the written packets changes"""
    R, T = SHAPES[n]
    st = (None, None)
    written = 0
    for call in range(2):
        counts = [(T, 0, T - 1, 1)[r % 4] for r in range(R)] if call else None
        c = ref.with_state(_case(n, group, call, counts=counts, flush=[r & 1 for r in range(R)] if call else None), *st, acc_stride=416)
        want = _plan_encode(c)
        got = _encode(dev, dec, c)
        _same(got, want, (n, group, call))
        assert (got["fec_wire"][~ref.owned(c, got)] == ref.FILL).all()
        st = (got["state"], got["acc"])
        written += int(got["route_stats"][:, 1].sum())
    c = _case(n, group, 2)
    _same(_encode(dev, dec, c), _plan_encode(c), (n, group, "no state"))
    assert written > 0 or group == 16 or n == 1


def test_a_chain_of_one_frame_calls(dev, dec):
    """twenty calls of one frame each, six routes with groups of 1, 2, 5, 16, 0 and 3, the group sizes changing at call 9 while groups are open: each call equals
    the plan, and the packets of the chain are those of one twenty-frame call over the same packets"""
    api = _amd().api
    R, calls = 6, 20
    rng = np.random.RandomState(3)
    sizes = rng.randint(20, 401, (R, calls))
    present = rng.rand(R, calls) > 0.15
    pk = [[ref.rtp_packet(rng, 65530 + 100 * r + t, 12 + int(sizes[r, t])) for t in range(calls)] for r in range(R)]
    seq_base = (65530 + 100 * np.arange(R)) & 0xFFFF
    st, fec_seq, packets = (None, None), 7 + np.arange(R), [[] for _ in range(R)]
    for t in range(calls):
        group = [1, 2, 5, 16, 0, 3] if t < 9 else [2, 5, 1, 16, 4, 0]
        rows = [r for r in range(R) if present[r, t]]
        wire = np.frombuffer(b"".join(pk[r][t] for r in rows) + bytes(4), np.uint8)
        off = np.cumsum([0] + [len(pk[r][t]) for r in rows])[:len(rows)]
        c = dict(pkt_route=np.array(rows + [0], np.int32), pkt_frame=np.zeros(len(rows) + 1, np.int32), pkt_offset=np.append(off, 0).astype(np.int64),
                 pkt_size=np.array([len(pk[r][t]) for r in rows] + [0], np.int32), pkt_status=None, n_packets=len(rows), wire=wire, wire_capacity=len(wire) - 4, header_room=12,
                 payload_room=0, n_frames=1, seq_base=(seq_base + t) & 0xFFFF, route_stats=None, group=np.array(group, np.int32),
                 flush=np.ones(R, np.uint8) if t == calls - 1 else None, fec_seq_base=fec_seq, fec_wire=np.full(R * 448 + 5, ref.FILL, np.uint8), fec_capacity=R * 448,
                 fec_stride=448, fec_header_room=12, max_fec_packets=R)
        c = ref.with_state(c, *st, acc_stride=400)
        want = _plan_encode(c)
        got = _encode(dev, dec, c)
        _same(got, want, t)
        for q in range(got["n_fec"]):
            if not got["fec_flags"][q]:
                a = int(got["fec_offset"][q])
                packets[got["fec_route"][q]].append(got["fec_wire"][a + 12:a + got["fec_size"][q]].tobytes())
        st, fec_seq = (got["state"], got["acc"]), got["next_fec_seq"]
    assert not st[0][:, 0].any(), "the flush left a group open"
    # by hand: route 1 opens groups of 2 at calls 0, 2, 4, 6, 8 - the one open at call 9 closes with its own size - and groups of 5 at calls 10 and 15
    want = []
    for t, k in [(t, 2) for t in range(0, 10, 2)] + [(10, 5), (15, 5)]:
        members = [(pk[1][t + i], i) for i in range(k) if present[1, t + i]]
        if members:
            want.append(ref.fec_packet([m for m, _ in members], int(seq_base[1]) + t, [i for _, i in members]))
    assert packets[1] == want


def test_next_fec_seq_in_place(dev, dec):
    """calls of 3 frames with groups of 2 close 1, 2, 1, 2 groups a route; 1 100 routes, so that the scan has a second tile: with the device array fec_seq_base
    given as next_fec_seq too, every call gives what the plan gives with an array of its own, and a route's FEC packets are numbered without a step or a repeat"""
    R, T = 1100, 3
    st, seq, numbers = (None, None), 900 + 7 * np.arange(R), [[] for _ in range(R)]
    for call in range(4):
        c = ref.encode_case(70 + call, R, T, 2, hostile=False, lo=20, hi=60, seq_base=(50 + 13 * np.arange(R) + call * T) & 0xFFFF, fec_seq_base=seq)
        c = ref.with_state(c, *st, acc_stride=64)
        want = _plan_encode(c)
        got = _encode(dev, dec, c, seq_in_place=True)
        _same(got, want, call)
        for q in range(got["n_fec"]):
            numbers[got["fec_route"][q]].append(int(got["fec_seq"][q]))
        st, seq = (got["state"], got["acc"]), got["next_fec_seq"]
    assert numbers == [list(range(900 + 7 * r, 900 + 7 * r + 6)) for r in range(R)]


def test_the_convenience_calls(dev, decs):
    """Batch.fec_encode, DecBatch.fec_encode and DecBatch.fec_recover - the arrays uploaded, the call, the arrays downloaded - with the workspace filled with POISON:
    what the plans give, next_fec_seq in place included"""
    enc = _amd().Batch(2, 48000, 1, 10.0, 0, [64000] * 2, device=0)
    st = (None, None)
    for call, bat in enumerate((enc, decs(2), enc)):
        c = ref.with_state(_case(65, "mixed", call), *st, acc_stride=416)
        want = _plan_encode(c)
        got = bat.fec_encode(c["pkt_route"], c["pkt_frame"], c["pkt_offset"], c["pkt_size"], c["wire"], c["n_frames"], c["seq_base"], c["group"], c["fec_seq_base"],
                             c["fec_wire"], c["fec_stride"], c["header_room"], c["payload_room"], c["fec_header_room"], c["pkt_status"], c["n_packets"], c["route_stats"],
                             c["flush"], c["state"], c["acc"], c["acc_stride"], c["max_fec_packets"], c["wire_capacity"], c["fec_capacity"], poison_work=POISON,
                             seq_in_place=call == 2)
        _same(got, want, ("fec_encode()", call))
        st = (got["state"], got["acc"])
    enc.close()
    r, lost = ref.recover_case(8, 2, 9, 4, lambda s, g: [g % 4] if g % 3 else [])
    got = decs(2).fec_recover(r["ring"], r["dg_offsets"], r["dg_sizes"], r["stream"], r["seq"], r["fec_stream"], r["fec_offsets"], r["fec_num_bytes"], r["ssrc"],
                              r["rec_offset"], r["rec_stride"], r["window"], r["ring_capacity"], poison_work=POISON)
    _same(got, _plan_recover(r), "fec_recover()")
    assert got["stats"][ref.RECOVERED] == sum(len(x) == 1 for x in lost) > 0


def _plan_recover(c):
    return _amd().api.plan_fec_recover(c["n_streams"], c["ring"], c["dg_offsets"], c["dg_sizes"], c["stream"], c["seq"], c["fec_stream"], c["fec_offsets"],
                                       c["fec_num_bytes"], c["ssrc"], c["rec_offset"], c["rec_stride"], c["window"], c["ring_capacity"])


def _recover(dev, bat, c, hip_stream=None, sync=True):
    api = _amd().api
    n, m = len(c["stream"]), len(c["fec_stream"])
    ring = dev.put(np.concatenate([c["ring"], np.full(8, ref.FILL, np.uint8)]))
    d = [dev.put(c[k]) for k in ("dg_offsets", "dg_sizes", "stream")] + [dev.put(_u32(c["seq"]))] + [dev.put(c[k]) for k in ("fec_stream", "fec_offsets", "fec_num_bytes")]
    ssrc = dev.put(_u32(c["ssrc"]))
    types = dict(rec_dg_offsets=((m,), np.int64), rec_dg_sizes=((m,), np.int32), rec_seq=((m,), np.int32), status=((m,), np.uint8), stats=((16,), np.int32))
    o = {k: _out(dev, int(np.prod(s)), dt) for k, (s, dt) in types.items()}
    work = dev.put(np.full(api.fec_recover_work_bytes(c["n_streams"], c["window"]) + 8, POISON, np.uint8))
    bat.fec_recover_device(n, ring, c["ring_capacity"], d[0], d[1], d[2], d[3], m, d[4], d[5], d[6], c["window"], ssrc, c["rec_offset"], c["rec_stride"],
                           o["rec_dg_offsets"], o["rec_dg_sizes"], o["rec_seq"], work, o["status"], o["stats"], hip_stream, sync)
    if not sync:
        dev.sync()
    got = {k: _back(dev, o[k], s, dt, k) for k, (s, dt) in types.items()}
    r = dev.get(ring, (len(c["ring"]) + 8,), np.uint8)
    assert (r[len(c["ring"]):] == ref.FILL).all()
    got["ring"] = r[:len(c["ring"])]
    return got


def test_recover_on_crafted_items(dev, decs):
    c, lab = ref.crafted_recover()
    dec = decs(c["n_streams"])
    want = _plan_recover(c)
    assert all(want["status"][f] == st for f, st in lab.values())
    _same(_recover(dev, dec, c), want, "crafted")
    _same(_recover(dev, dec, c, hip_stream=dev.stream(), sync=False), want, "second stream")


@pytest.mark.parametrize("shape", [(1, 1, 1, 2), (63, 3, 21, 1), (64, 4, 1, 16), (65, 1, 13, 5), (257, 1, 257, 1), (1025, 1, 205, 5), (1024, 4, 16, 16)])
def test_recover_equals_the_host_plan(dev, decs, shape):
    """n media packets sent in groups of k, of which no, one or two a group are lost, the datagram list shuffled: every output and the whole ring, the recovery region with
    it; a recovered packet is the lost one but for its SSRC field, which is the table's"""
    n, S, G, k = shape
    rng = np.random.RandomState(n)
    pick = {(s, g): sorted(rng.choice(k, min(k, int(rng.randint(0, 3))), replace=False).tolist()) if n > 1 else [0] for s in range(S) for g in range(G)}
    c, lost = ref.recover_case(n, S, G, k, lambda s, g: pick[(s, g)], long_mask=n == 65, window=2048 if G * k > 1024 else 1024)
    want = _plan_recover(c)
    got = _recover(dev, decs(S), c)
    _same(got, want, shape)
    for f, gone in enumerate(lost):
        assert got["status"][f] == (ref.COMPLETE, ref.RECOVERED, ref.MISSING)[len(gone)]
        if len(gone) == 1:
            a = int(got["rec_dg_offsets"][f])
            assert got["ring"][a:a + got["rec_dg_sizes"][f]].tobytes() == gone[0], f
    slots = got["ring"][c["rec_offset"]:c["rec_offset"] + len(lost) * c["rec_stride"]].reshape(len(lost), c["rec_stride"])
    assert (slots[got["rec_dg_sizes"] == 0] == ref.FILL).all()


def test_every_fec_kernel_ran_under_a_comparison(dev, dec, decs):
    """the sibling library counts its launches: every kernel its code object holds has run - here, once more, under a comparison - no kernel uses scratch, and a
    name the library does not hold is answered with -1"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels
    table = kernels(LIB, "gfx950")
    assert sorted(table) == KERNELS and all(v[3] == 0 for v in table.values()), table          # v[3]: the bytes of scratch
    before = {k: sibling_launches("fec", k) for k in KERNELS}
    c = ref.with_state(_case(65, 5), acc_stride=416)
    _same(_encode(dev, dec, c), _plan_encode(c), "encode")
    r, _ = ref.recover_case(5, 2, 6, 4, lambda s, g: [g % 4])
    _same(_recover(dev, decs(2), r), _plan_recover(r), "recover")
    for k in KERNELS:
        assert sibling_launches("fec", k) == before[k] + (2 if k == "lc3_fec_fill_kernel" else 1), k
    assert sibling_launches("fec", "lc3_red_copy_kernel") == -1


@pytest.mark.parametrize("drops", [1, 2])
def test_sender_to_receiver_through_dropped_packets(dev, drops):
    """encode_device_packed, egress into a wire buffer, stamp, fec_encode (groups of 4), stamp of the FEC list, the sizes of `drops` media packets of one group per
    stream overwritten with -1 by an asynchronous copy (the parse refuses them: never arrived), parse of the media and of the FEC datagrams, fec_recover, parse of
    the recovered datagrams behind the media items, probe, ingest, set_frame_counts + decode_device_packed: 48k_10_128B, 4 streams x 16 frames, all queued on one
    HIP stream with sync = 0 and one wait at the end.  One drop a group: no cell is a gap and PCM and status equal the oracle decoder's over the loss-free
    frames.  Two drops in a group: exactly those frames are concealed."""
    api = _amd().api
    geom = "48k_10_128B"
    fs, ms, hr, ch, sizes = hf.GEOMS[geom]
    S, T, N, size, k = 4, 16, hf.frame_len(fs, ms), int(sizes[0]), 4
    room, n, nf = 12, S * T, S * T // k
    pkt = room + size
    W, fstride = n * pkt, (12 + 14 + size + 15) & ~15
    F, rstride = nf * fstride, (pkt + 3) & ~3
    cap = W + F + nf * rstride
    pcm_in = synth_pcm(S, T, N, fs, seed=43).reshape(S, T, ch, N)
    buf = n * size + 64
    enc = _amd().Batch(S, fs, ch, ms, hr, [size * 800] * S, device=0)
    dec = _amd().DecBatch(S, fs, ch, ms, hr, None, device=0)
    i32, i64, u8 = (lambda k_, v=-7: dev.put(np.full(k_, v, np.int32))), (lambda k_, v=-7: dev.put(np.full(k_, v, np.int64))), (lambda k_, v=0xEE: dev.put(np.full(k_, v, np.uint8)))
    d_pcm_in, d_out = dev.put(pcm_in), u8(buf, 0xC3)
    d_off, d_tot, d_nb, d_fl = i64((S, T)), i64(1), i32((S, T)), u8((S, T))
    seq_base = (65530 + np.arange(S)).astype(np.int32)
    ssrc, fssrc, ts_base = 0x7FFFFFF0 + 7 * np.arange(S), 0x100 + np.arange(S), 0xFFFFF000 + 100000 * np.arange(S)
    d_base, d_ssrc, d_fssrc, d_tsb = dev.put(seq_base), dev.put(_u32(ssrc)), dev.put(_u32(fssrc)), dev.put(_u32(ts_base))
    d_pt, d_fpt, d_sid = dev.put(np.full(S, 96, np.int32)), dev.put(np.full(S, 97, np.int32)), dev.put(np.arange(S, dtype=np.int32))
    d_ring = u8(cap + 8, ref.FILL)
    d_fwire = d_ring + W
    p_route, p_seq, p_frame, p_off, p_size, p_flags = i32(n), i32(n), i32(n), i64(n, -1), i32(n, 0), u8(n)
    d_np, d_next, d_stats, d_cs = i64(1), i32(S), i32((S, 4)), u8((S, T))
    e_work = dev.put(np.zeros(api.egress_work_bytes(S, T) // 8 + 1, np.int64))
    d_pst, d_nts = u8(n), i32(S)
    d_group, d_fbase = dev.put(np.full(S, k, np.int32)), dev.put(np.full(S, 500, np.int32))
    f_n, f_route, f_seq, f_frame, f_off, f_size, f_flags, f_mask, f_next, f_stats = i64(1), i32(nf), i32(nf), i32(nf), i64(nf, -1), i32(nf, 0), u8(nf), i32(nf), i32(S), i32((S, 4))
    f_work = dev.put(np.full(api.fec_work_bytes(S, T) + 8, POISON, np.uint8))
    f_pst = u8(nf)
    f_dg = dev.put(W + fstride * np.arange(nf, dtype=np.int64))           # where the receiver finds the FEC datagrams in its ring
    m = n + nf
    i_stream, i_seq, i_off, i_nb, i_st = i32(m), i32(m), i64(m), i32(m), u8(m)
    g_stream, g_seq, g_off, g_nb, g_st = i32(nf), i32(nf), i64(nf), i32(nf), u8(nf)
    r_off, r_size, r_seq, r_st, r_stats = i64(nf), i32(nf), i32(nf), u8(nf), i32(16)
    r_work = dev.put(np.full(api.fec_recover_work_bytes(S, 64) + 8, POISON, np.uint8))
    d_info = dev.put(np.zeros((m, ch, api.FRAME_INFO_WORDS), np.int32))
    d_oo, d_onb, d_ci, d_cnt2, d_nb2, d_ist = i64((S, T)), i32((S, T)), i32((S, T)), i32(S), i32(S), i32((S, 4))
    d_pcm, d_st = dev.put(np.full((S, T, ch, N), 0x5555, np.int16)), u8((S, T))
    lost = np.zeros((S, T), bool)
    for s in range(S):                                                # group s of stream s loses its position s; with two drops two of its first three (the last
        for j in range(drops):                                        # frame of a call has to arrive for the ingest to count up to it)
            lost[s, 4 * s + (s if drops == 1 else (s + j) % 3)] = True
    gone = dev.pin(np.full(1, -1, np.int32))
    dev.sync()
    s1 = dev.stream()
    enc.encode_device_packed(d_pcm_in, 16, T, d_out, buf, api.PACK_STREAM_MAJOR, None, None, d_off, d_tot, d_nb, d_fl, s1, sync=False)
    enc.egress_device(T, d_out, buf, d_off, d_nb, size, S, d_base, p_route, p_seq, p_frame, p_off, p_size, d_np, e_work, d_fl, api.ENC_FL_PACK_CAP, None, None, 16,
                      api.PACK_STREAM_MAJOR, d_ring, W, room, 1, p_flags, None, d_next, d_stats, d_cs, s1, sync=False)
    enc.rtp_stamp_device(n, d_np, p_route, p_seq, p_frame, p_off, p_size, S, T, d_ssrc, d_tsb, d_pt, N, d_ring, W, room, 0, p_flags, api.RTP_MARKER_NEVER, None, None,
                         d_stats, d_pst, d_nts, None, s1, sync=False)
    enc.fec_encode_device(n, d_np, p_route, p_frame, p_off, p_size, d_ring, W, S, T, d_base, d_group, d_fbase, d_fwire, F, fstride, nf, f_n, f_route, f_seq, f_frame, f_off,
                          f_size, f_work, room, 0, 12, d_pst, d_stats, None, None, None, None, None, 0, f_flags, f_mask, f_next, f_stats, s1, sync=False)
    enc.rtp_stamp_device(nf, f_n, f_route, f_seq, f_frame, f_off, f_size, S, T, d_fssrc, d_tsb, d_fpt, N, d_fwire, F, 12, 0, f_flags, api.RTP_MARKER_NEVER, None, None,
                         d_stats, f_pst, None, None, s1, sync=False)
    for s, t in np.argwhere(lost):                                    # stream-major, every cell SENT: packet s * T + t is frame t of stream s
        dev.copy_async(p_size + 4 * int(s * T + t), gone, s1)
    dec.rtp_parse_device(n, d_ring, cap, p_off, p_size, S, d_ssrc, d_sid, i_stream, i_seq, i_off, i_nb, d_pt, 0, None, None, i_st, None, s1, sync=False)
    dec.rtp_parse_device(nf, d_ring, cap, f_dg, f_size, S, d_fssrc, d_sid, g_stream, g_seq, g_off, g_nb, d_fpt, 0, None, None, g_st, None, s1, sync=False)
    dec.fec_recover_device(n, d_ring, cap, p_off, p_size, i_stream, i_seq, nf, g_stream, g_off, g_nb, 64, d_ssrc, W + F, rstride, r_off, r_size, r_seq, r_work, r_st,
                           r_stats, s1, sync=False)
    dec.rtp_parse_device(nf, d_ring, cap, r_off, r_size, S, d_ssrc, d_sid, i_stream + 4 * n, i_seq + 4 * n, i_off + 8 * n, i_nb + 4 * n, d_pt, 0, None, None, i_st + n, None,
                         s1, sync=False)
    dec.probe_device(d_ring, cap, i_off, i_nb, size, m, d_info, api.PROBE_FULL, s1, sync=False)
    dec.ingest_device(m, i_stream, i_seq, i_off, i_nb, d_base, T, d_oo, d_onb, d_ci, d_cnt2, 16, d_info, None, d_nb2, d_ist, None, s1, sync=False)
    dec.set_frame_counts(d_cnt2)
    dec.decode_device_packed(d_ring, cap, d_oo, T, d_pcm, d_onb, size, None, d_st, 16, s1, sync=False)
    dev.stream_sync(s1)
    # the sender: every group closed, every FEC packet stamped, and the FEC buffer is the plan's over the stamped wire buffer
    assert int(dev.get(d_np, (1,), np.int64)[0]) == n and int(dev.get(f_n, (1,), np.int64)[0]) == nf and (dev.get(d_pst, (n,), np.uint8) == 1).all()
    assert (dev.get(f_pst, (nf,), np.uint8) == 1).all() and not dev.get(f_flags, (nf,), np.uint8).any() and (dev.get(f_mask, (nf,), np.int32) == 0xF000).all()
    ring = dev.get(d_ring, (cap + 8,), np.uint8)
    frames, off = dev.get(d_out, (buf,), np.uint8), dev.get(d_off, (S, T), np.int64)
    want = api.plan_fec_encode(np.repeat(np.arange(S), T), np.tile(np.arange(T), S), pkt * np.arange(n), np.full(n, pkt), ring[:W], T, seq_base, np.full(S, k), np.full(S, 500),
                               np.full(F, ref.FILL, np.uint8), fstride, room, max_fec_packets=nf)
    blank = ring[W:W + F].copy()
    for q in range(nf):
        blank[q * fstride:q * fstride + 12] = ref.FILL                # the stamp's bytes
    assert np.array_equal(blank, want["fec_wire"]) and np.array_equal(dev.get(f_size, (nf,), np.int32), want["fec_size"])
    assert np.array_equal(dev.get(f_seq, (nf,), np.int32), want["fec_seq"]) and np.array_equal(dev.get(f_stats, (S, 4), np.int32), want["route_stats"])
    # the receiver
    st = dev.get(i_st, (m,), np.uint8)
    assert np.array_equal(st[:n] != 0, lost.ravel()) and not dev.get(g_st, (nf,), np.uint8).any()
    rst = dev.get(r_st, (nf,), np.uint8).reshape(S, T // k)
    hit = lost.reshape(S, T // k, k).sum(axis=2)
    assert np.array_equal(rst, np.where(hit == 0, api.FEC_COMPLETE, np.where(hit == 1, api.FEC_RECOVERED, api.FEC_MISSING)))
    assert np.array_equal(st[n:] == 0, (rst == api.FEC_RECOVERED).ravel())
    ist, counts2, onb = dev.get(d_ist, (S, 4), np.int32), dev.get(d_cnt2, (S,), np.int32), dev.get(d_onb, (S, T), np.int32)
    gaps = lost if drops == 2 else np.zeros((S, T), bool)
    assert (counts2 == T).all() and np.array_equal(ist[:, 1], gaps.sum(axis=1)) and np.array_equal(onb, np.where(gaps, 0, size))
    oo = dev.get(d_oo, (S, T), np.int64)
    for s in range(S):
        for t in range(T):
            if not gaps[s, t]:
                assert np.array_equal(ring[oo[s, t]:oo[s, t] + size], frames[off[s, t]:off[s, t] + size]), (s, t)
    if drops == 1:                                                    # a recovered packet is the sent one, header and all
        for s in range(S):
            f, p = s * (T // k) + s, s * T + 4 * s + s
            a = W + F + f * rstride
            assert np.array_equal(ring[a:a + pkt], ring[p * pkt:(p + 1) * pkt]), s
    fr = np.stack([[frames[off[s, t]:off[s, t] + size] for t in range(T)] for s in range(S)])
    o = hf.decode(geom, fr, np.where(gaps, 0, size), np.zeros((S, T), np.uint8))
    pcm, dst = dev.get(d_pcm, (S, T, ch, N), np.int16), dev.get(d_st, (S, T), np.uint8)
    assert np.array_equal(dst, o["status"]) and np.array_equal(dst != 0, gaps)
    bad = np.argwhere((pcm != o["pcm"]).any(axis=(2, 3)))
    assert len(bad) == 0, ("first differing (stream, frame)", bad[:4].tolist())
    enc.close()
    dec.close()
