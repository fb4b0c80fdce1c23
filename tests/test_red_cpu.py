"""Redundant audio without a GPU (include/lc3plus_batch.h "Redundant audio"): the exported symbols and constants, every refusal of the three batch calls in the
header's order (their checks run before anything of the batch or the device is touched), lc3plus_plan_red_pack and lc3plus_plan_red_unpack - the text the kernels
run - against the restatement of the rules (red_ref.pack, red_ref.unpack) on every output, one packet written out by hand, the host round trip through dropped
bursts over three consecutive calls, and the host code once more in a program of its own under AddressSanitizer + UndefinedBehaviorSanitizer
(tools/red_plan_driver.c).  Every comparison is equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import audio_codec_amd
from audio_codec_amd import api
import red_ref as ref

NEW = ["lc3plus_enc_batch_red_pack", "lc3plus_dec_batch_red_pack", "lc3plus_plan_red_pack", "lc3plus_red_work_bytes", "lc3plus_dec_batch_red_unpack",
       "lc3plus_plan_red_unpack"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_codec_amd", "csrc")
LC3_OK, LC3_ERROR, LC3_NULL_ERROR = 0, 1, 3
K_ARGS = ("n_frames", "frames", "frames_capacity", "offsets", "num_bytes", "max_frame_bytes", "flags", "skip_mask", "counts", "n_routes", "route_src", "max_packets",
          "n_packets", "pkt_route", "pkt_frame", "max_depth", "depth", "block_pt", "ts_step", "max_packet_bytes", "tail_bytes_in", "tail_sizes_in", "tail_stride",
          "tail_bytes_out", "tail_sizes_out", "wire", "wire_capacity", "header_room", "align", "red_offset", "red_size", "red_flags", "red_blocks", "wire_total",
          "route_stats", "work", "hip_stream", "sync")
K_REQUIRED = ("frames", "offsets", "num_bytes", "n_packets", "pkt_route", "pkt_frame", "block_pt", "wire", "red_offset", "red_size", "work")
K_NULLABLE = ("flags", "counts", "depth", "red_flags", "red_blocks", "wire_total", "route_stats")
K_VALUES = dict(n_frames=1, frames_capacity=100, max_frame_bytes=40, skip_mask=0, n_routes=1, max_packets=1, max_depth=1, ts_step=480, max_packet_bytes=1400, tail_stride=48,
                wire_capacity=100, header_room=12, align=1, hip_stream=None, sync=1)
K_BAD = (dict(n_frames=0), dict(n_frames=-1), dict(n_routes=0), dict(max_frame_bytes=0), dict(frames_capacity=-1), dict(wire_capacity=-1), dict(max_packets=0),
         dict(max_packets=-1), dict(max_packets=1 << 31), dict(max_depth=-1), dict(max_depth=5), dict(ts_step=0), dict(ts_step=-480), dict(max_packet_bytes=-1),
         dict(tail_bytes_in=None), dict(tail_sizes_in=None), dict(tail_bytes_out=None), dict(tail_sizes_out=None), dict(tail_stride=40), dict(tail_stride=32),
         dict(tail_stride=0), dict(max_frame_bytes=2000, tail_stride=1008), dict(header_room=-1), dict(header_room=(1 << 31) - 1), dict(align=0), dict(align=3),
         dict(align=8192), dict(n_routes=2, route_src=None), dict(work="odd"), dict(n_frames=0, max_depth=9))
U_ARGS = ("n_items", "stream", "seq", "offsets", "num_bytes", "timestamp", "ring", "ring_capacity", "max_red", "block_pt", "ts_step", "out_stream", "out_seq",
          "out_offsets", "out_num_bytes", "out_timestamp", "out_gen", "status", "stats", "hip_stream", "sync")
U_REQUIRED = ("stream", "seq", "offsets", "num_bytes", "ring", "out_stream", "out_seq", "out_offsets", "out_num_bytes")
U_NULLABLE = ("timestamp", "block_pt", "out_timestamp", "out_gen", "status", "stats")
U_VALUES = dict(n_items=1, ring_capacity=100, max_red=1, ts_step=480, hip_stream=None, sync=1)
U_BAD = (dict(n_items=0), dict(n_items=-1), dict(n_items=1 << 29), dict(ring_capacity=-1), dict(max_red=-1), dict(max_red=5), dict(ts_step=0), dict(ts_step=-1),
         dict(n_items=0, max_red=7))


def test_symbols_are_exported():
    L = audio_codec_amd.load_library()
    text = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    for s in NEW:
        assert s in api.EXPORTS and hasattr(L, s) and re.search(r"\b%s\s*\(" % s, text), s
    for cls in (api.Batch, api.DecBatch):
        assert callable(cls.red_pack_device)
    assert callable(api.DecBatch.red_unpack_device) and callable(api.DecBatch.red_unpack) and callable(api.plan_red_pack) and callable(api.plan_red_unpack)
    assert os.path.exists(os.path.join(ROOT, "audio_codec_amd", "liblc3plus_red_hip.so"))
    assert "several frames per packet are not handled" not in text.replace("\n * ", " ") and 'Redundant audio' in text


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define\s+LC3PLUS_RED_(\w+)\s+(\d+)", text)}
    want = dict(MAX_DEPTH=4, PKT_BAD=2, STATS_WORDS=4, OK=0, DROPPED=1, RANGE=2, SHORT=3, DEPTH=4, LENGTH=5, PAYLOAD_TYPE=6, DROP_TYPE=8, DROP_OFFSET=9, DROP_EMPTY=10,
                UNPACK_STATS_WORDS=16)
    assert header == want
    for k, v in want.items():
        assert getattr(api, "RED_" + k) == v == getattr(ref, k), k
    assert api.EGR_PKT_OVERFLOW == ref.PKT_OVERFLOW and api.RED_PKT_BAD != api.EGR_PKT_OVERFLOW
    assert api.RED_UNPACK_OUTPUTS == ref.UNPACK_KEYS and set(api.RED_PACK_OUTPUTS) < set(ref.PACK_KEYS)
    shim = open(os.path.join(CSRC, "lc3_red_shim.h")).read()
    assert '#include "lc3_egress_shim.h"' in shim and not re.search(r"\blc3e_(route|class|copy_layout)\s*\([^;{]*\)\s*\{", shim), "the egress's rules are restated"
    assert api.red_work_bytes(0) == 0 and api.red_work_bytes(1 << 31) == 0 and api.red_work_bytes(1) > 0 and api.red_work_bytes(1025) % 8 == 0


def _refusals(call, required, nullable, bad):
    """call(**overrides) -> the return code; the arguments are good unless overridden"""
    for k in required:
        assert call(**{k: None}) == LC3_NULL_ERROR, k
    for k in nullable:
        for kw in bad[:2]:
            assert call(**dict(kw, **{k: None})) == LC3_ERROR, (k, kw)                # an optional NULL is no refusal: the value check behind it answers
    for kw in bad:
        assert call(**kw) == LC3_ERROR, kw
    for k in required:                                                                 # NULL first
        assert call(**dict(bad[0], **{k: None})) == LC3_NULL_ERROR, k
        assert call(**dict(bad[-1], **{k: None})) == LC3_NULL_ERROR, k


def _good(args, values, arr, **more):
    p = C.cast(arr, C.c_void_p)
    return dict({k: p for k in args}, **values, **more)


def _args(a, names):
    a = dict(a)
    if a.get("work") == "odd":
        a["work"] = C.c_void_p(a["frames"].value + 4)
    return [a[k] for k in names]


@pytest.mark.parametrize("name", ["lc3plus_enc_batch_red_pack", "lc3plus_dec_batch_red_pack"])
def test_pack_refusals_need_no_device(name):
    """a zero-filled block stands in for the batch: no refusal writes to it or to an array"""
    L = audio_codec_amd.load_library()
    fake, arr = C.create_string_buffer(4096), C.create_string_buffer(256)
    good = _good(K_ARGS, K_VALUES, arr, b=C.cast(fake, C.c_void_p))

    def call(**kw):
        a = dict(good, **kw)
        return getattr(L, name)(a["b"], *_args(a, K_ARGS))
    assert call(b=None) == LC3_NULL_ERROR and call(b=None, n_frames=0) == LC3_NULL_ERROR and call(b=None, wire=None, max_depth=9) == LC3_NULL_ERROR
    _refusals(call, K_REQUIRED, K_NULLABLE, K_BAD)
    assert fake.raw == bytes(4096) and arr.raw == bytes(256)


def test_unpack_refusals_need_no_device():
    L = audio_codec_amd.load_library()
    fake, arr = C.create_string_buffer(4096), C.create_string_buffer(256)
    good = _good(U_ARGS, U_VALUES, arr, b=C.cast(fake, C.c_void_p))

    def call(**kw):
        a = dict(good, **kw)
        return L.lc3plus_dec_batch_red_unpack(a["b"], *[a[k] for k in U_ARGS])
    assert call(b=None) == LC3_NULL_ERROR and call(b=None, n_items=0) == LC3_NULL_ERROR and call(b=None, ring=None, max_red=9) == LC3_NULL_ERROR
    _refusals(call, U_REQUIRED, U_NULLABLE, U_BAD)
    assert fake.raw == bytes(4096) and arr.raw == bytes(256)


def test_plan_refusals():
    L = audio_codec_amd.load_library()
    arr = C.create_string_buffer(256)
    good = _good(K_ARGS, K_VALUES, arr, S=1)

    def pack(**kw):
        a = dict(good, **kw)
        return L.lc3plus_plan_red_pack(a["S"], *_args(a, K_ARGS))
    _refusals(pack, K_REQUIRED, K_NULLABLE, K_BAD)
    assert pack(S=0) == LC3_ERROR and pack(S=-1) == LC3_ERROR and pack(S=0, wire=None) == LC3_NULL_ERROR
    assert pack(S=2, route_src=None) == LC3_ERROR and pack(S=1, route_src=None) == LC3_OK and pack(S=2, n_routes=2) == LC3_OK      # the arrays of zeros are a good call
    assert pack(max_depth=0, tail_stride=7, tail_bytes_in=None, tail_sizes_in=None) == LC3_OK   # nothing of the tails is looked at without depth
    good = _good(U_ARGS, U_VALUES, arr, S=1)

    def unpack(**kw):
        a = dict(good, **kw)
        return L.lc3plus_plan_red_unpack(a["S"], *[a[k] for k in U_ARGS])
    _refusals(unpack, U_REQUIRED, U_NULLABLE, U_BAD)
    assert unpack(S=0) == LC3_ERROR and unpack(S=0, ring=None) == LC3_NULL_ERROR
    with pytest.raises(api.LC3Error):
        api.plan_red_unpack(1, [0], [0], [0], [4], np.zeros(8, np.uint8), 480, max_red=5)
    with pytest.raises(api.LC3Error):
        api.plan_red_pack(1, np.zeros(8, np.uint8), [[0]], [[4]], 40, [0], [0], [96], 480, np.zeros(64, np.uint8), max_depth=5)


def plan_pack(c, optional=api.RED_PACK_OPTIONAL):
    return api.plan_red_pack(c["n_streams"], c["frames"], c["offsets"], c["num_bytes"], c["max_frame_bytes"], c["pkt_route"], c["pkt_frame"], c["block_pt"], c["ts_step"],
                             c["wire"], c["max_depth"], c["depth"], c["max_packet_bytes"], c["n_packets"], c["flags"], c["skip_mask"], c["counts"], c["route_src"],
                             c["tail_bytes"], c["tail_sizes"], c["tail_stride"], c["wire_capacity"], c["header_room"], c["align"], optional, c["frames_capacity"])


def plan_unpack(c, optional=api.RED_UNPACK_OPTIONAL):
    return api.plan_red_unpack(c["n_streams"], c["stream"], c["seq"], c["offsets"], c["num_bytes"], c["ring"], c["ts_step"], c["max_red"], c["timestamp"], c["block_pt"],
                               optional, c["ring_capacity"])


def same(got, want, name, keys=None):
    for k in keys or want:
        g, w = got[k], want[k]
        if w is None or np.isscalar(w):
            assert g == w, (name, k, g, w)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (name, k, "first differences at", bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("n", [1, 40, 257, 1025])
def test_plan_pack_equals_the_rule(n):
    """the tables of red_ref.pack_tables through three consecutive calls, each call's tails the next call's history: every output, the whole wire buffer, both tail
    buffers; and what the tables are there to reach is reached"""
    tails = None
    seen_blocks, missed, over, flags = set(), 0, 0, set()
    for call in range(3):
        c = ref.pack_case(call, n, tails)
        c["tail_fill"] = np.zeros_like(c["tail_fill"])                # the binding's tail buffers start as zeros
        want = ref.pack(c)
        got = plan_pack(c)
        same(got, want, (n, call))
        assert (got["wire"][c["wire_capacity"]:] == ref.WIRE_FILL).all()
        own = np.zeros(c["wire"].size, bool)
        for p in range(n):
            if want["red_size"][p] and not want["red_flags"][p]:
                own[want["red_offset"][p] + c["header_room"]:want["red_offset"][p] + want["red_size"][p]] = True
        assert (got["wire"][~own] == ref.WIRE_FILL).all()
        assert (want["red_size"][n:] == 0).all() and (want["red_offset"][n:] == 0).all()
        seen_blocks |= set(want["red_blocks"][:n].tolist())
        missed += int(want["route_stats"][:, 3].sum())
        over += int((want["red_flags"][:n] == ref.PKT_OVERFLOW).sum())
        flags |= set(want["red_flags"][:n].tolist())
        tails = (got["tail_bytes"], got["tail_sizes"])
        if n == 40:
            for optional in ((),) + tuple((k,) for k in api.RED_PACK_OPTIONAL):
                g = plan_pack(c, optional)
                keys = ("red_offset", "red_size", "wire") + tuple(k for k in optional if k != "tail") + (("tail_bytes", "tail_sizes") if "tail" in optional else ())
                assert all(g[k] is None for k in ref.PACK_KEYS if k not in keys)
                same(g, want, (call, optional), keys)
    if n >= 40:
        assert {0, 1, 3, 7, 15} <= seen_blocks and missed > 0 and over > 0 and flags == {0, ref.PKT_OVERFLOW, ref.PKT_BAD}
        assert any(b not in (0, 1, 3, 7, 15) for b in seen_blocks), "no generation was skipped with a later one carried"


def test_pack_by_hand():
    """one packet written out: primary type 96, one block, ts_step 480.  Frame 1 of 3 bytes behind frame 0 of 2 bytes"""
    frames = np.frombuffer(b"\xAA\xBB\x01\x02\x03", np.uint8)
    r = api.plan_red_pack(1, frames, [[0, 2]], [[2, 3]], 40, [0, 0], [0, 1], [96], 480, np.full(64, ref.WIRE_FILL, np.uint8), max_depth=1, header_room=12, align=4)
    assert r["red_size"].tolist() == [12 + 1 + 2, 12 + 4 + 1 + 2 + 3] and r["red_offset"].tolist() == [0, 16] and r["red_blocks"].tolist() == [0, 1]
    w = r["wire"]
    assert w[12:15].tobytes() == bytes.fromhex("60aabb")
    # F | 96, offset 480 = 0b00000111100000 and length 2 = 0b0000000010 -> 0x07 0x80 0x02; then 0 | 96, the block, the primary
    assert w[16 + 12:16 + 22].tobytes() == bytes.fromhex("e0078002" "60" "aabb" "010203")
    assert (np.delete(w, np.r_[12:15, 28:38]) == ref.WIRE_FILL).all() and r["wire_total"] == 16 + 24
    assert r["route_stats"].tolist() == [[2, 1, 2, 0]] and r["tail_sizes"].tolist() == [[3]] and r["tail_bytes"][0, 0, :3].tobytes() == b"\x01\x02\x03"
    u = api.plan_red_unpack(1, [0, 0], [10, 11], [12, 28], [3, 10], w, 480, max_red=1, timestamp=[5000, 5480], block_pt=[96])
    assert u["status"].tolist() == [0, 0] and u["stream"].tolist() == [0, -1, 0, 0] and u["seq"].tolist() == [10, 0, 11, 10]
    assert u["offsets"].tolist() == [13, 0, 35, 33] and u["num_bytes"].tolist() == [2, 0, 3, 2] and u["timestamp"].tolist() == [5000, 0, 5480, 5000]
    assert u["gen"].tolist() == [0, 0, 0, 1] and u["stats"].tolist() == [2] + [0] * 15


@pytest.mark.parametrize("max_red", [4, 2, 0])
def test_plan_unpack_on_crafted_packets(max_red):
    c, lab = ref.crafted_unpack(max_red)
    want = ref.unpack(c)
    same(plan_unpack(c), want, max_red)
    st = lambda label: int(want["status"][lab[label]])
    K = max_red + 1
    assert all(st("valid%d_%d" % (k, a)) == (ref.OK if k <= max_red else ref.DEPTH) for k in range(5) for a in range(4))
    assert all(st("cut%d" % k) == ref.SHORT for k in range(17)) and st("cut17") == (ref.DEPTH if max_red < 4 else ref.LENGTH)
    assert st("five") == st("six") == ref.DEPTH and st("five_cut") == ref.SHORT and st("no_f") == ref.OK
    assert st("dropped") == st("stream_out") == ref.DROPPED and st("neg") == st("neg_size") == st("past") == st("huge") == ref.RANGE
    if max_red == 4:
        assert all(st("cut%d" % k) == ref.LENGTH for k in range(17, 17 + 20)) and st("cut39") == ref.OK and st("length") == st("length_big") == ref.LENGTH
        i = lab["valid4_1"]
        assert want["stream"][i * K:i * K + K].tolist() == [1] * 5 and want["gen"][i * K:i * K + K].tolist() == [0, 4, 3, 2, 1]
        assert want["num_bytes"][i * K:i * K + K].tolist() == [20, 7, 6, 5, 4]
        assert (want["seq"][i * K + 1:i * K + K] == (want["seq"][i * K] - np.array([4, 3, 2, 1])) & 0xFFFF).all()
        assert want["stats"][8:11].tolist() == [2, 4, 2] and st("pt") == ref.PAYLOAD_TYPE and st("pt_any") == st("empty_primary") == st("drop_all") == ref.OK
        i = lab["far"]
        assert want["gen"][i * K + 1] == 34 and want["seq"][i * K + 1] == (want["seq"][i * K] - 34) & 0xFFFF
        assert want["num_bytes"][lab["empty_primary"] * K] == 0 and want["stream"][lab["empty_primary"] * K] == 0
    bad = np.repeat(want["status"] != 0, K)
    assert (want["stream"][bad] == -1).all() and all((want[k][bad] == 0).all() for k in ("seq", "offsets", "num_bytes", "timestamp", "gen"))
    assert want["stats"][:8].sum() == len(c["stream"])
    for optional in ((),) + tuple((k,) for k in api.RED_UNPACK_OPTIONAL):
        got = plan_unpack(c, optional)
        assert all(got[k] is None for k in api.RED_UNPACK_OPTIONAL if k not in optional)
        same(got, want, optional, ref.UNPACK_KEYS[:4] + optional)
    same(plan_unpack(dict(c, timestamp=None, block_pt=None)), ref.unpack(dict(c, timestamp=None, block_pt=None)), "no timestamp, any type")


@pytest.mark.parametrize("max_red", [4, 1])
def test_plan_unpack_on_random_bytes(max_red):
    c = ref.random_unpack(1000, max_red=max_red)
    want = ref.unpack(c)
    assert all(want["stats"][k] > 0 for k in (0, 1, 3, 4, 5, 6, 8, 9, 10))
    same(plan_unpack(c), want, max_red)


def _round_trip(d, bursts, S=2, T=8, calls=3, size=40):
    """plan_egress (in place) -> plan_red_pack -> plan_rtp_stamp over `calls` consecutive calls with tails; the packets of `bursts` [(stream, first, length)], counted
    over all calls, are dropped; then one plan_rtp_parse -> plan_red_unpack -> plan_ingest over everything that arrived -> the ingest's result, and the frames sent"""
    rng = np.random.RandomState(d)
    room, N = 12, 480
    seq_base, ts_base = np.array([65530, 100]), np.array([0xFFFFF000, 7])
    ssrc = np.array([0x11111111, 0x22222222])
    lost = {(s, a + k) for s, a, n in bursts for k in range(n)}
    tails, ring, dg_off, dg_size, sent = None, [], [], [], []
    for call in range(calls):
        frames = rng.randint(0, 256, S * T * size).astype(np.uint8)
        off = (np.arange(S * T, dtype=np.int64) * size).reshape(S, T)
        nb = np.full((S, T), size, np.int32)
        sent.append(frames.reshape(S, T, size))
        e = api.plan_egress(S, frames, off, nb, seq_base, size)
        n = e["n_packets"]
        assert n == S * T
        wire = np.full(n * (room + 17 + 5 * size), ref.WIRE_FILL, np.uint8)
        tb, tz = tails if tails else (None, None)
        k = api.plan_red_pack(S, frames, off, nb, size, e["pkt_route"], e["pkt_frame"], [96] * S, N, wire, max_depth=d, n_packets=n, tail_bytes=tb, tail_sizes=tz,
                              header_room=room)
        assert not k["red_flags"].any()
        st = api.plan_rtp_stamp(e["pkt_route"], e["pkt_seq"], e["pkt_frame"], k["red_offset"], k["red_size"], ssrc, ts_base, [97] * S, N, T, k["wire"], room, 0,
                                k["red_flags"], n, optional=("pkt_status", "next_ts"))
        assert (st["pkt_status"] == 1).all()
        base = sum(len(x) for x in ring)
        ring.append(st["wire"])
        for p in range(n):
            if (int(e["pkt_route"][p]), call * T + int(e["pkt_frame"][p])) not in lost:
                dg_off.append(base + int(k["red_offset"][p]))
                dg_size.append(int(k["red_size"][p]))
        tails = (k["tail_bytes"], k["tail_sizes"])
        seq_base, ts_base = e["next_seq"], st["next_ts"]
    ring = np.concatenate(ring)
    p = api.plan_rtp_parse(S, ring, dg_off, dg_size, ssrc, np.arange(S), [97] * S)
    assert (p["status"] == 0).all()
    u = api.plan_red_unpack(S, p["stream"], p["seq"], p["offsets"], p["num_bytes"], ring, N, max_red=d, timestamp=p["timestamp"], block_pt=[96] * S)
    assert (u["status"] == 0).all() and not u["stats"][8:11].any()
    i = api.plan_ingest(S, 1, u["stream"], u["seq"], u["offsets"], u["num_bytes"], np.array([65530, 100]), calls * T, 16)
    return i, ring, np.concatenate(sent, axis=1), u


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_host_round_trip_through_dropped_bursts(d):
    """with depth d, bursts of at most d dropped packets - inside a call, across both call boundaries, at a stream's very start - leave no gap, and every cell
    points at its frame's bytes, whichever copy arrived; the timestamps of the blocks are their frames'; a burst of d + 1 leaves exactly one gap"""
    S, T, calls, size = 2, 8, 3, 40
    bursts = [(0, 0, d), (0, T - (d + 1) // 2, d), (1, 2, 1), (1, 2 * T - 1, d), (0, calls * T - 2 * d, d)]
    i, ring, sent, u = _round_trip(d, bursts)
    assert i["stats"][:, 1].tolist() == [0, 0] and i["counts"].tolist() == [calls * T] * S      # word 1: the gaps
    for s in range(S):
        for t in range(calls * T):
            a = int(i["offsets"][s, t])
            assert i["num_bytes"][s, t] == size and np.array_equal(ring[a:a + size], sent[s, t]), (s, t)
    kept = u["stream"] >= 0
    base_ts = np.array([0xFFFFF000, 7])[u["stream"][kept]]
    frame = (u["seq"][kept] - np.array([65530, 100])[u["stream"][kept]]) & 0xFFFF
    assert np.array_equal(u["timestamp"][kept].view(np.uint32), ((base_ts + frame * 480) & 0xFFFFFFFF).astype(np.uint32))
    i, _, _, _ = _round_trip(d, [(1, 5, d + 1)])
    assert i["stats"][:, 1].tolist() == [0, 1] and i["cell_item"][1, 5] == -1 and (np.delete(i["cell_item"][1], 5) >= 0).all()


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-C", CSRC, "red_driver"])
    return os.path.join(ROOT, "audio_codec_amd", "_stub", "red_plan_driver")


def _run(driver, *argv):
    p = subprocess.run([driver] + [str(a) for a in argv], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-2000:])
    return {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in p.stdout.splitlines()}


class _Lcg:
    def __init__(self, seed):
        self.x = seed

    def __call__(self):
        self.x = (self.x * 1103515245 + 12345) & 0x7FFFFFFF
        return self.x >> 8


def _driver_pack_case(seed, N, D, room, align):
    """the case tools/red_plan_driver.c draws from these arguments"""
    lcg = _Lcg(seed)
    S, T, R, M, stride = 3, 6, 4, 60, 64
    nb, off, flags, at = np.zeros((S, T), np.int32), np.zeros((S, T), np.int64), np.zeros((S, T), np.uint8), 0
    for s in range(S):
        for t in range(T):
            d = lcg()
            nb[s, t] = 0 if d % 11 == 0 else M + 5 if d % 13 == 0 else 1 + d % M
            flags[s, t] = d >> 4 & 3
            at += lcg() & 3
            off[s, t] = at
            at += int(nb[s, t]) if nb[s, t] <= M else 0
    frames = np.array([lcg() & 255 for _ in range(at)], np.uint8)
    counts = np.array([lcg() % (T + 3) - 1 for _ in range(S)], np.int32)
    route_src = np.array([lcg() % (S + 1) for _ in range(R)], np.int32)
    depth = np.array([lcg() % 7 - 1 for _ in range(R)], np.int32)
    m = N + 2
    route = np.array([lcg() % (R + 2) - 1 for _ in range(m)], np.int32)
    frame = np.array([lcg() % (T + 2) - 1 for _ in range(m)], np.int32)
    tz = np.array([lcg() % (stride + 8) - 4 for _ in range(S * D)], np.int32).reshape(S, D)
    tb = np.array([lcg() & 255 for _ in range(S * D * stride)], np.uint8).reshape(S, D, stride)
    cap = lcg() % (N * (room + 80) + 1)
    return dict(n_streams=S, frames=frames, frames_capacity=at, offsets=off, num_bytes=nb, max_frame_bytes=M, flags=flags, skip_mask=2, counts=counts, route_src=route_src,
                block_pt=96 + np.arange(R), depth=depth, max_depth=D, ts_step=480, max_packet_bytes=room + 150, header_room=room, align=align, tail_stride=stride,
                pkt_route=route, pkt_frame=frame, n_packets=N, tail_bytes=tb, tail_sizes=tz, tail_fill=np.full((S, D, stride), 0x5A, np.uint8),
                wire=np.full(cap, 0x5A, np.uint8), wire_capacity=cap)


@pytest.mark.parametrize("argv", [(3, 200, 4, 12, 1), (7, 1100, 2, 13, 4), (11, 1, 1, 12, 8), (5, 64, 3, 30, 16), (15, 300, 0, 12, 2)])
def test_pack_under_sanitizers(driver, argv):
    """lc3plus_plan_red_pack in a program of its own under ASan + UBSan, frames, tails and wire buffer heap blocks of their exact sizes: a clean exit, and its
    output is the rule's"""
    out = _run(driver, "pack", *argv)
    assert out["rc"] == [0]
    c = _driver_pack_case(*argv)
    want = ref.pack(c)
    n = c["n_packets"]
    for k in ("red_offset", "red_size", "red_flags", "red_blocks"):
        sentinel = {"red_offset": 0x5A5A5A5A5A5A5A5A, "red_size": 0x5A5A5A5A}.get(k, 0x5A)
        assert out[k] == want[k][:n].tolist() + [sentinel] * 2, k     # entries behind n_packets are not written
    assert out["wire_total"] == [want["wire_total"]] and out["route_stats"] == want["route_stats"].ravel().tolist() and out["wire"] == want["wire"].tolist()
    assert out["tail_sizes"] == want["tail_sizes"].ravel().tolist() and out["tail_bytes"] == want["tail_bytes"].ravel().tolist()
    assert argv[1] < 100 or (want["route_stats"][:, 1].sum() > 0 or argv[2] == 0)


@pytest.mark.parametrize("argv", [(1, 1000, 4), (2, 257, 2), (3, 1, 0), (4, 400, 1)])
def test_unpack_under_sanitizers(driver, argv):
    """lc3plus_plan_red_unpack likewise over red_ref.random_unpack's kind of items, drawn by the driver's generator, the ring a heap block of its exact size"""
    out = _run(driver, "unpack", *argv)
    assert out["rc"] == [0]
    seed, N, max_red = argv
    lcg = _Lcg(seed)
    off, size, at = [], [], 0
    for _ in range(N):
        at += lcg() & 3
        off.append(at)
        size.append(lcg() % 41)
        at += size[-1]
    ring = np.array([lcg() & 255 for _ in range(at)], np.uint8)
    for i in range(N):
        if lcg() & 1:
            k, p = lcg() % 6, off[i]
            for _ in range(k):
                if p + 4 <= off[i] + size[i]:
                    ring[p:p + 4] = np.frombuffer(ref.block_header(96 + (lcg() & 1), 480 * (lcg() % 4) + (lcg() % 5 == 0), lcg() % 9), np.uint8)
                    p += 4
            if p < off[i] + size[i]:
                ring[p] = 96 + (lcg() % 3 == 0)
    stream = np.array([lcg() % 5 - 1 for _ in range(N)], np.int32)
    if N > 3:
        off[0], size[1], off[2], size[2] = -1, -5, at, 1
    c = dict(n_streams=3, stream=stream, seq=np.arange(N) * 3 & 0xFFFF, offsets=np.array(off, np.int64), num_bytes=np.array(size, np.int32),
             timestamp=(0xFFFFFE00 + 480 * np.arange(N)) & 0xFFFFFFFF, ring=ring, ring_capacity=at, max_red=max_red, block_pt=np.array([96, -1, 97], np.int32), ts_step=480)
    want = ref.unpack(c)
    for k in ref.UNPACK_KEYS:
        assert out[k] == want[k].tolist(), k


def test_refusals_under_sanitizers(driver):
    p = subprocess.run([driver, "refuse"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("refusals ok"), (p.stdout[-400:], p.stderr[-2000:])
