"""RTP framing without a GPU (include/lc3plus_batch.h "RTP framing"): the exported symbols and constants, every refusal of the three batch calls in the header's
order (their checks run before anything of the batch or the device is touched), lc3plus_plan_rtp_parse and lc3plus_plan_rtp_stamp - the text the kernels run -
against the numpy restatement of the rules (rtp_ref.parse, rtp_ref.stamp) on every output, the inverse property egress -> stamp -> parse -> ingest on the host,
and the host code once more in a program of its own under AddressSanitizer + UndefinedBehaviorSanitizer (tools/rtp_plan_driver.c).  Every comparison is
equality."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import audio_codec_amd
from audio_codec_amd import api
import egress_ref
import rtp_ref as ref

NEW = ["lc3plus_dec_batch_rtp_parse", "lc3plus_plan_rtp_parse", "lc3plus_rtp_sort_ssrc", "lc3plus_enc_batch_rtp_stamp", "lc3plus_dec_batch_rtp_stamp",
       "lc3plus_plan_rtp_stamp"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_codec_amd", "csrc")
LC3_OK, LC3_ERROR, LC3_NULL_ERROR = 0, 1, 3
P_ARGS = ("n_items", "ring", "ring_capacity", "dg_offsets", "dg_sizes", "n_ssrc", "ssrc_key", "ssrc_stream", "payload_type", "payload_room", "stream", "seq",
          "offsets", "num_bytes", "timestamp", "marker", "status", "stats", "hip_stream", "sync")
P_REQUIRED = ("ring", "dg_offsets", "dg_sizes", "ssrc_key", "ssrc_stream", "stream", "seq", "offsets", "num_bytes")
P_NULLABLE = ("payload_type", "timestamp", "marker", "status", "stats")
P_VALUES = dict(n_items=1, ring_capacity=100, n_ssrc=1, payload_room=0, hip_stream=None, sync=1)
P_BAD = (dict(n_items=0), dict(n_items=-1), dict(n_items=1 << 29), dict(n_items=(1 << 63) - 1), dict(ring_capacity=-1), dict(n_ssrc=0), dict(n_ssrc=-2),
         dict(payload_room=-1), dict(payload_room=4097))
S_ARGS = ("max_packets", "n_packets", "pkt_route", "pkt_seq", "pkt_frame", "pkt_offset", "pkt_size", "pkt_flags", "n_routes", "n_frames", "ssrc", "ts_base",
          "payload_type", "ts_step", "marker_mode", "cell_status", "resume", "route_stats", "wire", "wire_capacity", "header_room", "payload_room", "pkt_status",
          "next_ts", "next_resume", "hip_stream", "sync")
S_REQUIRED = ("n_packets", "pkt_route", "pkt_seq", "pkt_frame", "pkt_offset", "pkt_size", "ssrc", "ts_base", "payload_type", "wire")
S_NULLABLE = ("pkt_flags", "resume", "route_stats", "pkt_status", "next_ts")
S_VALUES = dict(max_packets=1, n_routes=1, n_frames=1, ts_step=480, marker_mode=0, wire_capacity=100, header_room=12, payload_room=0, hip_stream=None, sync=1)
S_BAD = (dict(max_packets=0), dict(max_packets=-1), dict(n_routes=0), dict(n_routes=-1), dict(n_frames=0), dict(n_frames=-5), dict(wire_capacity=-1),
         dict(payload_room=-1), dict(header_room=11), dict(header_room=0), dict(header_room=-12), dict(payload_room=1), dict(header_room=14, payload_room=3),
         dict(payload_room=(1 << 31) - 1), dict(marker_mode=2), dict(marker_mode=-1), dict(marker_mode=1, cell_status=None), dict(cell_status=None),
         dict(cell_status=None, marker_mode=1, next_resume=None))


def test_symbols_are_exported():
    L = audio_codec_amd.load_library()
    text = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    for s in NEW:
        assert s in api.EXPORTS and hasattr(L, s) and re.search(r"\b%s\s*\(" % s, text), s
    assert callable(api.DecBatch.rtp_parse_device) and callable(api.DecBatch.rtp_parse)
    for cls in (api.Batch, api.DecBatch):
        assert callable(cls.rtp_stamp_device) and callable(cls.rtp_stamp)
    assert callable(api.plan_rtp_parse) and callable(api.plan_rtp_stamp) and callable(api.rtp_sort_ssrc)
    assert os.path.exists(os.path.join(ROOT, "audio_codec_amd", "liblc3plus_rtp_hip.so"))


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define\s+LC3PLUS_RTP_(\w+)\s+(\d+)", text)}
    want = dict(OK=0, RANGE=1, SHORT=2, VERSION=3, RTCP=4, HEADER=5, PADDING=6, PAYLOAD_ROOM=7, UNKNOWN_SSRC=8, PAYLOAD_TYPE=9, STATS_WORDS=16, STAMPED=1,
                ST_BAD_ROUTE=2, ST_OVERFLOW=4, ST_RANGE=8, MARKER_NEVER=0, MARKER_AFTER_HOLE=1)
    assert header == want
    for k, v in want.items():
        assert getattr(api, "RTP_" + k) == v == getattr(ref, k), k
    assert (api.EGR_SENT, api.EGR_PKT_OVERFLOW, api.EGR_STATS_WORDS) == (ref.EGR_SENT, ref.EGR_PKT_OVERFLOW, ref.EGR_STATS_WORDS)
    assert api.RTP_PARSE_OUTPUTS == ref.PARSE_KEYS


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
        assert call(**dict(bad[-3], **{k: None})) == LC3_NULL_ERROR, k


def test_parse_refusals_need_no_device():
    """a zero-filled block stands in for the batch: no refusal writes to it or to an array"""
    L = audio_codec_amd.load_library()
    fake, arr = C.create_string_buffer(4096), C.create_string_buffer(256)
    p = C.cast(arr, C.c_void_p)
    good = dict({k: p for k in P_ARGS}, b=C.cast(fake, C.c_void_p), **P_VALUES)

    def call(**kw):
        a = dict(good, **kw)
        return L.lc3plus_dec_batch_rtp_parse(a["b"], *[a[k] for k in P_ARGS])
    assert call(b=None) == LC3_NULL_ERROR and call(b=None, n_items=0) == LC3_NULL_ERROR and call(b=None, ring=None, payload_room=-1) == LC3_NULL_ERROR
    _refusals(call, P_REQUIRED, P_NULLABLE, P_BAD)
    assert fake.raw == bytes(4096) and arr.raw == bytes(256)


@pytest.mark.parametrize("name", ["lc3plus_enc_batch_rtp_stamp", "lc3plus_dec_batch_rtp_stamp"])
def test_stamp_refusals_need_no_device(name):
    L = audio_codec_amd.load_library()
    fake, arr = C.create_string_buffer(4096), C.create_string_buffer(256)
    p = C.cast(arr, C.c_void_p)
    good = dict({k: p for k in S_ARGS}, b=C.cast(fake, C.c_void_p), **S_VALUES)

    def call(**kw):
        a = dict(good, **kw)
        return getattr(L, name)(a["b"], *[a[k] for k in S_ARGS])
    assert call(b=None) == LC3_NULL_ERROR and call(b=None, n_frames=0) == LC3_NULL_ERROR and call(b=None, wire=None, marker_mode=5) == LC3_NULL_ERROR
    _refusals(call, S_REQUIRED, S_NULLABLE, S_BAD)
    assert fake.raw == bytes(4096) and arr.raw == bytes(256)


def test_plan_refusals():
    L = audio_codec_amd.load_library()
    arr = C.create_string_buffer(256)
    p = C.cast(arr, C.c_void_p)
    good = dict({k: p for k in P_ARGS}, S=1, **P_VALUES)

    def parse(**kw):
        a = dict(good, **kw)
        return L.lc3plus_plan_rtp_parse(a["S"], *[a[k] for k in P_ARGS])
    _refusals(parse, P_REQUIRED, P_NULLABLE, P_BAD)
    assert parse(S=0) == LC3_ERROR and parse(S=-1) == LC3_ERROR and parse(S=0, ring=None) == LC3_NULL_ERROR
    good = dict({k: p for k in S_ARGS}, **S_VALUES)

    def stamp(**kw):
        a = dict(good, **kw)
        return L.lc3plus_plan_rtp_stamp(*[a[k] for k in S_ARGS])
    _refusals(stamp, S_REQUIRED, S_NULLABLE, S_BAD)
    assert arr.raw == bytes(256)
    assert stamp(cell_status=None, next_resume=None) == LC3_OK                           # neither AFTER_HOLE nor next_resume: cell_status is not needed
    with pytest.raises(api.LC3Error):
        api.plan_rtp_parse(1, np.zeros(16, np.uint8), [0], [12], [1], [0], payload_room=5000)
    with pytest.raises(api.LC3Error):
        api.plan_rtp_stamp([0], [0], [0], [0], [20], [1], [0], [96], 480, 1, np.zeros(32, np.uint8), header_room=8)


def test_sort_ssrc():
    key, stream = api.rtp_sort_ssrc([7, 0xFFFFFFFF, 3, 0x80000000, 5], [0, 1, 2, 3, 4])
    assert key.view(np.uint32).tolist() == [3, 5, 7, 0x80000000, 0xFFFFFFFF] and stream.tolist() == [2, 4, 0, 3, 1]
    assert api.rtp_sort_ssrc([-1, 1], [0, 1])[0].tolist() == [1, -1]                     # -1 is 0xFFFFFFFF
    for bad in (([], []), ([4, 9, 4], [0, 1, 2])):
        with pytest.raises(api.LC3Error):
            api.rtp_sort_ssrc(*bad)
    L = audio_codec_amd.load_library()
    a = (C.c_int32 * 2)(1, 2)
    assert L.lc3plus_rtp_sort_ssrc(2, None, a) == LC3_NULL_ERROR and L.lc3plus_rtp_sort_ssrc(2, a, None) == LC3_NULL_ERROR


def plan_parse(c, optional=api.RTP_PARSE_OPTIONAL):
    return api.plan_rtp_parse(c["n_streams"], c["ring"], c["dg_offsets"], c["dg_sizes"], c["ssrc_key"], c["ssrc_stream"], c["payload_type"], c["payload_room"],
                              optional, c["ring_capacity"])


def plan_stamp(c, optional=None):
    if optional is None:                                              # next_resume needs cell_status
        optional = tuple(k for k in api.RTP_STAMP_OPTIONAL if k != "next_resume" or c["cell_status"] is not None)
    return api.plan_rtp_stamp(c["pkt_route"], c["pkt_seq"], c["pkt_frame"], c["pkt_offset"], c["pkt_size"], c["ssrc"], c["ts_base"], c["payload_type"], c["ts_step"],
                              c["n_frames"], c["wire"], c["header_room"], c["payload_room"], c["pkt_flags"], c["n_packets"], c["marker_mode"], c["cell_status"],
                              c["resume"], c["route_stats"], c["wire_capacity"], optional)


def same(got, want, name, keys=None):
    for k in keys or want:
        g, w = got[k], want[k]
        if w is None:
            assert g is None, (name, k)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (name, k, "first differences at", bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("payload_room", [0, 2, 21])
def test_plan_parse_on_crafted_datagrams(payload_room):
    """every CC, X with three extension lengths, the four padding cases, every truncation of one full-featured datagram, versions, the RTCP range's edges,
    payload_room 0, 2 and one more than the 20-byte payloads, unknown SSRCs around every key (keys with the top bit set among them), a stream out of range,
    payload types, all four offset alignments: the plan against the restatement, and the restatement against values worked out by hand"""
    c, lab = ref.crafted(payload_room)
    want = ref.parse(c)
    same(plan_parse(c), want, payload_room)
    for optional in ((),) + tuple((k,) for k in api.RTP_PARSE_OPTIONAL):
        got = plan_parse(c, optional)
        assert all(got[k] is None for k in api.RTP_PARSE_OPTIONAL if k not in optional)
        same(got, want, optional, ref.PARSE_KEYS[:4] + optional)
    st = lambda label: int(want["status"][lab[label]])
    assert st("v0") == st("v1") == st("v3") == ref.VERSION and st("b1_192") == st("b1_223") == ref.RTCP
    assert all(st("cut%d" % k) == ref.SHORT for k in range(12)) and all(st("cut%d" % k) == ref.HEADER for k in range(12, 36))
    assert st("pad0") == st("pad_large") == ref.PADDING and st("room_short") == (ref.PAYLOAD_ROOM if payload_room else ref.OK)
    assert st("pt_mismatch") == (ref.PAYLOAD_TYPE if payload_room <= 20 else ref.PAYLOAD_ROOM)
    if payload_room <= 20:
        assert all(st("unknown%d" % k) == ref.UNKNOWN_SSRC for k in range(10)) and st("stream_out") == ref.UNKNOWN_SSRC
        for cc in range(16):
            i = lab["cc%d" % cc]
            assert (want["status"][i], want["stream"][i], want["seq"][i], want["timestamp"][i], want["num_bytes"][i]) == (0, 3, cc, 1000 + cc, 20 - payload_room)
            assert want["offsets"][i] == c["dg_offsets"][i] + 12 + 4 * cc + payload_room
        for words in (0, 1, 5):
            i = lab["x%d" % words]
            assert (want["status"][i], want["stream"][i], want["marker"][i]) == (0, 0, 1) and want["offsets"][i] - c["dg_offsets"][i] == 16 + 4 * words + payload_room
        i = lab["cut61"]                                              # the full-featured datagram, whole: 3 CSRCs, 2 extension words, 5 bytes of padding
        assert (want["status"][i], want["stream"][i], want["seq"][i], want["timestamp"][i], want["marker"][i]) == (0, 1, 0xFFFE, -16, 1)
        assert want["offsets"][i] - c["dg_offsets"][i] == 36 + payload_room and want["num_bytes"][i] == 20 - payload_room
        assert st("pad1") == st("b1_191") == st("b1_224") == st("pt_any") == st("top_bit") == st("top_key") == ref.OK
        assert want["stream"][lab["top_bit"]] == 1 and want["stream"][lab["top_key"]] == 2
        for a in range(4):
            i = lab["align%d" % a]
            assert (want["status"][i], want["seq"][i], want["timestamp"][i], want["num_bytes"][i]) == (0, 500 + a, 0x01020304, 20 - payload_room)
    assert st("pad_all") == (ref.OK if payload_room == 0 else ref.PAYLOAD_ROOM) and want["num_bytes"][lab["pad_all"]] == 0
    assert want["stats"].sum() == len(lab) and (want["stats"][10:] == 0).all()
    bad = want["status"] != 0
    assert (want["stream"][bad] == -1).all() and all((want[k][bad] == 0).all() for k in ("seq", "offsets", "num_bytes", "timestamp", "marker"))


@pytest.mark.parametrize("table", [5, 1, 4097])
def test_plan_parse_on_random_datagrams(table):
    """20 000 datagrams of random bytes and sizes 0 ... 80 on every output array, over a table of 5 senders, of one, and of 4 097"""
    c = ref.random_set(table=table)
    want = ref.parse(c)
    assert len(want["status"]) == 20000 and all(want["stats"][k] > 0 for k in range(10) if not (table == 1 and k == ref.PAYLOAD_TYPE))
    same(plan_parse(c), want, table)


def test_plan_parse_on_an_unsorted_table():
    """the answer for a table that is not sorted is the search's, as the restatement walks it"""
    c, _ = ref.crafted(0)
    swap = [1, 0, 2, 3, 4]                                            # the first two senders change places: the search misses one of them and finds the rest
    c = dict(c, ssrc_key=np.array(ref.KEYS5, np.int64)[swap], ssrc_stream=np.array(ref.STREAMS5, np.int32)[swap])
    want = ref.parse(c)
    assert 0 < want["stats"][0] < ref.parse(ref.crafted(0)[0])["stats"][0]
    same(plan_parse(c), want, "unsorted")


STAMP_CASES = {"%d_%d_%d_%s" % (n, hr, pr, "hole" if mode else "never"): dict(n=n, seed=n + hr, header_room=hr, payload_room=pr, marker_mode=mode, resume=res,
                                                                               route_stats=rs, flags=fl, slack=slack, spare=3, shift=shift)
               for n, hr, pr, mode, res, rs, fl, slack, shift in ((1, 12, 0, 1, True, True, True, 0, 0), (40, 12, 0, 1, True, True, True, 0, 0),
                                                                  (300, 12, 0, 0, False, False, False, 3, 1), (300, 16, 3, 1, False, True, True, 1, 2),
                                                                  (300, 17, 5, 1, True, False, True, 0, 3), (64, 20, 0, 0, True, True, False, 2, 0))}


@pytest.mark.parametrize("name", list(STAMP_CASES))
def test_plan_stamp_equals_the_rule(name):
    """bad routes, overflow flags, out-of-range packets, both marker modes with holes at t - 1 and at t = 0 with and without resume, route_stats given and
    NULL, sequence and timestamp wrap; every wire byte outside the stamped headers keeps its sentinel"""
    c = ref.stamp_case(**STAMP_CASES[name])
    want = ref.stamp(c)
    got = plan_stamp(c)
    same(got, want, name)
    n = c["n_packets"]
    stamped = want["pkt_status"][:n] == ref.STAMPED
    assert stamped.any() and (want["pkt_status"][n:] == 0).all()
    if n > 8:
        assert set(want["pkt_status"][:n].tolist()) == ({1, 2, 4, 8} if c["pkt_flags"] is not None else {1, 2, 8})
        assert want["pkt_status"][n - 1] == ref.ST_RANGE               # the packet cut by wire_capacity
    own = np.zeros(c["wire"].size, bool)
    for p in np.flatnonzero(stamped):
        at = int(c["pkt_offset"][p]) + c["header_room"] - c["payload_room"] - 12
        own[at:at + 12] = True
        assert got["wire"][at] == 0x80 and struct.unpack(">H", got["wire"][at + 2:at + 4].tobytes())[0] == int(c["pkt_seq"][p]) & 0xFFFF
    assert own.sum() == 12 * stamped.sum() and (got["wire"][~own] == ref.WIRE_FILL).all() and (got["wire"][c["wire_capacity"]:] == ref.WIRE_FILL).all()
    if c["marker_mode"] == ref.MARKER_AFTER_HOLE:
        marks = {(int(c["pkt_route"][p]), int(c["pkt_frame"][p])): got["wire"][int(c["pkt_offset"][p]) + c["header_room"] - c["payload_room"] - 11] >> 7
                 for p in np.flatnonzero(stamped)}
        assert n <= 8 or set(marks.values()) == {0, 1}
        for (r, t), m in marks.items():
            assert m == (int(not c["cell_status"][r, t - 1] & 1) if t else int(c["resume"] is not None and c["resume"][r] != 0)), (r, t)
    for optional in ((),) + tuple((k,) for k in api.RTP_STAMP_OPTIONAL if k != "next_resume" or c["cell_status"] is not None):
        g = plan_stamp(c, optional)
        assert all(g[k] is None for k in api.RTP_STAMP_OPTIONAL if k not in optional)
        same(g, want, (name, optional), ("wire",) + optional)


def test_stamp_by_hand():
    """two routes, three frames: sequence numbers wrap at 65535, timestamps at 2^32, the marker follows the hole in route 1 and the resume flag of route 0"""
    cs = np.array([[1, 1, 1], [1, 2, 1]], np.uint8)
    r = api.plan_rtp_stamp([0, 1, 0, 1, 1], [65535, 65536 + 7, 0, 8, 9], [0, 0, 1, 1, 2], [0, 40, 80, 120, 160], [32, 32, 32, 32, 32], [0xDEADBEEF, 1],
                           [0xFFFFFF00, 1000], [96, 111], 480, 3, np.full(200, ref.WIRE_FILL, np.uint8), 14, 2, None, None, ref.MARKER_AFTER_HOLE, cs, [1, 0],
                           [[2, 0, 0, 0], [3, 0, 0, 0]])
    w = r["wire"]
    assert w[0:12].tobytes() == bytes.fromhex("80e0ffffffffff00deadbeef") and w[40:52].tobytes() == bytes.fromhex("806f0007000003e800000001")
    assert w[80:92].tobytes() == bytes.fromhex("80600000000000e0deadbeef") and w[120:132].tobytes() == bytes.fromhex("806f0008000005c800000001")
    assert w[160:172].tobytes() == bytes.fromhex("80ef0009000007a800000001")
    assert r["pkt_status"].tolist() == [1] * 5 and r["next_ts"].tolist() == [0x2C0, 1000 + 3 * 480] and r["next_resume"].tolist() == [0, 0]
    assert (np.delete(w, np.r_[0:12, 40:52, 80:92, 120:132, 160:172]) == ref.WIRE_FILL).all()


@pytest.mark.parametrize("payload_room", [0, 3])
@pytest.mark.parametrize("align", [1, 4, 8])
@pytest.mark.parametrize("name", ["inplace_16_sm_identity", "inplace_16_fm_fan_bad", "plain"])
def test_stamp_and_parse_invert_egress_and_ingest(name, align, payload_room):
    """plan_egress (wire mode) -> plan_rtp_stamp -> plan_rtp_parse -> plan_ingest with pkt_offset / pkt_size as the datagrams, one ingest stream per route: the
    offsets (shifted into the wire), the sizes and the counts of every SENT cell come back, and the frames' bytes lie where the parse points"""
    c = dict(egress_ref.cpu_cases()[name])
    room = 12 + payload_room
    R, T = len(c["seq_base"]), c["n_frames"]
    cells = R * T
    wire_bytes = cells * (room + c["max_frame_bytes"] + align)
    e = api.plan_egress(c["n_streams"], c["frames"], c["offsets"], c["num_bytes"], c["seq_base"], c["max_frame_bytes"], c["flags"], c["skip_mask"], c["counts"],
                        c["route_src"], 16, c["order"], np.full(wire_bytes, ref.WIRE_FILL, np.uint8), wire_bytes, room, align, frames_capacity=c["frames_capacity"])
    n = e["n_packets"]
    assert n > 0 and not e["pkt_flags"][:n].any()
    ssrc = (0x7FFFFF00 + 977 * np.arange(R)).astype(np.int64)          # ascending, on both sides of 2^31
    s = api.plan_rtp_stamp(e["pkt_route"], e["pkt_seq"], e["pkt_frame"], e["pkt_offset"], e["pkt_size"], ssrc, np.arange(R) * 1000, np.full(R, 96), 480, T, e["wire"],
                           room, payload_room, e["pkt_flags"], n, ref.MARKER_AFTER_HOLE, e["cell_status"], None, e["stats"])
    assert (s["pkt_status"][:n] == ref.STAMPED).all()
    p = api.plan_rtp_parse(R, s["wire"], e["pkt_offset"][:n], e["pkt_size"][:n], ssrc, np.arange(R), np.full(R, 96), payload_room)
    assert (p["status"] == 0).all() and np.array_equal(p["stream"], e["pkt_route"][:n]) and np.array_equal(p["seq"], e["pkt_seq"][:n])
    assert np.array_equal(p["offsets"], e["pkt_offset"][:n] + room) and np.array_equal(p["num_bytes"], e["pkt_size"][:n] - room)
    assert np.array_equal(p["timestamp"], e["pkt_route"][:n] * 1000 + e["pkt_frame"][:n] * 480)
    i = api.plan_ingest(R, 1, p["stream"], p["seq"], p["offsets"], p["num_bytes"], c["seq_base"], T, 16)
    sent = (e["cell_status"] & egress_ref.SENT) != 0
    rr, tt = e["pkt_route"][:n], e["pkt_frame"][:n]
    assert np.array_equal(i["cell_item"] >= 0, sent) and np.array_equal(i["cell_item"][rr, tt], np.arange(n))
    assert np.array_equal(i["offsets"][rr, tt], e["pkt_offset"][:n] + room) and np.array_equal(i["num_bytes"][rr, tt], e["pkt_size"][:n] - room)
    last = np.where(sent.any(axis=1), T - np.argmax(sent[:, ::-1], axis=1), 0)
    assert np.array_equal(i["counts"], last) and (i["item_status"] == api.ING_USED).all()
    src = np.arange(R) if c["route_src"] is None else np.asarray(c["route_src"])
    for k in range(n):                                                # the parse points at the frame's bytes
        a, z, o = int(p["offsets"][k]), int(p["num_bytes"][k]), int(c["offsets"][src[rr[k]], tt[k]])
        assert np.array_equal(s["wire"][a:a + z], c["frames"][o:o + z]), k
    marks = s["wire"][e["pkt_offset"][:n] + 1] >> 7                    # a talkspurt starts behind every hole
    assert np.array_equal(marks, np.where(tt > 0, ~sent[rr, np.maximum(tt - 1, 0)], False).astype(np.uint8))


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-C", CSRC, "rtp_driver"])
    return os.path.join(ROOT, "audio_codec_amd", "_stub", "rtp_plan_driver")


class _Lcg:
    def __init__(self, seed):
        self.x = seed

    def __call__(self):
        self.x = (self.x * 1103515245 + 12345) & 0x7FFFFFFF
        return self.x >> 8


def _driver_parse_case(seed, N, K, room):
    """the case tools/rtp_plan_driver.c draws from these arguments"""
    lcg = _Lcg(seed)
    key = [(k * 0x0F0F0F0F + 5) & 0xFFFFFFFF for k in range(K)]
    off, size, at = [], [], 0
    for _ in range(N):
        at += lcg() & 3
        off.append(at)
        size.append(lcg() % 61)
        at += size[-1]
    ring = np.array([lcg() & 255 for _ in range(at)], np.uint8)
    for i in range(N):
        if (lcg() & 1) and size[i] >= 12:
            b = ring[off[i]:off[i] + size[i]]
            k = key[lcg() % K]
            b[0] = 0x80 | (b[0] & 0x33)
            b[1] = (b[1] & 0x80) | (96 if lcg() & 1 else 97)
            b[8:12] = np.frombuffer(struct.pack(">I", k), np.uint8)
            if b[0] & 0x20:
                b[-1] = lcg() % 4
    if N > 3:
        off[0], size[1], off[2], size[2] = -1, -5, at, 1
    return dict(n_streams=3, ring=ring, ring_capacity=at, dg_offsets=np.array(off, np.int64), dg_sizes=np.array(size, np.int32), ssrc_key=np.array(key, np.int64),
                ssrc_stream=np.array([k % 5 - 1 for k in range(K)], np.int32), payload_type=np.array([96, -1, 97], np.int32), payload_room=room)


def _driver_stamp_case(seed, N, room, proom, mode):
    lcg = _Lcg(seed)
    R, T, m = 3, 4, N + 2
    route, frame, size, flags, off, at = [], [], [], [], [], 0
    for p in range(m):
        d = lcg()
        route.append(-1 if d % 9 == 0 else R if d % 11 == 0 else d % R)
        frame.append(T if d % 13 == 0 else (d >> 3) % T)
        size.append(room - 1 if d % 17 == 0 else room + 1 + (d >> 5) % 20)
        flags.append(int(d % 7 == 0))
        off.append(-1 if d % 19 == 0 else at)
        at += size[-1] + (lcg() & 3)
    wcap = at - 3 if at > 3 else at
    cs = np.array([lcg() & 1 for _ in range(R * T)], np.uint8).reshape(R, T)
    resume, rs = [], np.zeros((R, 4), np.int32)
    for r in range(R):
        resume.append(lcg() & 1)
        rs[r, 0] = lcg() % (T + 3) - 1
    return dict(pkt_route=np.array(route, np.int32), pkt_seq=65533 + np.arange(m), pkt_frame=np.array(frame, np.int32), pkt_offset=np.array(off, np.int64),
                pkt_size=np.array(size, np.int32), pkt_flags=np.array(flags, np.uint8), n_packets=N, ssrc=0x80000001 + np.arange(R) * 0x3FFFFFFF,
                ts_base=0xFFFFFF00 + np.arange(R) * 100, payload_type=96 + np.arange(R), ts_step=480, n_frames=T, marker_mode=mode, cell_status=cs,
                resume=np.array(resume, np.uint8), route_stats=rs, wire=np.full(wcap, 0x5A, np.uint8), wire_capacity=wcap, header_room=room, payload_room=proom)


def _run(driver, *argv):
    p = subprocess.run([driver] + [str(a) for a in argv], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-2000:])
    return {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in p.stdout.splitlines()}


@pytest.mark.parametrize("argv", [(1, 400, 5, 0), (2, 1000, 16, 2), (3, 3, 1, 0), (4, 257, 2, 7), (5, 1, 3, 0)])
def test_parse_under_sanitizers(driver, argv):
    """lc3plus_plan_rtp_parse in a program of its own under ASan + UBSan, the ring a heap block of its exact size: a clean exit, and its output is the rule's"""
    out = _run(driver, "parse", *argv)
    assert out["rc"] == [0]
    want = ref.parse(_driver_parse_case(*argv))
    for k in ref.PARSE_KEYS:
        assert out[k] == want[k].tolist(), k
    assert argv[1] < 100 or want["stats"][0] > 0


@pytest.mark.parametrize("argv", [(1, 200, 12, 0, 1), (2, 500, 15, 3, 1), (3, 1, 12, 0, 0), (4, 64, 40, 28, 0), (5, 333, 13, 0, 1)])
def test_stamp_under_sanitizers(driver, argv):
    out = _run(driver, "stamp", *argv)
    assert out["rc"] == [0]
    c = _driver_stamp_case(*argv)
    want = ref.stamp(c)
    n = c["n_packets"]
    assert out["pkt_status"] == want["pkt_status"][:n].tolist() + [0x5A, 0x5A]          # entries behind n_packets are not written
    assert out["next_ts"] == want["next_ts"].tolist() and out["next_resume"] == want["next_resume"].tolist() and out["wire"] == want["wire"].tolist()


def test_refusals_under_sanitizers(driver):
    p = subprocess.run([driver, "refuse"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("refusals ok"), (p.stdout[-400:], p.stderr[-2000:])
