"""Packet egress without a GPU (include/lc3plus_batch.h "Packet egress"): the exported symbols and constants, every refusal of the two batch calls in the header's
order (their checks run before anything of the batch or the device is touched), lc3plus_plan_egress - the text the kernels run - against the numpy restatement of
the rule (egress_ref.rule) on every output over the generated cases, the inverse property egress -> ingest on the host, and the host code once more in a program
of its own under AddressSanitizer + UndefinedBehaviorSanitizer (tools/egress_plan_driver.c).  Every comparison is equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import audio_codec_amd
from audio_codec_amd import api
import egress_ref as ref

NEW = ["lc3plus_enc_batch_egress", "lc3plus_dec_batch_egress", "lc3plus_plan_egress", "lc3plus_egress_work_bytes"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_codec_amd", "csrc")
LC3_ERROR, LC3_NULL_ERROR = 1, 3
ARGS = ("n_frames", "frames", "frames_capacity", "offsets", "num_bytes", "max_frame_bytes", "flags", "skip_mask", "counts", "n_routes", "route_src", "seq_base",
        "seq_bits", "order", "wire", "wire_capacity", "header_room", "align", "pkt_route", "pkt_seq", "pkt_frame", "pkt_offset", "pkt_size", "pkt_flags",
        "n_packets", "wire_total", "next_seq", "stats", "cell_status", "work", "hip_stream", "sync")
REQUIRED = ("frames", "offsets", "num_bytes", "seq_base", "pkt_route", "pkt_seq", "pkt_frame", "pkt_offset", "pkt_size", "n_packets", "work")
NULLABLE = ("flags", "counts", "pkt_flags", "wire_total", "next_seq", "stats", "cell_status")
VALUES = dict(n_frames=1, frames_capacity=100, max_frame_bytes=10, skip_mask=0, n_routes=1, seq_bits=16, order=0, wire_capacity=100, header_room=0, align=1,
              hip_stream=None, sync=1)
BAD = (dict(n_frames=0), dict(n_frames=-3), dict(n_routes=0), dict(n_routes=-1), dict(n_routes=1 << 16, n_frames=1 << 15), dict(n_routes=(1 << 31) - 1, n_frames=2),
       dict(max_frame_bytes=0), dict(max_frame_bytes=-5), dict(frames_capacity=-1), dict(wire_capacity=-1), dict(order=2), dict(order=-1), dict(seq_bits=0),
       dict(seq_bits=15), dict(seq_bits=17), dict(seq_bits=24), dict(seq_bits=64), dict(header_room=-1), dict(header_room=(1 << 31) - 1), dict(align=0),
       dict(align=3), dict(align=48), dict(align=8192), dict(align=-2), dict(wire=None, header_room=1), dict(wire=None, align=2), dict(route_src=None, n_routes=3))


def test_symbols_are_exported():
    L = audio_codec_amd.load_library()
    text = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    for s in NEW:
        assert s in api.EXPORTS and hasattr(L, s) and re.search(r"\b%s\s*\(" % s, text), s
    for cls in (api.Batch, api.DecBatch):
        assert callable(cls.egress_device) and callable(cls.egress)
    assert os.path.exists(os.path.join(ROOT, "audio_codec_amd", "liblc3plus_egress_hip.so"))


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define\s+LC3PLUS_EGR_(\w+)\s+(\d+)", text)}
    want = dict(SENT=1, LOST=2, INVALID=4, SKIPPED=8, ABSENT=16, BAD_ROUTE=32, OVERFLOW=64, PKT_OVERFLOW=1, STATS_WORDS=4)
    assert header == want
    for k, v in want.items():
        assert getattr(api, "EGR_" + k) == v == getattr(ref, k), k
    assert api.ENC_FL_PACK_CAP == ref.PACK_CAP and (api.PACK_STREAM_MAJOR, api.PACK_FRAME_MAJOR) == (ref.STREAM_MAJOR, ref.FRAME_MAJOR)
    assert api.EGR_OPTIONAL == ref.OPTIONAL


def _refusals(call):
    """call(**overrides) -> the return code; the arguments are good unless overridden"""
    for k in REQUIRED:
        assert call(**{k: None}) == LC3_NULL_ERROR, k
    for k in NULLABLE:
        for kw in BAD[:2] + BAD[12:14]:
            assert call(**dict(kw, **{k: None})) == LC3_ERROR, (k, kw)                # an optional NULL is no refusal: the value check behind it answers
    for kw in BAD:
        assert call(**kw) == LC3_ERROR, kw
    for k in REQUIRED:                                                                 # NULL first
        assert call(n_frames=0, seq_bits=3, align=3, order=9, **{k: None}) == LC3_NULL_ERROR, k


@pytest.mark.parametrize("name", ["lc3plus_enc_batch_egress", "lc3plus_dec_batch_egress"])
def test_egress_refusals_need_no_device(name):
    """a zero-filled block stands in for the batch: no refusal writes to it or to an array, and the only thing read of it is its stream count (0, so that
    identity routes are refused whatever n_routes is)"""
    L = audio_codec_amd.load_library()
    fake = C.create_string_buffer(4096)
    arr = C.create_string_buffer(256)
    p = C.cast(arr, C.c_void_p)
    good = dict({k: p for k in ARGS}, b=C.cast(fake, C.c_void_p), **VALUES)

    def call(**kw):
        a = dict(good, **kw)
        return getattr(L, name)(a["b"], *[a[k] for k in ARGS])
    assert call(b=None) == LC3_NULL_ERROR and call(b=None, n_frames=0) == LC3_NULL_ERROR and call(b=None, frames=None, seq_bits=1) == LC3_NULL_ERROR
    _refusals(call)
    assert call(route_src=None) == LC3_ERROR and call(work=C.c_void_p(p.value + 4)) == LC3_ERROR
    assert fake.raw == bytes(4096) and arr.raw == bytes(256)


def test_plan_refusals():
    L = audio_codec_amd.load_library()
    arr = C.create_string_buffer(256)
    p = C.cast(arr, C.c_void_p)
    good = dict({k: p for k in ARGS}, S=1, **VALUES)

    def call(**kw):
        a = dict(good, **kw)
        return L.lc3plus_plan_egress(a["S"], *[a[k] for k in ARGS])
    _refusals(call)
    for kw in (dict(S=0), dict(S=-1)):
        assert call(**kw) == LC3_ERROR, kw
    assert call(S=0, frames=None) == LC3_NULL_ERROR
    assert arr.raw == bytes(256)
    assert api.egress_work_bytes(0, 3) == 0 and api.egress_work_bytes(3, 0) == 0 and api.egress_work_bytes(1 << 16, 1 << 15) == 0
    assert api.egress_work_bytes(3, 5) >= 3 * 5 * 5 and api.egress_work_bytes((1 << 31) - 1, 1) > 1 << 33
    with pytest.raises(api.LC3Error):
        api.plan_egress(1, np.zeros(8, np.uint8), [[0]], [[4]], [0], 8, seq_bits=12)


def plan(c, optional=api.EGR_OPTIONAL):
    return api.plan_egress(c["n_streams"], c["frames"], c["offsets"], c["num_bytes"], c["seq_base"], c["max_frame_bytes"], c["flags"], c["skip_mask"], c["counts"],
                           c["route_src"], c["seq_bits"], c["order"], c["wire"], c["wire_capacity"], c["header_room"], c["align"], optional, c["frames_capacity"])


def same(got, want, name, keys=ref.KEYS):
    """equality of the outputs; the list arrays over the whole array: behind n_packets both hold what they held before the call"""
    for k in keys + ("wire",):
        g, w = got[k], want[k]
        if isinstance(w, int) or w is None:
            assert g == w, (name, k, g, w)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (name, k, "first differences at", bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("name", list(ref.cpu_cases()))
def test_plan_equals_the_rule(name):
    c = ref.cpu_cases()[name]
    want = ref.rule(c)
    same(plan(c), want, name)
    for optional in ((),) + tuple((k,) for k in api.EGR_OPTIONAL):                       # the optional outputs NULL: the others are what they were
        got = plan(c, optional)
        assert all(got[k] is None for k in api.EGR_OPTIONAL if k not in optional)
        same(got, want, (name, optional), ref.LIST[:5] + ("n_packets",) + optional)


def test_rule_on_a_case_by_hand():
    """the restatement itself on 2 streams, 3 routes, 4 frames: route 0 sends stream 1 (3 frames of it, the second too large), routes 1 and 2 both stream 0 (its
    second frame lost, its third skipped); bases 65534, 65534 and 9"""
    c = ref.by_hand()
    r = ref.rule(c)
    S = ref
    assert r["n_packets"] == 6 and r["wire_total"] == 5 + 5 + 2 * (10 + 10)
    assert r["pkt_route"][:6].tolist() == [0, 0, 1, 1, 2, 2] and r["pkt_frame"][:6].tolist() == [0, 2, 0, 3, 0, 3]
    assert r["pkt_seq"][:6].tolist() == [65534, 0, 65534, 1, 9, 12] and r["pkt_offset"][:6].tolist() == [40, 60, 0, 30, 0, 30]
    assert r["pkt_size"][:6].tolist() == [5, 5, 10, 10, 10, 10] and r["pkt_flags"][:6].tolist() == [0] * 6
    assert r["cell_status"].tolist() == [[S.SENT, S.INVALID, S.SENT, S.ABSENT], [S.SENT, S.LOST, S.SKIPPED, S.SENT], [S.SENT, S.LOST, S.SKIPPED, S.SENT]]
    assert r["next_seq"].tolist() == [1, 2, 13] and r["stats"].tolist() == [[3, 2, 1, 0], [4, 2, 2, 0], [4, 2, 2, 0]]
    same(plan(c), r, "by hand")
    # frame-major, into a wire buffer of 70 bytes with 4 bytes of header room and packets aligned to 8: the last two packets overflow
    c = dict(c, order=ref.FRAME_MAJOR, wire=np.full(100, ref.WIRE_FILL, np.uint8), wire_capacity=70, header_room=4, align=8)
    r = ref.rule(c)
    assert r["pkt_route"][:6].tolist() == [0, 1, 2, 0, 1, 2] and r["pkt_frame"][:6].tolist() == [0, 0, 0, 2, 3, 3]
    assert r["pkt_size"][:6].tolist() == [9, 14, 14, 9, 14, 14] and r["pkt_offset"][:6].tolist() == [0, 16, 32, 48, 64, 80] and r["wire_total"] == 96
    assert r["pkt_flags"][:6].tolist() == [0, 0, 0, 0, 1, 1] and r["stats"].tolist() == [[3, 2, 1, 0], [4, 2, 2, 1], [4, 2, 2, 1]]
    assert r["cell_status"][1].tolist() == [S.SENT, S.LOST, S.SKIPPED, S.SENT | S.OVERFLOW]
    w = r["wire"]
    assert w[4:9].tolist() == [40, 41, 42, 43, 44] and w[20:30].tolist() == list(range(10)) and w[52:57].tolist() == [60, 61, 62, 63, 64]
    assert (np.delete(w, np.r_[4:9, 20:30, 36:46, 52:57]) == ref.WIRE_FILL).all()
    same(plan(c), r, "by hand, wire")


@pytest.mark.parametrize("name", [n for n in ref.cpu_cases() if not n.startswith("copy")])
def test_egress_is_the_inverse_of_ingest(name):
    """the list fed to lc3plus_plan_ingest with one ingest stream per route (stream = pkt_route, base = seq_base): SENT cells come back with the packet's offset
    and size, every other cell in front of the route's count comes back lost, counts are 1 + the last SENT frame, and next_base is next_seq wherever the last
    cell in front of the count is SENT"""
    c = ref.cpu_cases()[name]
    e = plan(c)
    n, T = e["n_packets"], c["n_frames"]
    R = len(c["seq_base"])
    if n == 0:
        return
    i = api.plan_ingest(R, 1, e["pkt_route"][:n], e["pkt_seq"][:n], e["pkt_offset"][:n], e["pkt_size"][:n], c["seq_base"], T, c["seq_bits"])
    sent = (e["cell_status"] & ref.SENT) != 0
    assert np.array_equal(i["cell_item"] >= 0, sent)
    rr, tt = e["pkt_route"][:n], e["pkt_frame"][:n]
    assert np.array_equal(i["offsets"][rr, tt], e["pkt_offset"][:n]) and np.array_equal(i["num_bytes"][rr, tt], e["pkt_size"][:n])
    assert np.array_equal(i["cell_item"][rr, tt], np.arange(n))
    assert (i["num_bytes"][~sent] == 0).all() and (i["offsets"][~sent] == 0).all()
    last = np.where(sent.any(axis=1), T - np.argmax(sent[:, ::-1], axis=1), 0)
    assert np.array_equal(i["counts"], last)
    whole = last == e["stats"][:, 0]                                                   # the last cell in front of c is SENT (or c is 0)
    bad = (e["cell_status"] == ref.BAD_ROUTE).all(axis=1)
    assert whole.any() and np.array_equal(i["next_base"][whole & ~bad], e["next_seq"][whole & ~bad])
    assert (i["item_status"] == api.ING_USED).all()


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-C", CSRC, "egress_driver"])
    return os.path.join(ROOT, "audio_codec_amd", "_stub", "egress_plan_driver")


def _lcg_case(seed, S, T, R, order, bits, room, align, wcap):
    """the case tools/egress_plan_driver.c draws from these arguments"""
    x = [seed]
    def lcg():
        x[0] = (x[0] * 1103515245 + 12345) & 0x7FFFFFFF
        return x[0] >> 8
    off, nb, fl = np.zeros(S * T, np.int64), np.zeros(S * T, np.int32), np.zeros(S * T, np.uint8)
    at = 0
    for k in range(S * T):
        d = lcg()
        at += d & 3
        nb[k] = 0 if d % 7 == 0 else -3 if d % 11 == 0 else 41 if d % 13 == 0 else 1 + (d >> 4) % 40
        off[k] = -1 if d % 17 == 0 else at
        if 0 < nb[k] <= 40:
            at += int(nb[k])
        fl[k] = lcg() & 15
    cap = at - 5 if at > 5 else at
    frames = np.array([lcg() & 255 for _ in range(cap)], np.uint8)
    counts = np.array([lcg() % (T + 3) - 1 for _ in range(S)], np.int32)
    src = np.array([lcg() % (S + 2) - 1 for _ in range(R)], np.int32)
    return dict(n_streams=S, n_frames=T, frames=frames, frames_capacity=cap, offsets=off.reshape(S, T), num_bytes=nb.reshape(S, T), max_frame_bytes=40,
                flags=fl.reshape(S, T), skip_mask=8, counts=counts, route_src=src, seq_base=65530 + np.arange(R) % 6, seq_bits=bits, order=order,
                wire=np.full(wcap, 0x5A, np.uint8) if wcap >= 0 else None, wire_capacity=max(wcap, 0), header_room=room, align=align)


@pytest.mark.parametrize("argv", [(1, 3, 5, 4, 0, 16, 0, 1, -1), (2, 5, 9, 11, 1, 16, 12, 4, 3000), (3, 2, 40, 7, 0, 32, 3, 64, 700), (4, 7, 3, 7, 1, 32, 13, 1, 0),
                                  (5, 4, 300, 4, 1, 16, 16, 16, 20001), (6, 1, 1, 1, 0, 16, 0, 1, 1)])
def test_host_code_under_sanitizers(driver, argv):
    """lc3plus_plan_egress in a program of its own under ASan + UBSan, every array a heap block of its exact size: a clean exit, and its output is the rule's"""
    p = subprocess.run([driver, "plan"] + [str(a) for a in argv], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-2000:])
    out = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in p.stdout.splitlines()}
    assert out["rc"] == [0]
    want = ref.rule(_lcg_case(*argv))
    n = want["n_packets"]
    assert out["n_packets"] == [n] and out["wire_total"] == [want["wire_total"]]
    for k in ref.LIST:
        assert out[k] == want[k][:n].tolist(), k
    for k in ("next_seq", "stats", "cell_status"):
        assert out[k] == want[k].reshape(-1).tolist(), k
    assert out["wire"] == (want["wire"].tolist() if want["wire"] is not None else [])


def test_refusals_under_sanitizers(driver):
    p = subprocess.run([driver, "refuse"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("refusals ok"), (p.stdout[-400:], p.stderr[-2000:])
