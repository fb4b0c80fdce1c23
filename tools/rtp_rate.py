"""RTP framing rates (lc3plus_enc_batch_rtp_stamp, lc3plus_dec_batch_rtp_parse) beside the calls they stand between and the host detours they replace: 4096
mono streams x 64 frames, 48 kHz / 10 ms, 80-byte frames, one encoder batch and one decoder batch, one process.  One stream in 16 is ragged (40 frames) and the
capacity cuts the last 64 frames, as in tools/enc_egress_rate.py.  Variants, alternated run by run:
  enc         lc3plus_enc_batch_encode_packed (set_frame_counts on)
  egress      the egress into a wire buffer, identity routes, 12 bytes of header room, packets aligned to 4: the call in front of the stamp
  stamp       the stamp on the egress's list: marker after a hole, pkt_status, next_ts and next_resume asked for
  parse       the parse of the wire buffer, the egress's list as the datagrams, a table of one sender per stream (staged in LDS), every output asked for
  dec         set_frame_counts + lc3plus_dec_batch_decode_packed from the wire buffer over the ingest's tables: the call behind the parse
  stamp_host  the path the stamp replaces: synchronise, the list, cell_status and stats to the host, lc3plus_plan_rtp_stamp there, the headers back (one strided copy:
              the packets are equally spaced)
  parse_host  the path the parse replaces: synchronise, the list and the fixed headers to the host (one strided copy), lc3plus_plan_rtp_parse there, the four item
              arrays back
Device variants: device events around the call on the call's stream (sync = 0).  Host variants: the host clock from before the synchronise (nothing is
pending) to the return of the last copy.  Per variant the median, the fastest and the slowest of --calls runs after --warmup rounds.  Before timing, the stamped
wire buffer and every output of the parse are checked against the host plans.  Writes one JSON object to --out and prints it.
    python tools/rtp_rate.py [--calls 20] [--warmup 3] [--out profiles/rtp_rate.json] [--streams 4096] [--variants a,b]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from audio_codec_amd import api
from tests.lc3_harness import synth_pcm

T, U, FS, MS, NB, ROOM, ALIGN, N = 64, 64, 48000, 10.0, 80, 12, 4, 480
ALL = ("enc", "egress", "stamp", "parse", "dec", "stamp_host", "parse_host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--variants", default=",".join(ALL))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rtp_rate.json"))
    a = ap.parse_args()
    B = a.streams
    assert B % U == 0
    hip = C.CDLL("libamdhip64.so")
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    ptrs = []

    def put(x):
        x = np.ascontiguousarray(x); p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(max(x.nbytes, 8))) == 0
        assert hip.hipMemcpy(p, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
        ptrs.append(p); return p.value

    def get(p, shape, dtype):
        out = np.zeros(shape, dtype)
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(p), C.c_size_t(out.nbytes), C.c_int(2)) == 0
        return out

    def down(x, p):
        assert hip.hipMemcpy(C.c_void_p(x.ctypes.data), C.c_void_p(p), C.c_size_t(x.nbytes), C.c_int(2)) == 0

    def up(p, x):
        assert hip.hipMemcpy(C.c_void_p(p), C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
    cells = B * T
    counts = np.where(np.arange(B) % 16 == 5, 40, T).astype(np.int32)
    present = int(counts.sum())
    cap = (present - 64) * NB
    room = present * NB + 64
    pitch = (ROOM + NB + ALIGN - 1) // ALIGN * ALIGN                   # every packet is ROOM + NB bytes: the wire buffer is a table of rows
    wire_bytes = cells * pitch
    enc = amd.Batch(B, FS, 1, MS, 0, [NB * 800] * B, device=0)
    dec = amd.DecBatch(B, FS, 1, MS, 0, None, device=0)
    d_pcm = put(np.tile(synth_pcm(U, T, N, FS, seed=9), (B // U, 1, 1)))
    d_out, d_cnt = put(np.zeros(room, np.uint8)), put(counts)
    d_off, d_tot, d_nb, d_fl = put(np.zeros(cells, np.int64)), put(np.zeros(1, np.int64)), put(np.zeros(cells, np.int32)), put(np.zeros(cells, np.uint8))
    enc.set_frame_counts(d_cnt)
    seq_base = (np.arange(B) * 7 % 65536).astype(np.int32)
    ssrc = (0x7FFF0000 + 13 * np.arange(B)).astype(np.int64)           # ascending as uint32, on both sides of 2^31
    ssrc32 = (ssrc & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    ts_base = (np.arange(B) * 100003 % (1 << 32)).astype(np.uint32).view(np.int32)
    pt = np.full(B, 96, np.int32)
    d_base, d_ssrc, d_tsb, d_pt, d_sid = put(seq_base), put(ssrc32), put(ts_base), put(pt), put(np.arange(B, dtype=np.int32))
    q = dict(route=put(np.zeros(cells, np.int32)), seq=put(np.zeros(cells, np.int32)), frame=put(np.zeros(cells, np.int32)), offset=put(np.full(cells, -1, np.int64)),
             size=put(np.zeros(cells, np.int32)), flags=put(np.zeros(cells, np.uint8)), np_=put(np.zeros(1, np.int64)), total=put(np.zeros(1, np.int64)),
             next=put(np.zeros(B, np.int32)), stats=put(np.zeros((B, api.EGR_STATS_WORDS), np.int32)), status=put(np.zeros(cells, np.uint8)),
             work=put(np.zeros(api.egress_work_bytes(B, T) // 8 + 1, np.int64)), wire=put(np.zeros(wire_bytes, np.uint8)))
    s = dict(pst=put(np.zeros(cells, np.uint8)), nts=put(np.zeros(B, np.int32)), nres=put(np.zeros(B, np.uint8)))
    it = dict(stream=put(np.zeros(cells, np.int32)), seq=put(np.zeros(cells, np.int32)), offsets=put(np.zeros(cells, np.int64)), num_bytes=put(np.zeros(cells, np.int32)),
              timestamp=put(np.zeros(cells, np.int32)), marker=put(np.zeros(cells, np.uint8)), status=put(np.zeros(cells, np.uint8)),
              stats=put(np.zeros(api.RTP_STATS_WORDS, np.int32)))
    g = dict(oo=put(np.zeros(cells, np.int64)), onb=put(np.zeros(cells, np.int32)), ci=put(np.zeros(cells, np.int32)), cnt=put(np.zeros(B, np.int32)))
    d_pcm_out, d_st = put(np.zeros((B, T, 1, N), np.int16)), put(np.zeros(cells, np.uint8))
    sv = stream.value

    def egress(sync=False):
        enc.egress_device(T, d_out, room, d_off, d_nb, NB, B, d_base, q["route"], q["seq"], q["frame"], q["offset"], q["size"], q["np_"], q["work"], d_fl,
                          api.ENC_FL_PACK_CAP, d_cnt, None, 16, api.PACK_STREAM_MAJOR, q["wire"], wire_bytes, ROOM, ALIGN, q["flags"], q["total"], q["next"], q["stats"],
                          q["status"], sv, sync)

    def stamp(sync=False):
        enc.rtp_stamp_device(cells, q["np_"], q["route"], q["seq"], q["frame"], q["offset"], q["size"], B, T, d_ssrc, d_tsb, d_pt, N, q["wire"], wire_bytes, ROOM, 0,
                             q["flags"], api.RTP_MARKER_AFTER_HOLE, q["status"], None, q["stats"], s["pst"], s["nts"], s["nres"], sv, sync)

    def parse(sync=False):
        dec.rtp_parse_device(cells, q["wire"], wire_bytes, q["offset"], q["size"], B, d_ssrc, d_sid, it["stream"], it["seq"], it["offsets"], it["num_bytes"], d_pt, 0,
                             it["timestamp"], it["marker"], it["status"], it["stats"], sv, sync)

    def decode(sync=False):
        dec.set_frame_counts(g["cnt"])
        dec.decode_device_packed(q["wire"], wire_bytes, g["oo"], T, d_pcm_out, g["onb"], NB, None, d_st, 16, sv, sync)
    lst = dict(route=np.zeros(cells, np.int32), seq=np.zeros(cells, np.int32), frame=np.zeros(cells, np.int32), offset=np.zeros(cells, np.int64),
               size=np.zeros(cells, np.int32), flags=np.zeros(cells, np.uint8))
    h_np, h_cs, h_stats = np.zeros(1, np.int64), np.zeros((B, T), np.uint8), np.zeros((B, api.EGR_STATS_WORDS), np.int32)
    h_wire = np.zeros(wire_bytes, np.uint8)                           # the host's image of the wire buffer: only its header columns are ever filled

    def strided(dst, src, rows, kind):                                # 12 bytes of each of `rows` rows of the wire buffer
        assert hip.hipMemcpy2D(C.c_void_p(dst), C.c_size_t(pitch), C.c_void_p(src), C.c_size_t(pitch), C.c_size_t(12), C.c_size_t(rows), C.c_int(kind)) == 0

    lib = api.load_library()                                          # the plans through the C calls themselves: no copy of the host's wire image per call
    h_pst, h_nts, h_nres = np.zeros(cells, np.uint8), np.zeros(B, np.int32), np.zeros(B, np.uint8)
    h_items = dict(stream=np.zeros(cells, np.int32), seq=np.zeros(cells, np.int32), offsets=np.zeros(cells, np.int64), num_bytes=np.zeros(cells, np.int32))
    sid = np.arange(B, dtype=np.int32)
    at = lambda x: x.ctypes.data

    def stamp_host():
        assert hip.hipStreamSynchronize(stream) == 0
        down(h_np, q["np_"])
        k = int(h_np[0])
        for name in lst:
            down(lst[name][:k], q[name])
        down(h_cs, q["status"]); down(h_stats, q["stats"])
        assert lib.lc3plus_plan_rtp_stamp(k, at(h_np), at(lst["route"]), at(lst["seq"]), at(lst["frame"]), at(lst["offset"]), at(lst["size"]), at(lst["flags"]), B, T,
                                          at(ssrc32), at(ts_base), at(pt), N, api.RTP_MARKER_AFTER_HOLE, at(h_cs), None, at(h_stats), at(h_wire), wire_bytes, ROOM, 0,
                                          at(h_pst), at(h_nts), at(h_nres), None, 0) == 0
        strided(q["wire"], at(h_wire), k, 1)
        up(s["pst"], h_pst[:k]); up(s["nts"], h_nts); up(s["nres"], h_nres)

    def parse_host():
        assert hip.hipStreamSynchronize(stream) == 0
        down(h_np, q["np_"])
        k = int(h_np[0])
        down(lst["offset"][:k], q["offset"]); down(lst["size"][:k], q["size"])
        strided(at(h_wire), q["wire"], k, 2)
        assert lib.lc3plus_plan_rtp_parse(B, k, at(h_wire), wire_bytes, at(lst["offset"]), at(lst["size"]), B, at(ssrc32), at(sid), at(pt), 0, at(h_items["stream"]),
                                          at(h_items["seq"]), at(h_items["offsets"]), at(h_items["num_bytes"]), None, None, None, None, None, 0) == 0
        for name in h_items:
            up(it[name], h_items[name][:k])
    calls = {"enc": lambda: enc.encode_device_packed(d_pcm, 16, T, d_out, cap, api.PACK_STREAM_MAJOR, None, None, d_off, d_tot, d_nb, d_fl, sv, False),
             "egress": egress, "stamp": stamp, "parse": parse, "dec": decode, "stamp_host": stamp_host, "parse_host": parse_host}
    chosen = [k for k in ALL if k in a.variants.split(",")]
    times = {k: [] for k in chosen}
    try:
        calls["enc"]()
        egress(sync=True)
        k = int(get(q["np_"], 1, np.int64)[0])
        assert k == present - 64
        before = get(q["wire"], wire_bytes, np.uint8)
        stamp(sync=True)
        L = {name: get(q[name], cells, lst[name].dtype) for name in lst}
        cs, stats = get(q["status"], (B, T), np.uint8), get(q["stats"], (B, api.EGR_STATS_WORDS), np.int32)
        want = api.plan_rtp_stamp(L["route"], L["seq"], L["frame"], L["offset"], L["size"], ssrc, ts_base, pt, N, T, before, ROOM, 0, L["flags"], k,
                                  api.RTP_MARKER_AFTER_HOLE, cs, None, stats)
        wire = get(q["wire"], wire_bytes, np.uint8)
        assert np.array_equal(wire, want["wire"]) and np.array_equal(get(s["pst"], cells, np.uint8)[:k], want["pkt_status"][:k])
        assert np.array_equal(get(s["nts"], B, np.int32), want["next_ts"]) and np.array_equal(get(s["nres"], B, np.uint8), want["next_resume"])
        parse(sync=True)
        want = api.plan_rtp_parse(B, wire, L["offset"], L["size"], ssrc, np.arange(B), pt, 0)
        for name, dt in (("stream", np.int32), ("seq", np.int32), ("offsets", np.int64), ("num_bytes", np.int32), ("timestamp", np.int32), ("marker", np.uint8),
                         ("status", np.uint8)):
            assert np.array_equal(get(it[name], cells, dt), want[name]), name
        assert np.array_equal(get(it["stats"], api.RTP_STATS_WORDS, np.int32), want["stats"]) and want["stats"][0] == k
        dec.ingest_device(cells, it["stream"], it["seq"], it["offsets"], it["num_bytes"], d_base, T, g["oo"], g["onb"], g["ci"], g["cnt"], 16, None, None, None, None, None,
                          sv, True)
        for rnd in range(a.warmup + a.calls):
            for name in times:
                if name.endswith("_host"):
                    t0 = time.perf_counter(); calls[name](); ms = (time.perf_counter() - t0) * 1e3
                else:
                    assert hip.hipEventRecord(ev0, stream) == 0
                    calls[name]()
                    assert hip.hipEventRecord(ev1, stream) == 0 and hip.hipEventSynchronize(ev1) == 0
                    f = C.c_float(0); assert hip.hipEventElapsedTime(C.byref(f), ev0, ev1) == 0
                    ms = f.value
                if rnd >= a.warmup:
                    times[name].append(ms)
    finally:
        enc.set_frame_counts(None)
        dec.set_frame_counts(None)
        enc.close()
        dec.close()
        for p in ptrs:
            hip.hipFree(p)
    hip.hipEventDestroy(ev0); hip.hipEventDestroy(ev1); hip.hipStreamDestroy(stream)
    out = {"tool": "rtp_rate", "streams": B, "frames": T, "frame_bytes": NB, "cells": cells, "packets": k, "header_room": ROOM, "payload_room": 0, "align": ALIGN,
           "ssrc_table_entries": B, "calls": a.calls, "warmup": a.warmup, "variants": {}}
    for name, v in times.items():
        out["variants"][name] = {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    va = out["variants"]
    ms = lambda name: va[name]["ms_median"]
    if set(ALL) <= set(va):
        out["stamp_over_egress"] = round(ms("stamp") / ms("egress"), 5)
        out["stamp_over_enc"] = round(ms("stamp") / ms("enc"), 5)
        out["stamp_over_host"] = round(ms("stamp") / ms("stamp_host"), 5)
        out["parse_over_dec"] = round(ms("parse") / ms("dec"), 5)
        out["parse_over_host"] = round(ms("parse") / ms("parse_host"), 5)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
