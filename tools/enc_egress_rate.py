"""Packet egress rate (lc3plus_enc_batch_egress) behind an encode_packed call, beside that call, the host detour it replaces and a plain device copy of the same
bytes: 4096 mono streams x 64 frames, 48 kHz / 10 ms, 80-byte frames, one batch, one process.  One stream in 16 is ragged (40 frames) and the capacity cuts the
last 64 frames, so the list is shorter than the table.  Variants, alternated run by run:
  enc       lc3plus_enc_batch_encode_packed (set_frame_counts on), the call the egress follows
  inplace1  egress in place, identity routes, every output asked for
  inplace4  the same with four routes per stream (nothing is copied: what fan-out costs the list alone)
  wire1     egress into a wire buffer, identity routes, 12 bytes of header room, packets aligned to 4
  wire4     the same with four routes per stream
  host      the path the call replaces: synchronise, offsets, num_bytes and flags to the host, api.plan_egress there (in place), the five list arrays and the
            length back
  copy1     hipMemcpyAsync device to device of as many bytes as wire1's payloads, copy4 of wire4's: the yardstick for the copy kernel
Device variants: device events around the call on the call's stream (sync = 0).  host: the host clock from before the synchronise (nothing is pending: the wait
itself is not in the figure) to the return of the last copy.  Per variant the median, the fastest and the slowest of --calls runs after --warmup rounds.  What
wire mode adds to a call is given as wire minus inplace of the same routes, a difference of two medians and named as such; the copy kernel's own duration is not
in these figures: read it under rocprofv3 --kernel-trace --stats, one fan-out per run (--variants wire4 --out ''; profiles/egress_kernel_stats.txt).  Before timing,
every device output is checked against api.plan_egress.  Writes one JSON object to --out and prints it.
    python tools/enc_egress_rate.py [--calls 20] [--warmup 3] [--out profiles/enc_egress_rate.json] [--streams 4096] [--variants a,b]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from audio_codec_amd import api
from tests.lc3_harness import synth_pcm

T, U, FS, MS, NB, ROOM, ALIGN, FAN = 64, 64, 48000, 10.0, 80, 12, 4, 4
ALL = ("enc", "inplace1", "inplace4", "wire1", "wire4", "host", "copy1", "copy4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--variants", default=",".join(ALL))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enc_egress_rate.json"))
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
    cells = B * T
    counts = np.where(np.arange(B) % 16 == 5, 40, T).astype(np.int32)
    present = int(counts.sum())
    cap = (present - 64) * NB
    room = present * NB + 64
    enc = amd.Batch(B, FS, 1, MS, 0, [NB * 800] * B, device=0)
    d_pcm = put(np.tile(synth_pcm(U, T, 480, FS, seed=9), (B // U, 1, 1)))
    d_out, d_cnt = put(np.zeros(room, np.uint8)), put(counts)
    d_off, d_tot, d_nb, d_fl = put(np.zeros(cells, np.int64)), put(np.zeros(1, np.int64)), put(np.zeros(cells, np.int32)), put(np.zeros(cells, np.uint8))
    enc.set_frame_counts(d_cnt)
    routes = {1: None, FAN: np.repeat(np.arange(B), FAN).astype(np.int32)}
    dev = {}
    for fan, src in routes.items():
        R = B * fan
        n = R * T
        dev[fan] = dict(R=R, n=n, src=src, d_src=put(src) if src is not None else None, base=(np.arange(R) * 7 % 65536).astype(np.int32),
                        route=put(np.zeros(n, np.int32)), seq=put(np.zeros(n, np.int32)), frame=put(np.zeros(n, np.int32)), offset=put(np.zeros(n, np.int64)),
                        size=put(np.zeros(n, np.int32)), flags=put(np.zeros(n, np.uint8)), np_=put(np.zeros(1, np.int64)), total=put(np.zeros(1, np.int64)),
                        next=put(np.zeros(R, np.int32)), stats=put(np.zeros((R, api.EGR_STATS_WORDS), np.int32)), status=put(np.zeros(n, np.uint8)),
                        work=put(np.zeros(api.egress_work_bytes(R, T) // 8 + 1, np.int64)), wire_bytes=n * ((ROOM + NB + ALIGN - 1) // ALIGN * ALIGN))
        dev[fan]["d_base"] = put(dev[fan]["base"])
        dev[fan]["wire"] = put(np.zeros(dev[fan]["wire_bytes"], np.uint8))
    d_scratch = put(np.zeros(cells * FAN * NB, np.uint8))               # the plain copy's destination

    def egress(fan, wire, sync=False):
        q = dev[fan]
        enc.egress_device(T, d_out, room, d_off, d_nb, NB, q["R"], q["d_base"], q["route"], q["seq"], q["frame"], q["offset"], q["size"], q["np_"], q["work"], d_fl,
                          api.ENC_FL_PACK_CAP, d_cnt, q["d_src"], 16, api.PACK_STREAM_MAJOR, q["wire"] if wire else None, q["wire_bytes"] if wire else 0,
                          ROOM if wire else 0, ALIGN if wire else 1, q["flags"], q["total"], q["next"], q["stats"], q["status"], stream.value, sync)
    tables = [np.zeros((B, T), np.int64), np.zeros((B, T), np.int32), np.zeros((B, T), np.uint8)]

    def host():
        assert hip.hipStreamSynchronize(stream) == 0
        for x, p in zip(tables, (d_off, d_nb, d_fl)):
            assert hip.hipMemcpy(C.c_void_p(x.ctypes.data), C.c_void_p(p), C.c_size_t(x.nbytes), C.c_int(2)) == 0
        r = api.plan_egress(B, np.zeros(8, np.uint8), tables[0], tables[1], dev[1]["base"], NB, tables[2], api.ENC_FL_PACK_CAP, counts, None, 16,
                            api.PACK_STREAM_MAJOR, optional=(), frames_capacity=room)
        k = r["n_packets"]
        q = dev[1]
        for p, x in ((q["route"], r["pkt_route"][:k]), (q["seq"], r["pkt_seq"][:k]), (q["frame"], r["pkt_frame"][:k]), (q["offset"], r["pkt_offset"][:k]),
                     (q["size"], r["pkt_size"][:k]), (q["np_"], np.array([k], np.int64))):
            assert hip.hipMemcpy(C.c_void_p(p), C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
    payload = {}

    def plain(fan):
        assert hip.hipMemcpyAsync(C.c_void_p(d_scratch), C.c_void_p(dev[fan]["wire"]), C.c_size_t(payload[fan]), C.c_int(3), stream) == 0
    calls = {
        "enc": lambda: enc.encode_device_packed(d_pcm, 16, T, d_out, cap, api.PACK_STREAM_MAJOR, None, None, d_off, d_tot, d_nb, d_fl, stream.value, False),
        "inplace1": lambda: egress(1, False), "inplace4": lambda: egress(FAN, False), "wire1": lambda: egress(1, True), "wire4": lambda: egress(FAN, True),
        "host": host, "copy1": lambda: plain(1), "copy4": lambda: plain(FAN),
    }
    chosen = [k for k in ALL if k in a.variants.split(",")]
    times = {k: [] for k in chosen}
    packets = {}
    try:
        calls["enc"]()
        assert hip.hipStreamSynchronize(stream) == 0
        off, nb, fl = get(d_off, (B, T), np.int64), get(d_nb, (B, T), np.int32), get(d_fl, (B, T), np.uint8)
        frames = get(d_out, room, np.uint8)
        for fan in routes:                                              # every output of both modes against the host plan
            q = dev[fan]
            for wire in (False, True):
                egress(fan, wire, sync=True)
                want = api.plan_egress(B, frames, off, nb, q["base"], NB, fl, api.ENC_FL_PACK_CAP, counts, q["src"], 16, api.PACK_STREAM_MAJOR,
                                       np.zeros(q["wire_bytes"], np.uint8) if wire else None, None, ROOM if wire else 0, ALIGN if wire else 1, frames_capacity=room)
                k = want["n_packets"]
                assert int(get(q["np_"], 1, np.int64)[0]) == k == fan * (present - 64) and int(get(q["total"], 1, np.int64)[0]) == want["wire_total"]
                for name, key, dt in (("route", "pkt_route", np.int32), ("seq", "pkt_seq", np.int32), ("frame", "pkt_frame", np.int32), ("offset", "pkt_offset", np.int64),
                                      ("size", "pkt_size", np.int32), ("flags", "pkt_flags", np.uint8)):
                    assert np.array_equal(get(q[name], q["n"], dt)[:k], want[key][:k]), (fan, wire, key)
                assert np.array_equal(get(q["next"], q["R"], np.int32), want["next_seq"]) and np.array_equal(get(q["stats"], (q["R"], 4), np.int32), want["stats"])
                assert np.array_equal(get(q["status"], (q["R"], T), np.uint8), want["cell_status"])
                if wire:
                    assert np.array_equal(get(q["wire"], q["wire_bytes"], np.uint8), want["wire"]), (fan, "wire")
            packets[fan], payload[fan] = k, k * NB
        for rnd in range(a.warmup + a.calls):
            for k in times:
                if k == "host":
                    t0 = time.perf_counter(); calls[k](); ms = (time.perf_counter() - t0) * 1e3
                else:
                    assert hip.hipEventRecord(ev0, stream) == 0
                    calls[k]()
                    assert hip.hipEventRecord(ev1, stream) == 0 and hip.hipEventSynchronize(ev1) == 0
                    f = C.c_float(0); assert hip.hipEventElapsedTime(C.byref(f), ev0, ev1) == 0
                    ms = f.value
                if rnd >= a.warmup:
                    times[k].append(ms)
    finally:
        enc.set_frame_counts(None)
        enc.close()
        for p in ptrs:
            hip.hipFree(p)
    hip.hipEventDestroy(ev0); hip.hipEventDestroy(ev1); hip.hipStreamDestroy(stream)
    out = {"tool": "enc_egress_rate", "streams": B, "frames": T, "frame_bytes": NB, "cells": cells, "present_frames": present, "frames_cut_by_capacity": 64,
           "header_room": ROOM, "align": ALIGN, "fan_out": FAN, "packets": {"fan1": packets[1], "fan%d" % FAN: packets[FAN]},
           "payload_bytes": {"fan1": payload[1], "fan%d" % FAN: payload[FAN]}, "calls": a.calls, "warmup": a.warmup, "variants": {}}
    for k, v in times.items():
        med = float(np.median(v))
        out["variants"][k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    va = out["variants"]
    ms = lambda k: va[k]["ms_median"]
    if set(ALL) <= set(va):
        out["inplace1_over_enc"] = round(ms("inplace1") / ms("enc"), 5)
        out["wire1_over_enc"] = round(ms("wire1") / ms("enc"), 5)
        out["wire4_over_enc"] = round(ms("wire4") / ms("enc"), 5)
        out["inplace1_over_host"] = round(ms("inplace1") / ms("host"), 5)
        for fan, w, i, c in ((1, "wire1", "inplace1", "copy1"), (FAN, "wire4", "inplace4", "copy4")):
            out["wire_mode_fan%d" % fan] = {"ms_wire_minus_inplace": round(ms(w) - ms(i), 4), "plain_copy_ms": ms(c),     # differences of two medians
                                            "plain_copy_payload_GB_per_s": round(payload[fan] / ms(c) / 1e6, 1)}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
