"""Redundant-audio rates (lc3plus_enc_batch_red_pack, lc3plus_dec_batch_red_unpack) beside the calls they stand between and what they could be replaced by: 4096
mono streams x 64 frames, 48 kHz / 10 ms, 80-byte frames, every frame present, one encoder batch and one decoder batch, one process.  Variants, alternated round
by round:
  egress_wire   the wire-mode egress of the same frames, identity routes, 12 bytes of header room, packets aligned to 4: what a sender without redundancy runs
  pack_dK       the pack behind the in-place egress at depth K = 0, 1, 2, 4 for every route, no tails in, tails out, every output asked for
  memcpy_dK     one hipMemcpyAsync, device to device, of as many bytes as pack_dK's wire_total
  pack_host_dK  the path the pack replaces, K = 1 and 4: synchronise, the list, the tables and the frames to the host, lc3plus_plan_red_pack there, the wire
                buffer's wire_total bytes and the records back
  parse         the RTP parse of the stamped depth-2 wire buffer, the pack's records as the datagrams: the call in front of the unpack
  unpack        the unpack of the parse's items at max_red 2, every output asked for
Device variants: device events around --reps calls queued back to back on one stream (sync = 0), divided by --reps.  Host variants: the host clock from before
the synchronise (nothing is pending) to the return of the last copy.  Per variant the median, the fastest and the slowest of --calls rounds after --warmup
rounds.  Before timing, the depth-2 wire buffer, records and tails and every output of the unpack are checked against the host plans.  Writes one JSON object to
--out and prints it.
    python tools/red_rate.py [--calls 20] [--warmup 3] [--reps 10] [--out profiles/red_rate.json] [--streams 4096] [--variants a,b]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from audio_codec_amd import api
from tests.lc3_harness import synth_pcm

T, U, FS, MS, NB, ROOM, ALIGN, N = 64, 64, 48000, 10.0, 80, 12, 4, 480
DEPTHS, HOST_DEPTHS, CHECK_DEPTH = (0, 1, 2, 4), (1, 4), 2
ALL = (("egress_wire",) + tuple("pack_d%d" % k for k in DEPTHS) + tuple("memcpy_d%d" % k for k in DEPTHS) + tuple("pack_host_d%d" % k for k in HOST_DEPTHS) +
       ("parse", "unpack"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--variants", default=",".join(ALL))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "red_rate.json"))
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
    room = cells * NB + 64
    pitch = lambda k: (ROOM + 4 * k + 1 + (k + 1) * NB + ALIGN - 1) // ALIGN * ALIGN            # the largest packet at depth k
    wire_bytes = cells * pitch(max(DEPTHS))
    stride = api.red_tail_stride(NB)
    enc = amd.Batch(B, FS, 1, MS, 0, [NB * 800] * B, device=0)
    dec = amd.DecBatch(B, FS, 1, MS, 0, None, device=0)
    d_pcm = put(np.tile(synth_pcm(U, T, N, FS, seed=9), (B // U, 1, 1)))
    d_out = put(np.zeros(room, np.uint8))
    d_off, d_tot, d_nb, d_fl = put(np.zeros(cells, np.int64)), put(np.zeros(1, np.int64)), put(np.zeros(cells, np.int32)), put(np.zeros(cells, np.uint8))
    seq_base = (np.arange(B) * 7 % 65536).astype(np.int32)
    ssrc = (0x7FFF0000 + 13 * np.arange(B)).astype(np.int64)           # ascending as uint32, on both sides of 2^31
    ssrc32 = (ssrc & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    ts_base = (np.arange(B) * 100003 % (1 << 32)).astype(np.uint32).view(np.int32)
    red_pt, blk_pt = np.full(B, 97, np.int32), np.full(B, 96, np.int32)
    d_base, d_ssrc, d_tsb, d_red_pt, d_blk_pt, d_sid = put(seq_base), put(ssrc32), put(ts_base), put(red_pt), put(blk_pt), put(np.arange(B, dtype=np.int32))
    mk = lambda: dict(route=put(np.zeros(cells, np.int32)), seq=put(np.zeros(cells, np.int32)), frame=put(np.zeros(cells, np.int32)), offset=put(np.full(cells, -1, np.int64)),
                      size=put(np.zeros(cells, np.int32)), flags=put(np.zeros(cells, np.uint8)), np_=put(np.zeros(1, np.int64)), total=put(np.zeros(1, np.int64)),
                      next=put(np.zeros(B, np.int32)), stats=put(np.zeros((B, api.EGR_STATS_WORDS), np.int32)), status=put(np.zeros(cells, np.uint8)),
                      work=put(np.zeros(api.egress_work_bytes(B, T) // 8 + 1, np.int64)))
    q, w = mk(), mk()                                                 # the in-place egress's list, and the wire-mode egress's
    d_wire, d_wire2 = put(np.zeros(wire_bytes, np.uint8)), put(np.zeros(wire_bytes, np.uint8))
    r = dict(offset=put(np.full(cells, -1, np.int64)), size=put(np.zeros(cells, np.int32)), flags=put(np.zeros(cells, np.uint8)), blocks=put(np.zeros(cells, np.uint8)),
             total=put(np.zeros(1, np.int64)), stats=put(np.zeros((B, api.RED_STATS_WORDS), np.int32)), work=put(np.zeros(api.red_work_bytes(cells) // 8 + 1, np.int64)),
             tb=put(np.zeros(B * max(DEPTHS) * stride, np.uint8)), tz=put(np.zeros(B * max(DEPTHS), np.int32)), pst=put(np.zeros(cells, np.uint8)))
    it = dict(stream=put(np.zeros(cells, np.int32)), seq=put(np.zeros(cells, np.int32)), offsets=put(np.zeros(cells, np.int64)), num_bytes=put(np.zeros(cells, np.int32)),
              timestamp=put(np.zeros(cells, np.int32)), status=put(np.zeros(cells, np.uint8)), stats=put(np.zeros(api.RTP_STATS_WORDS, np.int32)))
    K = CHECK_DEPTH + 1
    o = dict(stream=put(np.zeros(cells * K, np.int32)), seq=put(np.zeros(cells * K, np.int32)), offsets=put(np.zeros(cells * K, np.int64)),
             num_bytes=put(np.zeros(cells * K, np.int32)), timestamp=put(np.zeros(cells * K, np.int32)), gen=put(np.zeros(cells * K, np.uint8)),
             status=put(np.zeros(cells, np.uint8)), stats=put(np.zeros(api.RED_UNPACK_STATS_WORDS, np.int32)))
    sv = stream.value

    def egress(lst, wire, sync=False):
        enc.egress_device(T, d_out, room, d_off, d_nb, NB, B, d_base, lst["route"], lst["seq"], lst["frame"], lst["offset"], lst["size"], lst["np_"], lst["work"], d_fl,
                          api.ENC_FL_PACK_CAP, None, None, 16, api.PACK_STREAM_MAJOR, wire, wire_bytes if wire else 0, ROOM if wire else 0, ALIGN if wire else 1,
                          lst["flags"], lst["total"], lst["next"], lst["stats"], lst["status"], sv, sync)

    def pack(depth, sync=False):
        enc.red_pack_device(T, d_out, room, d_off, d_nb, NB, B, cells, q["np_"], q["route"], q["frame"], depth, d_blk_pt, N, 1400, d_wire, wire_bytes, r["offset"], r["size"],
                            r["work"], ROOM, ALIGN, d_fl, api.ENC_FL_PACK_CAP, None, None, None, None, None, stride, r["tb"] if depth else None, r["tz"] if depth else None,
                            r["flags"], r["blocks"], r["total"], r["stats"], sv, sync)

    def stamp(sync=False):
        enc.rtp_stamp_device(cells, q["np_"], q["route"], q["seq"], q["frame"], r["offset"], r["size"], B, T, d_ssrc, d_tsb, d_red_pt, N, d_wire, wire_bytes, ROOM, 0,
                             r["flags"], api.RTP_MARKER_NEVER, None, None, q["stats"], r["pst"], None, None, sv, sync)

    def parse(sync=False):
        dec.rtp_parse_device(cells, d_wire, wire_bytes, r["offset"], r["size"], B, d_ssrc, d_sid, it["stream"], it["seq"], it["offsets"], it["num_bytes"], d_red_pt, 0,
                             it["timestamp"], None, it["status"], it["stats"], sv, sync)

    def unpack(sync=False):
        dec.red_unpack_device(cells, it["stream"], it["seq"], it["offsets"], it["num_bytes"], d_wire, wire_bytes, CHECK_DEPTH, N, o["stream"], o["seq"], o["offsets"],
                              o["num_bytes"], it["timestamp"], d_blk_pt, o["timestamp"], o["gen"], o["status"], o["stats"], sv, sync)
    totals = {}

    def memcpy(depth):
        assert hip.hipMemcpyAsync(C.c_void_p(d_wire2), C.c_void_p(d_wire), C.c_size_t(totals[depth]), C.c_int(3), stream) == 0
    lib = api.load_library()                                          # the plan through the C call itself: no copy of the host's arrays per call
    at = lambda x: x.ctypes.data
    h = dict(np_=np.zeros(1, np.int64), route=np.zeros(cells, np.int32), frame=np.zeros(cells, np.int32), off=np.zeros(cells, np.int64), nb=np.zeros(cells, np.int32),
             fl=np.zeros(cells, np.uint8), frames=np.zeros(room, np.uint8), wire=np.zeros(wire_bytes, np.uint8), r_off=np.zeros(cells, np.int64),
             r_size=np.zeros(cells, np.int32), r_flags=np.zeros(cells, np.uint8), total=np.zeros(1, np.int64), work=np.zeros(api.red_work_bytes(cells) // 8 + 1, np.int64),
             tb=np.zeros(B * max(DEPTHS) * stride, np.uint8), tz=np.zeros(B * max(DEPTHS), np.int32))

    def pack_host(depth):
        assert hip.hipStreamSynchronize(stream) == 0
        down(h["np_"], q["np_"])
        k = int(h["np_"][0])
        down(h["route"][:k], q["route"]); down(h["frame"][:k], q["frame"])
        down(h["off"], d_off); down(h["nb"], d_nb); down(h["fl"], d_fl); down(h["frames"], d_out)
        assert lib.lc3plus_plan_red_pack(B, T, at(h["frames"]), room, at(h["off"]), at(h["nb"]), NB, at(h["fl"]), api.ENC_FL_PACK_CAP, None, B, None, k, at(h["np_"]),
                                         at(h["route"]), at(h["frame"]), depth, None, at(blk_pt), N, 1400, None, None, stride, at(h["tb"]), at(h["tz"]), at(h["wire"]),
                                         wire_bytes, ROOM, ALIGN, at(h["r_off"]), at(h["r_size"]), at(h["r_flags"]), None, at(h["total"]), None, at(h["work"]), None, 0) == 0
        up(d_wire, h["wire"][:int(h["total"][0])])
        up(r["offset"], h["r_off"][:k]); up(r["size"], h["r_size"][:k]); up(r["flags"], h["r_flags"][:k])
        up(r["tb"], h["tb"][:B * depth * stride]); up(r["tz"], h["tz"][:B * depth])
    calls = {"egress_wire": lambda: egress(w, d_wire2), "parse": parse, "unpack": unpack}
    for k in DEPTHS:
        calls["pack_d%d" % k] = lambda k=k: pack(k)
        calls["memcpy_d%d" % k] = lambda k=k: memcpy(k)
    for k in HOST_DEPTHS:
        calls["pack_host_d%d" % k] = lambda k=k: pack_host(k)
    chosen = [k for k in ALL if k in a.variants.split(",")]
    times = {k: [] for k in chosen}
    try:
        enc.encode_device_packed(d_pcm, 16, T, d_out, room, api.PACK_STREAM_MAJOR, None, None, d_off, d_tot, d_nb, d_fl, sv, False)
        egress(q, None, sync=True)
        n = int(get(q["np_"], 1, np.int64)[0])
        assert n == cells
        for k in DEPTHS:                                              # the bytes each depth writes
            pack(k, sync=True)
            totals[k] = int(get(r["total"], 1, np.int64)[0])
        # the depth-2 pack, its stamp and parse, and the unpack against the host plans
        assert hip.hipMemset(C.c_void_p(d_wire), 0, C.c_size_t(wire_bytes)) == 0
        pack(CHECK_DEPTH, sync=True)
        frames, off, nb, fl = get(d_out, room, np.uint8), get(d_off, (B, T), np.int64), get(d_nb, (B, T), np.int32), get(d_fl, (B, T), np.uint8)
        route, frame = get(q["route"], cells, np.int32), get(q["frame"], cells, np.int32)
        want = api.plan_red_pack(B, frames, off, nb, NB, route, frame, blk_pt, N, np.zeros(wire_bytes, np.uint8), CHECK_DEPTH, None, 1400, n, fl, api.ENC_FL_PACK_CAP,
                                 header_room=ROOM, align=ALIGN, tail_stride=stride)
        assert np.array_equal(get(d_wire, wire_bytes, np.uint8), want["wire"]) and want["wire_total"] == totals[CHECK_DEPTH]
        for name, key, dt in (("offset", "red_offset", np.int64), ("size", "red_size", np.int32), ("flags", "red_flags", np.uint8), ("blocks", "red_blocks", np.uint8)):
            assert np.array_equal(get(r[name], cells, dt), want[key]), name
        assert np.array_equal(get(r["stats"], (B, api.RED_STATS_WORDS), np.int32), want["route_stats"]) and not want["red_flags"].any()
        assert np.array_equal(get(r["tz"], (B, CHECK_DEPTH), np.int32), want["tail_sizes"])
        assert np.array_equal(get(r["tb"], (B, CHECK_DEPTH, stride), np.uint8)[:, :, :NB], want["tail_bytes"][:, :, :NB])
        stamp(sync=True)
        parse(sync=True)
        unpack(sync=True)
        wire = get(d_wire, wire_bytes, np.uint8)
        items = {name: get(it[name], cells, np.int64 if name == "offsets" else np.int32) for name in ("stream", "seq", "offsets", "num_bytes", "timestamp")}
        assert get(it["stats"], api.RTP_STATS_WORDS, np.int32)[0] == n
        u = api.plan_red_unpack(B, items["stream"], items["seq"], items["offsets"], items["num_bytes"], wire, N, CHECK_DEPTH, items["timestamp"], blk_pt)
        for name in api.RED_UNPACK_OUTPUTS:
            assert np.array_equal(get(o[name], u[name].shape, u[name].dtype), u[name]), name
        assert u["stats"][0] == n and int((u["stream"] >= 0).sum()) == n + int(want["route_stats"][:, 1].sum())
        for rnd in range(a.warmup + a.calls):
            for name in times:
                if name in ("parse", "unpack"):                       # what these read, which the packs in between overwrite: the depth-2 packets, stamped, and their items
                    pack(CHECK_DEPTH); stamp(); parse(sync=True)
                if "_host" in name:
                    t0 = time.perf_counter(); calls[name](); ms = (time.perf_counter() - t0) * 1e3
                else:
                    assert hip.hipEventRecord(ev0, stream) == 0
                    for _ in range(a.reps):
                        calls[name]()
                    assert hip.hipEventRecord(ev1, stream) == 0 and hip.hipEventSynchronize(ev1) == 0
                    f = C.c_float(0); assert hip.hipEventElapsedTime(C.byref(f), ev0, ev1) == 0
                    ms = f.value / a.reps
                if rnd >= a.warmup:
                    times[name].append(ms)
    finally:
        enc.close()
        dec.close()
        for p in ptrs:
            hip.hipFree(p)
    hip.hipEventDestroy(ev0); hip.hipEventDestroy(ev1); hip.hipStreamDestroy(stream)
    out = {"tool": "red_rate", "streams": B, "frames": T, "frame_bytes": NB, "packets": n, "header_room": ROOM, "align": ALIGN, "calls": a.calls, "warmup": a.warmup,
           "reps": a.reps, "wire_total_bytes": {"d%d" % k: v for k, v in totals.items()}, "variants": {}}
    for name, v in times.items():
        out["variants"][name] = {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    va = out["variants"]
    ms = lambda name: va[name]["ms_median"]
    if set(ALL) <= set(va):
        out["pack_d0_over_egress_wire"] = round(ms("pack_d0") / ms("egress_wire"), 4)
        for k in DEPTHS:
            out["pack_d%d_over_memcpy" % k] = round(ms("pack_d%d" % k) / ms("memcpy_d%d" % k), 4)
            out["pack_d%d_GBps_written" % k] = round(totals[k] / ms("pack_d%d" % k) / 1e6, 2)
        for k in HOST_DEPTHS:
            out["pack_d%d_over_host" % k] = round(ms("pack_d%d" % k) / ms("pack_host_d%d" % k), 5)
        out["unpack_over_parse"] = round(ms("unpack") / ms("parse"), 4)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
