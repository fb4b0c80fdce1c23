"""Generic-FEC rates (lc3plus_enc_batch_fec_encode, lc3plus_dec_batch_fec_recover) beside the calls they stand between and what they could be replaced by: 4096
routes x 64 frames of 80 bytes (random bytes: these kernels move and XOR bytes, whatever they hold), every frame present, one encoder batch and one decoder
batch, one process.  Variants, alternated round by round:
  egress_wire     the wire-mode egress of the frames, identity routes, 12 bytes of header room: the call that wrote the packets the encoder reads
  encode_kK       the encoder behind egress and stamp with groups of K = 2, 4, 16 for every route, no state buffers, every output asked for
  memcpy_kK       one hipMemcpyAsync, device to device, of as many bytes as encode_kK reads plus writes (the wire buffer and the FEC packets)
  encode_host_kK  the path the encoder replaces: synchronise, the list and the wire buffer to the host, lc3plus_plan_fec_encode there, the FEC buffer and
                  the records back
  parse           the RTP parse of the media datagrams: the call in front of the recovery
  recover_pP      the recovery over groups of 4 with P = 2, 10 per cent of the media packets lost at random, every output asked for
  recover_host_pP the path it replaces: synchronise, the datagram list, the items and the ring to the host, lc3plus_plan_fec_recover there, the recovery region
                  and the records back
Device variants: device events around --reps calls queued back to back on one stream (sync = 0), divided by --reps.  Host variants: the host clock from before
the synchronise (nothing is pending) to the return of the last copy.  Per variant the median, the fastest and the slowest of --calls rounds after --warmup
rounds.  Before timing, the FEC buffer and records at every K and every output of the recovery at both loss rates are checked against the host plans.  Writes one JSON
object to --out and prints it.
    python tools/fec_rate.py [--calls 20] [--warmup 3] [--reps 10] [--out profiles/fec_rate.json] [--streams 4096] [--variants a,b]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from audio_codec_amd import api

T, FS, MS, NB, ROOM, N = 64, 48000, 10.0, 80, 12, 480
GROUPS, HOST_GROUPS, CHECK_GROUP, LOSSES, WINDOW = (2, 4, 16), (2, 4, 16), 4, (2, 10), 64
ALL = (("egress_wire",) + tuple("encode_k%d" % k for k in GROUPS) + tuple("memcpy_k%d" % k for k in GROUPS) + tuple("encode_host_k%d" % k for k in HOST_GROUPS) +
       ("parse",) + tuple("recover_p%d" % p for p in LOSSES) + tuple("recover_host_p%d" % p for p in LOSSES))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--variants", default=",".join(ALL))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fec_rate.json"))
    a = ap.parse_args()
    B = a.streams
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
    rng = np.random.RandomState(5)
    cells, pkt = B * T, ROOM + NB
    W = cells * pkt
    fstride = (12 + 14 + NB + 15) & ~15
    nf_max = cells // min(GROUPS)
    F = nf_max * fstride
    rstride = (pkt + 3) & ~3
    cap = W + F + (cells // CHECK_GROUP) * rstride
    enc = amd.Batch(B, FS, 1, MS, 0, [NB * 800] * B, device=0)
    dec = amd.DecBatch(B, FS, 1, MS, 0, None, device=0)
    d_frames = put(rng.randint(0, 256, cells * NB).astype(np.uint8))
    d_off, d_nb = put(np.arange(cells, dtype=np.int64) * NB), put(np.full(cells, NB, np.int32))
    seq_base = (np.arange(B) * 7 % 65536).astype(np.int32)
    u32 = lambda x: (np.asarray(x, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    ssrc, fssrc = u32(0x7FFF0000 + 13 * np.arange(B)), u32(0x100 + np.arange(B))
    d_base, d_ssrc, d_fssrc, d_tsb = put(seq_base), put(ssrc), put(fssrc), put(u32(np.arange(B) * 100003))
    d_pt, d_fpt, d_sid = put(np.full(B, 96, np.int32)), put(np.full(B, 97, np.int32)), put(np.arange(B, dtype=np.int32))
    i32, i64, u8 = (lambda n: put(np.zeros(n, np.int32))), (lambda n: put(np.zeros(n, np.int64))), (lambda n: put(np.zeros(n, np.uint8)))
    q = dict(route=i32(cells), seq=i32(cells), frame=i32(cells), offset=i64(cells), size=i32(cells), flags=u8(cells), np_=i64(1), next=i32(B), stats=i32(B * 4),
             work=put(np.zeros(api.egress_work_bytes(B, T) // 8 + 1, np.int64)), pst=u8(cells))
    d_ring, d_copy = put(np.zeros(cap + 8, np.uint8)), put(np.zeros(W + F, np.uint8))
    d_fwire = d_ring + W
    f = dict(n=i64(1), route=i32(nf_max), seq=i32(nf_max), frame=i32(nf_max), offset=i64(nf_max), size=i32(nf_max), flags=u8(nf_max), mask=i32(nf_max), next=i32(B),
             stats=i32(B * 4), work=put(np.zeros(api.fec_work_bytes(B, T) // 8 + 1, np.int64)), pst=u8(nf_max), fbase=put(np.full(B, 500, np.int32)))
    d_group = {k: put(np.full(B, k, np.int32)) for k in GROUPS}
    nf = cells // CHECK_GROUP
    f_dg = put(W + fstride * np.arange(nf, dtype=np.int64))
    g = dict(stream=i32(nf), seq=i32(nf), offsets=i64(nf), num_bytes=i32(nf))
    sizes = {p: np.where(rng.rand(cells) < p / 100.0, -1, pkt).astype(np.int32) for p in LOSSES}
    d_sizes = {p: put(sizes[p]) for p in LOSSES}
    it = {p: dict(stream=i32(cells), seq=i32(cells), offsets=i64(cells), num_bytes=i32(cells)) for p in LOSSES}
    r = dict(off=i64(nf), size=i32(nf), seq=i32(nf), status=u8(nf), stats=i32(16), work=put(np.zeros(api.fec_recover_work_bytes(B, WINDOW) // 8 + 1, np.int64)))
    sv = stream.value

    def egress(sync=False):
        enc.egress_device(T, d_frames, cells * NB, d_off, d_nb, NB, B, d_base, q["route"], q["seq"], q["frame"], q["offset"], q["size"], q["np_"], q["work"], None, 0, None,
                          None, 16, api.PACK_STREAM_MAJOR, d_ring, W, ROOM, 1, q["flags"], None, q["next"], q["stats"], None, sv, sync)

    def stamp(sync=False):
        enc.rtp_stamp_device(cells, q["np_"], q["route"], q["seq"], q["frame"], q["offset"], q["size"], B, T, d_ssrc, d_tsb, d_pt, N, d_ring, W, ROOM, 0, q["flags"],
                             api.RTP_MARKER_NEVER, None, None, q["stats"], q["pst"], None, None, sv, sync)

    def encode(k, sync=False):
        enc.fec_encode_device(cells, q["np_"], q["route"], q["frame"], q["offset"], q["size"], d_ring, W, B, T, d_base, d_group[k], f["fbase"], d_fwire, F, fstride, nf_max,
                              f["n"], f["route"], f["seq"], f["frame"], f["offset"], f["size"], f["work"], ROOM, 0, 12, q["pst"], q["stats"], None, None, None, None, None, 0,
                              f["flags"], f["mask"], f["next"], f["stats"], sv, sync)

    def fec_stamp(sync=False):
        enc.rtp_stamp_device(nf_max, f["n"], f["route"], f["seq"], f["frame"], f["offset"], f["size"], B, T, d_fssrc, d_tsb, d_fpt, N, d_fwire, F, 12, 0, f["flags"],
                             api.RTP_MARKER_NEVER, None, None, q["stats"], f["pst"], None, None, sv, sync)

    def parse(p, sync=False):
        dec.rtp_parse_device(cells, d_ring, cap, q["offset"], d_sizes[p], B, d_ssrc, d_sid, it[p]["stream"], it[p]["seq"], it[p]["offsets"], it[p]["num_bytes"], d_pt, 0,
                             None, None, None, None, sv, sync)

    def fec_parse(sync=False):
        dec.rtp_parse_device(nf, d_ring, cap, f_dg, f["size"], B, d_fssrc, d_sid, g["stream"], g["seq"], g["offsets"], g["num_bytes"], d_fpt, 0, None, None, None, None, sv,
                             sync)

    def recover(p, sync=False):
        dec.fec_recover_device(cells, d_ring, cap, q["offset"], d_sizes[p], it[p]["stream"], it[p]["seq"], nf, g["stream"], g["offsets"], g["num_bytes"], WINDOW, d_ssrc,
                               W + F, rstride, r["off"], r["size"], r["seq"], r["work"], r["status"], r["stats"], sv, sync)
    moved = {k: W + (cells // k) * (14 + NB) for k in GROUPS}

    def memcpy(k):
        assert hip.hipMemcpyAsync(C.c_void_p(d_copy), C.c_void_p(d_ring), C.c_size_t(moved[k]), C.c_int(3), stream) == 0
    lib = api.load_library()                                          # the plans through the C calls themselves: no copy of the host's arrays per call
    at = lambda x: x.ctypes.data
    h = dict(np_=np.zeros(1, np.int64), route=np.zeros(cells, np.int32), frame=np.zeros(cells, np.int32), off=np.zeros(cells, np.int64), size=np.zeros(cells, np.int32),
             pst=np.zeros(cells, np.uint8), stats=np.zeros(B * 4, np.int32), ring=np.zeros(cap, np.uint8), n_fec=np.zeros(1, np.int64), f_route=np.zeros(nf_max, np.int32),
             f_seq=np.zeros(nf_max, np.int32), f_frame=np.zeros(nf_max, np.int32), f_off=np.zeros(nf_max, np.int64), f_size=np.zeros(nf_max, np.int32),
             f_flags=np.zeros(nf_max, np.uint8), work=np.zeros(api.fec_work_bytes(B, T) // 8 + 1, np.int64), stream=np.zeros(cells, np.int32), seq=np.zeros(cells, np.int32),
             g_stream=np.zeros(nf, np.int32), g_off=np.zeros(nf, np.int64), g_nb=np.zeros(nf, np.int32), r_off=np.zeros(nf, np.int64), r_size=np.zeros(nf, np.int32),
             r_seq=np.zeros(nf, np.int32), r_status=np.zeros(nf, np.uint8), r_work=np.zeros(api.fec_recover_work_bytes(B, WINDOW) // 8 + 1, np.int64))
    groups = {k: np.full(B, k, np.int32) for k in GROUPS}
    fbase = np.full(B, 500, np.int32)

    def encode_host(k):
        assert hip.hipStreamSynchronize(stream) == 0
        down(h["np_"], q["np_"])
        n = int(h["np_"][0])
        for name, key in (("route", "route"), ("frame", "frame"), ("off", "offset"), ("size", "size"), ("pst", "pst")):
            down(h[name][:n], q[key])
        down(h["stats"], q["stats"]); down(h["ring"][:W], d_ring)
        assert lib.lc3plus_plan_fec_encode(n, at(h["np_"]), at(h["route"]), at(h["frame"]), at(h["off"]), at(h["size"]), at(h["pst"]), at(h["ring"]), W, ROOM, 0, B, T,
                                           at(seq_base), at(h["stats"]), at(groups[k]), None, at(fbase), None, None, None, None, 0, at(h["ring"]) + W, F, fstride, 12, nf_max,
                                           at(h["n_fec"]), at(h["f_route"]), at(h["f_seq"]), at(h["f_frame"]), at(h["f_off"]), at(h["f_size"]), at(h["f_flags"]), None, None,
                                           None, at(h["work"]), None, 0) == 0
        m = int(h["n_fec"][0])
        up(d_fwire, h["ring"][W:W + m * fstride])
        for name, key in (("f_route", "route"), ("f_seq", "seq"), ("f_frame", "frame"), ("f_off", "offset"), ("f_size", "size"), ("f_flags", "flags")):
            up(f[key], h[name][:m])

    def recover_host(p):
        assert hip.hipStreamSynchronize(stream) == 0
        down(h["off"], q["offset"]); down(h["size"], d_sizes[p]); down(h["stream"], it[p]["stream"]); down(h["seq"], it[p]["seq"])
        down(h["g_stream"], g["stream"]); down(h["g_off"], g["offsets"]); down(h["g_nb"], g["num_bytes"]); down(h["ring"][:W + F], d_ring)
        assert lib.lc3plus_plan_fec_recover(B, cells, at(h["ring"]), cap, at(h["off"]), at(h["size"]), at(h["stream"]), at(h["seq"]), nf, at(h["g_stream"]), at(h["g_off"]),
                                            at(h["g_nb"]), WINDOW, at(ssrc), W + F, rstride, at(h["r_off"]), at(h["r_size"]), at(h["r_seq"]), at(h["r_status"]), None,
                                            at(h["r_work"]), None, 0) == 0
        up(d_ring + W + F, h["ring"][W + F:W + F + nf * rstride])
        up(r["off"], h["r_off"]); up(r["size"], h["r_size"]); up(r["seq"], h["r_seq"]); up(r["status"], h["r_status"])
    calls = {"egress_wire": egress, "parse": lambda: parse(LOSSES[0])}
    for k in GROUPS:
        calls["encode_k%d" % k] = lambda k=k: encode(k)
        calls["memcpy_k%d" % k] = lambda k=k: memcpy(k)
    for k in HOST_GROUPS:
        calls["encode_host_k%d" % k] = lambda k=k: encode_host(k)
    for p in LOSSES:
        calls["recover_p%d" % p] = lambda p=p: recover(p)
        calls["recover_host_p%d" % p] = lambda p=p: recover_host(p)
    chosen = [k for k in ALL if k in a.variants.split(",")]
    times = {k: [] for k in chosen}
    recovered = {}

    def receiver_ready():
        """what the recovery reads, which the encodes in between overwrite: the FEC packets of groups of 4, stamped, and their items"""
        encode(CHECK_GROUP); fec_stamp(); fec_parse(sync=True)
    try:
        egress(); stamp(sync=True)
        n = int(get(q["np_"], 1, np.int64)[0])
        assert n == cells and (get(q["pst"], cells, np.uint8) == 1).all()
        # the encoder at every K and the recovery (groups of CHECK_GROUP) at both loss rates against the host plans
        lst = {name: get(q[key], cells, dt) for name, key, dt in (("route", "route", np.int32), ("frame", "frame", np.int32), ("offset", "offset", np.int64),
                                                                  ("size", "size", np.int32), ("pst", "pst", np.uint8))}
        egr_stats = get(q["stats"], (B, 4), np.int32)
        for k in tuple(x for x in GROUPS if x != CHECK_GROUP) + (CHECK_GROUP,):       # the last one's packets stay for the recovery
            assert hip.hipMemset(C.c_void_p(d_fwire), 0x5A, C.c_size_t(F)) == 0
            encode(k, sync=True)
            ring = get(d_ring, cap, np.uint8)
            want = api.plan_fec_encode(lst["route"], lst["frame"], lst["offset"], lst["size"], ring[:W], T, seq_base, groups[k], fbase, np.full(F, 0x5A, np.uint8), fstride,
                                       ROOM, pkt_status=lst["pst"], route_stats=egr_stats, max_fec_packets=nf_max)
            m = cells // k
            assert want["n_fec"] == m == int(get(f["n"], 1, np.int64)[0]) and np.array_equal(ring[W:W + F], want["fec_wire"]) and not want["fec_flags"].any(), k
            for name, key, dt in (("route", "fec_route", np.int32), ("seq", "fec_seq", np.int32), ("frame", "fec_frame", np.int32), ("offset", "fec_offset", np.int64),
                                  ("size", "fec_size", np.int32), ("mask", "fec_mask", np.int32)):
                assert np.array_equal(get(f[name], m, dt), want[key][:m]), (k, name)
            assert np.array_equal(get(f["stats"], (B, 4), np.int32), want["route_stats"]), k
        fec_stamp(); fec_parse()
        for p in LOSSES:
            assert hip.hipMemset(C.c_void_p(d_ring + W + F), 0, C.c_size_t(nf * rstride)) == 0
            parse(p)
            recover(p, sync=True)
            ring = get(d_ring, cap, np.uint8)
            before = ring.copy()
            before[W + F:] = 0
            u = api.plan_fec_recover(B, before, lst["offset"], sizes[p], get(it[p]["stream"], cells, np.int32), get(it[p]["seq"], cells, np.int32),
                                     get(g["stream"], nf, np.int32), get(g["offsets"], nf, np.int64), get(g["num_bytes"], nf, np.int32), ssrc, W + F, rstride, window=WINDOW)
            assert np.array_equal(get(r["status"], nf, np.uint8), u["status"]) and np.array_equal(get(r["size"], nf, np.int32), u["rec_dg_sizes"]), p
            assert np.array_equal(get(r["off"], nf, np.int64), u["rec_dg_offsets"]) and np.array_equal(get(r["seq"], nf, np.int32), u["rec_seq"]), p
            assert np.array_equal(get(r["stats"], 16, np.int32), u["stats"]), p
            assert np.array_equal(ring[:cap], u["ring"][:cap]), p     # the whole ring: the recovery region started as zeros on both sides
        for p in LOSSES:
            recover(p, sync=True)
            recovered[p] = get(r["stats"], 16, np.int32)[:10].tolist()
        for rnd in range(a.warmup + a.calls):
            for name in times:
                if name.startswith("recover"):
                    receiver_ready()
                if "_host" in name:
                    t0 = time.perf_counter(); calls[name](); ms = (time.perf_counter() - t0) * 1e3
                else:
                    assert hip.hipEventRecord(ev0, stream) == 0
                    for _ in range(a.reps):
                        calls[name]()
                    assert hip.hipEventRecord(ev1, stream) == 0 and hip.hipEventSynchronize(ev1) == 0
                    t = C.c_float(0); assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
                    ms = t.value / a.reps
                if rnd >= a.warmup:
                    times[name].append(ms)
    finally:
        enc.close()
        dec.close()
        for p in ptrs:
            hip.hipFree(p)
    hip.hipEventDestroy(ev0); hip.hipEventDestroy(ev1); hip.hipStreamDestroy(stream)
    out = {"tool": "fec_rate", "streams": B, "frames": T, "frame_bytes": NB, "packets": n, "header_room": ROOM, "calls": a.calls, "warmup": a.warmup, "reps": a.reps,
           "bytes_read_plus_written": {"k%d" % k: v for k, v in moved.items()}, "recover_lanes_per_item": 64, "window": WINDOW,
           "recover_status_counts": {"p%d" % p: v for p, v in recovered.items()}, "variants": {}}
    for name, v in times.items():
        out["variants"][name] = {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    va = out["variants"]
    ms = lambda name: va[name]["ms_median"]
    if set(ALL) <= set(va):
        for k in GROUPS:
            out["encode_k%d_over_egress_wire" % k] = round(ms("encode_k%d" % k) / ms("egress_wire"), 4)
            out["encode_k%d_over_memcpy" % k] = round(ms("encode_k%d" % k) / ms("memcpy_k%d" % k), 4)
            out["encode_k%d_GBps_moved" % k] = round(moved[k] / ms("encode_k%d" % k) / 1e6, 2)
        for k in HOST_GROUPS:
            out["encode_k%d_over_host" % k] = round(ms("encode_k%d" % k) / ms("encode_host_k%d" % k), 5)
        for p in LOSSES:
            out["recover_p%d_over_parse" % p] = round(ms("recover_p%d" % p) / ms("parse"), 4)
            out["recover_p%d_over_host" % p] = round(ms("recover_p%d" % p) / ms("recover_host_p%d" % p), 5)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
