"""Reception report rates (lc3plus_dec_batch_rtcp_stats) beside the parse call in front of it and the host detour it replaces: 4096 streams x 64 frames of
RTP datagrams (12-byte header, 80-byte frame), one decoder batch, one process.  The loss mix is that of tools/rtp_rate.py: one stream in 16 stops after 40
frames and the last 64 packets are missing; on top of it one packet in 64 arrives one frame late (reordered behind its successor), since the walk's sort and the
REORDERED path should be paid for.  The list is in arrival order - frame-major, the streams interleaved - and once more stream-major (every sender's packets in
one burst), the order in which every wave of the count kernel meets one stream.  Variants, alternated run by run:
  parse          lc3plus_dec_batch_rtp_parse over the datagrams, a table of one sender per stream, stream / seq / timestamp and the rest asked for
  stats          the stats call on the parse's arrays, make_report 0: state, ext_seq, item_status and stream_stats
  stats_report   the same with make_report 1: the blocks too, lsr and dlsr given
  stats_sm, stats_report_sm   both on the stream-major list
  stats_host     the path the call replaces: synchronise, stream / seq / timestamp / arrival and the state to the host, lc3plus_plan_rtcp_stats there with
                 make_report 1, the state and the blocks back
Device variants: device events around the call on the call's stream (sync = 0).  Host variant: the host clock from before the synchronise (nothing is pending)
to the return of the last copy.  Per variant the median, the fastest and the slowest of --calls runs after --warmup rounds.  Before timing, every output of the
stats call is checked against the host plan, on both lists.  Writes one JSON object to --out and prints it.
    python tools/rtcp_rate.py [--calls 20] [--warmup 3] [--out profiles/rtcp_rate.json] [--streams 4096] [--variants a,b]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from audio_codec_amd import api

T, NB, ROOM, N = 64, 80, 12, 480
ALL = ("parse", "stats", "stats_report", "stats_sm", "stats_report_sm", "stats_host")


def datagrams(B, order):
    """the headers of the packets that arrive, in list order -> (ring, dg_offsets, dg_sizes, arrival, ssrc keys)"""
    rng = np.random.RandomState(17)
    counts = np.where(np.arange(B) % 16 == 5, 40, T)
    s, t = np.meshgrid(np.arange(B), np.arange(T), indexing="ij")
    keep = t < counts[:, None]
    keep.reshape(-1)[np.flatnonzero(keep.reshape(-1))[-64:]] = False
    late = rng.rand(B, T) < 1.0 / 64
    when = t + 1.5 * late + s / (2.0 * B)                             # a late packet arrives behind its successor
    s, t, when = s[keep], t[keep], when[keep]
    idx = np.lexsort((when, s)) if order == "stream_major" else np.argsort(when, kind="stable")
    s, t, when = s[idx], t[idx], when[idx]
    n = s.size
    seq = (s * 7 + t) % 65536
    ts = (s * 100003 + t * N) % (1 << 32)
    ssrc = 0x7FFF0000 + 13 * np.arange(B, dtype=np.int64)
    pitch = ROOM + NB
    ring = np.zeros((n, pitch), np.uint8)
    ring[:, 0], ring[:, 1] = 0x80, 96
    ring[:, 2], ring[:, 3] = seq >> 8, seq & 255
    for k in range(4):
        ring[:, 4 + k] = (ts >> (24 - 8 * k)) & 255
        ring[:, 8 + k] = (ssrc[s] >> (24 - 8 * k)) & 255
    arrival = (ts + 9000 + (when * N).astype(np.int64) - t * N + rng.randint(-100, 100, size=n)) % (1 << 32)
    return ring.reshape(-1), np.arange(n, dtype=np.int64) * pitch, np.full(n, pitch, np.int32), arrival.astype(np.uint32).view(np.int32), ssrc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--variants", default=",".join(ALL))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rtcp_rate.json"))
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
    dec = amd.DecBatch(B, 48000, 1, 10.0, 0, None, device=0)
    sv = stream.value
    W = api.RR_STATE_WORDS
    sid, pt = np.arange(B, dtype=np.int32), np.full(B, 96, np.int32)
    lsr, dlsr = (np.arange(B) * 65537 % (1 << 31)).astype(np.int32), (np.arange(B) * 31).astype(np.int32)
    zero_state = np.zeros((B, W), np.int32)
    d_sid, d_pt, d_lsr, d_dlsr, d_state0 = put(sid), put(pt), put(lsr), put(dlsr), put(zero_state)
    lists = {}
    for order in ("frame_major", "stream_major"):
        ring, off, size, arrival, ssrc = datagrams(B, order)
        n = off.size
        ssrc32 = (ssrc & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        lists[order] = dict(n=n, ring=put(np.concatenate([ring, np.zeros(8, np.uint8)])), ring_bytes=ring.size, off=put(off), size=put(size), arrival=put(arrival),
                            ssrc=put(ssrc32), ssrc32=ssrc32, h_arrival=arrival,
                            it={k: put(np.zeros(n, dt)) for k, dt in (("stream", np.int32), ("seq", np.int32), ("offsets", np.int64), ("num_bytes", np.int32),
                                                                      ("timestamp", np.int32), ("marker", np.uint8), ("status", np.uint8))},
                            stats=put(np.zeros(api.RTP_STATS_WORDS, np.int32)), state=put(zero_state), blocks=put(np.zeros((B, api.RR_BLOCK_BYTES), np.uint8)),
                            ext=put(np.zeros(n, np.int32)), ist=put(np.zeros(n, np.uint8)), sst=put(np.zeros((B, api.RR_STATS_WORDS), np.int32)),
                            wb=api.rtcp_workspace_bytes(n, B), work=put(np.zeros(api.rtcp_workspace_bytes(n, B), np.uint8)))

    def parse(q, sync=False):
        it = q["it"]
        dec.rtp_parse_device(q["n"], q["ring"], q["ring_bytes"], q["off"], q["size"], B, q["ssrc"], d_sid, it["stream"], it["seq"], it["offsets"], it["num_bytes"], d_pt, 0,
                             it["timestamp"], it["marker"], it["status"], q["stats"], sv, sync)

    def stats(q, report, sync=False):
        it = q["it"]
        dec.rtcp_stats_device(q["n"], it["stream"], it["seq"], it["timestamp"], q["arrival"], B, d_state0, q["state"], q["work"], q["wb"], report,
                              q["ssrc"] if report else None, d_lsr if report else None, d_dlsr if report else None, q["blocks"] if report else None, q["ext"], q["ist"],
                              q["sst"], sv, sync)
    fm, sm = lists["frame_major"], lists["stream_major"]
    n = fm["n"]
    h = dict(stream=np.zeros(n, np.int32), seq=np.zeros(n, np.int32), timestamp=np.zeros(n, np.int32), arrival=np.zeros(n, np.int32), state=np.zeros((B, W), np.int32),
             out=np.zeros((B, W), np.int32), blocks=np.zeros((B, api.RR_BLOCK_BYTES), np.uint8))
    lib = api.load_library()
    at = lambda x: x.ctypes.data

    def stats_host():
        assert hip.hipStreamSynchronize(stream) == 0
        for name in ("stream", "seq", "timestamp"):
            down(h[name], fm["it"][name])
        down(h["arrival"], fm["arrival"]); down(h["state"], d_state0)
        assert lib.lc3plus_plan_rtcp_stats(n, at(h["stream"]), at(h["seq"]), at(h["timestamp"]), at(h["arrival"]), B, at(h["state"]), at(h["out"]), 1, at(fm["ssrc32"]),
                                           at(lsr), at(dlsr), at(h["blocks"]), None, None, None) == 0
        up(fm["state"], h["out"]); up(fm["blocks"], h["blocks"])
    calls = {"parse": lambda: parse(fm), "stats": lambda: stats(fm, False), "stats_report": lambda: stats(fm, True), "stats_sm": lambda: stats(sm, False),
             "stats_report_sm": lambda: stats(sm, True), "stats_host": stats_host}
    chosen = [k for k in ALL if k in a.variants.split(",")]
    times = {k: [] for k in chosen}
    tallies = {}
    try:
        for order, q in lists.items():
            parse(q, sync=True)
            items = {k: get(q["it"][k], q["n"], np.int32) for k in ("stream", "seq", "timestamp")}
            assert (get(q["it"]["status"], q["n"], np.uint8) == 0).all()
            want = api.plan_rtcp_stats(items["stream"], items["seq"], items["timestamp"], q["h_arrival"], zero_state, True, q["ssrc32"], lsr, dlsr)
            stats(q, True, sync=True)
            got = dict(state=get(q["state"], (B, W), np.int32), blocks=get(q["blocks"], (B, api.RR_BLOCK_BYTES), np.uint8), ext_seq=get(q["ext"], q["n"], np.int32),
                       item_status=get(q["ist"], q["n"], np.uint8), stream_stats=get(q["sst"], (B, api.RR_STATS_WORDS), np.int32))
            for k in api.RR_OUTPUTS:
                assert np.array_equal(got[k], want[k]), (order, k)
            tallies[order] = want["stream_stats"].sum(axis=0).tolist()
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
        dec.close()
        for p in ptrs:
            hip.hipFree(p)
    hip.hipEventDestroy(ev0); hip.hipEventDestroy(ev1); hip.hipStreamDestroy(stream)
    out = {"tool": "rtcp_rate", "streams": B, "frames": T, "frame_bytes": NB, "items": n, "ssrc_table_entries": B, "workspace_bytes": fm["wb"],
           "counted_jump_restart_reordered": tallies, "calls": a.calls, "warmup": a.warmup, "variants": {}}
    for name, v in times.items():
        out["variants"][name] = {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    va = out["variants"]
    ms = lambda name: va[name]["ms_median"]
    if set(ALL) <= set(va):
        out["stats_over_parse"] = round(ms("stats") / ms("parse"), 5)
        out["stats_report_over_parse"] = round(ms("stats_report") / ms("parse"), 5)
        out["stats_report_over_host"] = round(ms("stats_report") / ms("stats_host"), 5)
        out["stats_over_host"] = round(ms("stats") / ms("stats_host"), 5)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
