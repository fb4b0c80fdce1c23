"""Secure RTP rates (lc3plus_enc_batch_srtp_protect, lc3plus_dec_batch_srtp_unprotect) beside the stamp and parse calls they stand next to, the host detours
they replace and a plain copy of the same bytes: 4096 streams x 64 frames of RTP packets (12-byte header, 80-byte frame), one route and one source per stream,
the list frame-major (arrival order, the streams interleaved), one encoder and one decoder batch, one process.  Variants, alternated run by run, the SRTP ones
for both tag lengths (10 and 4):
  stamp            lc3plus_enc_batch_rtp_stamp over the packet list
  protect_T        the protect call on the stamped wire buffer, tag length T, next_roc asked for
  protect_T_host   the path the call replaces: synchronise, the wire buffer, the list and the status to the host, lc3plus_plan_srtp_protect there, the
                   destination and the three output arrays back
  parse            lc3plus_dec_batch_rtp_parse over the unprotected datagrams
  unprotect_T      the unprotect call on the protect call's output (status, index and stats asked for); the ring is restored from a copy in front of every run,
                   outside the timed span, since the call decrypts in place
  auth_only_T      the unprotect call on a ring it has already decrypted: every item is hashed in full, fails the comparison and is not decrypted - the
                   cost of the call without its AES pass
  unprotect_T_host synchronise, the ring, the list and the state to the host, lc3plus_plan_srtp_unprotect there, the ring, sizes and state back
  copy_T           hipMemcpyAsync, device to device, of the protected packets' bytes
Device variants: device events around the call on the call's stream (sync = 0).  Host variants: the host clock from before the synchronise (nothing is pending)
to the return of the last copy; they run --host-calls times.  Per variant the median, the fastest and the slowest of --calls runs after --warmup rounds.  Before
timing, every output of both calls is checked against the host plans.  Writes one JSON object to --out and prints it.
    python tools/srtp_rate.py [--calls 20] [--warmup 3] [--host-calls 5] [--out profiles/srtp_rate.json] [--streams 4096] [--variants a,b]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from audio_codec_amd import api

T, NB, ROOM, N = 64, 80, 12, 480
TAGS = (10, 4)
ALL = ("stamp", "parse") + tuple(k % t for t in TAGS for k in ("protect_%d", "protect_%d_host", "unprotect_%d", "auth_only_%d",
                                                                "unprotect_%d_host", "copy_%d"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=5)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--variants", default=",".join(ALL))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srtp_rate.json"))
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
    enc = amd.Batch(B, 48000, 1, 10.0, 0, [64000] * B, device=0)
    dec = amd.DecBatch(B, 48000, 1, 10.0, 0, None, device=0)
    sv = stream.value
    # the egress's list, frame-major, every stream sending T packets; the wire buffer holds random frames behind empty header rooms
    rng = np.random.RandomState(23)
    n = B * T
    pitch = ROOM + NB
    t, s = np.meshgrid(np.arange(T), np.arange(B), indexing="ij")
    route, frame = s.reshape(-1).astype(np.int32), t.reshape(-1).astype(np.int32)
    seq_base = ((65500 + 3 * np.arange(B)) % 65536).astype(np.int32)          # a third of the streams cross 65535 inside the call
    seq = ((seq_base[route] + frame) & 0xFFFF).astype(np.int32)
    off, size = np.arange(n, dtype=np.int64) * pitch, np.full(n, pitch, np.int32)
    wire = rng.randint(0, 256, size=n * pitch).astype(np.uint8)
    ssrc = (0x7FFF0000 + 13 * np.arange(B, dtype=np.int64)).astype(np.uint32).view(np.int32)
    ts_base, pt = (np.arange(B) * 100003 % (1 << 31)).astype(np.int32), np.full(B, 96, np.int32)
    roc = (np.arange(B) % 5 + 1).astype(np.int32)
    next_seq = (seq_base + T).astype(np.int32)
    ctx = np.stack([api.srtp_make_context(bytes((k * 7 + j) & 255 for j in range(16)), bytes((k * 3 + j) & 255 for j in range(14))) for k in range(B)])
    state = np.zeros((B, api.SRTP_STATE_WORDS), np.int32)
    state[:, api.SRTP_FLAGS], state[:, api.SRTP_ROC], state[:, api.SRTP_S_L], state[:, api.SRTP_WIN_LO] = 1, roc - (seq_base == 0), (seq_base - 1) & 0xFFFF, 1
    # (a receiver that has seen each sender's packet in front of the first: S_L = seq_base - 1, in the rollover period before where seq_base is 0)
    d = dict(np=put(np.array([n], np.int64)), route=put(route), seq=put(seq), frame=put(frame), off=put(off), size=put(size), wire=put(wire), ssrc=put(ssrc),
             tsb=put(ts_base), pt=put(pt), pst=put(np.zeros(n, np.uint8)), ctx=put(ctx), roc=put(roc), base=put(seq_base), next=put(next_seq),
             nroc=put(np.zeros(B, np.int32)), state=put(state), state_out=put(state), sid=put(np.arange(B, dtype=np.int32)))
    it = {k: put(np.zeros(n, dt)) for k, dt in (("stream", np.int32), ("seq", np.int32), ("offsets", np.int64), ("num_bytes", np.int32), ("status", np.uint8))}
    wb = api.srtp_workspace_bytes(n, B)
    d_work = put(np.zeros(wb, np.uint8))

    def stamp(sync=False):
        enc.rtp_stamp_device(n, d["np"], d["route"], d["seq"], d["frame"], d["off"], d["size"], B, T, d["ssrc"], d["tsb"], d["pt"], N, d["wire"], wire.size, ROOM, 0, None,
                             api.RTP_MARKER_NEVER, None, None, None, d["pst"], None, None, sv, sync)
    stamp(sync=True)
    h_wire, h_pst = get(d["wire"], wire.size, np.uint8), get(d["pst"], n, np.uint8)
    assert (h_pst == api.RTP_STAMPED).all()
    per = {}
    for tag in TAGS:
        stride = (pitch + tag + 3) & ~3                               # slots at word boundaries: 104 and 96 bytes
        q = dict(tag=tag, stride=stride, dst_bytes=n * stride, dst=put(np.zeros(n * stride, np.uint8)), keep=put(np.zeros(n * stride, np.uint8)),
                 oo=put(np.zeros(n, np.int64)), os=put(np.zeros(n, np.int32)), ost=put(np.zeros(n, np.uint8)), usz=put(np.zeros(n, np.int32)),
                 ust=put(np.zeros(n, np.uint8)), uidx=put(np.zeros(n, np.int64)), ustats=put(np.zeros(api.SRTP_STATS_WORDS, np.int32)))
        per[tag] = q

    def protect(q, sync=False):
        enc.srtp_protect_device(n, d["np"], d["route"], d["off"], d["size"], d["pst"], d["wire"], wire.size, B, d["ctx"], d["roc"], d["base"], q["dst"], q["dst_bytes"],
                                q["stride"], q["oo"], q["os"], q["ost"], q["tag"], ROOM, 0, d["next"], d["nroc"], sv, sync)

    def restore(q):
        assert hip.hipMemcpyAsync(C.c_void_p(q["dst"]), C.c_void_p(q["keep"]), C.c_size_t(q["dst_bytes"]), C.c_int(3), stream) == 0

    def unprotect(q, sync=False):
        dec.srtp_unprotect_device(n, q["dst"], q["dst_bytes"], q["oo"], q["os"], B, d["ssrc"], d["ctx"], d["state"], d["state_out"], q["usz"], d_work, wb, q["tag"],
                                  q["ust"], q["uidx"], q["ustats"], sv, sync)

    def parse(q, sync=False):
        dec.rtp_parse_device(n, q["dst"], q["dst_bytes"], q["oo"], q["usz"], B, d["ssrc"], d["sid"], it["stream"], it["seq"], it["offsets"], it["num_bytes"], d["pt"], 0,
                             None, None, it["status"], None, sv, sync)
    lib = api.load_library()
    at = lambda x: x.ctypes.data
    h = dict(wire=np.zeros(wire.size, np.uint8), route=np.zeros(n, np.int32), off=np.zeros(n, np.int64), size=np.zeros(n, np.int32), pst=np.zeros(n, np.uint8),
             oo=np.zeros(n, np.int64), os=np.zeros(n, np.int32), ost=np.zeros(n, np.uint8), nroc=np.zeros(B, np.int32), count=np.array([n], np.int64),
             usz=np.zeros(n, np.int32), state=np.zeros_like(state), state_out=np.zeros_like(state))

    def protect_host(q):
        assert hip.hipStreamSynchronize(stream) == 0
        for name in ("wire", "route", "off", "size", "pst"):
            down(h[name], d[name])
        assert lib.lc3plus_plan_srtp_protect(n, at(h["count"]), at(h["route"]), at(h["off"]), at(h["size"]), at(h["pst"]), at(h["wire"]), wire.size, ROOM, 0, B, at(ctx),
                                             at(roc), at(seq_base), at(next_seq), at(q["h_dst"]), q["dst_bytes"], q["stride"], q["tag"], at(h["oo"]), at(h["os"]),
                                             at(h["ost"]), at(h["nroc"])) == 0
        up(q["dst"], q["h_dst"]); up(q["oo"], h["oo"]); up(q["os"], h["os"]); up(q["ost"], h["ost"]); up(d["nroc"], h["nroc"])

    def unprotect_host(q):
        assert hip.hipStreamSynchronize(stream) == 0
        down(q["h_dst"], q["dst"]); down(h["oo"], q["oo"]); down(h["os"], q["os"]); down(h["state"], d["state"])
        assert lib.lc3plus_plan_srtp_unprotect(n, at(q["h_dst"]), q["dst_bytes"], at(h["oo"]), at(h["os"]), B, at(ssrc), at(ctx), at(h["state"]), at(h["state_out"]),
                                               q["tag"], at(h["usz"]), None, None, None) == 0
        up(q["dst"], q["h_dst"]); up(q["usz"], h["usz"]); up(d["state_out"], h["state_out"])

    chosen = [k for k in ALL if k in a.variants.split(",")]
    times = {k: [] for k in chosen}
    checked = {}
    try:
        for tag, q in per.items():                                    # both calls against the host plans
            want = api.plan_srtp_protect(route, off, size, h_pst, h_wire, ctx, roc, seq_base, np.zeros(q["dst_bytes"], np.uint8), q["stride"], tag, ROOM, 0,
                                         next_seq=next_seq)
            uwant = api.plan_srtp_unprotect(want["dst"], want["out_offset"], want["out_size"], ssrc, ctx, state, tag)
            assert (want["out_status"] == api.SRTP_PROTECTED).all() and (uwant["status"] == api.SRTP_OK).all()
            assert hip.hipMemset(C.c_void_p(q["dst"]), 0, C.c_size_t(q["dst_bytes"])) == 0
            protect(q, sync=True)
            assert np.array_equal(get(q["dst"], q["dst_bytes"], np.uint8), want["dst"]) and np.array_equal(get(q["os"], n, np.int32), want["out_size"])
            assert np.array_equal(get(q["oo"], n, np.int64), want["out_offset"]) and np.array_equal(get(d["nroc"], B, np.int32), want["next_roc"])
            assert hip.hipMemcpy(C.c_void_p(q["keep"]), C.c_void_p(q["dst"]), C.c_size_t(q["dst_bytes"]), C.c_int(3)) == 0
            unprotect(q, sync=True)
            assert np.array_equal(get(q["dst"], q["dst_bytes"], np.uint8), uwant["ring"]) and np.array_equal(get(d["state_out"], state.shape, np.int32), uwant["state"])
            assert np.array_equal(get(q["usz"], n, np.int32), uwant["sizes"]) and np.array_equal(get(q["uidx"], n, np.int64), uwant["index"])
            assert np.array_equal(get(q["ustats"], api.SRTP_STATS_WORDS, np.int32), uwant["stats"])
            q["h_dst"] = np.zeros(q["dst_bytes"], np.uint8)
            checked[tag] = int(want["out_size"].sum())
            parse(q, sync=True)
            assert (get(it["status"], n, np.uint8) == 0).all()

        def run(name):
            kind = name.split("_")[0]
            if name == "stamp":
                return stamp, None
            if name == "parse":
                return (lambda: parse(per[TAGS[0]])), None
            q = per[int([x for x in name.split("_") if x.isdigit()][0])]
            if kind == "protect":
                return (lambda: protect(q)), None
            if kind == "unprotect":
                return (lambda: unprotect(q)), (lambda: restore(q))
            if kind == "auth":
                return (lambda: unprotect(q)), (lambda: (restore(q), unprotect(q)))
            return (lambda: restore(q)), None                           # copy_T
        for rnd in range(a.warmup + a.calls):
            for name in times:
                if name.endswith("_host"):
                    if rnd >= a.warmup + a.host_calls:
                        continue
                    q = per[int(name.split("_")[1])]
                    if name.startswith("unprotect"):
                        restore(q)
                    t0 = time.perf_counter(); (protect_host if name.startswith("protect") else unprotect_host)(q); ms = (time.perf_counter() - t0) * 1e3
                else:
                    call, before = run(name)
                    if before:
                        before()
                    assert hip.hipEventRecord(ev0, stream) == 0
                    call()
                    assert hip.hipEventRecord(ev1, stream) == 0 and hip.hipEventSynchronize(ev1) == 0
                    f = C.c_float(0); assert hip.hipEventElapsedTime(C.byref(f), ev0, ev1) == 0
                    ms = f.value
                if rnd >= a.warmup:
                    times[name].append(ms)
    finally:
        enc.close(); dec.close()
        for p in ptrs:
            hip.hipFree(p)
    hip.hipEventDestroy(ev0); hip.hipEventDestroy(ev1); hip.hipStreamDestroy(stream)
    out = {"tool": "srtp_rate", "streams": B, "frames": T, "frame_bytes": NB, "packets": n, "rtp_bytes": n * pitch, "srtp_bytes": checked, "workspace_bytes": wb,
           "calls": a.calls, "host_calls": a.host_calls, "warmup": a.warmup, "variants": {}}
    for name, v in times.items():
        out["variants"][name] = {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "runs": len(v)}
    va = out["variants"]
    ms = lambda name: va[name]["ms_median"]
    ratios = {}
    for tag in TAGS:
        for side, beside in (("protect", "stamp"), ("unprotect", "parse")):
            k = "%s_%d" % (side, tag)
            if k in va:
                for other, label in ((beside, "over_" + beside), (k + "_host", "over_host"), ("copy_%d" % tag, "over_copy")):
                    if other in va:
                        ratios["%s_%s" % (k, label)] = round(ms(k) / ms(other), 5)
                ratios[k + "_GB_per_s"] = round(checked[tag] / ms(k) / 1e6, 1)
    out["ratios"] = ratios
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
