"""AES-GCM Secure RTP rates (lc3plus_enc_batch_srtp_gcm_protect, lc3plus_dec_batch_srtp_gcm_unprotect) beside the HMAC-SHA1-80 calls on the same packets, a plain
copy of the same bytes and the host detour the calls replace: the workload of tools/srtp_rate.py - 4096 streams x 64 frames of RTP packets (12-byte header,
80-byte frame), one route and one source per stream, the list frame-major, one encoder and one decoder batch, one process.  Variants, alternated run by run:
  gcm128_protect, gcm256_protect       the GCM protect call on the stamped wire buffer under 16- and 32-byte keys, next_roc asked for
  gcm128_unprotect, gcm256_unprotect   the GCM unprotect call on that output (status, index and stats asked for); the ring is restored from a copy in front of
                                       every run, outside the timed span, since the call decrypts in place
  hmac80_protect, hmac80_unprotect     lc3plus_enc_batch_srtp_protect / lc3plus_dec_batch_srtp_unprotect with tag_len 10 on the same packets
  copy                                 hipMemcpyAsync, device to device, of the GCM-protected packets' bytes
  gcm128_protect_host, gcm128_unprotect_host, gcm256_protect_host, gcm256_unprotect_host
                                       the detour: synchronise, the buffers and the list to the host, the plan function there on one core, the results back
With --ab LIB (a build of lc3_gcm.hip with -DLC3G_LDS_TABLE=0: make -C audio_codec_amd/csrc gcm_global) the two placements of the GHASH table are measured
against each other, both through the sibling's own C ABI so that the host path in front of the launches is the same: ab_lds_* (the product library, a
lane-interleaved copy of the table in LDS) and ab_global_* (LIB, the table read from the context in global memory); --ab-out writes that table as text.
Device variants: device events around the call on the call's stream (sync = 0).  Host variants: the host clock from before the synchronise (nothing is pending)
to the return of the last copy; they run --host-calls times.  Per variant the median, the fastest and the slowest of --calls runs after --warmup rounds.  Before
timing, every output of every device variant is checked against the host plans.  Writes one JSON object to --out and prints it.
    python tools/gcm_rate.py [--calls 20] [--warmup 3] [--host-calls 3] [--out profiles/gcm_rate.json] [--streams 4096] [--ab audio_codec_amd/_var/liblc3plus_gcm_global_hip.so --ab-out profiles/gcm_tables_ab.txt]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from audio_codec_amd import api

T, NB, ROOM, N = 64, 80, 12, 480
P, L, I, V = C.c_void_p, C.c_longlong, C.c_int32, C.c_void_p


class ProtectIn(C.Structure):                                         # lc3s_protect_in (lc3_srtp_shim.h)
    _fields_ = [(k, P) for k in ("route", "offset", "size", "status", "wire", "ctx", "roc", "seq_base", "next_seq", "dst")] + \
               [(k, L) for k in ("wire_capacity", "dst_capacity", "dst_stride")] + [(k, I) for k in ("header_room", "payload_room", "n_routes", "tag_len")]


class ProtectCall(C.Structure):                                       # lc3srtp_protect_call
    _fields_ = [("device", I), ("sync", I), ("max_packets", L), ("n_packets", P), ("q", ProtectIn), ("out_offset", P), ("out_size", P), ("out_status", P),
                ("next_roc", P), ("hip_stream", V)]


class UnprotectCall(C.Structure):                                     # lc3srtp_unprotect_call
    _fields_ = [("device", I), ("sync", I), ("n_ssrc", I), ("tag_len", I), ("n_items", L), ("ring_capacity", L)] + \
               [(k, P) for k in ("ring", "dg_offsets", "dg_sizes", "ssrc_key", "ctx", "state_in", "state_out", "sizes_out", "status", "index", "stats", "workspace")] + \
               [("workspace_bytes", L), ("hip_stream", V)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--ab", default=None)
    ap.add_argument("--ab-out", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcm_rate.json"))
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
    state = np.zeros((B, api.SRTP_STATE_WORDS), np.int32)
    state[:, api.SRTP_FLAGS], state[:, api.SRTP_ROC], state[:, api.SRTP_S_L], state[:, api.SRTP_WIN_LO] = 1, roc - (seq_base == 0), (seq_base - 1) & 0xFFFF, 1
    d = dict(np=put(np.array([n], np.int64)), route=put(route), seq=put(seq), frame=put(frame), off=put(off), size=put(size), wire=put(wire), ssrc=put(ssrc),
             tsb=put(ts_base), pt=put(pt), pst=put(np.zeros(n, np.uint8)), roc=put(roc), base=put(seq_base), next=put(next_seq),
             nroc=put(np.zeros(B, np.int32)), state=put(state), state_out=put(state))
    wb = api.srtp_workspace_bytes(n, B)
    d_work = put(np.zeros(wb, np.uint8))
    enc.rtp_stamp_device(n, d["np"], d["route"], d["seq"], d["frame"], d["off"], d["size"], B, T, d["ssrc"], d["tsb"], d["pt"], N, d["wire"], wire.size, ROOM, 0, None,
                         api.RTP_MARKER_NEVER, None, None, None, d["pst"], None, None, sv, True)
    h_wire, h_pst = get(d["wire"], wire.size, np.uint8), get(d["pst"], n, np.uint8)
    assert (h_pst == api.RTP_STAMPED).all()
    key = lambda k, nb: bytes((k * 7 + j) & 255 for j in range(nb))
    suites = {}
    for name, tag, ctx in (("gcm128", 16, np.stack([api.srtp_gcm_make_context(key(k, 16), key(3 * k, 12)) for k in range(B)])),
                           ("gcm256", 16, np.stack([api.srtp_gcm_make_context(key(k, 32), key(3 * k, 12)) for k in range(B)])),
                           ("hmac80", 10, np.stack([api.srtp_make_context(key(k, 16), key(3 * k, 14)) for k in range(B)]))):
        stride = (pitch + tag + 3) & ~3
        suites[name] = dict(name=name, gcm=name != "hmac80", tag=tag, h_ctx=ctx, ctx=put(ctx), stride=stride, dst_bytes=n * stride, dst=put(np.zeros(n * stride, np.uint8)),
                            keep=put(np.zeros(n * stride, np.uint8)), oo=put(np.zeros(n, np.int64)), os=put(np.zeros(n, np.int32)), ost=put(np.zeros(n, np.uint8)),
                            usz=put(np.zeros(n, np.int32)), ust=put(np.zeros(n, np.uint8)), uidx=put(np.zeros(n, np.int64)),
                            ustats=put(np.zeros(api.SRTP_STATS_WORDS, np.int32)), h_dst=np.zeros(n * stride, np.uint8))

    def protect(q, sync=False):
        if q["gcm"]:
            enc.srtp_gcm_protect_device(n, d["np"], d["route"], d["off"], d["size"], d["pst"], d["wire"], wire.size, B, q["ctx"], d["roc"], d["base"], q["dst"],
                                        q["dst_bytes"], q["stride"], q["oo"], q["os"], q["ost"], ROOM, 0, d["next"], d["nroc"], sv, sync)
        else:
            enc.srtp_protect_device(n, d["np"], d["route"], d["off"], d["size"], d["pst"], d["wire"], wire.size, B, q["ctx"], d["roc"], d["base"], q["dst"], q["dst_bytes"],
                                    q["stride"], q["oo"], q["os"], q["ost"], q["tag"], ROOM, 0, d["next"], d["nroc"], sv, sync)

    def unprotect(q, sync=False):
        if q["gcm"]:
            dec.srtp_gcm_unprotect_device(n, q["dst"], q["dst_bytes"], q["oo"], q["os"], B, d["ssrc"], q["ctx"], d["state"], d["state_out"], q["usz"], d_work, wb,
                                          q["ust"], q["uidx"], q["ustats"], sv, sync)
        else:
            dec.srtp_unprotect_device(n, q["dst"], q["dst_bytes"], q["oo"], q["os"], B, d["ssrc"], q["ctx"], d["state"], d["state_out"], q["usz"], d_work, wb, q["tag"],
                                      q["ust"], q["uidx"], q["ustats"], sv, sync)

    def restore(q):
        assert hip.hipMemcpyAsync(C.c_void_p(q["dst"]), C.c_void_p(q["keep"]), C.c_size_t(q["dst_bytes"]), C.c_int(3), stream) == 0

    # the two table placements through the sibling's own entry points
    def direct(lib):
        def pr(q):
            c = ProtectCall(0, 0, n, d["np"], ProtectIn(d["route"], d["off"], d["size"], d["pst"], d["wire"], q["ctx"], d["roc"], d["base"], d["next"], q["dst"], wire.size,
                                                          q["dst_bytes"], q["stride"], ROOM, 0, B, 16), q["oo"], q["os"], q["ost"], d["nroc"], sv)
            assert lib.lc3gcm_protect_run(C.byref(c)) == 0

        def un(q):
            c = UnprotectCall(0, 0, B, 16, n, q["dst_bytes"], q["dst"], q["oo"], q["os"], d["ssrc"], q["ctx"], d["state"], d["state_out"], q["usz"], q["ust"], q["uidx"],
                              q["ustats"], d_work, wb, sv)
            assert lib.lc3gcm_unprotect_run(C.byref(c)) == 0
        return pr, un
    placements = {}
    if a.ab:
        placements["lds"] = direct(C.CDLL(os.path.join(ROOT, "audio_codec_amd", "liblc3plus_gcm_hip.so")))
        placements["global"] = direct(C.CDLL(os.path.abspath(a.ab)))
    lib = api.load_library()
    at = lambda x: x.ctypes.data
    h = dict(wire=np.zeros(wire.size, np.uint8), route=np.zeros(n, np.int32), off=np.zeros(n, np.int64), size=np.zeros(n, np.int32), pst=np.zeros(n, np.uint8),
             oo=np.zeros(n, np.int64), os=np.zeros(n, np.int32), ost=np.zeros(n, np.uint8), nroc=np.zeros(B, np.int32), count=np.array([n], np.int64),
             usz=np.zeros(n, np.int32), state=np.zeros_like(state), state_out=np.zeros_like(state))

    def protect_host(q):
        assert hip.hipStreamSynchronize(stream) == 0
        for name in ("wire", "route", "off", "size", "pst"):
            down(h[name], d[name])
        assert lib.lc3plus_plan_srtp_gcm_protect(n, at(h["count"]), at(h["route"]), at(h["off"]), at(h["size"]), at(h["pst"]), at(h["wire"]), wire.size, ROOM, 0, B,
                                                 at(q["h_ctx"]), at(roc), at(seq_base), at(next_seq), at(q["h_dst"]), q["dst_bytes"], q["stride"], at(h["oo"]), at(h["os"]),
                                                 at(h["ost"]), at(h["nroc"])) == 0
        up(q["dst"], q["h_dst"]); up(q["oo"], h["oo"]); up(q["os"], h["os"]); up(q["ost"], h["ost"]); up(d["nroc"], h["nroc"])

    def unprotect_host(q):
        assert hip.hipStreamSynchronize(stream) == 0
        down(q["h_dst"], q["dst"]); down(h["oo"], q["oo"]); down(h["os"], q["os"]); down(h["state"], d["state"])
        assert lib.lc3plus_plan_srtp_gcm_unprotect(n, at(q["h_dst"]), q["dst_bytes"], at(h["oo"]), at(h["os"]), B, at(ssrc), at(q["h_ctx"]), at(h["state"]),
                                                   at(h["state_out"]), at(h["usz"]), None, None, None) == 0
        up(q["dst"], q["h_dst"]); up(q["usz"], h["usz"]); up(d["state_out"], h["state_out"])

    variants = {}                                                     # name -> (call, before or None, host?)
    for q in suites.values():
        variants[q["name"] + "_protect"] = ((lambda q=q: protect(q)), None, False)
        variants[q["name"] + "_unprotect"] = ((lambda q=q: unprotect(q)), (lambda q=q: restore(q)), False)
        if q["gcm"]:
            variants[q["name"] + "_protect_host"] = ((lambda q=q: protect_host(q)), None, True)
            variants[q["name"] + "_unprotect_host"] = ((lambda q=q: unprotect_host(q)), (lambda q=q: restore(q)), True)
            for where, (pr, un) in placements.items():
                variants["ab_%s_%s_protect" % (where, q["name"])] = ((lambda q=q, pr=pr: pr(q)), None, False)
                variants["ab_%s_%s_unprotect" % (where, q["name"])] = ((lambda q=q, un=un: un(q)), (lambda q=q: restore(q)), False)
    variants["copy"] = ((lambda: restore(suites["gcm128"])), None, False)
    times = {k: [] for k in variants}
    checked = {}
    try:
        for q in suites.values():                                     # every device path against the host plans
            if q["gcm"]:
                want = api.plan_srtp_gcm_protect(route, off, size, h_pst, h_wire, q["h_ctx"], roc, seq_base, np.zeros(q["dst_bytes"], np.uint8), q["stride"], ROOM, 0,
                                                 next_seq=next_seq)
                uwant = api.plan_srtp_gcm_unprotect(want["dst"], want["out_offset"], want["out_size"], ssrc, q["h_ctx"], state)
            else:
                want = api.plan_srtp_protect(route, off, size, h_pst, h_wire, q["h_ctx"], roc, seq_base, np.zeros(q["dst_bytes"], np.uint8), q["stride"], q["tag"], ROOM, 0,
                                             next_seq=next_seq)
                uwant = api.plan_srtp_unprotect(want["dst"], want["out_offset"], want["out_size"], ssrc, q["h_ctx"], state, q["tag"])
            assert (want["out_status"] == api.SRTP_PROTECTED).all() and (uwant["status"] == api.SRTP_OK).all()
            paths = [(protect, unprotect)] + ([(lambda q, sync, pr=pr: (pr(q), hip.hipStreamSynchronize(stream)), lambda q, sync, un=un: (un(q), hip.hipStreamSynchronize(stream)))
                                               for pr, un in placements.values()] if q["gcm"] else [])
            for pr, un in paths:
                assert hip.hipMemset(C.c_void_p(q["dst"]), 0, C.c_size_t(q["dst_bytes"])) == 0
                pr(q, True)
                assert np.array_equal(get(q["dst"], q["dst_bytes"], np.uint8), want["dst"]) and np.array_equal(get(q["os"], n, np.int32), want["out_size"])
                assert np.array_equal(get(q["oo"], n, np.int64), want["out_offset"]) and np.array_equal(get(d["nroc"], B, np.int32), want["next_roc"])
                assert hip.hipMemcpy(C.c_void_p(q["keep"]), C.c_void_p(q["dst"]), C.c_size_t(q["dst_bytes"]), C.c_int(3)) == 0
                un(q, True)
                assert np.array_equal(get(q["dst"], q["dst_bytes"], np.uint8), uwant["ring"]) and np.array_equal(get(d["state_out"], state.shape, np.int32), uwant["state"])
                assert np.array_equal(get(q["usz"], n, np.int32), uwant["sizes"]) and np.array_equal(get(q["uidx"], n, np.int64), uwant["index"])
                assert np.array_equal(get(q["ustats"], api.SRTP_STATS_WORDS, np.int32), uwant["stats"])
            checked[q["name"]] = int(want["out_size"].sum())
        for rnd in range(a.warmup + a.calls):
            for name, (call, before, host) in variants.items():
                if host and rnd >= a.warmup + a.host_calls:
                    continue
                if before:
                    before()
                if host:
                    t0 = time.perf_counter(); call(); ms = (time.perf_counter() - t0) * 1e3
                else:
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
    out = {"tool": "gcm_rate", "streams": B, "frames": T, "frame_bytes": NB, "packets": n, "rtp_bytes": n * pitch, "srtp_bytes": checked, "workspace_bytes": wb,
           "calls": a.calls, "host_calls": a.host_calls, "warmup": a.warmup, "variants": {}}
    for name, v in times.items():
        if v:
            out["variants"][name] = {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "runs": len(v)}
    ms = lambda name: out["variants"][name]["ms_median"]
    ratios = {}
    for g in ("gcm128", "gcm256"):
        for side in ("protect", "unprotect"):
            k = "%s_%s" % (g, side)
            ratios[k + "_over_hmac80"] = round(ms(k) / ms("hmac80_" + side), 4)
            if k + "_host" in out["variants"]:
                ratios[k + "_over_host"] = round(ms(k) / ms(k + "_host"), 6)
            ratios[k + "_over_copy"] = round(ms(k) / ms("copy"), 3)
            ratios[k + "_GB_per_s"] = round(checked[g] / ms(k) / 1e6, 1)
    out["ratios"] = ratios
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if a.ab and a.ab_out:
        with open(a.ab_out, "w") as f:
            f.write("# The GHASH table of a lane's key as a lane-interleaved copy in LDS (64 KiB a workgroup; the product) against reads from its context in global memory\n"
                    "# (16 bytes a step, -DLC3G_LDS_TABLE=0): the GCM protect and unprotect calls of tools/gcm_rate.py's workload (%d streams x %d frames of %d bytes,\n"
                    "# %d packets, frame-major), both libraries in one process through their own entry points and alternated call by call, medians / fastest /\n"
                    "# slowest of %d calls between device events, ms.\n" % (B, T, NB, n, a.calls))
            f.write("%-34s %10s %10s %10s\n" % ("call", "median", "min", "max"))
            for g in ("gcm128", "gcm256"):
                for side in ("protect", "unprotect"):
                    for where in ("lds", "global"):
                        v = out["variants"]["ab_%s_%s_%s" % (where, g, side)]
                        f.write("%-34s %10.4f %10.4f %10.4f\n" % ("%s_%s %s" % (g, side, where), v["ms_median"], v["ms_min"], v["ms_max"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
