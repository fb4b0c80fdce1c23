"""FEC-repair rates (lc3plus_dec_batch_fec_repair) beside what the call could be replaced by: --streams streams of 80-byte frames (random bytes: these kernels
move and XOR bytes, whatever they hold), 92-byte RTP packets, parity over every four, one decoder batch, one process.

Real-time calls: one media packet a stream a call, the parity of a group beside its fourth packet, H = 16, P = 4; a script of 16 calls is replayed round after
round with the sequence numbers moved on by 16, so the stores run on as a receiver's do.  A call without parity is a "media" call, the fourth a "parity" call;
the two are timed apart.  Variants, alternated call by call within one run, each over stores of its own:
  repair_lL_pP   the repair call at L = 2, 10 per cent of the media packets lost at random (they never arrive: stream -1), P = 1, 3 passes
  recover_lL     lc3plus_dec_batch_fec_recover on the same call's lists, window 64: what the library could do before.  It rebuilds nothing across calls, so it is
                 a cost yardstick, not an equal; a call without FEC items it refuses, so it has parity calls only
  memcpy_lL      one hipMemcpyAsync, device to device, of the bytes the call copies into its stores (the arrived packets, the FEC payloads)
  host_l2_p1     the detour the call replaces: synchronise, the lists and the arrival area to the host, lc3plus_plan_fec_repair there over host stores, the history,
                 its metadata and the rec list back; the host clock from before the synchronise (nothing is pending) to the return of the last copy
One long call: 64 packets a stream and their 16 parity packets in one call, H = 64, P = 16, the state zeroed before every call (not timed):
  long_repair_p1, long_recover (window 64), long_memcpy
Device variants: device events around the one call, the stream idle before it.  Per variant and kind of call the median, the fastest and the slowest over
--rounds rounds after --warmup rounds.  Before timing counts for anything, every call's stats and rec_seq of repair_l2_p1 are held to the host detour's, which is
the plan.  Writes one JSON object to --out and prints it.
    python tools/fec_repair_rate.py [--rounds 12] [--warmup 2] [--streams 4096] [--out profiles/fec_repair_rate.json]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from audio_codec_amd import api, packet

NB, PKT, FEC, K, SCRIPT = 80, 92, 94, 4, 16
LOSSES, PASSES = (2, 10), (1, 3)


def stat(x):
    x = sorted(x)
    return dict(median_us=round(1e3 * x[len(x) // 2], 2), fastest_us=round(1e3 * x[0], 2), slowest_us=round(1e3 * x[-1], 2), samples=len(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fec_repair_rate.json"))
    a = ap.parse_args()
    B = a.streams
    hip = C.CDLL("libamdhip64.so")
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    sv = stream.value

    def put(x):
        x = np.ascontiguousarray(x); p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(max(x.nbytes, 8))) == 0
        assert hip.hipMemcpy(p, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
        return p.value

    def up(p, x):
        x = np.ascontiguousarray(x); assert hip.hipMemcpy(C.c_void_p(p), C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0

    def down(x, p):
        assert hip.hipMemcpy(C.c_void_p(x.ctypes.data), C.c_void_p(p), C.c_size_t(x.nbytes), C.c_int(2)) == 0

    def d2d(dst, src, n, async_=True):
        assert hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(n), C.c_int(3), stream) == 0

    def timed(fn):
        """device events around fn's launches on the idle stream -> ms"""
        assert hip.hipStreamSynchronize(stream) == 0 and hip.hipEventRecord(ev0, stream) == 0
        fn()
        assert hip.hipEventRecord(ev1, stream) == 0 and hip.hipEventSynchronize(ev1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
        return float(ms.value)

    rng = np.random.RandomState(5)
    dec = amd.DecBatch(B, 48000, 1, 10.0, 0, None, device=0)
    ssrc = (0x1000 + np.arange(B)).astype(np.int32)
    d_ssrc = put(ssrc)
    zeros = lambda n, dt: put(np.zeros(n, dt))

    def media(T, seq0):
        """[T, B, PKT] RTP packets of position t with sequence number seq0[b] + t"""
        p = rng.randint(0, 256, (T, B, PKT)).astype(np.uint8)
        sn = (seq0[None, :] + np.arange(T)[:, None]) & 0xFFFF
        p[..., 0], p[..., 1], p[..., 2], p[..., 3] = 0x80, 96, sn >> 8, sn & 255
        p[..., 8:12] = ssrc.astype(">u4").view(np.uint8).reshape(B, 4)[None]
        return p

    def parity(p):
        """[T / K, B, FEC] FEC payloads over every K packets of [T, B, PKT]"""
        g = p.reshape(-1, K, B, PKT)
        x = np.bitwise_xor.reduce(g, axis=1)
        f = np.zeros((g.shape[0], B, FEC), np.uint8)
        f[..., 0], f[..., 1], f[..., 2:4], f[..., 4:8] = x[..., 0] & 0x3F, x[..., 1], g[:, 0, :, 2:4], x[..., 4:8]
        f[..., 8:10] = 0                                                 # the XOR of K equal lengths, K even
        f[..., 10], f[..., 11], f[..., 12], f[..., 13] = 0, NB, 0xF0, 0
        f[..., 14:] = x[..., 12:]
        return f

    def move(p, f, by):
        """the script's packets with every sequence number moved on by `by`, in place"""
        for arr, at in ((p, 2), (f, 2)):
            sn = ((arr[..., at].astype(np.int64) << 8 | arr[..., at + 1]) + by) & 0xFFFF
            arr[..., at], arr[..., at + 1] = sn >> 8, sn & 255

    # ---- the real-time script ----
    H, P, MS, FS = 16, 4, 96, 96
    area = (B * PKT + B * FEC + 15) & ~15
    hist = B * H * MS
    seq0 = (rng.randint(0, 1 << 16, B)).astype(np.int64)
    pk = media(SCRIPT, seq0)
    fp = parity(pk)
    offs = np.arange(B, dtype=np.int64) * PKT
    foffs = B * PKT + np.arange(B, dtype=np.int64) * FEC
    d_off, d_size, d_foff, d_fsize, d_fstream = put(offs), put(np.full(B, PKT, np.int32)), put(foffs), put(np.full(B, FEC, np.int32)), put(np.arange(B, dtype=np.int32))
    arrive = {l: rng.rand(SCRIPT, B) >= l / 100.0 for l in LOSSES}
    d_stream = {l: [put(np.where(arrive[l][c], np.arange(B), -1).astype(np.int32)) for c in range(SCRIPT)] for l in LOSSES}
    d_area = [put(np.zeros(area, np.uint8)) for _ in range(SCRIPT)]
    d_seq, d_fseq = [zeros(B, np.int32) for _ in range(SCRIPT)], [zeros(B, np.int32) for _ in range(SCRIPT)]
    wb = api.fec_repair_work_bytes(B, H, P)

    def stores():
        return dict(ring=zeros(area + hist + 8, np.uint8), med_seq=zeros(B * H, np.int32), med_size=zeros(B * H, np.int32), store=zeros(B * P * FS, np.uint8),
                    cell_seq=zeros(B * P, np.int32), cell_size=zeros(B * P, np.int32), cell_status=zeros(B * P, np.uint8), state=zeros(B * 4, np.int32),
                    rec_off=zeros(B * P, np.int64), rec_size=zeros(B * P, np.int32), rec_seq=zeros(B * P, np.int32), stats=zeros(16, np.int32), work=zeros(wb + 8, np.uint8))
    var = {(l, p): stores() for l in LOSSES for p in PASSES}
    rstride, window = 96, 64
    rec = {l: dict(ring=zeros(area + B * rstride + 8, np.uint8), off=zeros(B, np.int64), size=zeros(B, np.int32), seq=zeros(B, np.int32), status=zeros(B, np.uint8),
                   stats=zeros(16, np.int32), work=zeros(api.fec_recover_work_bytes(B, window) + 8, np.uint8)) for l in LOSSES}
    d_sink = zeros(area, np.uint8)
    # the host detour's arrays, persistent: the plan advances them in place
    h = dict(ring=np.zeros(area + hist, np.uint8), med_seq=np.zeros(B * H, np.int32), med_size=np.zeros(B * H, np.int32), fec_store=np.zeros(B * P * FS, np.uint8),
             cell_seq=np.zeros(B * P, np.int32), cell_size=np.zeros(B * P, np.int32), cell_status=np.zeros(B * P, np.uint8), state=np.zeros(B * 4, np.int32),
             rec_dg_offsets=np.zeros(B * P, np.int64), rec_dg_sizes=np.zeros(B * P, np.int32), rec_seq=np.zeros(B * P, np.int32), stats=np.zeros(16, np.int32),
             work=np.zeros(wb // 8 + 1, np.int64), stream=np.zeros(B, np.int32), seq=np.zeros(B, np.int32), fec_seq=np.zeros(B, np.int32))
    hd = stores()                                                        # where the detour's results go back to
    L = amd.load_library()

    def repair(v, l, p, c, n_fec):
        dec.fec_repair_device(B, v["ring"], area + hist, d_off, d_size, d_stream[l][c], d_seq[c], n_fec, d_fstream, d_foff, d_fsize, d_fseq[c], d_ssrc, area, H, MS,
                              v["med_seq"], v["med_size"], v["store"], P, FS, v["cell_seq"], v["cell_size"], v["cell_status"], v["state"], v["rec_off"], v["rec_size"],
                              v["rec_seq"], v["work"], p, None, None, v["stats"], sv, False)

    def recover(r, l, c):
        dec.fec_recover_device(B, r["ring"], area + B * rstride, d_off, d_size, d_stream[l][c], d_seq[c], B, d_fstream, d_foff, d_fsize, window, d_ssrc, area, rstride,
                               r["off"], r["size"], r["seq"], r["work"], r["status"], r["stats"], sv, False)

    def detour(l, c, n_fec):
        t0 = time.perf_counter()
        assert hip.hipStreamSynchronize(stream) == 0
        down(h["ring"][:area], d_area[c]); down(h["stream"], d_stream[l][c]); down(h["seq"], d_seq[c]); down(h["fec_seq"], d_fseq[c])
        v = dict(n_streams=B, n_items=B, ring=h["ring"], ring_capacity=area + hist, dg_offsets=offs, dg_sizes=np.full(B, PKT, np.int32), stream=h["stream"], seq=h["seq"],
                 n_fec=n_fec, fec_stream=np.arange(B, dtype=np.int32), fec_offsets=foffs, fec_num_bytes=np.full(B, FEC, np.int32), fec_seq=h["fec_seq"], ssrc=ssrc,
                 med_offset=area, med_slots=H, med_stride=MS, med_seq=h["med_seq"], med_size=h["med_size"], fec_store=h["fec_store"], fec_slots=P, fec_stride=FS,
                 cell_seq=h["cell_seq"], cell_size=h["cell_size"], cell_status=h["cell_status"], state=h["state"], passes=1, rec_dg_offsets=h["rec_dg_offsets"],
                 rec_dg_sizes=h["rec_dg_sizes"], rec_seq=h["rec_seq"], item_status=None, fec_status=None, stats=h["stats"], work=h["work"], hip_stream=None, sync=0)
        packet._invoke(L, "lc3plus_plan_fec_repair", v, packet._host)
        up(hd["ring"] + area, h["ring"][area:]); up(hd["med_seq"], h["med_seq"]); up(hd["med_size"], h["med_size"])
        up(hd["rec_off"], h["rec_dg_offsets"]); up(hd["rec_size"], h["rec_dg_sizes"]); up(hd["rec_seq"], h["rec_seq"])
        return 1e3 * (time.perf_counter() - t0)

    times, rebuilt, checked = {}, {}, 0
    add = lambda name, kind, ms, keep: times.setdefault(name, {}).setdefault(kind, []).append(ms) if keep else None
    for r in range(a.warmup + a.rounds):
        keep = r >= a.warmup
        if r:
            move(pk, fp, SCRIPT)
        for c in range(SCRIPT):                                          # the round's datagrams and numbers, staged in device memory: not timed
            buf = np.zeros(area, np.uint8)
            buf[:B * PKT] = pk[c].ravel()
            if c % K == K - 1:
                buf[B * PKT:B * PKT + B * FEC] = fp[c // K].ravel()
            up(d_area[c], buf)
            up(d_seq[c], ((seq0 + SCRIPT * r + c) & 0xFFFF).astype(np.int32))
            up(d_fseq[c], np.full(B, (SCRIPT // K * r + c // K) & 0xFFFF, np.int32))
        for c in range(SCRIPT):
            n_fec = B if c % K == K - 1 else 0
            kind = "parity_call" if n_fec else "media_call"
            for l in LOSSES:
                for p in PASSES:
                    v = var[(l, p)]
                    d2d(v["ring"], d_area[c], area)
                    add("repair_l%d_p%d" % (l, p), kind, timed(lambda: repair(v, l, p, c, n_fec)), keep)
                    st = np.zeros(16, np.int32); down(st, v["stats"])
                    rebuilt["repair_l%d_p%d" % (l, p)] = rebuilt.get("repair_l%d_p%d" % (l, p), 0) + int(st[0])
                    if (l, p) == (2, 1):
                        want_stats = st
                        got_seq = np.zeros(B * P, np.int32); down(got_seq, v["rec_seq"])
                if n_fec:
                    d2d(rec[l]["ring"], d_area[c], area)
                    add("recover_l%d" % l, kind, timed(lambda: recover(rec[l], l, c)), keep)
                nbytes = int(arrive[l][c].sum()) * PKT + (B * FEC if n_fec else 0)
                add("memcpy_l%d" % l, kind, timed(lambda: d2d(d_sink, d_area[c], nbytes)), keep)
            add("host_l2_p1", kind, detour(2, c, n_fec), keep)
            assert np.array_equal(h["stats"], want_stats) and np.array_equal(h["rec_seq"], got_seq), ("the kernels and the plan differ", r, c)
            checked += 1

    # ---- one long call ----
    T, H2, P2 = 64, 64, 16
    area2 = (B * T * PKT + B * (T // K) * FEC + 15) & ~15
    pk2 = media(T, seq0)
    fp2 = parity(pk2)
    buf = np.zeros(area2, np.uint8)
    buf[:B * T * PKT] = pk2.transpose(1, 0, 2).ravel()                  # stream-major
    buf[B * T * PKT:B * T * PKT + B * (T // K) * FEC] = fp2.transpose(1, 0, 2).ravel()
    n2, m2 = B * T, B * (T // K)
    arr2 = rng.rand(n2) >= 0.02
    d2 = dict(ring=put(np.concatenate([buf, np.zeros(B * H2 * MS + 8, np.uint8)])), off=put(np.arange(n2, dtype=np.int64) * PKT), size=put(np.full(n2, PKT, np.int32)),
              stream=put(np.where(arr2, np.repeat(np.arange(B), T), -1).astype(np.int32)), seq=put(((np.repeat(seq0, T) + np.tile(np.arange(T), B)) & 0xFFFF).astype(np.int32)),
              foff=put(B * T * PKT + np.arange(m2, dtype=np.int64) * FEC), fsize=put(np.full(m2, FEC, np.int32)), fstream=put(np.repeat(np.arange(B), T // K).astype(np.int32)),
              fseq=put(np.tile(np.arange(T // K), B).astype(np.int32)), med_seq=zeros(B * H2, np.int32), med_size=zeros(B * H2, np.int32), store=zeros(B * P2 * FS, np.uint8),
              cell_seq=zeros(B * P2, np.int32), cell_size=zeros(B * P2, np.int32), cell_status=zeros(B * P2, np.uint8), state=zeros(B * 4, np.int32),
              rec_off=zeros(B * P2, np.int64), rec_size=zeros(B * P2, np.int32), rec_seq=zeros(B * P2, np.int32), stats=zeros(16, np.int32),
              work=zeros(api.fec_repair_work_bytes(B, H2, P2) + 8, np.uint8))
    r2 = dict(ring=put(np.concatenate([buf, np.zeros(m2 * rstride + 8, np.uint8)])), off=zeros(m2, np.int64), size=zeros(m2, np.int32), seq=zeros(m2, np.int32),
              status=zeros(m2, np.uint8), stats=zeros(16, np.int32), work=zeros(api.fec_recover_work_bytes(B, window) + 8, np.uint8))
    sink2 = zeros(area2, np.uint8)

    def long_repair():
        dec.fec_repair_device(n2, d2["ring"], area2 + B * H2 * MS, d2["off"], d2["size"], d2["stream"], d2["seq"], m2, d2["fstream"], d2["foff"], d2["fsize"], d2["fseq"], d_ssrc,
                              area2, H2, MS, d2["med_seq"], d2["med_size"], d2["store"], P2, FS, d2["cell_seq"], d2["cell_size"], d2["cell_status"], d2["state"], d2["rec_off"],
                              d2["rec_size"], d2["rec_seq"], d2["work"], 1, None, None, d2["stats"], sv, False)

    def long_recover():
        dec.fec_recover_device(n2, r2["ring"], area2 + m2 * rstride, d2["off"], d2["size"], d2["stream"], d2["seq"], m2, d2["fstream"], d2["foff"], d2["fsize"], window, d_ssrc,
                               area2, rstride, r2["off"], r2["size"], r2["seq"], r2["work"], r2["status"], r2["stats"], sv, False)
    for r in range(a.warmup + a.rounds):
        keep = r >= a.warmup
        assert hip.hipMemsetAsync(C.c_void_p(d2["state"]), 0, C.c_size_t(16 * B), stream) == 0
        add("long_repair_p1", "call", timed(long_repair), keep)
        add("long_recover", "call", timed(long_recover), keep)
        add("long_memcpy", "call", timed(lambda: d2d(sink2, d2["ring"], int(arr2.sum()) * PKT + m2 * FEC)), keep)
    st = np.zeros(16, np.int32); down(st, d2["stats"]); rebuilt["long_repair_p1"] = int(st[0])
    st = np.zeros(16, np.int32); down(st, r2["stats"]); rebuilt["long_recover"] = int(st[0])

    out = dict(streams=B, frame_bytes=NB, packet_bytes=PKT, group=K, realtime=dict(med_slots=H, fec_slots=P, script_calls=SCRIPT), long=dict(frames=T, med_slots=H2, fec_slots=P2),
               rounds=a.rounds, warmup=a.warmup, calls_held_to_the_plan=checked,
               note="us per call; device variants by device events around one call on an idle stream, host_l2_p1 by the host clock; recover rebuilds nothing across calls",
               variants={name: {kind: stat(x) for kind, x in kinds.items()} for name, kinds in sorted(times.items())},
               packets_rebuilt_over_all_rounds_or_in_the_last_long_call=rebuilt)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
