"""Packet ingest rate (lc3plus_dec_batch_ingest) beside the calls around it and the host detour it replaces: 4096 mono streams x 64 frames, 48 kHz / 10 ms, 80-byte
frames (the encoder's own), one batch, one process.  Of the 262 144 cells 5 % get no packet and 10 % get two; the packet list is shuffled.  Variants, alternated
run by run:
  ingest   (a) lc3plus_dec_batch_ingest with the SIDE records, every output asked for
  side     (b) the probe at LC3PLUS_PROBE_SIDE over the same items
  dec      (c) lc3plus_dec_batch_decode_packed with set_frame_counts on the tables the ingest call wrote
  host     (d) the path the ingest call replaces: synchronise, copy the records to the host, api.plan_ingest there, copy offsets, num_bytes and counts back
(a) - (c): device events around the call on the call's stream (sync = 0).  (d): the host clock from before the synchronise (nothing is pending: the wait itself
is not in the figure) to the return of the last copy.  Per variant the median, the fastest and the slowest of --calls runs after --warmup rounds.  Before timing
the device tables are checked against api.plan_ingest.  Writes one JSON object to --out and prints it.
    python tools/dec_ingest_rate.py [--calls 20] [--warmup 3] [--out profiles/dec_ingest_rate.json] [--streams 4096]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from audio_codec_amd import api
from tests.lc3_harness import synth_pcm

T, U, FS, MS, NB = 64, 64, 48000, 10.0, 80


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dec_ingest_rate.json"))
    a = ap.parse_args()
    B = a.streams
    assert B % U == 0
    hip = C.CDLL("libamdhip64.so")
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    ptrs = []

    def put(x):
        x = np.ascontiguousarray(x); p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(x.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
        ptrs.append(p); return p.value

    def get(p, shape, dtype):
        out = np.zeros(shape, dtype)
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(p), C.c_size_t(out.nbytes), C.c_int(2)) == 0
        return out
    e = amd.Batch(U, FS, 1, MS, 0, [NB * 800] * U, device=0)
    frames = np.ascontiguousarray(np.tile(e.encode(synth_pcm(U, T, 480, FS, seed=9))[:, :, :NB], (B // U, 1, 1)))
    e.close()
    cells = B * T
    rng = np.random.RandomState(17)
    draw = rng.randint(0, 100, size=cells)
    cell = np.concatenate([np.flatnonzero(draw >= 5), np.flatnonzero(draw >= 90)])        # 5 % missing; 10 % twice
    cell = cell[rng.permutation(cell.size)]
    n = int(cell.size)
    base = rng.randint(0, 65536, size=B).astype(np.int32)
    i_stream, i_seq = (cell // T).astype(np.int32), ((base[cell // T] + cell % T) & 0xFFFF).astype(np.int32)
    i_off, i_nb = cell.astype(np.int64) * NB, np.full(n, NB, np.int32)
    d_in, d_stream, d_seq, d_off, d_nb, d_base = put(frames), put(i_stream), put(i_seq), put(i_off), put(i_nb), put(base)
    d_info = put(np.zeros((n, api.FRAME_INFO_WORDS), np.int32))
    d_oo, d_onb, d_ci, d_counts = put(np.zeros(cells, np.int64)), put(np.zeros(cells, np.int32)), put(np.zeros(cells, np.int32)), put(np.zeros(B, np.int32))
    d_next, d_stats, d_ist = put(np.zeros(B, np.int32)), put(np.zeros((B, api.ING_STATS_WORDS), np.int32)), put(np.zeros(n, np.uint8))
    d_pcm, d_st = put(np.zeros(cells * 480, np.int16)), put(np.zeros(cells, np.uint8))
    dec = amd.DecBatch(B, FS, 1, MS, 0, None, device=0)
    dec.set_frame_counts(d_counts)
    info = np.zeros((n, 1, api.FRAME_INFO_WORDS), np.int32)

    def host():
        assert hip.hipStreamSynchronize(stream) == 0
        assert hip.hipMemcpy(C.c_void_p(info.ctypes.data), C.c_void_p(d_info), C.c_size_t(info.nbytes), C.c_int(2)) == 0
        r = api.plan_ingest(B, 1, i_stream, i_seq, i_off, i_nb, base, T, 16, info, None, ())
        for p, x in ((d_oo, r["offsets"]), (d_onb, r["num_bytes"]), (d_counts, r["counts"])):
            assert hip.hipMemcpy(C.c_void_p(p), C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
    calls = {
        "ingest": lambda: dec.ingest_device(n, d_stream, d_seq, d_off, d_nb, d_base, T, d_oo, d_onb, d_ci, d_counts, 16, d_info, None, d_next, d_stats, d_ist,
                                            stream.value, False),
        "side": lambda: dec.probe_device(d_in, frames.size, d_off, d_nb, NB, n, d_info, api.PROBE_SIDE, stream.value, False),
        "dec": lambda: dec.decode_device_packed(d_in, frames.size, d_oo, T, d_pcm, d_onb, NB, None, d_st, hip_stream=stream.value, sync=False),
        "host": host,
    }
    times = {k: [] for k in calls}
    try:
        calls["side"](); calls["ingest"]()
        assert hip.hipStreamSynchronize(stream) == 0
        info[:] = get(d_info, info.shape, np.int32)
        want = api.plan_ingest(B, 1, i_stream, i_seq, i_off, i_nb, base, T, 16, info, None)
        got = dict(offsets=get(d_oo, (B, T), np.int64), num_bytes=get(d_onb, (B, T), np.int32), cell_item=get(d_ci, (B, T), np.int32), counts=get(d_counts, B, np.int32),
                   next_base=get(d_next, B, np.int32), stats=get(d_stats, (B, api.ING_STATS_WORDS), np.int32), item_status=get(d_ist, n, np.uint8))
        for k, w in want.items():
            assert np.array_equal(got[k], w), k
        assert not info[:, 0, api.FI_STATUS].any() and int((got["cell_item"] < 0).sum()) == cells - int((draw >= 5).sum())
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
        dec.close()
        for p in ptrs:
            hip.hipFree(p)
    hip.hipEventDestroy(ev0); hip.hipEventDestroy(ev1); hip.hipStreamDestroy(stream)
    out = {"tool": "dec_ingest_rate", "streams": B, "frames": T, "frame_bytes": NB, "cells": cells, "items": n, "duplicated_cells": int((draw >= 90).sum()),
           "missing_cells": int((draw < 5).sum()), "calls": a.calls, "warmup": a.warmup, "variants": {}}
    for k, v in times.items():
        med = float(np.median(v))
        out["variants"][k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "Mitems_per_s": round(n / med / 1e3, 2)}
    va = out["variants"]
    out["host_record_bytes"] = int(info.nbytes)
    out["ingest_over_dec"] = round(va["ingest"]["ms_median"] / va["dec"]["ms_median"], 4)
    out["ingest_over_host"] = round(va["ingest"]["ms_median"] / va["host"]["ms_median"], 4)
    out["ingest_over_side"] = round(va["ingest"]["ms_median"] / va["side"]["ms_median"], 4)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
