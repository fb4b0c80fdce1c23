"""Decoder rate with per-stream frame counts (lc3plus_dec_batch_set_frame_counts): 4096 mono streams x 16 frames per call, 48 kHz / 10 ms, 80-byte frames,
lc3plus_dec_batch_decode_sizes_device with sync = 0, everything in device memory, one batch, one process.  Variants, alternated call by call:
  a, a2   the call without counts, twice: the difference between the two is the spread a variant has to exceed to mean anything
  b       counts all 16
  c       counts uniform in 0 ... 16
  d       half the streams 16, half 0 (even and odd streams: every wave of the one-lane-per-stream kernels holds both)
Device events around every call on the call's stream; per variant the median, the fastest and the slowest of --calls calls after --warmup rounds, the number
of present frames and present frames per second.  Writes one JSON object to --out and prints it.
--variants a,d runs only those (under rocprofv3 --kernel-trace --stats the _rag kernels' durations are then one variant's) and writes no file unless --out is given.
    python tools/dec_ragged_rate.py [--calls 60] [--warmup 5] [--out profiles/dec_ragged_rate.json] [--variants a,a2,b,c,d]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from tests.lc3_harness import synth_pcm

B, T, U, FS, MS, NB = 4096, 16, 64, 48000, 10.0, 80


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--variants", default="a,a2,b,c,d")
    a = ap.parse_args()
    assert a.calls >= 50
    if a.variants == "a,a2,b,c,d" and not a.out:
        a.out = os.path.join(ROOT, "profiles", "dec_ragged_rate.json")
    e = amd.Batch(U, FS, 1, MS, 0, [NB * 800] * U, device=0)
    frames = np.ascontiguousarray(np.tile(e.encode(synth_pcm(U, T, 480, FS, seed=9))[:, :, :NB], (B // U, 1, 1)))
    e.close()
    hip = C.CDLL("libamdhip64.so")
    ptrs = []

    def put(x):
        x = np.ascontiguousarray(x); p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(x.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
        ptrs.append(p); return p.value
    rng = np.random.default_rng(16)
    counts = {"a": None, "a2": None, "b": np.full(B, T, np.int32), "c": rng.integers(0, T + 1, B).astype(np.int32),
              "d": np.where(np.arange(B) % 2 == 0, T, 0).astype(np.int32)}
    counts = {k: counts[k] for k in a.variants.split(",")}
    d_counts = {k: put(v) if v is not None else None for k, v in counts.items()}
    d_in, d_nb, d_pcm, d_st = put(frames), put(np.full((B, T), NB, np.int32)), put(np.zeros(B * T * 480, np.int16)), put(np.zeros((B, T), np.uint8))
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    dec = amd.DecBatch(B, FS, 1, MS, 0, [NB] * B, device=0)
    times = {k: [] for k in counts}
    try:
        for rnd in range(a.warmup + a.calls):
            for k in counts:
                dec.set_frame_counts(d_counts[k])
                assert hip.hipEventRecord(ev0, stream) == 0
                dec.decode_device_sizes(d_in, NB, T, d_pcm, d_nb, None, d_st, hip_stream=stream.value, sync=False)
                assert hip.hipEventRecord(ev1, stream) == 0 and hip.hipEventSynchronize(ev1) == 0
                ms = C.c_float(0); assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
                if rnd >= a.warmup:
                    times[k].append(ms.value)
        dec.set_frame_counts(None)
    finally:
        dec.close()
        hip.hipEventDestroy(ev0); hip.hipEventDestroy(ev1); hip.hipStreamDestroy(stream)
        for p in ptrs:
            hip.hipFree(p)
    out = {"tool": "dec_ragged_rate", "streams": B, "frames": T, "frame_bytes": NB, "calls": a.calls, "warmup": a.warmup, "variants": {}}
    for k, v in times.items():
        present = B * T if counts[k] is None else int(counts[k].sum())
        med = float(np.median(v))
        out["variants"][k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "present_frames": present,
                              "present_Mframes_per_s": round(present / med / 1e3, 2)}
    va = out["variants"]
    if len(va) == 5:
        out["spread_a2_over_a"] = round(va["a2"]["ms_median"] / va["a"]["ms_median"], 4)
        for k in ("b", "c", "d"):
            out[k + "_over_a"] = round(va[k]["ms_median"] / va["a"]["ms_median"], 4)
        for k in ("c", "d"):
            out[k + "_over_b"] = round(va[k]["ms_median"] / va["b"]["ms_median"], 4)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
