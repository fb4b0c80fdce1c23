"""Encoder rate with per-stream frame counts (lc3plus_enc_batch_set_frame_counts): 4096 mono streams, 48 kHz / 10 ms, 80-byte frames, calls of 4 and of 16
frames, lc3plus_enc_batch_encode_rates_device (per-frame bitrates, all 64 kbit/s) with sync = 0, everything in device memory, one batch per call length, one
process.  Variants, alternated call by call:
  a, a2   the call without counts, twice: the difference between the two is the spread a variant has to exceed to mean anything
  b       counts all n_frames
  c       counts uniform in 0 ... n_frames
  d       alternating n_frames and 0 (even and odd streams)
A dense call with per-frame bitrates runs the one-wave kernel at either length (lc3_encode_kernel_var behind the 12.8 kHz pre-kernels); --dense-words bw gives
the dense call per-frame bandwidths instead, which at 16 frames runs the pipelined kernels: what a ragged call of that length gives up today.
Device events around every call on the call's stream; per variant the median, the fastest and the slowest of --calls calls after --warmup rounds, the number
of present frames and present frames per second.  Writes one JSON object to --out and prints it.
    python tools/enc_ragged_rate.py [--calls 60] [--warmup 5] [--out profiles/enc_ragged_rate.json] [--variants a,a2,b,c,d] [--frames 4,16] [--dense-words br,bw]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from tests.lc3_harness import synth_pcm

B, U, FS, MS, NB, N = 4096, 64, 48000, 10.0, 80, 480


def run(hip, put, T, words, variants, calls, warmup):
    pcm = np.ascontiguousarray(np.tile(synth_pcm(U, T, N, FS, seed=9)[:, :, None, :], (B // U, 1, 1, 1)))
    rng = np.random.default_rng(T)
    counts = {"a": None, "a2": None, "b": np.full(B, T, np.int32), "c": rng.integers(0, T + 1, B).astype(np.int32),
              "d": np.where(np.arange(B) % 2 == 0, T, 0).astype(np.int32)}
    counts = {k: counts[k] for k in variants}
    d_counts = {k: put(v) if v is not None else None for k, v in counts.items()}
    d_pcm, d_out = put(pcm), put(np.zeros((B, T, NB), np.uint8))
    d_br = put(np.full((B, T), NB * 800, np.int32)) if words == "br" else None
    d_bw = put(np.zeros((B, T), np.int32)) if words == "bw" else None
    d_nb, d_fl = put(np.zeros((B, T), np.int32)), put(np.zeros((B, T), np.uint8))
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    enc = amd.Batch(B, FS, 1, MS, 0, [NB * 800] * B, device=0)
    times = {k: [] for k in counts}
    try:
        for rnd in range(warmup + calls):
            for k in counts:
                enc.set_frame_counts(d_counts[k])
                assert hip.hipEventRecord(ev0, stream) == 0
                enc.encode_device_rates(d_pcm, 16, T, d_out, NB, d_br, d_bw, d_nb, d_fl, hip_stream=stream.value, sync=False)
                assert hip.hipEventRecord(ev1, stream) == 0 and hip.hipEventSynchronize(ev1) == 0
                ms = C.c_float(0); assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
                if rnd >= warmup:
                    times[k].append(ms.value)
        enc.set_frame_counts(None)
    finally:
        enc.close()
        hip.hipEventDestroy(ev0); hip.hipEventDestroy(ev1); hip.hipStreamDestroy(stream)
    out = {"frames": T, "dense_words": words, "variants": {}}
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--variants", default="a,a2,b,c,d")
    ap.add_argument("--frames", default="4,16")
    ap.add_argument("--dense-words", default="br,bw")
    a = ap.parse_args()
    assert a.calls >= 50
    if a.variants == "a,a2,b,c,d" and a.frames == "4,16" and a.dense_words == "br,bw" and not a.out:
        a.out = os.path.join(ROOT, "profiles", "enc_ragged_rate.json")
    hip = C.CDLL("libamdhip64.so")
    ptrs = []

    def put(x):
        x = np.ascontiguousarray(x); p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(x.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
        ptrs.append(p); return p.value
    out = {"tool": "enc_ragged_rate", "streams": B, "frame_bytes": NB, "calls": a.calls, "warmup": a.warmup, "runs": []}
    try:
        for words in a.dense_words.split(","):
            for T in (int(x) for x in a.frames.split(",")):
                out["runs"].append(run(hip, put, T, words, a.variants.split(","), a.calls, a.warmup))
    finally:
        for p in ptrs:
            hip.hipFree(p)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
