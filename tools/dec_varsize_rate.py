"""Decoder rate with per-frame frame sizes against fixed sizes (d5's shape: 4096 streams x 64 frames per call, 48 kHz / 10 ms, the twelve rates of
bench.py's c5 / d5).  Bitstreams: one GPU encode per rate of 64 streams x 64 frames; stream s takes its frame t from the pool of rate k at stream
s % 64, frame t.  Fixed: k = s % 12 for every frame (lc3plus_dec_batch_decode with device pointers, one size per stream).  Per-frame: k = (s + t) % 12,
so every stream changes size every frame (lc3plus_dec_batch_decode_sizes with device pointers).  Both calls synchronous, frames and PCM in device
memory, the same size mix; wall time per call over --calls calls after --warmup.  Prints one JSON line.
    python tools/dec_varsize_rate.py [--calls 20] [--warmup 5]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from tests.lc3_harness import synth_pcm

RATES12 = [16000, 24000, 32000, 48000, 64000, 80000, 96000, 128000, 160000, 192000, 256000, 320000]
B, T, U, FS, MS = 4096, 64, 64, 48000, 10.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    pcm = synth_pcm(U, T, 480, FS, seed=9)
    pool = []
    for r in RATES12:
        e = amd.Batch(U, FS, 1, MS, 0, [r] * U, device=0)
        pool.append(e.encode(pcm)[:, :, :r // 800]); e.close()
    stride = max(p.shape[2] for p in pool)
    s_idx = np.arange(B)[:, None]; t_idx = np.arange(T)[None, :]
    out = {"tool": "dec_varsize_rate", "streams": B, "frames": T, "rates": RATES12}
    hip = C.CDLL("libamdhip64.so")
    ptrs = []

    def put(x):
        p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(x.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
        ptrs.append(p); return p.value
    d_pcm = C.c_void_p(); assert hip.hipMalloc(C.byref(d_pcm), C.c_size_t(B * T * 480 * 2)) == 0; ptrs.append(d_pcm)
    try:
        for mode, k in (("fixed", (s_idx + 0 * t_idx) % 12), ("per_frame", (s_idx + t_idx) % 12)):
            frames = np.zeros((B, T, stride), np.uint8); nb = np.zeros((B, T), np.int32)
            for kk in range(12):
                m = k == kk
                src = pool[kk][(s_idx % U).repeat(T, 1)[m], t_idx.repeat(B, 0)[m]]
                frames[m, :src.shape[1]] = src; nb[m] = src.shape[1]
            d_in = put(frames)
            dec = amd.DecBatch(B, FS, 1, MS, 0, nb[:, 0].tolist(), device=0)

            def call():
                if mode == "fixed":
                    dec.decode_device(d_in, stride, T, d_pcm.value, 16, sync=True)
                else:
                    dec.decode_device(d_in, stride, T, d_pcm.value, 16, sync=True, num_bytes=nb)
            for _ in range(a.warmup):
                call()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call()
            ms = (time.perf_counter() - t0) * 1e3 / a.calls
            out[mode] = {"ms_per_call": round(ms, 4), "Mframes_per_s": round(B * T / ms / 1e3, 2), "kernel_ms_last_call": round(dec.last_kernel_ms(), 4),
                         "size_changes_per_stream": int((np.diff(nb, axis=1) != 0).sum(axis=1).mean())}
            dec.close()
        out["per_frame_vs_fixed"] = round(out["per_frame"]["Mframes_per_s"] / out["fixed"]["Mframes_per_s"], 4)
    finally:
        for p in ptrs:
            hip.hipFree(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
