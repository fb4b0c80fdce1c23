"""Decoder rate with per-frame frame sizes in device memory (lc3plus_dec_batch_decode_sizes_device) against fixed sizes and host per-frame sizes, at
tools/dec_varsize_rate.py's shape and size mix (4096 streams x 64 frames per call, 48 kHz / 10 ms, the twelve rates of bench.py's c5 / d5; per-frame:
every stream changes size every frame).  Frames, PCM and (for the device call) sizes in device memory.  Modes:
  fixed           lc3plus_dec_batch_decode, one size per stream, synchronous
  host_sizes      lc3plus_dec_batch_decode_sizes, sizes from a host array, synchronous
  device_sizes    lc3plus_dec_batch_decode_sizes_device, synchronous
  device_async    lc3plus_dec_batch_decode_sizes_device with sync = 0, --calls calls back to back, one synchronise at the end
Wall time per call over --calls calls after --warmup.  Prints one JSON line.
    python tools/dec_varsize_device_rate.py [--calls 20] [--warmup 5]"""
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
    out = {"tool": "dec_varsize_device_rate", "streams": B, "frames": T, "rates": RATES12, "calls": a.calls}
    hip = C.CDLL("libamdhip64.so")
    ptrs = []

    def put(x):
        p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(x.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
        ptrs.append(p); return p.value
    d_pcm = C.c_void_p(); assert hip.hipMalloc(C.byref(d_pcm), C.c_size_t(B * T * 480 * 2)) == 0; ptrs.append(d_pcm)
    try:
        for mode in ("fixed", "host_sizes", "device_sizes", "device_async"):
            k = (s_idx + 0 * t_idx) % 12 if mode == "fixed" else (s_idx + t_idx) % 12
            frames = np.zeros((B, T, stride), np.uint8); nb = np.zeros((B, T), np.int32)
            for kk in range(12):
                m = k == kk
                src = pool[kk][(s_idx % U).repeat(T, 1)[m], t_idx.repeat(B, 0)[m]]
                frames[m, :src.shape[1]] = src; nb[m] = src.shape[1]
            d_in, d_nb = put(frames), put(nb)
            dec = amd.DecBatch(B, FS, 1, MS, 0, nb[:, 0].tolist(), device=0)

            def call():
                if mode == "fixed":
                    dec.decode_device(d_in, stride, T, d_pcm.value, 16, sync=True)
                elif mode == "host_sizes":
                    dec.decode_device(d_in, stride, T, d_pcm.value, 16, sync=True, num_bytes=nb)
                else:
                    dec.decode_device_sizes(d_in, stride, T, d_pcm.value, d_nb, sync=mode == "device_sizes")
            for _ in range(a.warmup):
                call()
            assert hip.hipDeviceSynchronize() == 0
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call()
            assert hip.hipDeviceSynchronize() == 0
            ms = (time.perf_counter() - t0) * 1e3 / a.calls
            out[mode] = {"ms_per_call": round(ms, 4), "Mframes_per_s": round(B * T / ms / 1e3, 2),
                         "size_changes_per_stream": int((np.diff(nb, axis=1) != 0).sum(axis=1).mean())}
            if mode != "device_async":
                out[mode]["kernel_ms_last_call"] = round(dec.last_kernel_ms(), 4)
            dec.close()
        for mode in ("host_sizes", "device_sizes", "device_async"):
            out[mode + "_vs_fixed"] = round(out[mode]["Mframes_per_s"] / out["fixed"]["Mframes_per_s"], 4)
    finally:
        for p in ptrs:
            hip.hipFree(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
