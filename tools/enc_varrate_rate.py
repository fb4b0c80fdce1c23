"""Encoder rate with per-frame bitrates against fixed rates (c5's shape: 4096 streams x 64 frames per call, 48 kHz / 10 ms, bench.py's twelve rates,
PCM and bitstreams in device memory, every call synchronous).  Cases:
  fixed          k = s % 12 for every frame: lc3plus_enc_batch_encode (the pipelined path);
  every_frame    k = (s + t) % 12, every stream changes rate every frame: lc3plus_enc_batch_encode_bitrates;
  runs_8_32      every stream keeps a rate for 8 to 32 frames (random, per stream), then draws another: encode_bitrates;
  workaround     the every-frame case as it had to be done before: lc3plus_enc_batch_set_bitrate for every stream, then a one-frame
                 encode() call, per frame (timed over --work-frames frames and scaled to the call's 64).
Wall time per call over --calls calls after --warmup.  Prints one JSON line.
    python tools/enc_varrate_rate.py [--calls 10] [--warmup 3] [--work-frames 4]"""
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
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--work-frames", type=int, default=4)
    a = ap.parse_args()
    pcm = np.ascontiguousarray(np.tile(synth_pcm(U, T, 480, FS, seed=9), (B // U, 1, 1)))
    s_idx = np.arange(B)[:, None]; t_idx = np.arange(T)[None, :]
    rng = np.random.default_rng(3)
    runs = np.zeros((B, T), np.int64)
    for s in range(B):
        t = 0
        while t < T:
            n = int(rng.integers(8, 33)); runs[s, t:t + n] = rng.integers(12); t += n
    R = np.array(RATES12, np.int32)
    cases = {"fixed": R[(s_idx + 0 * t_idx) % 12], "every_frame": R[(s_idx + t_idx) % 12], "runs_8_32": R[runs]}
    stride = 400
    hip = C.CDLL("libamdhip64.so")
    ptrs = []

    def alloc(n):
        p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0; ptrs.append(p); return p.value
    d_pcm = alloc(pcm.nbytes)
    assert hip.hipMemcpy(C.c_void_p(d_pcm), C.c_void_p(pcm.ctypes.data), C.c_size_t(pcm.nbytes), C.c_int(1)) == 0
    d_out = alloc(B * T * stride)
    out = {"tool": "enc_varrate_rate", "streams": B, "frames": T, "rates": RATES12}
    try:
        for mode, br in cases.items():
            enc = amd.Batch(B, FS, 1, MS, 0, br[:, 0].tolist(), device=0)

            def call():
                if mode == "fixed":
                    enc.encode_device(d_pcm, 16, T, d_out, stride, sync=True)
                else:
                    enc.encode_device(d_pcm, 16, T, d_out, stride, sync=True, bitrates=br)
            for _ in range(a.warmup):
                call()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call()
            ms = (time.perf_counter() - t0) * 1e3 / a.calls
            out[mode] = {"ms_per_call": round(ms, 3), "Mframes_per_s": round(B * T / ms / 1e3, 2), "kernel_ms_last_call": round(enc.last_kernel_ms(), 3),
                         "rate_changes_per_stream": round(float((np.diff(br, axis=1) != 0).sum(axis=1).mean()), 2)}
            enc.close()
        # the workaround: per frame, set_bitrate on every stream, then a one-frame call (PCM: frame 0 of each stream's block, same work)
        br = cases["every_frame"]
        enc = amd.Batch(B, FS, 1, MS, 0, br[:, 0].tolist(), device=0)
        d_pcm1 = alloc(B * 480 * 2)
        p1 = np.ascontiguousarray(pcm[:, 0])
        assert hip.hipMemcpy(C.c_void_p(d_pcm1), C.c_void_p(p1.ctypes.data), C.c_size_t(p1.nbytes), C.c_int(1)) == 0

        def frame(t):
            for s in range(B):
                assert enc.set_bitrate(s, int(br[s, t])) == 0
            enc.encode_device(d_pcm1, 16, 1, d_out, stride, sync=True)
        frame(0)
        t0 = time.perf_counter()
        for t in range(1, 1 + a.work_frames):
            frame(t)
        ms = (time.perf_counter() - t0) * 1e3 / a.work_frames * T
        out["workaround"] = {"ms_per_call": round(ms, 3), "Mframes_per_s": round(B * T / ms / 1e3, 3), "frames_timed": a.work_frames}
        enc.close()
        out["every_frame_vs_workaround"] = round(out["every_frame"]["Mframes_per_s"] / out["workaround"]["Mframes_per_s"], 2)
        out["runs_8_32_vs_fixed"] = round(out["runs_8_32"]["Mframes_per_s"] / out["fixed"]["Mframes_per_s"], 4)
        out["every_frame_vs_fixed"] = round(out["every_frame"]["Mframes_per_s"] / out["fixed"]["Mframes_per_s"], 4)
    finally:
        for p in ptrs:
            hip.hipFree(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
