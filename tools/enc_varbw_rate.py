"""Encoder rate with per-frame bandwidths against bandwidths set per stream (c1's shape: 4096 streams x 64 frames per call, 48 kHz / 10 ms / 64 kbps,
PCM and bitstreams in device memory), each case once with synchronous calls and once under the input-ready promise (calls queued with sync = 0,
one device synchronisation at the end).  Bandwidths are drawn from 0 (off), 4, 8, 12, 16 and 20 kHz.  Cases:
  encode_fixed   stream s keeps bandwidth k = s % 6, set once with lc3plus_enc_batch_set_bandwidth: lc3plus_enc_batch_encode;
  constant       the same bandwidths given per frame: lc3plus_enc_batch_encode_bandwidths;
  every_frame    k = (s + t) % 6, every stream changes bandwidth every frame: encode_bandwidths;
  runs_8_32      every stream keeps a bandwidth for 8 to 32 frames (random, per stream), then draws another: encode_bandwidths;
  workaround     every_frame as it had to be done before: set_bandwidth for every stream that changes, then a call up to the next change - with
                 every stream changing every frame, a one-frame encode() per frame (timed over --work-frames frames, scaled to the call's 64).
Wall time per call over --calls calls after --warmup.  Prints one JSON line.
    python tools/enc_varbw_rate.py [--calls 10] [--warmup 3] [--work-frames 4]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from tests.lc3_harness import synth_pcm

BWS = [0, 4000, 8000, 12000, 16000, 20000]
B, T, U, FS, MS, RATE = 4096, 64, 64, 48000, 10.0, 64000


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
            n = int(rng.integers(8, 33)); runs[s, t:t + n] = rng.integers(len(BWS)); t += n
    W = np.array(BWS, np.int32)
    cases = {"encode_fixed": W[(s_idx + 0 * t_idx) % 6], "constant": W[(s_idx + 0 * t_idx) % 6], "every_frame": W[(s_idx + t_idx) % 6], "runs_8_32": W[runs]}
    stride = 80
    hip = C.CDLL("libamdhip64.so")
    ptrs = []

    def alloc(n):
        p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0; ptrs.append(p); return p.value
    d_pcm = alloc(pcm.nbytes)
    assert hip.hipMemcpy(C.c_void_p(d_pcm), C.c_void_p(pcm.ctypes.data), C.c_size_t(pcm.nbytes), C.c_int(1)) == 0
    d_out = alloc(B * T * stride)
    out = {"tool": "enc_varbw_rate", "streams": B, "frames": T, "samplerate": FS, "frame_ms": MS, "bitrate": RATE, "bandwidths": BWS}
    try:
        for promise in (False, True):
            res = {}
            for mode, bw in cases.items():
                enc = amd.Batch(B, FS, 1, MS, 0, [RATE] * B, device=0)
                for s in range(B):
                    assert enc.set_bandwidth(s, int(bw[s, 0])) == 0
                enc.set_input_ready(promise)

                def call():
                    if mode == "encode_fixed":
                        enc.encode_device(d_pcm, 16, T, d_out, stride, sync=not promise)
                    else:
                        enc.encode_device(d_pcm, 16, T, d_out, stride, sync=not promise, bandwidths=bw)
                for _ in range(a.warmup):
                    call()
                assert hip.hipDeviceSynchronize() == 0
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    call()
                assert hip.hipDeviceSynchronize() == 0
                ms = (time.perf_counter() - t0) * 1e3 / a.calls
                res[mode] = {"ms_per_call": round(ms, 3), "Mframes_per_s": round(B * T / ms / 1e3, 2),
                             "bandwidth_changes_per_stream": round(float((np.diff(bw, axis=1) != 0).sum(axis=1).mean()), 2)}
                enc.close()
            for mode in ("constant", "every_frame", "runs_8_32"):
                res[mode + "_vs_encode_fixed"] = round(res[mode]["Mframes_per_s"] / res["encode_fixed"]["Mframes_per_s"], 4)
            res["every_frame_vs_constant"] = round(res["every_frame"]["Mframes_per_s"] / res["constant"]["Mframes_per_s"], 4)
            out["promise" if promise else "sync"] = res
        # the workaround (synchronous): per frame, set_bandwidth on every stream, then a one-frame call (PCM: frame 0 of each stream's block, same work)
        bw = cases["every_frame"]
        enc = amd.Batch(B, FS, 1, MS, 0, [RATE] * B, device=0)
        d_pcm1 = alloc(B * 480 * 2)
        p1 = np.ascontiguousarray(pcm[:, 0])
        assert hip.hipMemcpy(C.c_void_p(d_pcm1), C.c_void_p(p1.ctypes.data), C.c_size_t(p1.nbytes), C.c_int(1)) == 0

        def frame(t):
            for s in range(B):
                assert enc.set_bandwidth(s, int(bw[s, t])) == 0
            enc.encode_device(d_pcm1, 16, 1, d_out, stride, sync=True)
        frame(0)
        t0 = time.perf_counter()
        for t in range(1, 1 + a.work_frames):
            frame(t)
        ms = (time.perf_counter() - t0) * 1e3 / a.work_frames * T
        out["workaround"] = {"ms_per_call": round(ms, 3), "Mframes_per_s": round(B * T / ms / 1e3, 3), "frames_timed": a.work_frames}
        enc.close()
        out["every_frame_vs_workaround"] = round(out["sync"]["every_frame"]["Mframes_per_s"] / out["workaround"]["Mframes_per_s"], 2)
    finally:
        for p in ptrs:
            hip.hipFree(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
