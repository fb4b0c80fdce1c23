"""Encoder rate with per-frame rates and bandwidths in device memory (lc3plus_enc_batch_encode_rates_device) against the same values from host arrays
(lc3plus_enc_batch_encode_bitrates / _encode_bandwidths), c1's shape: 4096 streams x 64 frames per call, 48 kHz / 10 ms, PCM and bitstreams in device
memory, every stream changing every frame.  Cases:
  rates        bitrate (s + t) % 4 of RATES: host arrays against device memory, synchronous calls, and calls with sync = 0 and one device
               synchronisation at the end;
  bandwidths   bandwidth (s + t) % 6 of BWS at 64 kbps, no rates: synchronous, and under the input-ready promise (sync = 0);
  host_us      host time of one sync = 0 device-memory call with rates (the call returns without waiting: what it costs the caller's thread).
Wall time per call over --calls calls after --warmup.  Prints one JSON line.
    python tools/enc_rates_device_rate.py [--calls 10] [--warmup 3]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from tests.lc3_harness import synth_pcm

RATES = [48000, 64000, 80000, 96000]
BWS = [0, 4000, 8000, 12000, 16000, 20000]
B, T, U, FS, MS, RATE = 4096, 64, 64, 48000, 10.0, 64000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    pcm = np.ascontiguousarray(np.tile(synth_pcm(U, T, 480, FS, seed=9), (B // U, 1, 1)))
    s_idx = np.arange(B)[:, None]; t_idx = np.arange(T)[None, :]
    br = np.ascontiguousarray(np.array(RATES, np.int32)[(s_idx + t_idx) % 4])
    bw = np.ascontiguousarray(np.array(BWS, np.int32)[(s_idx + t_idx) % 6])
    stride = 120
    hip = C.CDLL("libamdhip64.so")
    ptrs = []

    def alloc(n):
        p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0; ptrs.append(p); return p.value

    def put(x):
        p = alloc(x.nbytes)
        assert hip.hipMemcpy(C.c_void_p(p), C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
        return p
    d_pcm, d_br, d_bw = put(pcm), put(br), put(bw)
    d_out, d_nb, d_fl = alloc(B * T * stride), alloc(B * T * 4), alloc(B * T)
    out = {"tool": "enc_rates_device_rate", "streams": B, "frames": T, "samplerate": FS, "frame_ms": MS, "bitrates": RATES, "bandwidths": BWS,
           "bandwidth_bitrate": RATE}

    def timed(call, sync):
        for _ in range(a.warmup):
            call()
        assert hip.hipDeviceSynchronize() == 0
        t0 = time.perf_counter()
        for _ in range(a.calls):
            call()
        assert hip.hipDeviceSynchronize() == 0
        ms = (time.perf_counter() - t0) * 1e3 / a.calls
        return {"ms_per_call": round(ms, 3), "Mframes_per_s": round(B * T / ms / 1e3, 2)}
    try:
        res = {}
        for sync in (True, False):
            key = "sync" if sync else "sync0"
            enc = amd.Batch(B, FS, 1, MS, 0, [RATES[s % 4] for s in range(B)], device=0)
            res["host_arrays_" + key] = timed(lambda: enc.encode_device(d_pcm, 16, T, d_out, stride, sync=sync, bitrates=br), sync)
            enc.close()
            enc = amd.Batch(B, FS, 1, MS, 0, [RATES[s % 4] for s in range(B)], device=0)
            res["device_" + key] = timed(lambda: enc.encode_device_rates(d_pcm, 16, T, d_out, stride, d_br, None, d_nb, d_fl, sync=sync), sync)
            if not sync:                                                      # the host side of one call that does not wait
                assert hip.hipDeviceSynchronize() == 0
                hs = []
                for _ in range(a.calls):
                    t0 = time.perf_counter()
                    enc.encode_device_rates(d_pcm, 16, T, d_out, stride, d_br, None, d_nb, d_fl, sync=False)
                    hs.append((time.perf_counter() - t0) * 1e6)
                    assert hip.hipDeviceSynchronize() == 0
                out["host_us"] = round(float(np.median(hs)), 1)
            enc.close()
            res["device_vs_host_arrays_" + key] = round(res["device_" + key]["Mframes_per_s"] / res["host_arrays_" + key]["Mframes_per_s"], 4)
        out["rates"] = res
        res = {}
        for promise in (False, True):
            key = "promise" if promise else "sync"
            enc = amd.Batch(B, FS, 1, MS, 0, [RATE] * B, device=0)
            enc.set_input_ready(promise)
            res["host_arrays_" + key] = timed(lambda: enc.encode_device(d_pcm, 16, T, d_out, 80, sync=not promise, bandwidths=bw), not promise)
            enc.close()
            enc = amd.Batch(B, FS, 1, MS, 0, [RATE] * B, device=0)
            enc.set_input_ready(promise)
            res["device_" + key] = timed(lambda: enc.encode_device_rates(d_pcm, 16, T, d_out, 80, None, d_bw, d_nb, d_fl, sync=not promise), not promise)
            enc.close()
            res["device_vs_host_arrays_" + key] = round(res["device_" + key]["Mframes_per_s"] / res["host_arrays_" + key]["Mframes_per_s"], 4)
        out["bandwidths"] = res
    finally:
        for p in ptrs:
            hip.hipFree(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
