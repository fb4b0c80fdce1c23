"""Cost of the stream-lifecycle calls (lc3plus_{enc,dec}_batch_{reset,export,import}_streams) at c1 (encoder: 4096 mono streams, 48 kHz / 10 ms, 64 kbps)
and d1 (the decoder of those streams):
  1. device time (HIP events around the call on a stream of the tool's) of a reset, an export into device memory and an import from device memory of
     1, 64 and 4096 streams, and the bytes each moves (reset: the rows written; export / import: rows read + written) as a share of 8 TB/s;
  2. host time of a reset with sync = 0 (the call returns after queueing);
  3. c1 steady state under set_input_ready(1) with device pointers, calls of 64 frames back to back: Mframes/s without resets, and with a reset of 1 % of
     the streams (41) queued before every call - each such call runs ordered, without the overlap with the call before.
Prints one JSON line; --out writes it to a file as well.
    python tools/stream_state_rate.py [--reps 20] [--calls 30] [--out profiles/stream_state_rate.json]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from tests.lc3_harness import synth_pcm

B, T, FS, MS, PEAK = 4096, 64, 48000, 10.0, 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    hip = C.CDLL("libamdhip64.so")
    ptrs = []

    def zeros(n):
        p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0 and hip.hipMemset(p, 0, C.c_size_t(n)) == 0
        ptrs.append(p); return p.value

    def put(x):
        p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(x.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
        ptrs.append(p); return p.value

    s = C.c_void_p(); assert hip.hipStreamCreate(C.byref(s)) == 0
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    def device_ms(fn):
        """median over reps of the HIP-event time of fn() queued on s"""
        fn(); assert hip.hipStreamSynchronize(s) == 0
        t = []
        for _ in range(a.reps):
            assert hip.hipEventRecord(ev[0], s) == 0
            fn()
            assert hip.hipEventRecord(ev[1], s) == 0 and hip.hipEventSynchronize(ev[1]) == 0
            ms = C.c_float(); assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
            t.append(ms.value)
        return float(np.median(t))

    out = {"tool": "stream_state_rate", "streams": B, "peak_TBps": PEAK / 1e12, "reps": a.reps}
    pcm = np.tile(synth_pcm(64, T, 480, FS, seed=5), (B // 64, 1, 1))[:, :, None, :].copy()
    enc = amd.Batch(B, FS, 1, MS, 0, [64000] * B, device=0)
    frames = enc.encode(pcm[:, :8])
    dec = amd.DecBatch(B, FS, 1, MS, 0, [80] * B, device=0)
    dec.decode(frames)
    for tag, bt in (("c1_encoder", enc), ("d1_decoder", dec)):
        size = bt.stream_state_size
        rows = size - 16
        blob = zeros(B * size)
        st = zeros(B)
        res = {"blob_bytes": size}
        for n in (1, 64, 4096):
            lst = np.random.default_rng(n).permutation(B)[:n]
            bt.export_streams_device(lst, blob, hip_stream=s.value, sync=True)
            r = {}
            for op, fn, moved in (("reset", lambda: bt.reset_streams(lst, hip_stream=s.value, sync=False), n * rows),
                                  ("export_device", lambda: bt.export_streams_device(lst, blob, hip_stream=s.value), 2 * n * size),
                                  ("import_device", lambda: bt.import_streams_device(lst, blob, st, hip_stream=s.value), 2 * n * size)):
                ms = device_ms(fn)
                r[op] = {"device_ms": round(ms, 4), "bytes": moved, "share_of_peak": round(moved / (ms * 1e-3) / PEAK, 4)}
            assert hip.hipStreamSynchronize(s) == 0
            hl = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); bt.reset_streams(lst, hip_stream=s.value, sync=False); hl.append(time.perf_counter() - t0)
            assert hip.hipStreamSynchronize(s) == 0
            r["reset_host_us_sync0"] = round(float(np.median(hl)) * 1e6, 1)
            res["n%d" % n] = r
        out[tag] = res
    dec.close()
    # 3. c1 steady state under the input-ready promise
    d_pcm = put(pcm)
    stride = enc.stride
    d_out = [zeros(B * T * stride) for _ in range(3)]
    enc.set_input_ready(True)
    k = max(1, B // 100)
    rng = np.random.default_rng(7)
    lists = [rng.permutation(B)[:k] for _ in range(a.calls)]
    steady = {}
    for mode in ("no_reset", "reset_1pct"):
        for i in range(5):
            enc.encode_device(d_pcm, 16, T, d_out[i % 3], stride, sync=False)
        assert hip.hipDeviceSynchronize() == 0
        t0 = time.perf_counter()
        for i in range(a.calls):
            if mode == "reset_1pct":
                enc.reset_streams(lists[i], sync=False)
            enc.encode_device(d_pcm, 16, T, d_out[i % 3], stride, sync=False)
        assert hip.hipDeviceSynchronize() == 0
        sec = time.perf_counter() - t0
        steady[mode] = {"Mframes_s": round(B * T * a.calls / sec / 1e6, 2), "ms_per_call": round(sec / a.calls * 1e3, 3)}
    steady["reset_streams_per_call"] = k
    steady["ratio"] = round(steady["reset_1pct"]["Mframes_s"] / steady["no_reset"]["Mframes_s"], 3)
    out["c1_steady_input_ready"] = steady
    enc.close()
    for p in ptrs:
        hip.hipFree(p)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
