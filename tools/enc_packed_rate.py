"""Packed frames (lc3plus_enc_batch_encode_packed, lc3plus_dec_batch_decode_packed) against the slotted calls for the same workload, c1's shape:
4096 streams x 64 frames per call, 48 kHz / 10 ms, everything in device memory, calls with sync = 0 and one device synchronisation at the end.  Cases:
  fixed        rates fixed per stream: encode_device (slots) against encode_device_packed without rates, under the input-ready promise;
  switching    bitrate (s + t) % 4 of RATES, every stream changing every frame: encode_device_rates (slots) against encode_device_packed with rates;
  decoder      the switching case's frames: decode_device_sizes on slots against decode_device_packed on the same frames back to back.
Wall time per call over --calls calls after --warmup.  Prints one JSON line.
    python tools/enc_packed_rate.py [--calls 10] [--warmup 3]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from tests.lc3_harness import synth_pcm

RATES = [48000, 64000, 80000, 96000]
B, T, U, FS, MS, RATE = 4096, 64, 64, 48000, 10.0, 64000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    pcm = np.ascontiguousarray(np.tile(synth_pcm(U, T, 480, FS, seed=9), (B // U, 1, 1)))
    s_idx = np.arange(B)[:, None]; t_idx = np.arange(T)[None, :]
    br = np.ascontiguousarray(np.array(RATES, np.int32)[(s_idx + t_idx) % 4])
    stride = 120
    hip = C.CDLL("libamdhip64.so")
    ptrs = []

    def alloc(n):
        p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0; ptrs.append(p); return p.value

    def put(x):
        p = alloc(x.nbytes)
        assert hip.hipMemcpy(C.c_void_p(p), C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
        return p
    d_pcm, d_br = put(pcm), put(br)
    cap = B * T * stride
    d_out, d_pk, d_nb, d_fl, d_off, d_tot = alloc(cap), alloc(cap), alloc(B * T * 4), alloc(B * T), alloc(B * T * 8), alloc(8)
    d_dpcm, d_st = alloc(B * T * 480 * 2), alloc(B * T)
    out = {"tool": "enc_packed_rate", "streams": B, "frames": T, "samplerate": FS, "frame_ms": MS, "bitrates": RATES, "fixed_bitrate": RATE}

    def timed(call):
        for _ in range(a.warmup):
            call()
        assert hip.hipDeviceSynchronize() == 0
        t0 = time.perf_counter()
        for _ in range(a.calls):
            call()
        assert hip.hipDeviceSynchronize() == 0
        ms = (time.perf_counter() - t0) * 1e3 / a.calls
        return {"ms_per_call": round(ms, 3), "Mframes_per_s": round(B * T / ms / 1e3, 2)}

    def ab(name, slotted, packed, ready=False):
        res = {}
        for key, fn in (("slotted", slotted), ("packed", packed), ("slotted_again", slotted), ("packed_again", packed)):
            bat = amd.Batch(B, FS, 1, MS, 0, [RATE] * B, device=0)
            bat.set_input_ready(ready)
            res[key] = timed(lambda: fn(bat))
            bat.close()
        res["packed_vs_slotted"] = round((res["packed"]["Mframes_per_s"] + res["packed_again"]["Mframes_per_s"])
                                         / (res["slotted"]["Mframes_per_s"] + res["slotted_again"]["Mframes_per_s"]), 4)
        out[name] = res
    try:
        ab("fixed", lambda b: b.encode_device(d_pcm, 16, T, d_out, 80, sync=False),
           lambda b: b.encode_device_packed(d_pcm, 16, T, d_pk, cap, 0, d_offsets_ptr=d_off, d_total_ptr=d_tot, d_num_bytes_ptr=d_nb), ready=True)
        ab("switching", lambda b: b.encode_device_rates(d_pcm, 16, T, d_out, stride, d_br, None, d_nb, d_fl),
           lambda b: b.encode_device_packed(d_pcm, 16, T, d_pk, cap, 0, d_br, None, d_off, d_tot, d_nb, d_fl))
        res = {}
        for key in ("slotted", "packed", "slotted_again", "packed_again"):
            dec = amd.DecBatch(B, FS, 1, MS, 0, [80] * B, device=0)
            if key.startswith("slotted"):
                res[key] = timed(lambda: dec.decode_device_sizes(d_out, stride, T, d_dpcm, d_nb, None, d_st))
            else:
                res[key] = timed(lambda: dec.decode_device_packed(d_pk, cap, d_off, T, d_dpcm, d_nb, stride, None, d_st))
            dec.close()
        res["packed_vs_slotted"] = round((res["packed"]["Mframes_per_s"] + res["packed_again"]["Mframes_per_s"])
                                         / (res["slotted"]["Mframes_per_s"] + res["slotted_again"]["Mframes_per_s"]), 4)
        out["decoder"] = res
    finally:
        for p in ptrs:
            hip.hipFree(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
