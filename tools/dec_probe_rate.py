"""Frame probe rate (lc3plus_dec_batch_probe) beside the decode call of the same frames: 4096 mono streams x 64 frames, 48 kHz / 10 ms, everything in device
memory, one batch, one process.  Three frame sizes: 80 bytes (the shape of bench.py's d1), 20 bytes and 400 bytes (above 128 bytes the FULL probe and the
parser read their frames from global memory).  The frames are the encoder's own, packed back to back.  Variants, alternated call by call:
  dec, dec2   lc3plus_dec_batch_decode_packed, twice: the difference between the two is the spread a variant has to exceed to mean anything
  side        the probe at LC3PLUS_PROBE_SIDE over the same n_streams x n_frames items
  full        the probe at LC3PLUS_PROBE_FULL
Device events around every call on the call's stream (sync = 0); per variant the median, the fastest and the slowest of --calls calls after --warmup rounds
and items per second.  Before timing, the FULL records are checked: every frame accepted, byte count and global gain as lc3plus_frame_info_side gives them.
Writes one JSON object to --out and prints it.
    python tools/dec_probe_rate.py [--calls 60] [--warmup 5] [--out profiles/dec_probe_rate.json] [--streams 4096]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from audio_codec_amd import api
from tests.lc3_harness import synth_pcm

T, U, FS, MS = 64, 64, 48000, 10.0
SIZES = (80, 20, 400)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dec_probe_rate.json"))
    a = ap.parse_args()
    B = a.streams
    assert B % U == 0
    hip = C.CDLL("libamdhip64.so")
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    out = {"tool": "dec_probe_rate", "streams": B, "frames": T, "calls": a.calls, "warmup": a.warmup, "runs": []}
    for NB in SIZES:
        ptrs = []

        def put(x):
            x = np.ascontiguousarray(x); p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(x.nbytes)) == 0
            assert hip.hipMemcpy(p, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
            ptrs.append(p); return p.value
        e = amd.Batch(U, FS, 1, MS, 0, [NB * 800] * U, device=0)
        frames = np.ascontiguousarray(np.tile(e.encode(synth_pcm(U, T, 480, FS, seed=9))[:, :, :NB], (B // U, 1, 1)))
        e.close()
        n = B * T
        d_in, d_nb = put(frames), put(np.full(n, NB, np.int32))
        d_off = put(np.arange(n, dtype=np.int64) * NB)
        d_pcm, d_st, d_info = put(np.zeros(n * 480, np.int16)), put(np.zeros(n, np.uint8)), put(np.zeros((n, api.FRAME_INFO_WORDS), np.int32))
        dec = amd.DecBatch(B, FS, 1, MS, 0, None, device=0)
        calls = {
            "dec": lambda: dec.decode_device_packed(d_in, frames.size, d_off, T, d_pcm, d_nb, NB, None, d_st, hip_stream=stream.value, sync=False),
            "side": lambda: dec.probe_device(d_in, frames.size, d_off, d_nb, NB, n, d_info, api.PROBE_SIDE, stream.value, False),
            "full": lambda: dec.probe_device(d_in, frames.size, d_off, d_nb, NB, n, d_info, api.PROBE_FULL, stream.value, False),
        }
        calls["dec2"] = calls["dec"]
        times = {k: [] for k in ("dec", "dec2", "side", "full")}
        try:
            calls["full"]()
            assert hip.hipStreamSynchronize(stream) == 0
            info = np.zeros((n, api.FRAME_INFO_WORDS), np.int32)
            assert hip.hipMemcpy(C.c_void_p(info.ctypes.data), C.c_void_p(d_info), C.c_size_t(info.nbytes), C.c_int(2)) == 0
            assert not info[:, api.FI_STATUS].any() and (info[:, api.FI_NUM_BYTES] == NB).all()
            for i in range(0, U * T, 97):
                assert info[i, api.FI_GG_IDX] == api.frame_info_side(FS, 1, MS, 0, frames.reshape(n, NB)[i])[0, api.FI_GG_IDX]
            for rnd in range(a.warmup + a.calls):
                for k in times:
                    assert hip.hipEventRecord(ev0, stream) == 0
                    calls[k]()
                    assert hip.hipEventRecord(ev1, stream) == 0 and hip.hipEventSynchronize(ev1) == 0
                    ms = C.c_float(0); assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
                    if rnd >= a.warmup:
                        times[k].append(ms.value)
        finally:
            dec.close()
            for p in ptrs:
                hip.hipFree(p)
        run = {"frame_bytes": NB, "items": n, "variants": {}}
        for k, v in times.items():
            med = float(np.median(v))
            run["variants"][k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "Mitems_per_s": round(n / med / 1e3, 2)}
        va = run["variants"]
        run["spread_dec2_over_dec"] = round(va["dec2"]["ms_median"] / va["dec"]["ms_median"], 4)
        run["side_over_dec"] = round(va["side"]["ms_median"] / va["dec"]["ms_median"], 4)
        run["full_over_dec"] = round(va["full"]["ms_median"] / va["dec"]["ms_median"], 4)
        out["runs"].append(run)
    hip.hipEventDestroy(ev0); hip.hipEventDestroy(ev1); hip.hipStreamDestroy(stream)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
