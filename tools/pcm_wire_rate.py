"""The wire sample types of the batch calls (include/lc3plus_batch.h: LC3PLUS_PCM_S16_BE, _S24_3LE, _S24_3BE, _ULAW, _ALAW) against int16 and float32,
c1's shape: 4096 streams x 64 frames per call, 48 kHz / 10 ms / 64 kbps, everything in device memory, the input-ready promise given, calls with sync = 0
and one device synchronisation at the end.
Cases:
  enc_mono      int16, float32 and each wire type in the default layout;
  dec_mono      the encoder's frames decoded to int16, float32 and each wire type;
  enc_stereo    2048 stereo streams at 128 kbps: int16 default, int16 interleaved and S16_BE interleaved.
The cases of a group run alternately inside this one process, --rounds rounds (at least three): the median and the spread (min ... max) of each, the ratio
of the medians to the group's first case, and for the wire types of the mono groups the verdict against the yardstick: float32 (an existing wide loader
that moves more bytes) minus the int16 case's own spread (max - min) / median.  Wall time per call over --calls calls after --warmup.  Prints one JSON line.
    python tools/pcm_wire_rate.py [--rounds 3] [--calls 10] [--warmup 3]"""
import argparse, ctypes as C, json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as amd
from audio_codec_amd import api
from tests.lc3_harness import synth_pcm

B, T, U, FS, MS, RATE, N = 4096, 64, 64, 48000, 10.0, 64000, 480
WIRE = [("s16be", api.PCM_S16_BE), ("s24_3le", api.PCM_S24_3LE), ("s24_3be", api.PCM_S24_3BE), ("ulaw", api.PCM_ULAW), ("alaw", api.PCM_ALAW)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    a.rounds = max(a.rounds, 3)
    mono = np.ascontiguousarray(np.tile(synth_pcm(U, T, N, FS, seed=9), (B // U, 1, 1)))[:, :, None, :]               # [B, T, 1, N] int16
    stereo = np.ascontiguousarray(mono.reshape(B // 2, 2, T, N).transpose(0, 2, 1, 3))                                  # [B / 2, T, 2, N]
    f32 = lambda x: (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    inter = lambda x: np.ascontiguousarray(x.transpose(0, 1, 3, 2))                                                   # [S, T, N, C] = [S][time][channel]
    wire = lambda ty, x: api.pcm_from_native(ty, x.astype(np.int32) << 8 if ty in (api.PCM_S24_3LE, api.PCM_S24_3BE) else x)
    hip = C.CDLL("libamdhip64.so")
    ptrs = []

    def alloc(n):
        p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0; ptrs.append(p); return p.value

    def put(x):
        p = alloc(x.nbytes)
        assert hip.hipMemcpy(C.c_void_p(p), C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
        return p
    out = {"tool": "pcm_wire_rate", "streams": B, "frames": T, "samplerate": FS, "frame_ms": MS, "bitrate": RATE, "rounds": a.rounds, "calls": a.calls}

    def timed(call):
        for _ in range(a.warmup):
            call()
        assert hip.hipDeviceSynchronize() == 0
        t0 = time.perf_counter()
        for _ in range(a.calls):
            call()
        assert hip.hipDeviceSynchronize() == 0
        return B * T / ((time.perf_counter() - t0) * 1e3 / a.calls) / 1e3                                              # Mframes/s (channel-frames)

    def group(name, cases, yardstick=None):
        """cases: (key, make, call, close): alternately, a fresh batch per case and round"""
        runs = {k: [] for k, _, _, _ in cases}
        for _ in range(a.rounds):
            for key, make, call, close in cases:
                obj = make()
                runs[key].append(timed(lambda: call(obj)))
                close(obj)
        res = {k: {"median_Mframes_per_s": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in runs.items()}
        first = cases[0][0]
        med = {k: statistics.median(v) for k, v in runs.items()}
        for k in runs:
            if k != first:
                res[k]["vs_" + first] = round(med[k] / med[first], 4)
        if yardstick:
            spread = (max(runs[first]) - min(runs[first])) / med[first]
            floor = med[yardstick] * (1.0 - spread)
            res["yardstick"] = {"case": yardstick, "spread_of_" + first: round(spread, 4), "floor_Mframes_per_s": round(floor, 2)}
            for k in runs:
                if k not in (first, yardstick):
                    res[k]["at_or_above_floor"] = bool(med[k] >= floor)
        out[name] = res

    def enc(S, ch, rate):
        def make():
            b = amd.Batch(S, FS, ch, MS, 0, [rate] * S, device=0)
            b.set_input_ready(True)
            return b
        return make
    try:
        stride = 80
        d_out = alloc(B * T * 2 * stride)
        d_i16, d_f32 = put(mono), put(f32(mono))
        d_wire = {key: put(wire(ty, mono)) for key, ty in WIRE}
        one = lambda ptr, word: (lambda b: b.encode_device(ptr, word, T, d_out, stride, sync=False))
        group("enc_mono", [("int16", enc(B, 1, RATE), one(d_i16, 16), lambda b: b.close()),
                           ("float32", enc(B, 1, RATE), one(d_f32, api.PCM_FLOAT32), lambda b: b.close())] +
                          [(key, enc(B, 1, RATE), one(d_wire[key], ty), lambda b: b.close()) for key, ty in WIRE], yardstick="float32")
        b = amd.Batch(B, FS, 1, MS, 0, [RATE] * B, device=0)
        b.encode_device(d_i16, 16, T, d_out, stride, sync=True)                                                       # the decoder's input
        b.close()
        d_pcm = alloc(B * T * N * 4)

        def dec():
            d = amd.DecBatch(B, FS, 1, MS, 0, [stride] * B, device=0)
            d.set_input_ready(True)
            return d
        to = lambda word: (lambda d: d.decode_device(d_out, stride, T, d_pcm, bps=word, sync=False))
        group("dec_mono", [("int16", dec, to(16), lambda d: d.close()), ("float32", dec, to(api.PCM_FLOAT32), lambda d: d.close())] +
                          [(key, dec, to(ty), lambda d: d.close()) for key, ty in WIRE], yardstick="float32")
        S2 = B // 2
        IL = api.PCM_INTERLEAVED
        d_s16, d_s16i, d_sbei = put(stereo), put(inter(stereo)), put(wire(api.PCM_S16_BE, inter(stereo)))
        two = lambda ptr, word: (lambda b: b.encode_device(ptr, word, T, d_out, 2 * stride, sync=False))
        group("enc_stereo", [
            ("int16", enc(S2, 2, 2 * RATE), two(d_s16, 16), lambda b: b.close()),
            ("int16_interleaved", enc(S2, 2, 2 * RATE), two(d_s16i, 16 | IL), lambda b: b.close()),
            ("s16be_interleaved", enc(S2, 2, 2 * RATE), two(d_sbei, api.PCM_S16_BE | IL), lambda b: b.close()),
        ])
        out["enc_stereo"]["s16be_interleaved"]["vs_int16_interleaved"] = round(
            out["enc_stereo"]["s16be_interleaved"]["median_Mframes_per_s"] / out["enc_stereo"]["int16_interleaved"]["median_Mframes_per_s"], 4)
    finally:
        for p in ptrs:
            hip.hipFree(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
