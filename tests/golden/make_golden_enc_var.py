"""Generates tests/golden/e2_variable_bitrates.npz from the UNMODIFIED ETSI reference (oracle/_ref/liblc3_etsi_fl.so, built by oracle/Makefile).
Run in the build container only:  python tests/golden/make_golden_enc_var.py
Per operating point: B streams of test PCM, a bitrate per stream-frame that changes every one to three frames, and the frames the reference
ENCODER made with lc3_enc_set_bitrate before every frame (as R/codec_exe.c:296-302 does with a switching file): bytes and sizes.  Data only,
no reference code."""
import ctypes as C
import os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from lc3_harness import Ref, synth_pcm

CFGS = [  # tag, fs, frame_ms, hrmode, channels, bitrates the streams switch between (48 kHz / 10 ms: LPC weighting, LTPF and attack thresholds)
    ("fb48k_10", 48000, 10.0, 0, 1, [40000, 47200, 48000, 64000, 79200, 80000, 95200, 96000, 128000, 271200, 272000, 320000]),
    ("fb48k_5", 48000, 5.0, 0, 1, [32000, 47200, 48000, 64000, 110400, 112000, 256000, 640000]),
    ("fb48k_2p5", 48000, 2.5, 0, 1, [64000, 76800, 128000, 256000, 320000, 1280000]),
    ("cd44k_10", 44100, 10.0, 0, 1, [14700, 44100, 64000, 73400, 73500, 128000, 249800, 249900, 294000]),
    ("swb32k_10", 32000, 10.0, 0, 1, [16000, 38400, 64000, 64800, 96000, 271200, 272000, 320000]),
    ("wb16k_10", 16000, 10.0, 0, 1, [16000, 24000, 32000, 64000, 128000, 320000]),
    ("nb8k_10", 8000, 10.0, 0, 1, [16000, 24000, 32000, 64000, 320000]),
    # even stream-frame sizes only: the reference's lc3_enc_fl asserts that a frame has channels x the first channel's bytes (R/lc3.c:124-129, 232),
    # which an odd size does not (the CPU oracle covers odd splits)
    ("fb48k_10_stereo", 48000, 10.0, 0, 2, [80000, 96000, 128000, 160000, 200000, 232000, 544000, 640000]),
    ("hr48k_10", 48000, 10.0, 1, 1, [124800, 160000, 256000, 400000, 500000]),
    ("hr96k_2p5", 96000, 2.5, 1, 1, [198400, 256000, 400000, 672000]),
    ("hr96k_10", 96000, 10.0, 1, 1, [149600, 256000, 400000, 500000]),
]
B, T = 3, 30


def case(i, fs, ms, hr, ch, rates):
    rng = np.random.default_rng(500 + i)
    N = int((48000 if fs == 44100 else fs) * ms / 1000)
    pcm = synth_pcm(B * ch, T, N, fs, seed=500 + i).reshape(B, ch, T, N).transpose(0, 2, 1, 3).copy()
    br = np.zeros((B, T), np.int32)
    for b in range(B):
        t = 0
        while t < T:
            n = int(rng.integers(1, 4))
            br[b, t:t + n] = int(rates[rng.integers(len(rates))])
            t += n
    sizes = np.zeros((B, T), np.int32)
    frames = np.zeros((B, T, 1300), np.uint8)
    for b in range(B):
        e = Ref(fs, ch, ms, hr, int(br[b, 0]))
        for t in range(T):
            assert e.set_bitrate(int(br[b, t])) == 0
            planar = np.ascontiguousarray(pcm[b, t])
            ptrs = (C.c_void_p * ch)(*[planar[c].ctypes.data for c in range(ch)])
            buf = np.zeros(1300, np.uint8)
            nb = C.c_int(0)
            assert e.lib.lc3_enc_fl(e.p, ptrs, 16, buf.ctypes.data, C.byref(nb)) == 0
            sizes[b, t] = nb.value
            frames[b, t] = buf
    mx = int(sizes.max())
    return pcm, br, frames[:, :, :mx].copy(), sizes


def main():
    out = {}
    for i, (tag, fs, ms, hr, ch, rates) in enumerate(CFGS):
        pcm, br, frames, sizes = case(i, fs, ms, hr, ch, rates)
        out[tag + "/cfg"] = np.array([fs, ms, hr, ch], np.float64)
        out[tag + "/pcm"], out[tag + "/bitrates"], out[tag + "/frames"], out[tag + "/sizes"] = pcm, br, frames, sizes
        print(tag, "frames", sizes.size, "bytes", int(sizes.sum()))
    np.savez_compressed(os.path.join(HERE, "e2_variable_bitrates.npz"), **out)


if __name__ == "__main__":
    main()
