"""Generates tests/golden/d2_variable_frame_sizes.npz from the UNMODIFIED ETSI reference (oracle/_ref/liblc3_etsi_fl.so, built by
oracle/Makefile).  Run in the build container only:  python tests/golden/make_golden_dec_var.py
Per operating point: streams the reference ENCODER made with its bitrate changed every one to three frames (lc3_enc_set_bitrate between
frames, as a bitrate switching file does), damaged on purpose - frames given as lost by size 0 or by bfi, flipped bytes in good frames - and
what the reference DECODER made of them, one lc3_dec_fl call per frame with the frame's own size: 16-bit PCM and the LC3_DECODE_ERROR status.
The first two frames of every stream are lost (the decoder has no size yet).  Data only, no reference code."""
import os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from lc3_harness import Ref, RefDecoder, synth_pcm

CFGS = [  # tag, fs, frame_ms, hrmode, channels, bitrates the streams switch between
    ("fb48k_10", 48000, 10.0, 0, 1, [56000, 64000, 72000, 80000, 88000, 96000, 102400, 160000]),   # LTPF thresholds, the 128-byte staging limit
    ("fb48k_10_small", 48000, 10.0, 0, 1, [56000, 64000, 72000, 80000, 88000, 96000]),            # every frame staged in LDS
    ("fb48k_10_stereo", 48000, 10.0, 0, 2, [128000, 128800, 160800, 176000, 204800, 232800]),      # odd stream sizes: 161, 201, 291 bytes
    ("fb48k_5", 48000, 5.0, 0, 1, [32000, 64000, 128000, 256000]), ("fb48k_2p5", 48000, 2.5, 0, 1, [64000, 96000, 128000, 320000]),
    ("swb32k_5", 32000, 5.0, 0, 1, [32000, 64000, 96000, 192000]), ("wb16k_10", 16000, 10.0, 0, 1, [16000, 32000, 64000, 128000]),
    ("nb8k_2p5", 8000, 2.5, 0, 1, [64000, 96000, 128000, 160000]),
    ("hr48k_10", 48000, 10.0, 1, 1, [128000, 256000, 400000, 500000]), ("hr96k_2p5", 96000, 2.5, 1, 1, [198400, 256000, 320000, 672000]),
    ("hr96k_10", 96000, 10.0, 1, 1, [149600, 256000, 400000, 500000]),
]
B, T = 4, 24


def case(i, fs, ms, hr, ch, rates):
    rng = np.random.default_rng(300 + i)
    N = int(fs * ms / 1000)
    pcm = synth_pcm(B * ch, T, N, fs, seed=300 + i).reshape(B, ch, T, N).transpose(0, 2, 1, 3)
    per, sizes = [], np.zeros((B, T), np.int32)
    for b in range(B):
        # one mono encoder per channel: a stereo encoder splits its bitrate evenly, the decoder's split of an odd size gives the first channel a byte more
        enc = [Ref(fs, 1, ms, hr, 64000 if hr == 0 else 256000) for _ in range(ch)]
        row, left = [], 0
        for t in range(T):
            if left == 0:
                n = int(rates[rng.integers(len(rates))]) * int(ms * 10) // 80000       # bytes of the stream-frame
                for c, e in enumerate(enc):
                    assert e.set_bitrate((n // ch + (c < n % ch)) * 80000 // int(ms * 10)) == 0
                    e.nbytes = e.lib.lc3_enc_get_num_bytes(e.p)
                left = int(rng.integers(1, 4))
            left -= 1
            row.append(np.concatenate([e.encode(pcm[b, t, c][None]) for c, e in enumerate(enc)]))
            sizes[b, t] = row[-1].size
        per.append(row)
    frames = np.zeros((B, T, sizes.max()), np.uint8)
    for b in range(B):
        for t in range(T):
            frames[b, t, :sizes[b, t]] = per[b][t]
    num_bytes = sizes.copy(); bfi = np.zeros((B, T), np.uint8)
    u = rng.random((B, T))
    num_bytes[u < 0.1] = 0; bfi[(u >= 0.1) & (u < 0.2)] = 1; num_bytes[:, :2] = 0
    for b in range(B):
        last = 0
        for t in range(T):
            good = num_bytes[b, t] and not bfi[b, t]
            # stereo: no damage where the size changes (an earlier corrupt channel makes the reference skip the later channel's size update)
            if good and rng.random() < 0.1 and (ch == 1 or num_bytes[b, t] == last):
                k = rng.integers(0, num_bytes[b, t], size=3)
                frames[b, t, k] ^= rng.integers(1, 256, size=3).astype(np.uint8)
            if good:
                last = num_bytes[b, t]
    return frames, num_bytes, bfi


def main():
    out = {}
    for i, (tag, fs, ms, hr, ch, rates) in enumerate(CFGS):
        frames, num_bytes, bfi = case(i, fs, ms, hr, ch, rates)
        pcm = np.zeros((B, T, ch, int(fs * ms / 1000)), np.int16); status = np.zeros((B, T), np.uint8)
        for b in range(B):
            d = RefDecoder(fs, ch, ms, hr)
            for t in range(T):
                nb = int(num_bytes[b, t])
                rc, x = d.decode(frames[b, t, :nb], int(bfi[b, t]), 16)
                assert rc in (0, 2), (tag, b, t, rc)
                pcm[b, t] = x; status[b, t] = rc == 2
        out[tag + "_cfg"] = np.array([fs, int(ms * 10), hr, ch]); out[tag + "_frames"] = frames; out[tag + "_num_bytes"] = num_bytes
        out[tag + "_bfi"] = bfi; out[tag + "_pcm"] = pcm; out[tag + "_status"] = status
        print(tag, frames.shape, "sizes", sorted(set(num_bytes[num_bytes > 0].tolist())), "concealed", int(status.sum()))
    np.savez_compressed(os.path.join(HERE, "d2_variable_frame_sizes.npz"), tags=np.array([c[0] for c in CFGS]), **out)


if __name__ == "__main__":
    main()
