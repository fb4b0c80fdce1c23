"""Placed PCM (include/lc3plus_batch.h: lc3plus_{enc,dec}_batch_set_pcm_placement) against the dense call, bench.py's c1: 4096 streams x 64 frames per call,
48 kHz / 10 ms / 64 kbps, int16, everything in device memory, the input-ready promise given, calls with sync = 0 and one device synchronisation at the end;
and the decoder on the same frames.
Variants, alternately inside one session on one card, --rounds rounds (at least three), median and spread (min ... max) of each:
  a  dense_parent   the dense call of another checkout of the project (--parent-root: the parent commit's tree with its library built), in a child process
                    of its own per round
  b  dense          the dense call of this build
  c  placed_dense   placed, the offsets those of the dense call
  d  placed_rings   placed, per-stream rings of R frames in one arena, every frame 16-byte aligned, the ring position advancing call by call
  e  placed_odd     the same rings with every base one element (2 bytes) further: no frame is 16-byte aligned
  f  gather_dense   for d, what the caller does without this feature: one gather (decoder: scatter) copy kernel over the rings - torch.index_select /
                    index_copy_ on the call's stream - around the dense call.  The input-ready promise cannot be given then (the PCM of a call is not
                    complete when the call is made: the gather in front of it is still queued), so the calls do not overlap
  g  gather_promise f with the promise given all the same - what the copy kernel alone costs; the encoder's result of such calls is not defined
Ratios: b / a with a's spread (max - min) / median as the margin, c / b, d / b, e / b and d / f.  Nothing is asserted: the numbers are recorded.
Wall time per call over --calls calls after --warmup.  Prints one JSON line (and writes it to --out).
    python tools/pcm_placed_rate.py [--parent-root PATH] [--rounds 3] [--calls 10] [--warmup 3] [--out profiles/pcm_placed_rate.json]"""
import argparse, json, os, statistics, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, T, U, FS, MS, RATE, N, STRIDE = 4096, 64, 64, 48000, 10.0, 64000, 480, 80
R = T + 16                                                              # ring length in frames: every other call wraps
NPLAN = 5                                                               # ring positions cycled through (T * NPLAN is a multiple of R)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root")
    ap.add_argument("--root", default=ROOT, help="the checkout whose audio_codec_amd is imported (the child process of variant a: --parent-root)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--dense-only", action="store_true", help="variant b alone, as {enc, dec} Mframes/s: what the child process of variant a runs")
    a = ap.parse_args()
    a.rounds = max(a.rounds, 3)
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import audio_codec_amd as amd
    from audio_codec_amd import api
    from tests.lc3_harness import synth_pcm
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)                                      # the calls' stream, and torch's for the copy kernels of variant f
    torch.cuda.set_stream(stream)
    s = stream.cuda_stream
    mono = np.ascontiguousarray(np.tile(synth_pcm(U, T, N, FS, seed=9), (B // U, 1, 1)))                                  # [B, T, N] int16
    d_dense = torch.from_numpy(mono).to(dev)
    d_out = torch.zeros(B * T * STRIDE, dtype=torch.uint8, device=dev)
    d_pcm = torch.zeros(B * T * N, dtype=torch.int16, device=dev)

    def timed(call):
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            call()
        torch.cuda.synchronize()
        return B * T / ((time.perf_counter() - t0) * 1e3 / a.calls) / 1e3                                              # Mframes/s

    def enc(ready=True):
        b = amd.Batch(B, FS, 1, MS, 0, [RATE] * B, device=0)
        b.set_input_ready(ready)
        return b

    def dec(ready=True):
        d = amd.DecBatch(B, FS, 1, MS, 0, [STRIDE] * B, device=0)
        d.set_input_ready(ready)
        return d

    def enc_dense(b):
        b.encode_device(d_dense.data_ptr(), 16, T, d_out.data_ptr(), STRIDE, hip_stream=s, sync=False)

    def dec_dense(d):
        d.decode_device(d_out.data_ptr(), STRIDE, T, d_pcm.data_ptr(), bps=16, hip_stream=s, sync=False)
    if a.dense_only:
        res = {}
        for key, make, call in (("enc", enc, enc_dense), ("dec", dec, dec_dense)):
            if key == "dec":                                             # the decoder's input: this build's (or the parent's: the same) frames
                b = enc(); b.encode_device(d_dense.data_ptr(), 16, T, d_out.data_ptr(), STRIDE, hip_stream=s, sync=True); b.close()
            obj = make()
            res[key] = timed(lambda: call(obj))
            obj.close()
        print(json.dumps(res))
        return

    # rings: stream r's ring is R slots of N elements from element r * ring_stride (+ 1 in the odd variant) on; call k starts at slot (k * T) % R
    ring_stride = R * N + 8                                              # 8 elements = 16 bytes: the aligned variant stays aligned
    cap = B * ring_stride + 8
    arenas = {name: torch.zeros(cap, dtype=torch.int16, device=dev) for name in ("rings", "odd")}
    plans = {}
    for name, shift in (("rings", 0), ("odd", 1)):
        plans[name] = [torch.from_numpy(api.ring_offsets(np.full(B, (k * T) % R), T, R, N, ring_stride) + shift).to(dev) for k in range(NPLAN)]
    d_offs_dense = torch.from_numpy((np.arange(B * T, dtype=np.int64) * N).reshape(B, T)).to(dev)
    # the caller-side alternative gathers whole slots: the aligned arena as rows of N elements needs ring_stride % N == 0, so it gets an arena of its own
    d_rows = torch.zeros((B * R, N), dtype=torch.int16, device=dev)
    slot = [torch.from_numpy((np.arange(B)[:, None] * R + ((k * T) % R + np.arange(T)[None, :]) % R).reshape(-1)).to(dev) for k in range(NPLAN)]
    d_gath = torch.zeros((B * T, N), dtype=torch.int16, device=dev)
    # fill the rings with the signal so that every variant encodes the same PCM
    for k in range(NPLAN):
        d_rows.index_copy_(0, slot[k], d_dense.reshape(B * T, N))
        for name in arenas:
            arenas[name].index_copy_(0, (plans[name][k].reshape(-1, 1) + torch.arange(N, device=dev)).reshape(-1), d_dense.reshape(-1))
    torch.cuda.synchronize()
    count = {"k": 0}

    def placed(obj, offs, pcm_ptr, capacity, is_enc):
        obj.set_pcm_placement(offs.data_ptr(), capacity)
        if is_enc:
            obj.encode_device(pcm_ptr, 16, T, d_out.data_ptr(), STRIDE, hip_stream=s, sync=False)
        else:
            obj.decode_device(d_out.data_ptr(), STRIDE, T, pcm_ptr, bps=16, hip_stream=s, sync=False)

    def ring_call(name, is_enc):
        def call(obj):
            count["k"] += 1
            placed(obj, plans[name][count["k"] % NPLAN], arenas[name].data_ptr(), cap, is_enc)
        return call

    def enc_gather(b):
        count["k"] += 1
        torch.index_select(d_rows, 0, slot[count["k"] % NPLAN], out=d_gath)
        b.encode_device(d_gath.data_ptr(), 16, T, d_out.data_ptr(), STRIDE, hip_stream=s, sync=False)

    def dec_scatter(d):
        count["k"] += 1
        d.decode_device(d_out.data_ptr(), STRIDE, T, d_gath.data_ptr(), bps=16, hip_stream=s, sync=False)
        d_rows.index_copy_(0, slot[count["k"] % NPLAN], d_gath)

    def parent(key):
        if not a.parent_root:
            return None
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--dense-only", "--root", os.path.abspath(a.parent_root), "--calls", str(a.calls),
                            "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        return json.loads(p.stdout.strip().splitlines()[-1])

    out = {"tool": "pcm_placed_rate", "streams": B, "frames": T, "samplerate": FS, "frame_ms": MS, "bitrate": RATE, "ring_frames": R, "rounds": a.rounds,
           "calls": a.calls, "unit": "Mframes/s"}
    runs = {"enc": {}, "dec": {}}
    for _ in range(a.rounds):
        pa = parent(None)
        if pa:
            for key in ("enc", "dec"):
                runs[key].setdefault("a_dense_parent", []).append(pa[key])
        b = enc(); b.encode_device(d_dense.data_ptr(), 16, T, d_out.data_ptr(), STRIDE, hip_stream=s, sync=True); b.close()   # the decoder's input
        frames = d_out.clone()
        cases = {"enc": [("b_dense", enc, enc_dense), ("c_placed_dense", enc, lambda o: placed(o, d_offs_dense, d_dense.data_ptr(), B * T * N, True)),
                         ("d_placed_rings", enc, ring_call("rings", True)), ("e_placed_odd", enc, ring_call("odd", True)),
                         ("f_gather_dense", lambda: enc(False), enc_gather), ("g_gather_promise", enc, enc_gather)],
                 "dec": [("b_dense", dec, dec_dense), ("c_placed_dense", dec, lambda o: placed(o, d_offs_dense, d_pcm.data_ptr(), B * T * N, False)),
                         ("d_placed_rings", dec, ring_call("rings", False)), ("e_placed_odd", dec, ring_call("odd", False)),
                         ("f_scatter_dense", dec, dec_scatter)]}      # (the decoder's promise covers its frames, not the PCM: the scatter behind it is in stream order)
        for key in ("enc", "dec"):
            for name, make, call in cases[key]:
                d_out.copy_(frames)
                obj = make()
                runs[key].setdefault(name, []).append(timed(lambda: call(obj)))
                obj.close()
    for key in ("enc", "dec"):
        res = {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in runs[key].items()}
        med = {k: statistics.median(v) for k, v in runs[key].items()}
        f = "f_gather_dense" if key == "enc" else "f_scatter_dense"
        ratios = {"c_over_b": med["c_placed_dense"] / med["b_dense"], "d_over_b": med["d_placed_rings"] / med["b_dense"], "e_over_b": med["e_placed_odd"] / med["b_dense"],
                  "d_over_f": med["d_placed_rings"] / med[f]}
        if "g_gather_promise" in med:
            ratios["d_over_g"] = med["d_placed_rings"] / med["g_gather_promise"]
        if "a_dense_parent" in med:
            va = runs[key]["a_dense_parent"]
            ratios["b_over_a"] = med["b_dense"] / med["a_dense_parent"]
            ratios["spread_of_a"] = (max(va) - min(va)) / med["a_dense_parent"]
        res["ratios"] = {k: round(v, 4) for k, v in ratios.items()}
        out[key] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
