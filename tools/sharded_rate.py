"""Frames per second of a sharded batch (lc3plus_enc_sharded_*, one host thread per shard) against one unsharded batch of the same streams, c1's shape:
4096 streams x 64 frames per call, 48 kHz / 10 ms / 64 kbps mono.  Four cases - host pointers and device pointers, each unsharded (all streams on the first
device of the list) and sharded over --devices - each in a child process of its own under its own time limit; a child that fails or runs out of time stops the
script with a non-zero exit.  Every call waits for its result (the host-pointer calls always do; the device-pointer calls are made with sync = 1), so the wall
time per call is the whole call.  Prints the device list first, then per case the wall time per call, frames per second and the kernel time of the last call
of every shard (HIP events on each shard's stream).  With the default --devices 0,0 both shards share one device: that run says what two contexts and two
host threads cost or give on one GPU, and nothing about scaling over GPUs.
    python tools/sharded_rate.py [--devices 0,0] [--calls 10] [--warmup 3] [--limit 300] [--out profiles/sharded_rate.txt]"""
import argparse, ctypes as C, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, U, FS, MS, RATE, N, STRIDE = 4096, 64, 64, 48000, 10.0, 64000, 480, 80
CASES = ["host_unsharded", "host_sharded", "device_unsharded", "device_sharded"]


def child(case, devices, calls, warmup):
    import audio_codec_amd as amd
    from tests.lc3_harness import synth_pcm
    pcm = np.ascontiguousarray(np.tile(synth_pcm(U, T, N, FS, seed=9), (B // U, 1, 1)))                 # [B, T, N] int16
    out = np.zeros((B, T, STRIDE), np.uint8)
    hip = C.CDLL("libamdhip64.so")
    ptrs = []

    def put(x, device):
        p = C.c_void_p()
        assert hip.hipSetDevice(device) == 0 and hip.hipMalloc(C.byref(p), C.c_size_t(x.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0
        ptrs.append((device, p)); return p.value
    sharded = case.endswith("_sharded")
    if sharded:
        b = amd.ShardedBatch(B, FS, 1, MS, 0, [RATE] * B, devices)
        blocks, devs = b.blocks, b.devices
    else:
        b = amd.Batch(B, FS, 1, MS, 0, [RATE] * B, device=devices[0])
        blocks, devs = [(0, B)], [devices[0]]
    if case.startswith("device"):
        d_pcm = [put(pcm[f:f + c], d) for (f, c), d in zip(blocks, devs)]
        d_out = [put(out[f:f + c], d) for (f, c), d in zip(blocks, devs)]
        call = (lambda: b.encode_device(d_pcm, 16, T, d_out, STRIDE, sync=True)) if sharded else (lambda: b.encode_device(d_pcm[0], 16, T, d_out[0], STRIDE, sync=True))
    elif sharded:
        def call():
            rc = b.lib.lc3plus_enc_sharded_encode(b.h, pcm.ctypes.data, 16, None, None, T, out.ctypes.data, STRIDE, None)
            assert rc == 0, rc
    else:
        call = lambda: b.encode_host(pcm, out)
    for _ in range(warmup):
        call()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    wall = (time.perf_counter() - t0) / calls
    ms = [b.last_kernel_ms(i) for i in range(len(blocks))] if sharded else [b.last_kernel_ms()]
    b.close()
    for d, p in ptrs:
        hip.hipSetDevice(d); hip.hipFree(p)
    print(json.dumps({"case": case, "shards": len(blocks), "streams_per_shard": [c for _, c in blocks], "wall_ms_per_call": round(wall * 1e3, 3),
                      "Mframes_per_s": round(B * T / wall / 1e6, 3), "last_kernel_ms_per_shard": [round(x, 3) for x in ms]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--devices", default="0,0")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds per case")
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    devices = [int(x) for x in a.devices.split(",")]
    if a.case:
        return child(a.case, devices, a.calls, a.warmup)
    lines = ["devices %s  (%d streams x %d frames per call, %d Hz / %.0f ms / %d bps, %d calls after %d)" % (a.devices, B, T, FS, MS, RATE, a.calls, a.warmup)]
    print(lines[0], flush=True)
    for case in CASES:                                               # one step at a time; the first that fails ends the script
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--devices", a.devices, "--calls", str(a.calls), "--warmup",
                                str(a.warmup)], capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s; stopping" % (case, a.limit), flush=True)
            return 124
        if r.returncode != 0:
            print("%s: exit %d; stopping\n%s" % (case, r.returncode, r.stderr[-2000:]), flush=True)
            return r.returncode if r.returncode > 0 else 1
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
