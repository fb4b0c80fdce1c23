#!/usr/bin/env python3
"""One call of every kind the host runtime (audio_codec_amd/csrc/lc3_runtime.hip) launches differently, on tiny batches in one process: the program to run
under a kernel trace when the runtime's launch code changes.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/launch_scenarios.py          (LC3PLUS_HIP_LIB selects another build of the library)
    python tools/launch_scenarios.py --compare OLD_kernel_trace.csv NEW_kernel_trace.csv

Two builds launch the same kernels when the sorted lists of (kernel name, grid, workgroup, LDS bytes) over the run are equal line for line; --compare
prints the two lengths, every line only one side has, and the verdict, and exits with status 1 on a difference.  (The trace reports a launch's whole LDS
block, static and dynamic; the static part belongs to the kernel, so with equal code objects equal blocks mean equal dynamic bytes.)  Needs a GPU to run,
none to compare.

Covered: encoder one-wave path (2 frames) and pipelined path (12 frames) at 48 kHz / 10 ms, 16 kHz / 10 ms and 96 kHz / 10 ms (large layout), host and device
pointers; the frontm frame lengths; int16, float32, a wire type and placed PCM; per-frame bitrates and bandwidths from the host and from device memory;
packed output; three calls in a row under the input-ready promise.  Decoder: fixed sizes, host sizes, device sizes, packed and ragged, with and without
placement and the promise.  2 streams, 3 where a kernel pairs streams.  Reads nothing but the library."""
import argparse
import csv
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Dev:
    """device buffers through hipMalloc / hipMemcpy"""
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so"); self.ptrs = []
    def put(self, arr):
        arr = np.ascontiguousarray(arr); p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(max(arr.nbytes, 1))) == 0
        assert self.hip.hipMemcpy(p, C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), C.c_int(1)) == 0
        self.ptrs.append(p); return p.value
    def get(self, ptr, shape, dtype):
        out = np.zeros(shape, dtype)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), C.c_int(2)) == 0
        return out
    def sync(self):
        assert self.hip.hipDeviceSynchronize() == 0
    def free(self):
        self.sync()
        for p in self.ptrs: self.hip.hipFree(p)
        self.ptrs = []


def noise(S, T, ch, N, seed):
    return np.random.default_rng(seed).integers(-8000, 8000, size=(S, T, ch, N)).astype(np.int16)


def encoder(dev, amd, fs, ms, hr, rate, S, extras):
    """host and device pointers, 2 and 12 frames; with extras the formats, per-frame words, packed output and the promise too ("nobw": all but the bandwidths)"""
    vbw = extras is True
    api = amd.api
    N = int(fs * ms / 1000)
    for T in (2, 12):
        pcm = noise(S, T, 1, N, T)
        b = amd.Batch(S, fs, 1, ms, hr, [rate] * S, device=0)
        d_pcm, d_out = dev.put(pcm), dev.put(np.zeros((S, T, 1024), np.uint8))
        b.encode(pcm)                                                             # host pointers: copies overlapped with the kernels
        b.encode_device(d_pcm, 16, T, d_out, 1024, sync=True)
        if extras:
            b.encode(pcm.astype(np.float32) / 32768)                              # float32 from the host
            b.encode_device(dev.put(pcm.astype(np.float32) / 32768), api.pcm_format(api.PCM_FLOAT32), T, d_out, 1024, sync=True)
            b.encode_device(dev.put(api.pcm_from_native(api.PCM_S16_BE, pcm)), api.pcm_format("s16be"), T, d_out, 1024, sync=True)
            b.encode_device(dev.put(api.pcm_from_native(api.PCM_ALAW, pcm)), api.pcm_format("alaw"), T, d_out, 1024, sync=True)
            offs = (np.arange(S * T, dtype=np.int64).reshape(S, T)[:, ::-1] * N).copy()            # placed PCM: each stream's frames in reverse
            b.set_pcm_placement(dev.put(offs), S * T * N)
            b.encode_device(d_pcm, 16, T, d_out, 1024, sync=True)
            b.set_pcm_placement(None)
            br = np.where(np.arange(T)[None, :] % 2 == 0, rate, rate // 2).astype(np.int32).repeat(S, axis=0)
            bw = np.where(np.arange(T)[None, :] % 3 == 0, 8000, 0).astype(np.int32).repeat(S, axis=0)
            b.encode(pcm, bitrates=br)
            b.encode_device(d_pcm, 16, T, d_out, 1024, sync=True, bitrates=br)
            if vbw:
                b.encode(pcm, bandwidths=bw); b.encode(pcm, bitrates=br, bandwidths=bw)
                b.encode_device(d_pcm, 16, T, d_out, 1024, sync=True, bandwidths=bw)
            d_br, d_bw, d_nb, d_fl = dev.put(br), dev.put(bw), dev.put(np.zeros((S, T), np.int32)), dev.put(np.zeros((S, T), np.uint8))
            b.encode_device_rates(d_pcm, 16, T, d_out, 1024, d_br, None, d_nb, d_fl, sync=True)
            if vbw:
                b.encode_device_rates(d_pcm, 16, T, d_out, 1024, None, d_bw, d_nb, d_fl, sync=True)
                b.encode_device_rates(d_pcm, 16, T, d_out, 1024, d_br, d_bw, d_nb, d_fl, sync=True)
            d_off, d_tot = dev.put(np.zeros((S, T), np.int64)), dev.put(np.zeros(1, np.int64))
            for r, w in ((None, None), (d_br, None)) + (((None, d_bw),) if vbw else ()):      # packed output
                b.encode_device_packed(d_pcm, 16, T, d_out, S * T * 1024, 0, r, w, d_off, d_tot, d_nb, d_fl, sync=True)
            b.set_input_ready(1)                                                  # three calls in a row: the second and third overlap their predecessor
            for k in range(3):
                b.encode_device(d_pcm, 16, T, d_out, 1024, sync=False)
            dev.sync()
            if vbw:
                b.encode_device(d_pcm, 16, T, d_out, 1024, sync=True, bandwidths=bw)
            b.set_input_ready(0)
        b.close()


def decoder(dev, amd, fs, ms, hr, rate, S):
    api = amd.api
    N = int(fs * ms / 1000)
    for T in (2, 12):
        e = amd.Batch(S, fs, 1, ms, hr, [rate] * S, device=0)
        frames = e.encode(noise(S, T, 1, N, 3 * T))
        nbytes = e.num_bytes(0)
        e.close()
        stride = frames.shape[2]
        nb = np.full((S, T), nbytes, np.int32); nb[0, T - 1] = 0
        bfi = np.zeros((S, T), np.uint8); bfi[S - 1, 0] = 1
        d = amd.DecBatch(S, fs, 1, ms, hr, [nbytes] * S, device=0)
        d.decode(frames); d.decode(frames, bfi)                                   # fixed sizes, host pointers
        d.decode(frames, bfi, num_bytes=nb)                                       # host sizes
        d_fr, d_pcm = dev.put(frames), dev.put(np.zeros((S, T, 1, N), np.int16))
        d_nb, d_bfi, d_st = dev.put(nb), dev.put(bfi), dev.put(np.zeros((S, T), np.uint8))
        rc, offs, total, _ = api.plan_packed(nb, 0)
        buf = np.zeros(total + 16, np.uint8)
        for s in range(S):
            for t in range(T):
                buf[offs[s, t]:offs[s, t] + nb[s, t]] = frames[s, t, :nb[s, t]]
        d_buf, d_offs, d_cnt = dev.put(buf), dev.put(offs.astype(np.int64)), dev.put(np.array([T, 1, 0][:S], np.int32))
        place = dev.put((np.arange(S * T, dtype=np.int64).reshape(S, T)[:, ::-1] * N).copy())
        for placed in (0, 1):
            if placed:
                d.set_pcm_placement(place, S * T * N)
            d.decode_device(d_fr, stride, T, d_pcm, sync=True)                    # fixed sizes, device pointers
            d.decode_device_sizes(d_fr, stride, T, d_pcm, d_nb, d_bfi, d_st, sync=True)
            d.decode_device_packed(d_buf, total, d_offs, T, d_pcm, d_nb, stride, d_bfi, d_st, sync=True)
            d.set_frame_counts(d_cnt)                                             # ragged
            d.decode_device_sizes(d_fr, stride, T, d_pcm, d_nb, d_bfi, d_st, sync=True)
            d.decode_device_packed(d_buf, total, d_offs, T, d_pcm, d_nb, stride, d_bfi, d_st, sync=True)
            d.set_frame_counts(None)
            d.set_input_ready(1)                                                  # three calls in a row: the parser runs ahead
            for k in range(3):
                d.decode_device(d_fr, stride, T, d_pcm, sync=False)
            dev.sync()
            d.decode_device_sizes(d_fr, stride, T, d_pcm, d_nb, d_bfi, d_st, sync=True)      # an ordered call behind them
            d.set_input_ready(0)
        d.close()


def run():
    import audio_codec_amd as amd
    dev = Dev()
    encoder(dev, amd, 48000, 10.0, 0, 64000, 3, True)
    encoder(dev, amd, 16000, 10.0, 0, 32000, 3, True)
    encoder(dev, amd, 96000, 10.0, 1, 400000, 2, "nobw")                          # the large layout (no bandwidths there)
    encoder(dev, amd, 48000, 5.0, 0, 64000, 3, False)                             # frontm, four frames a wave
    encoder(dev, amd, 48000, 2.5, 0, 128000, 3, False)                            # frontm, eight frames a wave
    decoder(dev, amd, 48000, 10.0, 0, 64000, 3)
    decoder(dev, amd, 16000, 10.0, 0, 32000, 2)
    decoder(dev, amd, 96000, 10.0, 1, 256000, 2)
    dev.free()
    print("launch_scenarios: done")


def launches(path, in_order=False):
    """the (kernel, grid, workgroup, LDS) lines of a rocprofv3 kernel trace (csv), sorted - or, in_order, as dispatched and with each launch's stream id"""
    out = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            g = lambda *names: next(r[n] for n in names if n in r)
            line = "%s grid %s,%s,%s wg %s,%s,%s lds %s" % (g("Kernel_Name"), g("Grid_Size_X"), g("Grid_Size_Y"), g("Grid_Size_Z"), g("Workgroup_Size_X"),
                                                            g("Workgroup_Size_Y"), g("Workgroup_Size_Z"), g("LDS_Block_Size", "Group_Segment_Size"))
            out.append((int(r["Dispatch_Id"]), line + " stream " + r["Stream_Id"]) if in_order else line)
    return [x[1] for x in sorted(out)] if in_order else sorted(out)


def compare(old, new):
    import collections
    a, b = launches(old), launches(new)
    ca, cb = collections.Counter(a), collections.Counter(b)
    print("# launches: %d old, %d new; distinct (kernel, grid, workgroup, LDS): %d old, %d new; kernels: %d old, %d new"
          % (len(a), len(b), len(ca), len(cb), len({x.split()[0] for x in a}), len({x.split()[0] for x in b})))
    bad = 0
    for side, x, y in (("old", ca, cb), ("new", cb, ca)):
        for line, n in sorted((x - y).items()):
            bad += n
            print("# only in %s (%d): %s" % (side, n, line))
    print("# %s" % ("%d lines differ" % bad if bad or len(a) != len(b) else "the sorted lists are equal line for line"))
    # stronger, and not required of a change that may reorder independent launches: the same launches on the same streams in the same order of dispatch
    oa, ob = launches(old, True), launches(new, True)
    first = next((i for i, (x, y) in enumerate(zip(oa, ob)) if x != y), None)
    print("# in dispatch order, stream ids included: %s" % ("equal" if oa == ob else "first difference at dispatch %s" % first))
    return 1 if bad or len(a) != len(b) else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--compare", nargs=2, metavar=("OLD_CSV", "NEW_CSV"))
    a = ap.parse_args()
    sys.exit(compare(*a.compare) if a.compare else run())
