"""GPU tests of per-frame frame sizes and bad-frame flags in device memory (lc3plus_dec_batch_decode_sizes_device, DecBatch.decode_device_sizes):
every comparison sample for sample against the CPU oracle decoder fed one frame at a time with the frame's own size, as in
test_gpu_dec_varsize.py.  Calls are queued with sync = 0 and synchronised once, unless a test says otherwise.  Device buffers through ctypes
(test_gpu_parity._Dev): the tests do not depend on torch."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_dec_varsize import CASES, make_var_case, oracle_var
from test_gpu_parity import _Dev

pytestmark = pytest.mark.gpu
LC3_ERROR, LC3_NULL_ERROR = 1, 3
INVALID = 2                                                          # status bit: concealed because the size or flag was invalid


def _amd():
    import audio_codec_amd
    return audio_codec_amd


class _Hip(_Dev):
    """_Dev with a stream, pinned host memory and asynchronous copies."""
    def __init__(self):
        super().__init__()
        self.streams, self.pinned = [], []
    def stream(self):
        s = C.c_void_p(); assert self.hip.hipStreamCreate(C.byref(s)) == 0
        self.streams.append(s); return s.value
    def pin(self, arr):
        arr = np.ascontiguousarray(arr); p = C.c_void_p()
        assert self.hip.hipHostMalloc(C.byref(p), C.c_size_t(arr.nbytes), C.c_uint(0)) == 0
        C.memmove(p, arr.ctypes.data, arr.nbytes); self.pinned.append(p); return p.value, arr.nbytes
    def copy_async(self, dst, src_nbytes, stream):
        src, n = src_nbytes
        assert self.hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(n), C.c_int(1), C.c_void_p(stream)) == 0
    def busy(self, stream):
        return self.hip.hipStreamQuery(C.c_void_p(stream)) != 0
    def stream_sync(self, stream):
        assert self.hip.hipStreamSynchronize(C.c_void_p(stream)) == 0
    def free(self):
        self.sync()
        for s in self.streams: self.hip.hipStreamDestroy(s)
        for p in self.pinned: self.hip.hipHostFree(p)
        self.streams, self.pinned = [], []
        super().free()


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


def _cmp(got, st, want, wst):
    bad = np.argwhere((got != want).any(axis=(2, 3)))
    assert len(bad) == 0, ("first differing (stream, frame)", bad[:6].tolist())
    assert (st == wst).all(), np.argwhere(st != wst)[:6].tolist()


def _device_calls(dev, d, frames, num_bytes, bfi, cuts, in_stride=None, sync=False):
    """One decode_device_sizes call per [cuts[k], cuts[k + 1]) frames, queued on the batch's stream; one synchronise at the end."""
    B, T = num_bytes.shape
    stride = in_stride or frames.shape[2]
    calls, outs = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):                            # every upload first: the calls then follow each other without a wait
        fr = np.zeros((B, b - a, stride), np.uint8); fr[:, :, :min(stride, frames.shape[2])] = frames[:, a:b, :stride]
        d_fr, d_nb = dev.put(fr), dev.put(num_bytes[:, a:b].astype(np.int32))
        d_bfi = dev.put(bfi[:, a:b].astype(np.uint8)) if bfi is not None else None
        pcm = dev.zeros(B * (b - a) * d.channels * d.N * 2)
        st = dev.put(np.full((B, b - a), 0xEE, np.uint8))
        calls.append((d_fr, stride, b - a, pcm, d_nb, d_bfi, st)); outs.append((pcm, st, (B, b - a)))
    for c in calls:
        d.decode_device_sizes(*c, sync=sync)
    dev.sync()
    pcm = np.concatenate([dev.get(p, (B, n, d.channels, d.N), np.int16) for p, _, (B, n) in outs], axis=1)
    st = np.concatenate([dev.get(x, (B, n), np.uint8) for _, x, (B, n) in outs], axis=1)
    return pcm, st


POINTS = CASES + [(44100, 10.0, 0, 1, [32000, 64000, 96000, 128000])]


@pytest.mark.parametrize("fs,ms,hr,channels,rates", POINTS)
def test_device_sizes_vs_oracle(dev, fs, ms, hr, channels, rates):
    B, T = 12, 40
    frames, num_bytes, bfi, _ = make_var_case(fs, ms, hr, channels, rates, B, T, seed=fs // 1000 + int(ms * 10) + hr + channels, lost_head=2)
    want, wst = oracle_var(frames, num_bytes, bfi, fs, ms, hr, channels)
    d = _amd().DecBatch(B, fs, channels, ms, hr, None, device=0)
    got, st = _device_calls(dev, d, frames, num_bytes, bfi, [0, 17, 40])
    _cmp(got, st, want, wst)
    d.close()


@pytest.mark.parametrize("fs,ms,hr,channels,rates", [CASES[0], CASES[6], CASES[10]])
def test_same_as_host_arrays(dev, fs, ms, hr, channels, rates):
    """decode(num_bytes=...) with host arrays and the device call give bit-identical PCM, status and num_bytes(stream)."""
    B, T = 16, 30
    frames, num_bytes, bfi, _ = make_var_case(fs, ms, hr, channels, rates, B, T, seed=31 + channels, lost_head=1)
    amd = _amd()
    d1 = amd.DecBatch(B, fs, channels, ms, hr, None, device=0)
    d2 = amd.DecBatch(B, fs, channels, ms, hr, None, device=0)
    a1, s1 = d1.decode(frames[:, :11], bfi[:, :11], num_bytes=num_bytes[:, :11])
    b1, t1 = d1.decode(frames[:, 11:], bfi[:, 11:], num_bytes=num_bytes[:, 11:])
    p2, s2 = _device_calls(dev, d2, frames, num_bytes, bfi, [0, 11, 30])
    assert (np.concatenate([a1, b1], axis=1) == p2).all() and (np.concatenate([s1, t1], axis=1) == s2).all()
    assert [d1.num_bytes(b) for b in range(B)] == [d2.num_bytes(b) for b in range(B)]
    d1.close(); d2.close()


@pytest.mark.parametrize("channels", [1, 2])
def test_invalid_entries_are_concealed(dev, channels):
    """Sizes above in_stride, negative sizes, sizes outside the geometry's table (an odd stereo size whose second channel alone is invalid) and
    flags 2 / 255, scattered and at streams' first frames: the output equals the oracle given those frames as lost; status bit 1 is set exactly there."""
    fs, ms = 48000, 10.0
    rates = [64000, 80000, 96000, 128000] if channels == 1 else [128000, 160800, 192000]
    B, T = 16, 32
    frames, num_bytes, bfi, _ = make_var_case(fs, ms, 0, channels, rates, B, T, seed=50 + channels, p_flip=0)
    # mono: a stride of 420 bytes, so that 401 is refused by the geometry's table alone, not by in_stride; stereo: 39 = 20 + 19 bytes
    stride = 420 if channels == 1 else frames.shape[2]
    rng = np.random.default_rng(channels)
    nb, fl = num_bytes.copy(), bfi.copy()
    inv = np.zeros((B, T), bool)
    bad_sizes = [stride + 1, -7, 19 * channels, 39 if channels == 2 else 401]
    for k, (s, t) in enumerate([(s, 0) for s in range(0, B, 3)] + [tuple(x) for x in rng.integers(0, (B, T), size=(24, 2))]):
        kind = k % 6
        if kind < 4:
            nb[s, t] = bad_sizes[kind]; fl[s, t] = 0
        else:
            fl[s, t] = (2, 255)[kind - 4]
        inv[s, t] = True
    # the oracle sees them as lost frames (size 0)
    o_nb, o_fl = nb.copy(), fl.copy()
    o_nb[inv] = 0; o_fl[inv] = 0
    want, wst = oracle_var(frames, o_nb, o_fl, fs, ms, 0, channels)
    d = _amd().DecBatch(B, fs, channels, ms, 0, None, device=0)        # the oracle, too, starts without a size
    got, st = _device_calls(dev, d, frames, nb, fl, [0, 13, 32], in_stride=stride)
    _cmp(got, st, want, wst | (inv.astype(np.uint8) * INVALID))
    last = [int([x for x, f, i in zip(o_nb[b], o_fl[b], inv[b]) if x and not f and not i][-1]) for b in range(B)]
    assert [d.num_bytes(b) for b in range(B)] == last
    d.close()


def test_call_does_not_wait(dev):
    """The sizes, flags and frames are copied onto the call's stream behind a long run of device work (encoder calls queued there first): the call
    returns while the stream is still busy, and the result is right after the synchronise.  A first call of the same shape has grown the batch's
    buffers, so the timed call has nothing to allocate."""
    fs, ms, B, T = 48000, 10.0, 12, 24
    frames, num_bytes, bfi, _ = make_var_case(fs, ms, 0, 1, [64000, 80000, 96000, 128000], B, 2 * T, seed=61, lost_head=1)
    want, wst = oracle_var(frames, num_bytes, bfi, fs, ms, 0, 1)
    stride = frames.shape[2]
    amd = _amd()
    d = amd.DecBatch(B, fs, 1, ms, 0, None, device=0)
    EB, ET = 4096, 64                                                # the delay: encoder calls of 4096 streams x 64 frames
    enc = amd.Batch(EB, fs, 1, ms, 0, [64000] * EB, device=0)
    d_epcm = dev.put(np.random.default_rng(0).integers(-8000, 8000, size=(EB, ET, 1, 480)).astype(np.int16))
    d_eout = dev.zeros(EB * ET * enc.stride)
    s = dev.stream()
    # first call (frames 0 .. T - 1): grows the batch's buffers; the encoder's first call grows its own
    d_fr0, d_nb0, d_bfi0 = dev.put(frames[:, :T]), dev.put(num_bytes[:, :T].astype(np.int32)), dev.put(bfi[:, :T])
    pcm0, st0 = dev.zeros(B * T * d.N * 2), dev.zeros(B * T)
    d.decode_device_sizes(d_fr0, stride, T, pcm0, d_nb0, d_bfi0, st0, hip_stream=s)
    enc.encode_device(d_epcm, 16, ET, d_eout, enc.stride, hip_stream=s, sync=False)
    # second call (frames T .. 2T - 1), its inputs copied behind the delay
    second = [np.ascontiguousarray(x[:, T:]) for x in (frames, num_bytes.astype(np.int32), bfi)]
    d_fr = dev.zeros(second[0].nbytes)
    d_nb = dev.put(np.full((B, T), -1, np.int32))                    # read before the copy: every frame invalid
    d_bfi = dev.put(np.full((B, T), 255, np.uint8))
    pcm, st = dev.zeros(B * T * d.N * 2), dev.zeros(B * T)
    h = [dev.pin(x) for x in second]
    dev.sync()
    for _ in range(8):
        enc.encode_device(d_epcm, 16, ET, d_eout, enc.stride, hip_stream=s, sync=False)
    for dst, src in zip((d_fr, d_nb, d_bfi), h):
        dev.copy_async(dst, src, s)
    d.decode_device_sizes(d_fr, stride, T, pcm, d_nb, d_bfi, st, hip_stream=s)
    busy = dev.busy(s)
    dev.stream_sync(s)
    assert busy, "the call waited for its stream"
    got = np.concatenate([dev.get(pcm0, (B, T, 1, d.N), np.int16), dev.get(pcm, (B, T, 1, d.N), np.int16)], axis=1)
    sts = np.concatenate([dev.get(st0, (B, T), np.uint8), dev.get(st, (B, T), np.uint8)], axis=1)
    _cmp(got, sts, want, wst)
    enc.close(); d.close()


def _encode_plan(plan, fs=48000, ms=10.0):
    """Frames of every (stream, frame) at plan's bitrate, no losses, no damage -> (frames, sizes)."""
    B, T = plan.shape
    frames, sizes, _, _ = make_var_case(fs, ms, 0, 1, None, B, T, seed=int(plan.sum()) % 1000, p_zero=0, p_bfi=0, p_flip=0, rate_plan=plan)
    return frames, sizes


def test_continuity_with_fixed_calls_and_checkpoint(dev):
    """Three sync = 0 device calls; a fixed-size decode() (the first host-side reader: the mirror is read back); a get_state / set_state hand-over to a
    fresh batch; a device call; set_num_bytes of one stream right after it (again the first reader); a fixed-size decode(); one more device call that
    starts with lost frames.  Identical to the oracle over the whole sequence."""
    fs, ms, B = 48000, 10.0, 8
    rng = np.random.default_rng(71)
    choice = np.array([48000, 64000, 80000, 96000, 120000, 160000])
    seg = [24, 8, 10, 6, 10]                                         # A: 3 device calls, B: fixed, C: device, D: fixed, E: device
    edges = np.cumsum([0] + seg)
    plan = choice[rng.integers(len(choice), size=(B, edges[-1]))]
    nb = np.zeros(plan.shape, np.int32)
    lostA = rng.random((B, seg[0])) < 0.15; lostA[:, 0] = False; lostA[:, -1] = False
    lostC = rng.random((B, seg[2])) < 0.15; lostC[:, -1] = False
    plan[:, edges[1]:edges[2]] = plan[:, edges[1] - 1:edges[1]]      # B at A's last size (A's last frame is good)
    plan[:, edges[3]:edges[4]] = plan[:, edges[3] - 1:edges[3]]      # D at C's last size ...
    Y = 112000
    plan[0, edges[3]:edges[4]] = Y                                   # ... but stream 0 set to Y first
    frames, sizes = _encode_plan(plan, fs, ms)
    nb[:] = sizes
    nb[:, :seg[0]][lostA] = 0
    nb[:, edges[2]:edges[3]][lostC] = 0
    nb[:, edges[4]:edges[4] + 2] = 0                                 # E starts with two lost frames: the carry of D's configuration
    bfi = np.zeros(nb.shape, np.uint8)
    want, wst = oracle_var(frames, nb, bfi, fs, ms, 0, 1)
    amd = _amd()
    d = amd.DecBatch(B, fs, 1, ms, 0, [int(x) for x in sizes[:, 0]], device=0)
    outs = []
    fa = frames[:, :edges[1]]
    outs.append(_device_calls(dev, d, fa, nb[:, :edges[1]], bfi[:, :edges[1]], [0, 8, 16, 24]))
    lastA = sizes[:, edges[1] - 1]
    fb = np.ascontiguousarray(frames[:, edges[1]:edges[2], :int(lastA.max())])
    outs.append(d.decode(fb))
    assert [d.num_bytes(b) for b in range(B)] == [int(x) for x in lastA]
    state = d.get_state()
    d.close()
    d = amd.DecBatch(B, fs, 1, ms, 0, [int(x) for x in lastA], device=0)
    d.set_state(state)
    outs.append(_device_calls(dev, d, frames[:, edges[2]:edges[3]], nb[:, edges[2]:edges[3]], bfi[:, edges[2]:edges[3]], [0, seg[2]]))
    d.set_num_bytes(0, Y // 800)
    lastC = sizes[:, edges[3] - 1].copy(); lastC[0] = Y // 800
    assert [d.num_bytes(b) for b in range(B)] == [int(x) for x in lastC]
    fd = np.ascontiguousarray(frames[:, edges[3]:edges[4], :int(lastC.max())])
    outs.append(d.decode(fd))
    outs.append(_device_calls(dev, d, frames[:, edges[4]:], nb[:, edges[4]:], bfi[:, edges[4]:], [0, seg[4]]))
    got = np.concatenate([o[0] for o in outs], axis=1); st = np.concatenate([o[1] for o in outs], axis=1)
    _cmp(got, st, want, wst)
    assert [d.num_bytes(b) for b in range(B)] == [int(x) for x in sizes[:, -1]]
    d.close()


def test_mixed_with_parse_ahead_calls(dev):
    """Under set_input_ready(1), sync = 0 throughout and one synchronise: parse-ahead calls (device frames, no flags), device-size calls whose last
    frames are lost, more parse-ahead calls, and a device-size call with flags that starts with a lost frame - against the oracle."""
    U, reps, T = 64, 32, 16                                          # 2048 streams: the calls overlap
    fs, ms = 48000, 10.0
    rng = np.random.default_rng(81)
    choice = np.array([64000, 80000, 96000, 104000, 128000])
    K = 7
    plan = choice[rng.integers(len(choice), size=(U, K * T))]
    plan[:, :2 * T] = plan[:, :1]                                    # calls 0, 1: parse-ahead at one size per stream
    last_good = 4 * T - 4                                            # calls 2, 3: device sizes, the last three frames of call 3 lost
    plan[:, 4 * T:6 * T] = plan[:, last_good:last_good + 1]          # calls 4, 5: parse-ahead at the last good size of call 3
    frames, sizes = _encode_plan(plan, fs, ms)
    nb = sizes.astype(np.int32).copy()
    nb[:, last_good + 1:4 * T] = 0
    bfi = np.zeros(nb.shape, np.uint8)
    nb[:, 6 * T] = 0                                                 # call 6 starts with a lost frame, and has flags
    bfi[:, 6 * T + 1:] = rng.random((U, T - 1)) < 0.1
    want, wst = oracle_var(frames, nb, bfi, fs, ms, 0, 1)
    B = U * reps
    stride = frames.shape[2]
    fr, tnb, tbfi = np.tile(frames, (reps, 1, 1)), np.tile(nb, (reps, 1)), np.tile(bfi, (reps, 1))
    ins = [dev.put(fr[:, k * T:(k + 1) * T]) for k in range(K)]
    nbs = [dev.put(tnb[:, k * T:(k + 1) * T]) for k in range(K)]
    bfis = [dev.put(tbfi[:, k * T:(k + 1) * T]) for k in range(K)]
    amd = _amd()
    dec = amd.DecBatch(B, fs, 1, ms, 0, [int(x) for x in np.tile(sizes[:, 0], reps)], device=0)
    outs = [dev.zeros(B * T * dec.N * 2) for _ in range(K)]
    dev.sync()
    dec.set_input_ready(True)
    for k in range(K):
        if k in (0, 1, 4, 5):
            dec.decode_device(ins[k], stride, T, outs[k], 16, sync=False)
        else:
            dec.decode_device_sizes(ins[k], stride, T, outs[k], nbs[k], bfis[k] if k == 6 else None, sync=False)
    dev.sync()
    out = np.concatenate([dev.get(o, (B, T, 1, dec.N), np.int16) for o in outs], axis=1)
    for r in range(reps):
        bad = np.argwhere((out[r * U:(r + 1) * U] != want).any(axis=(2, 3)))
        assert len(bad) == 0, ("copy", r, "first differing (stream, frame)", bad[:4].tolist())
    dec.close()


def test_argument_errors_leave_the_batch_unchanged(dev):
    fs, ms, B, T = 48000, 10.0, 6, 20
    frames, num_bytes, bfi, _ = make_var_case(fs, ms, 0, 1, [64000, 96000, 128000], B, T, seed=91, lost_head=1)
    want, wst = oracle_var(frames, num_bytes, bfi, fs, ms, 0, 1)
    amd = _amd()
    d = amd.DecBatch(B, fs, 1, ms, 0, None, device=0)
    stride = frames.shape[2]
    first = _device_calls(dev, d, frames[:, :8], num_bytes[:, :8], bfi[:, :8], [0, 8])
    d_fr, d_nb, d_bfi = dev.put(frames[:, 8:]), dev.put(num_bytes[:, 8:].astype(np.int32)), dev.put(bfi[:, 8:])
    n = T - 8
    pcm, st = dev.zeros(B * n * d.N * 2), dev.zeros(B * n)
    for args, code in (((0, stride, n, pcm, d_nb), LC3_NULL_ERROR), ((d_fr, stride, n, 0, d_nb), LC3_NULL_ERROR),
                       ((d_fr, stride, n, pcm, 0), LC3_NULL_ERROR), ((d_fr, stride, 0, pcm, d_nb), LC3_ERROR),
                       ((d_fr, 0, n, pcm, d_nb), LC3_ERROR)):
        with pytest.raises(amd.LC3Error) as e:
            d.decode_device_sizes(*args, d_bfi, st)
        assert e.value.code == code
    with pytest.raises(amd.LC3Error) as e:
        d.decode_device_sizes(d_fr, stride, n, pcm, d_nb, d_bfi, st, bps=20)
    assert e.value.code == LC3_ERROR
    dev.sync()
    assert not dev.get(pcm, (B, n, 1, d.N), np.int16).any() and not dev.get(st, (B, n), np.uint8).any()     # nothing was queued
    d.decode_device_sizes(d_fr, stride, n, pcm, d_nb, d_bfi, st)
    dev.sync()
    got = np.concatenate([first[0], dev.get(pcm, (B, n, 1, d.N), np.int16)], axis=1)
    sts = np.concatenate([first[1], dev.get(st, (B, n), np.uint8)], axis=1)
    _cmp(got, sts, want, wst)
    d.close()
