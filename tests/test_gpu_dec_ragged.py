"""GPU tests of per-stream frame counts in the batched decoder (lc3plus_dec_batch_set_frame_counts, DecBatch.set_frame_counts): ragged calls of
decode_device_sizes / decode_device_packed against the CPU oracle decoder fed each stream's frames densely (test_gpu_dec_varsize.make_var_case /
oracle_var).  Every comparison is equality: PCM sample for sample, status byte for byte, state byte for byte.  PCM and status buffers are filled with a
sentinel first; the entries of absent frames hold garbage that would be invalid if it were looked at.

One case of B streams x 14 frames per geometry; each stream's frames are dealt out over 8 calls of 6 frames with counts from {0, 1, 3, 4, 5, 6}, every call
holding at least one 0 and one 6 (_schedule)."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_dec_varsize import CASES, make_var_case, oracle_var
from test_gpu_parity import _Dev

pytestmark = pytest.mark.gpu
LC3_ERROR = 1
ABSENT, PLACE, INVALID = 8, 4, 2
T_TOTAL, NF, K = 14, 6, 8
SENT = 0x5A                                                          # every byte of a PCM buffer before a call
ST_SENT = 0xEE
# geometry -> (case of test_gpu_dec_varsize.CASES, streams)
SHAPES = {
    1: (CASES[9], 70),      # 48 kHz / 10 ms mono, <= 128 bytes: the LDS-staged parser, two waves of the concealment kernel, four frames per IMDCT wave
    2: (CASES[10], 35),     # 48 kHz / 10 ms stereo, odd sizes, > 128 bytes: the _g parser
    3: (CASES[8], 9),       # 96 kHz / 10 ms high resolution: the large layout
    4: (CASES[4], 20),      # 16 kHz / 10 ms: the generic IMDCT kernel with its runs of IMDCT_FPW frames
}


def _amd():
    import audio_codec_amd
    return audio_codec_amd


class _Hip(_Dev):
    """_Dev with a stream, pinned host memory and asynchronous copies (as in test_gpu_dec_varsize_device.py)."""
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


def _schedule(B, seed):
    """counts [K, B]: every column sums to T_TOTAL, every entry is one of 0, 1, 3, 4, 5, 6, every row holds a 0 and a 6.  Streams 0 .. 3 are pillars:
    pillar j has 6, 6, 1, 1 in calls 2j .. 2j + 3 (mod K) and 0 elsewhere, which gives every call a 6 and two 0s; the others split their 14 frames at
    random and place the parts in random calls, in order."""
    rng = np.random.default_rng(seed)
    sched = np.zeros((K, B), np.int32)
    for j in range(4):
        for i, c in enumerate((6, 6, 1, 1)):
            sched[(2 * j + i) % K, j] = c
    for s in range(4, B):
        while True:
            parts, left = [], T_TOTAL
            while left:
                c = int(rng.choice([x for x in (1, 3, 4, 5, 6) if x <= left]))
                parts.append(c); left -= c
            if len(parts) <= K:
                break
        sched[np.sort(rng.choice(K, len(parts), replace=False)), s] = parts
    assert (sched.sum(axis=0) == T_TOTAL).all() and np.isin(sched, (0, 1, 3, 4, 5, 6)).all()
    assert ((sched == 0).any(axis=1) & (sched == 6).any(axis=1)).all()
    return sched


@functools.lru_cache(maxsize=None)
def _case(shape):
    """The shared case of a geometry, computed once and left unchanged: frames, sizes, flags, the oracle's dense result and the schedule."""
    (fs, ms, hr, ch, rates), B = SHAPES[shape]
    frames, nb, bfi, sizes = make_var_case(fs, ms, hr, ch, rates, B, T_TOTAL, seed=90 + shape)
    want, wst = oracle_var(frames, nb, bfi, fs, ms, hr, ch)
    c = dict(fs=fs, ms=ms, hr=hr, ch=ch, B=B, N=want.shape[3], frames=frames, nb=nb.astype(np.int32), bfi=bfi, sizes=sizes, want=want, wst=wst,
             sched=_schedule(B, shape), stride=frames.shape[2])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def _batch(c):
    return _amd().DecBatch(c["B"], c["fs"], c["ch"], c["ms"], c["hr"], None, device=0)


def _call_inputs(c, pos, cnt):
    """One call's arrays: stream s holds its frames pos[s] .. pos[s] + cnt[s] - 1; the entries of its absent frames are garbage."""
    B, S = c["B"], c["stride"]
    fr = np.full((B, NF, S), 0xA5, np.uint8)
    tt, ss = np.meshgrid(np.arange(NF), np.arange(B))
    nb = np.where((ss + tt) % 2 == 0, -7, 100000).astype(np.int32)
    bfi = np.full((B, NF), 7, np.uint8)
    for s in range(B):
        p, n = int(pos[s]), int(cnt[s])
        fr[s, :n] = c["frames"][s, p:p + n]; nb[s, :n] = c["nb"][s, p:p + n]; bfi[s, :n] = c["bfi"][s, p:p + n]
    return fr, nb, bfi


def _frames_view(raw, fmt, B, T, ch, N):
    """the bytes of one call's PCM as [B, T, ch, N, element bytes], whatever the layout"""
    api = _amd().api
    eb = api.load_library().lc3plus_pcm_elem_bytes(fmt)
    if fmt & api.PCM_CHANNEL_MAJOR:
        return raw.reshape(B, ch, T, N, eb).transpose(0, 2, 1, 3, 4)
    assert not fmt & api.PCM_INTERLEAVED
    return raw.reshape(B, T, ch, N, eb)


def _run(dev, d, c, calls=range(K), fmt=16, packed=False, before=None, counts_of=None, async_counts=False):
    """The ragged calls `calls` of the schedule on batch d, which has decoded the frames of the calls before them.  Asserts what holds for absent frames
    (PCM keeps the sentinel, status is exactly ABSENT) and returns the present frames gathered per stream: PCM bytes [B, 14, ch, N, eb] (zeros where not
    yet decoded), status [B, 14], and the mask of gathered frames.  before(k): called in front of call k.  counts_of(k, cnt): the counts uploaded in place
    of the effective ones (out-of-range tests)."""
    api = _amd().api
    B, ch, N, sched = c["B"], c["ch"], c["N"], c["sched"]
    eb = api.load_library().lc3plus_pcm_elem_bytes(fmt)
    got = np.zeros((B, T_TOTAL, ch, N, eb), np.uint8); gst = np.zeros((B, T_TOTAL), np.uint8); seen = np.zeros((B, T_TOTAL), bool)
    stream = dev.stream() if async_counts else None
    d_cnt = dev.put(np.zeros(B, np.int32))
    d.set_frame_counts(d_cnt)
    for k in calls:
        pos, cnt = sched[:k].sum(axis=0), sched[k]
        if before:
            before(k)
        fr, nb, bfi = _call_inputs(c, pos, cnt)
        up = np.ascontiguousarray(counts_of(k, cnt) if counts_of else cnt, np.int32)
        d_pcm, d_st = dev.put(np.full(B * NF * ch * N * eb, SENT, np.uint8)), dev.put(np.full((B, NF), ST_SENT, np.uint8))
        d_nb, d_bfi = dev.put(nb), dev.put(bfi)
        if async_counts:                                              # the counts arrive on the call's stream, right in front of a call that does not wait
            dev.copy_async(d_cnt, dev.pin(up), stream)
        else:
            assert dev.hip.hipMemcpy(C.c_void_p(d_cnt), C.c_void_p(up.ctypes.data), C.c_size_t(up.nbytes), C.c_int(1)) == 0
        if packed:
            present = np.arange(NF)[None, :] < cnt[:, None]
            szs = np.zeros((B, NF), np.int32)
            for s in range(B):
                szs[s, :cnt[s]] = c["sizes"][s, pos[s]:pos[s] + cnt[s]]
            rc, offs, total, _ = api.plan_packed(szs)                # offsets over the present frames only
            assert rc == 0
            buf = np.full(total + 64, 0xC3, np.uint8)
            for s in range(B):
                for t in range(int(cnt[s])):
                    buf[offs[s, t]:offs[s, t] + szs[s, t]] = fr[s, t, :szs[s, t]]
            offs = np.where(present, offs, np.where((np.arange(B)[:, None] + np.arange(NF)[None, :]) % 2 == 0, -3, total + 1000)).astype(np.int64)
            d.decode_device_packed(dev.put(buf), total, dev.put(offs), NF, d_pcm, d_nb, c["stride"], d_bfi, d_st, bps=fmt, hip_stream=stream, sync=False)
        else:
            d.decode_device_sizes(dev.put(fr), c["stride"], NF, d_pcm, d_nb, d_bfi, d_st, bps=fmt, hip_stream=stream, sync=False)
        if async_counts:
            dev.stream_sync(stream)
        dev.sync()
        pcm = _frames_view(dev.get(d_pcm, (B * NF * ch * N * eb,), np.uint8), fmt, B, NF, ch, N)
        st = dev.get(d_st, (B, NF), np.uint8)
        for s in range(B):
            p, n = int(pos[s]), int(cnt[s])
            assert (pcm[s, n:] == SENT).all(), ("absent PCM written", k, s)
            assert (st[s, n:] == ABSENT).all(), ("absent status", k, s, st[s].tolist())
            got[s, p:p + n] = pcm[s, :n]; gst[s, p:p + n] = st[s, :n]; seen[s, p:p + n] = True
    d.set_frame_counts(None)
    return got, gst, seen


def _want16(c):
    return np.ascontiguousarray(c["want"]).view(np.uint8).reshape(c["B"], T_TOTAL, c["ch"], c["N"], 2)


def _dense_twin(dev, c, fmt=16):
    """a second batch that decodes the same streams densely, one call of 14 frames without counts -> (batch, PCM bytes [B, 14, ch, N, eb], status)"""
    api = _amd().api
    B, ch, N = c["B"], c["ch"], c["N"]
    eb = api.load_library().lc3plus_pcm_elem_bytes(fmt)
    d = _batch(c)
    d_pcm, d_st = dev.put(np.full(B * T_TOTAL * ch * N * eb, SENT, np.uint8)), dev.put(np.full((B, T_TOTAL), ST_SENT, np.uint8))
    d.decode_device_sizes(dev.put(c["frames"]), c["stride"], T_TOTAL, d_pcm, dev.put(c["nb"]), dev.put(c["bfi"]), d_st, bps=fmt, sync=True)
    return d, _frames_view(dev.get(d_pcm, (B * T_TOTAL * ch * N * eb,), np.uint8), fmt, B, T_TOTAL, ch, N), dev.get(d_st, (B, T_TOTAL), np.uint8)


def _sizes_after(d, B):
    return [d.num_bytes(s) for s in range(B)]


@pytest.mark.parametrize("shape", [1, 2, 3, 4])
def test_ragged_sequence_vs_oracle(dev, shape):
    c = _case(shape)
    d = _batch(c)
    got, gst, seen = _run(dev, d, c)
    assert seen.all()
    bad = np.argwhere((got != _want16(c)).any(axis=(2, 3, 4)))
    assert len(bad) == 0, ("first differing (stream, frame)", bad[:6].tolist())
    assert (gst == c["wst"]).all(), np.argwhere(gst != c["wst"])[:6].tolist()
    twin, tp, ts = _dense_twin(dev, c)
    assert (tp == got).all() and (ts == gst).all()
    assert (d.get_state() == twin.get_state()).all()
    assert _sizes_after(d, c["B"]) == _sizes_after(twin, c["B"])
    d.close(); twin.close()


def _one_call(dev, d, c, counts, fmt=16):
    """one call of NF frames from every stream's frame 0 with `counts` uploaded as they are -> PCM bytes [B, NF, ch, N, eb], status"""
    B, ch, N = c["B"], c["ch"], c["N"]
    eb = _amd().api.load_library().lc3plus_pcm_elem_bytes(fmt)
    eff = np.clip(counts, 0, NF)
    fr, nb, bfi = _call_inputs(c, np.zeros(B, np.int64), eff)
    d_pcm, d_st = dev.put(np.full(B * NF * ch * N * eb, SENT, np.uint8)), dev.put(np.full((B, NF), ST_SENT, np.uint8))
    d.set_frame_counts(dev.put(np.ascontiguousarray(counts, np.int32)))
    d.decode_device_sizes(dev.put(fr), c["stride"], NF, d_pcm, dev.put(nb), dev.put(bfi), d_st, bps=fmt, sync=True)
    d.set_frame_counts(None)
    return _frames_view(dev.get(d_pcm, (B * NF * ch * N * eb,), np.uint8), fmt, B, NF, ch, N), dev.get(d_st, (B, NF), np.uint8)


def test_counts_all_zero_change_nothing(dev):
    c = _case(1)
    d = _batch(c)
    _run(dev, d, c, calls=range(3))                                   # some history first: state and sizes that are not the initial ones
    st0, nb0 = d.get_state(), _sizes_after(d, c["B"])
    pcm, st = _one_call(dev, d, c, np.zeros(c["B"], np.int32))
    assert (pcm == SENT).all() and (st == ABSENT).all()
    assert (d.get_state() == st0).all() and _sizes_after(d, c["B"]) == nb0
    d.close()


def test_counts_all_n_frames_equal_the_dense_call(dev):
    c = _case(1)
    B = c["B"]
    d, twin = _batch(c), _batch(c)
    pcm, st = _one_call(dev, d, c, np.full(B, NF, np.int32))
    d_pcm, d_st = dev.put(np.full(B * NF * c["ch"] * c["N"] * 2, SENT, np.uint8)), dev.put(np.full((B, NF), ST_SENT, np.uint8))
    twin.decode_device_sizes(dev.put(c["frames"][:, :NF]), c["stride"], NF, d_pcm, dev.put(c["nb"][:, :NF]), dev.put(c["bfi"][:, :NF]), d_st, sync=True)
    assert (pcm.reshape(-1) == dev.get(d_pcm, (pcm.size,), np.uint8)).all() and (st == dev.get(d_st, (B, NF), np.uint8)).all()
    assert (pcm == _want16(c)[:, :NF]).all() and (st == c["wst"][:, :NF]).all()
    assert (d.get_state() == twin.get_state()).all() and _sizes_after(d, B) == _sizes_after(twin, B)
    d.close(); twin.close()


def test_out_of_range_counts_are_clamped(dev):
    """-5 behaves as 0 and n_frames + 3 as n_frames: the same bytes, status and state as the clamped counts on a twin batch"""
    c = _case(1)
    B = c["B"]
    raw = np.where(np.arange(B) % 3 == 0, -5, np.where(np.arange(B) % 3 == 1, NF + 3, 4)).astype(np.int32)
    raw[5], raw[6] = -2 ** 31, 2 ** 31 - 1
    d, twin = _batch(c), _batch(c)
    p1, s1 = _one_call(dev, d, c, raw)
    p2, s2 = _one_call(dev, twin, c, _amd().api.dec_plan_counts(raw, NF))
    eff = np.clip(raw.astype(np.int64), 0, NF)
    for s in range(B):
        assert (p1[s, :eff[s]] == _want16(c)[s, :eff[s]]).all() and (p1[s, eff[s]:] == SENT).all()
        assert (s1[s, :eff[s]] == c["wst"][s, :eff[s]]).all() and (s1[s, eff[s]:] == ABSENT).all()
    assert (p1 == p2).all() and (s1 == s2).all() and (d.get_state() == twin.get_state()).all()
    d.close(); twin.close()


def test_decode_packed_with_counts(dev):
    c = _case(1)
    d = _batch(c)
    got, gst, seen = _run(dev, d, c, packed=True)
    assert seen.all() and (got == _want16(c)).all() and (gst == c["wst"]).all()
    d.close()


def test_counts_produced_on_the_stream(dev):
    """the counts are copied from pinned memory on the call's hip_stream right before a sync = 0 call: as with counts uploaded beforehand"""
    c = _case(1)
    d = _batch(c)
    got, gst, seen = _run(dev, d, c, async_counts=True)
    assert seen.all() and (got == _want16(c)).all() and (gst == c["wst"]).all()
    d.close()


@pytest.mark.parametrize("name", ["s24_3be", "f32_channel_major"])
def test_wire_type_and_layout(dev, name):
    """present frames are what the dense call in the same format word writes; channel-major keeps the call's n_frames as the channel distance"""
    api = _amd().api
    fmt = api.PCM_S24_3BE if name == "s24_3be" else api.PCM_FLOAT32 | api.PCM_CHANNEL_MAJOR
    c = _case(2)
    d = _batch(c)
    got, gst, seen = _run(dev, d, c, fmt=fmt)
    twin, tp, ts = _dense_twin(dev, c, fmt)
    assert seen.all() and (got == tp).all() and (gst == ts).all() and (gst == c["wst"]).all()
    assert (d.get_state() == twin.get_state()).all()
    d.close(); twin.close()


def test_placed_pcm_with_counts(dev):
    """Every stream decodes into a ring of 16 slots from a start that makes it wrap; per call one present frame has an invalid offset (status bit 2, not
    written) and the absent frames' offsets are garbage (status exactly 8).  No byte of the arena outside the written frames changes."""
    api = _amd().api
    c = _case(1)
    B, ch, N, sched = c["B"], c["ch"], c["N"], c["sched"]
    R, fe = 16, ch * N
    rstride = R * fe + 5
    cap = B * rstride
    start = (np.arange(B) * 3) % R
    d = _batch(c)
    d_ring = dev.put(np.full(cap * 2, SENT, np.uint8))
    want_ring = np.full(cap, SENT | SENT << 8, np.uint16).view(np.int16)
    d_cnt = dev.put(np.zeros(B, np.int32))
    d.set_frame_counts(d_cnt)
    for k in range(K):
        pos, cnt = sched[:k].sum(axis=0), sched[k]
        fr, nb, bfi = _call_inputs(c, pos, cnt)
        offs = np.where((np.arange(B)[:, None] + np.arange(NF)[None, :]) % 2 == 0, -5, 2 ** 62).astype(np.int64)       # absent: garbage
        wst = np.full((B, NF), ABSENT, np.uint8)
        victim = int(np.flatnonzero(cnt > 0)[k % np.count_nonzero(cnt > 0)])
        for s in range(B):
            for t in range(int(cnt[s])):
                o = s * rstride + ((start[s] + pos[s] + t) % R) * fe
                wst[s, t] = c["wst"][s, pos[s] + t]
                if s == victim and t == cnt[s] - 1:
                    offs[s, t] = (cap - fe + 1, -1)[k % 2]; wst[s, t] |= PLACE
                else:
                    offs[s, t] = o; want_ring[o:o + fe] = c["want"][s, pos[s] + t].reshape(-1)
        assert dev.hip.hipMemcpy(C.c_void_p(d_cnt), C.c_void_p(np.ascontiguousarray(cnt).ctypes.data), C.c_size_t(4 * B), C.c_int(1)) == 0
        d_st = dev.put(np.full((B, NF), ST_SENT, np.uint8))
        d.set_pcm_placement(dev.put(offs), cap)
        d.decode_device_sizes(dev.put(fr), c["stride"], NF, d_ring, dev.put(nb), dev.put(bfi), d_st, sync=True)
        st = dev.get(d_st, (B, NF), np.uint8)
        assert (st == wst).all(), (k, np.argwhere(st != wst)[:6].tolist())
    ring = dev.get(d_ring, (cap,), np.int16)
    assert (ring == want_ring).all(), np.flatnonzero(ring != want_ring)[:6].tolist()
    assert (start + T_TOTAL > R).any()                                  # rings did wrap
    d.set_pcm_placement(None); d.set_frame_counts(None)
    d.close()


def test_reset_streams_between_ragged_calls(dev):
    """two streams are reset in front of call 3: from there on they give what a fresh decoder gives for their remaining frames, the others are untouched"""
    c = _case(1)
    sched = c["sched"]
    pos3 = sched[:3].sum(axis=0)
    # streams with frames left whose next frame is good (a fresh decoder has no size to carry into a lost first frame)
    pick = [s for s in range(4, c["B"]) if pos3[s] < T_TOTAL and c["nb"][s, pos3[s]] > 0 and c["bfi"][s, pos3[s]] == 0][:2]
    assert len(pick) == 2
    d = _batch(c)
    got, gst, seen = _run(dev, d, c, before=lambda k: d.reset_streams(pick, sync=False) if k == 3 else None)
    want, wst = _want16(c).copy(), c["wst"].copy()
    for s in pick:
        p = int(pos3[s])
        w, ws = oracle_var(c["frames"][s:s + 1, p:], c["nb"][s:s + 1, p:], c["bfi"][s:s + 1, p:], c["fs"], c["ms"], c["hr"], c["ch"])
        want[s, p:] = np.ascontiguousarray(w[0]).view(np.uint8).reshape(T_TOTAL - p, c["ch"], c["N"], 2); wst[s, p:] = ws[0]
    assert seen.all() and (got == want).all() and (gst == wst).all()
    d.close()


def test_ragged_call_directly_after_import(dev):
    """calls 0 .. 2 on one batch; its streams exported and imported into a fresh batch configured with their sizes; calls 3 .. 7 there: the oracle's result"""
    c = _case(1)
    B = c["B"]
    a, b = _batch(c), _batch(c)
    g1, s1, m1 = _run(dev, a, c, calls=range(3))
    blob = a.export_streams(list(range(B)))
    for s in range(B):
        if a.num_bytes(s):
            assert b.set_num_bytes(s, a.num_bytes(s)) == 0
    b.import_streams(list(range(B)), blob)
    g2, s2, m2 = _run(dev, b, c, calls=range(3, K))
    assert (m1 ^ m2).all()
    assert (np.where(m1[:, :, None, None, None], g1, g2) == _want16(c)).all() and (np.where(m1, s1, s2) == c["wst"]).all()
    a.close(); b.close()


def test_other_calls_refuse_on_a_real_batch(dev):
    """while counts are set decode() and decode(num_bytes=...) return LC3_ERROR and leave state and sizes alone; after set_frame_counts(None) they work"""
    api = _amd().api
    c = _case(1)
    B = c["B"]
    d = _batch(c)
    pcm, st = _one_call(dev, d, c, np.full(B, NF, np.int32))          # every stream has a history and, where it had a good frame, a size
    st0, nb0 = d.get_state(), _sizes_after(d, B)
    d.set_frame_counts(dev.put(np.full(B, 2, np.int32)))
    nxt = slice(NF, NF + 3)
    for kw in ({}, {"num_bytes": c["nb"][:, nxt]}):
        with pytest.raises(api.LC3Error) as e:
            d.decode(c["frames"][:, nxt], c["bfi"][:, nxt], **kw)
        assert e.value.code == LC3_ERROR
    with pytest.raises(api.LC3Error) as e:
        d.decode_device(dev.put(c["frames"][:, nxt]), c["stride"], 3, dev.zeros(B * 3 * c["N"] * 2))
    assert e.value.code == LC3_ERROR
    assert (d.get_state() == st0).all() and _sizes_after(d, B) == nb0
    d.set_frame_counts(None)
    p, s = d.decode(c["frames"][:, nxt], c["bfi"][:, nxt], num_bytes=c["nb"][:, nxt])
    assert (p == c["want"][:, nxt]).all() and (s == c["wst"][:, nxt]).all()
    p, s = d.decode(c["frames"][:, NF + 3:NF + 4])                      # the fixed-size call is back as well
    assert p.shape == (B, 1, c["ch"], c["N"])
    d.close()
