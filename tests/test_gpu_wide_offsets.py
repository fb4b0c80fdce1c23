"""GPU tests of offsets past 4 GiB (tests/wide_offsets.py): placed PCM of the encoder and the decoder, packed frames, the probe and the ingest tables at byte
offsets on either side of 2^31, 2^32, 3 * 2^31 and 2^33 inside ONE arena of 2^33 + 2^28 bytes (one hipMalloc, one hipMemset to 0xA5; 2^32 + 2^28 bytes where
the device has less free memory, and then every case that ran on it reports itself skipped: the two upper boundaries were not reached).

Every comparison is exact.  The expectation is the dense device-pointer call of the same build on the same frames, which never sees the arena and is held to
the CPU oracle by the other modules, and for the 16-bit type of every geometry the CPU oracle itself.  A wide run is never compared with a wide run.  Host memory
never holds the arena: frames go up and windows come down by hipMemcpy at base + byte offset, and every test puts the windows it wrote back to 0xA5, which the
last test of the file checks over the whole arena.  A case is the planner's five consecutive calls on one batch of six streams at two rates (call k: position
class k at every boundary), T = 4 (the one-wave kernels) and T = 12 (the smallest pipelined call); every case runs inside api.launch_census() and asserts that
the kernels it is meant to reach were launched.  Channel-major PCM has no placed form (the call is refused, here too), so the layouts that run are the default
and the interleaved one.  One process, no threads."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import wide_offsets as wo
from lc3_harness import Oracle, make_dec_case, oracle_decode_streams
from test_gpu_dec_varsize_device import _Hip
from test_gpu_pcm_format import _amd, _api, _same
from test_gpu_pcm_placed import CM, DEC_ST_PCM_PLACE, EB, ENC_FL_PCM_PLACE, F32, I64_MAX, IL, _frame_flat, _input
from test_gpu_pcm_wire import ALAW, G16S, G44, G48, G48ST, G96, S16BE, S24BE, S24LE, ULAW

pytestmark = pytest.mark.gpu

S = 6
CALLS = wo.CLASSES
CANARY = 0xA5
G48_5 = (48000, 5.0, 0, 1, 64000)                        # N = 240: lc3_enc_frontm_kernel
RATE2 = {G16S: 96000, G48: 96000, G48ST: 192000, G96: 400000, G48_5: 96000, G44: 96000}      # the second rate of every geometry
ALL9 = [16, 24, 32, F32, S16BE, S24LE, S24BE, ULAW, ALAW]
FEW = [16, S24LE, ULAW, F32]
CASES = [(G48ST, ty, 0) for ty in ALL9] + [(G48ST, ty, IL) for ty in FEW] + [(g, ty, 0) for g in (G16S, G48, G96, G48_5, G44) for ty in FEW]
PARAMS = [pytest.param(g, ty, lay, T, id="%d-%g-%dch-%#x-%#x-T%d" % (g[0], g[1], g[3], ty, lay, T)) for g, ty, lay in CASES for T in (4, 12)]
TIMES = {}


class _Arena:
    """the one allocation; windows written since the last restore() are remembered and put back to the canary by it"""
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        free, total = C.c_size_t(), C.c_size_t()
        assert self.hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        self.size = wo.ARENA if free.value >= wo.ARENA + 2 ** 32 else wo.ARENA_REDUCED
        self.reduced = self.size != wo.ARENA
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(self.size)) == 0, "hipMalloc of the arena"
        self.base = p.value
        assert self.hip.hipMemset(p, C.c_int(CANARY), C.c_size_t(self.size)) == 0 and self.hip.hipDeviceSynchronize() == 0
        self.dirty = []

    def _in(self, lo, n):
        assert 0 <= lo and lo + n <= self.size, (lo, n)

    def write(self, lo, arr):
        arr = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        self._in(lo, arr.size)
        assert self.hip.hipMemcpy(C.c_void_p(self.base + lo), C.c_void_p(arr.ctypes.data), C.c_size_t(arr.size), C.c_int(1)) == 0
        self.dirty.append((lo, arr.size))

    def written(self, lo, n):
        """a window the library is expected to write"""
        self._in(lo, n)
        self.dirty.append((lo, n))

    def read(self, lo, n):
        self._in(lo, n)
        out = np.zeros(n, np.uint8)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(self.base + lo), C.c_size_t(n), C.c_int(2)) == 0
        return out

    def restore(self):
        for lo, n in self.dirty:
            assert self.hip.hipMemset(C.c_void_p(self.base + lo), C.c_int(CANARY), C.c_size_t(n)) == 0
        assert self.hip.hipDeviceSynchronize() == 0
        self.dirty = []

    def free(self):
        self.hip.hipDeviceSynchronize()
        self.hip.hipFree(C.c_void_p(self.base))


@pytest.fixture(scope="module")
def arena():
    t0 = time.perf_counter()
    a = _Arena()
    TIMES["start"] = t0
    yield a
    a.free()


@pytest.fixture
def dev():
    h = _Hip()
    if h.hip.hipDeviceSynchronize() != 0:                                 # a fault in an earlier case: nothing more of this module is started on the device
        pytest.exit("the device reports an error left by an earlier case", 3)
    yield h
    h.free()


@pytest.fixture(autouse=True)
def _windows_put_back(request):
    """a case that fails half-way still puts its windows back: the cases behind it start from a clean arena"""
    yield
    if "arena" in request.fixturenames:
        request.getfixturevalue("arena").restore()


def _done(arena):
    """the end of every case that ran on the arena"""
    arena.restore()
    if arena.reduced:
        pytest.skip("ran on the reduced arena of 2^32 + 2^28 bytes: the boundaries 3 * 2^31 and 2^33 need the full one")


def _claims(census, names):
    missing = [n for n in names if census.get(n, 0) < 1]
    assert not missing, ("kernels this case is meant to reach were not launched", missing, sorted(census))


def _rates(g):
    return [g[4] if s % 2 == 0 else RATE2[g] for s in range(S)]


def _enc_kernels(g, T, how):
    """the placed kernels of an encoder case by the launch code (lc3_runtime.hip: enc_launch, enc_one_wave, enc_pipelined, launch_resample)"""
    big = "_big" if g is G96 else ""
    if how == "ragged":
        return ("lc3_enc_resample_plc_kernel_rag", "lc3_enc_front4_kernel_plc_rag", "lc3_pcm_placed_mark_kernel")
    if how == "rates":                                                     # per-frame bitrates: the one-wave kernel at every length
        return ("lc3_encode_kernel%s_var_plc" % big, "lc3_pcm_placed_mark_kernel")
    if T <= 8:
        return ("lc3_encode_kernel%s_plc" % big,)
    front = {G48: "lc3_enc_front4_kernel_plc", G48ST: "lc3_enc_front4_kernel_plc", G16S: "lc3_enc_front_kernel_plc", G96: "lc3_enc_front_kernel_big_plc",
             G48_5: "lc3_enc_frontm_kernel_plc"}
    return ("lc3_enc_resample_plc_kernel",) + ((front[g],) if g in front else ())      # (44.1 kHz: the resampler is what the case is for)


def _dec_kernels(g, ragged):
    big = "_big" if g is G96 else ""
    return ("lc3_dec_synth_kernel%s_rag_plc" % big,) if ragged else ("lc3_dec_synth_kernel%s_plc" % big, "lc3_pcm_placed_mark_kernel")


def _plan(arena, eb, g, T, seed, counts=None):
    """the planner's offsets for the geometry on this arena; counts [CALLS, S]: the frames behind a stream's count are absent and get INT64_MAX"""
    N = int((48000 if g[0] == 44100 else g[0]) * g[1] / 1000)
    offs, cap, aliases = wo.plan(eb, g[3], N, S, T, calls=CALLS, arena=arena.size, seed=seed)
    offs = offs.copy()
    if counts is not None:
        for k in range(CALLS):
            for s in range(S):
                offs[k, s, counts[k][s]:] = I64_MAX
    return offs, cap, aliases


# ---- encoder ----------------------------------------------------------------------------------------------------------------------------------------

def _enc_calls(dev, g, T, how, pcm_of, words=None, counts=None):
    """CALLS consecutive calls of T frames on one batch -> (bytes [S, CALLS T, stride], num_bytes, flags [S, CALLS T] or None).  pcm_of(bat, k) -> (device
    pointer, format word) after setting or clearing the placement.  how: device (encode_device), rates (encode_device_rates, per-frame bitrates words[k]),
    ragged (set_frame_counts(counts[k]) + encode_device_rates, per-frame bandwidths words[k])"""
    fs, ms, hr, ch, rate = g
    bat = _amd().Batch(S, fs, ch, ms, hr, _rates(g), device=0)
    try:
        stride, outs, nbs, fls = bat.stride, [], [], []
        for k in range(CALLS):
            d_pcm, word = pcm_of(bat, k)
            d_out = dev.zeros(S * T * stride)
            if how == "device":
                bat.encode_device(d_pcm, word, T, d_out, stride, sync=True)
            else:
                d_nb, d_fl, d_w = dev.put(np.full((S, T), -1, np.int32)), dev.put(np.full((S, T), 0xEE, np.uint8)), dev.put(words[k].astype(np.int32))
                if how == "ragged":
                    bat.set_frame_counts(dev.put(np.asarray(counts[k], np.int32)))
                bat.encode_device_rates(d_pcm, word, T, d_out, stride, d_bitrates_ptr=d_w if how == "rates" else None,
                                        d_bandwidths_ptr=d_w if how == "ragged" else None, d_num_bytes_ptr=d_nb, d_flags_ptr=d_fl, sync=True)
                nbs.append(dev.get(d_nb, (S, T), np.int32))
                fls.append(dev.get(d_fl, (S, T), np.uint8))
            outs.append(dev.get(d_out, (S, T, stride), np.uint8))
        cat = lambda x: np.concatenate(x, axis=1) if x else None
        return cat(outs), cat(nbs), cat(fls)
    finally:
        bat.close()


def _dense_feed(dev, xb, ty, T):
    def feed(bat, k):
        bat.set_pcm_placement(None)
        return dev.put(xb[:, k * T:(k + 1) * T]), ty
    return feed


def _placed_feed(dev, arena, xb, ty, lay, T, offs, cap, counts=None):
    eb = EB[ty]
    def feed(bat, k):
        arena.restore()                                                   # the frames of the call before this one
        for s in range(S):
            for t in range(T if counts is None else counts[k][s]):
                arena.write(int(offs[k, s, t]) * eb, _frame_flat(xb[s, k * T + t], lay))
        bat.set_pcm_placement(dev.put(offs[k]), cap)
        return arena.base, ty | lay
    return feed


@functools.lru_cache(maxsize=None)
def _oracle16(g, T, seed):
    """the CPU oracle on the 16-bit input of a geometry, one encoder per stream at the stream's rate -> [S][CALLS T, nbytes]"""
    fs, ms, hr, ch, rate = g
    _, nat = _input(16, g, CALLS * T, seed, streams=S)
    out = []
    for s, r in enumerate(_rates(g)):
        o = Oracle(fs, ch, ms, hr, r, portable_math=True)
        out.append(np.stack([o.encode(nat[s, t], 16) for t in range(nat.shape[1])]))
    return out


def _words(g, T, how, seed):
    rng = np.random.default_rng(seed)
    vals = [g[4], RATE2[g]] if how == "rates" else [0, 8000, 16000]
    return [rng.choice(vals, size=(S, T)) for _ in range(CALLS)]


def _enc_case(dev, arena, g, ty, lay, T, how, seed):
    api = _api()
    xb, nat = _input(ty, g, CALLS * T, seed, streams=S)
    counts = [[(12, 5, 0, 12, 5, 12)[(s + k) % S] for s in range(S)] for k in range(CALLS)] if how == "ragged" else None
    words = _words(g, T, how, seed) if how != "device" else None
    want = _enc_calls(dev, g, T, how, _dense_feed(dev, xb, ty, T), words, counts)
    offs, cap, _ = _plan(arena, EB[ty], g, T, seed, counts)
    assert cap * EB[ty] > 2 ** 32 and not api.plan_placed(ty, g[3], xb.shape[3], offs[offs != I64_MAX], cap).any()
    with api.launch_census() as census:
        got = _enc_calls(dev, g, T, how, _placed_feed(dev, arena, xb, ty, lay, T, offs, cap, counts), words, counts)
    _claims(census, _enc_kernels(g, T, how))
    _same(got[0], want[0], "the dense call")
    if how != "device":
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and not (got[2] & ENC_FL_PCM_PLACE).any()
        if how == "ragged":
            absent = np.concatenate([np.arange(T)[None, :] >= np.asarray(c)[:, None] for c in counts], axis=1)
            assert np.array_equal((got[2] & api.ENC_FL_ABSENT) != 0, absent) and absent.any() and not absent.all()
    if ty == 16 and how == "device":
        o = _oracle16(g, T, seed)
        for s in range(S):
            assert np.array_equal(got[0][s, :, :o[s].shape[1]], o[s]), ("oracle", s)


@pytest.mark.parametrize("g,ty,lay,T", PARAMS)
def test_encoder_reads_placed_pcm_past_4g(dev, arena, g, ty, lay, T):
    _enc_case(dev, arena, g, ty, lay, T, "device", seed=41)
    _done(arena)


@pytest.mark.parametrize("T", [4, 12])
def test_encoder_per_frame_bitrates_past_4g(dev, arena, T):
    _enc_case(dev, arena, G48ST, 16, 0, T, "rates", seed=43)
    _done(arena)


def test_encoder_ragged_past_4g_reads_no_absent_frame(dev, arena):
    """set_frame_counts with counts 0, 5 and 12 of 12: the absent frames' offset is INT64_MAX"""
    _enc_case(dev, arena, G48ST, S24LE, 0, 12, "ragged", seed=45)
    _done(arena)


def test_channel_major_is_refused_at_these_offsets_too(dev, arena):
    """the third layout has no placed form: both calls refuse it before anything runs (the arena stays as it is: the last test)"""
    api = _api()
    g, T = G48ST, 4
    fs, ms, hr, ch, rate = g
    offs, cap, _ = _plan(arena, 2, g, T, seed=47)
    bat, d = _amd().Batch(S, fs, ch, ms, hr, _rates(g), device=0), _amd().DecBatch(S, fs, ch, ms, hr, [160] * S, device=0)
    try:
        bat.set_pcm_placement(dev.put(offs[0]), cap)
        d.set_pcm_placement(dev.put(offs[0]), cap)
        with api.launch_census() as census:
            with pytest.raises(api.LC3Error):
                bat.encode_device(arena.base, 16 | CM, T, dev.zeros(S * T * bat.stride), bat.stride, sync=True)
            with pytest.raises(api.LC3Error):
                d.decode_device(dev.zeros(S * T * 160), 160, T, arena.base, bps=16 | CM, sync=True)
        assert not census, sorted(census)
    finally:
        bat.close()
        d.close()
    _done(arena)


# ---- decoder ----------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _dec_case(g, T, seed=51, rates=None):
    fs, ms, hr, ch, rate = g
    frames, nbytes, bfi = make_dec_case(fs, ms, hr, ch, list(rates) if rates else _rates(g), CALLS * T, seed=seed)
    frames.flags.writeable = bfi.flags.writeable = False
    return frames, tuple(nbytes), bfi


def _dec_calls(dev, g, case, T, ty, place=None, counts=None, packed=None):
    """CALLS consecutive decode_device_sizes calls (packed: decode_device_packed, packed(k) -> (frames pointer, capacity, offsets [S, T])) -> (elements as bytes
    [S, CALLS T, C, N, eb] or None, status [S, CALLS T]).  place(d, k) -> (pcm pointer, format word, after) sets the placement, after() checks the arena"""
    fs, ms, hr, ch, rate = g
    frames, nbytes, bfi = case
    d = _amd().DecBatch(S, fs, ch, ms, hr, list(nbytes), device=0)
    try:
        eb, N, out, sts = EB[ty], d.N, [], []
        nb = np.repeat(np.asarray(nbytes, np.int32)[:, None], T, axis=1)
        for k in range(CALLS):
            fr = np.ascontiguousarray(frames[:, k * T:(k + 1) * T])
            d_st, d_bfi = dev.put(np.full((S, T), 0xEE, np.uint8)), dev.put(bfi[:, k * T:(k + 1) * T])
            if counts is not None:
                d.set_frame_counts(dev.put(np.asarray(counts[k], np.int32)))
            if place is None:
                d_pcm, word, after = dev.put(np.full(S * T * ch * N * eb, CANARY, np.uint8)), ty, None
            else:
                d_pcm, word, after = place(d, k)
            if packed is None:
                d.decode_device_sizes(dev.put(fr), fr.shape[2], T, d_pcm, dev.put(nb), d_bfi, d_st, bps=word, sync=True)
            else:
                d_fr, fcap, fo = packed(k)
                d.decode_device_packed(d_fr, fcap, dev.put(fo), T, d_pcm, dev.put(nb), int(max(nbytes)), d_bfi, d_st, bps=word, sync=True)
            if after is None:
                out.append(dev.get(d_pcm, (S, T, ch, N, eb), np.uint8))
            else:
                after()
            sts.append(dev.get(d_st, (S, T), np.uint8))
        return (np.concatenate(out, axis=1) if out else None), np.concatenate(sts, axis=1)
    finally:
        d.close()


def _check_windows(arena, offs_k, aliases_k, want_k, lay, eb, counts_k=None):
    """after a placed decoder call: every present frame holds the dense call's bytes between guards that hold the canary, every alias window the canary"""
    G = wo.GUARD
    for s in range(S):
        for t in range(offs_k.shape[1] if counts_k is None else counts_k[s]):
            body = _frame_flat(want_k[s, t], lay)
            lo = int(offs_k[s, t]) * eb
            arena.written(lo, body.size)
            win = arena.read(lo - G, body.size + 2 * G)
            assert (win[:G] == CANARY).all() and (win[G + body.size:] == CANARY).all(), ("guard bytes were written", s, t, lo)
            bad = np.flatnonzero(win[G:G + body.size] != body)
            assert bad.size == 0, ("frame", s, t, "at byte", lo, "first differing bytes", bad[:6].tolist())
            for a_lo, a_hi in aliases_k[s][t]:
                assert (arena.read(a_lo, a_hi - a_lo) == CANARY).all(), ("the frame's alias was written", s, t, lo, a_lo)


def _dec_case_run(dev, arena, g, ty, lay, T, seed, counts=None):
    api = _api()
    fs, ms, hr, ch, rate = g
    case = _dec_case(g, T)
    want, wst = _dec_calls(dev, g, case, T, ty, counts=counts)
    eb = EB[ty]
    offs, cap, aliases = _plan(arena, eb, g, T, seed, counts)
    assert cap * eb > 2 ** 32

    def place(d, k):
        d.set_pcm_placement(dev.put(offs[k]), cap)
        def after():
            _check_windows(arena, offs[k], aliases[k], want[:, k * T:(k + 1) * T], lay, eb, counts[k] if counts is not None else None)
            arena.restore()
        return arena.base, ty | lay, after

    with api.launch_census() as census:
        _, st = _dec_calls(dev, g, case, T, ty, place=place, counts=counts)
    _claims(census, _dec_kernels(g, counts is not None))
    assert np.array_equal(st, wst) and not (st & DEC_ST_PCM_PLACE).any()
    if ty == 16 and counts is None:
        o, ost = oracle_decode_streams(case[0], list(case[1]), case[2], fs, ms, hr, ch, bps=16)
        assert np.array_equal(want.view(np.int16)[..., 0], o) and np.array_equal(wst, ost)


@pytest.mark.parametrize("g,ty,lay,T", PARAMS)
def test_decoder_writes_placed_pcm_past_4g(dev, arena, g, ty, lay, T):
    _dec_case_run(dev, arena, g, ty, lay, T, seed=53)
    _done(arena)


@pytest.mark.parametrize("T", [4, 12])
def test_decoder_ragged_past_4g_writes_no_absent_frame(dev, arena, T):
    counts = [[(T, 1, 0, T, T // 2, T)[(s + k) % S] for s in range(S)] for k in range(CALLS)]
    _dec_case_run(dev, arena, G48ST, F32, IL, T, seed=55, counts=counts)
    _done(arena)


# ---- the capacity edge above 2^32 -----------------------------------------------------------------------------------------------------------------------

def _edge_plan(eb, fe, T):
    """capacity C with C * eb = 2^32 + 12345 eb: every frame low, but (1, 1) at C - fe (valid: it ends with the buffer), (2, T - 1) at C - fe + 1 and (3, 0)
    at C (invalid)"""
    cap = 2 ** 32 // eb + 12345
    offs = (np.arange(S * T, dtype=np.int64) * (fe + 300) + 1024).reshape(S, T)
    offs[1, 1], offs[2, T - 1], offs[3, 0] = cap - fe, cap - fe + 1, cap
    inv = np.zeros((S, T), bool)
    inv[2, T - 1] = inv[3, 0] = True
    assert all((not (0 <= int(o) and int(o) + fe <= cap)) == bool(i) for o, i in zip(offs.reshape(-1), inv.reshape(-1)))
    return offs, cap, inv


@pytest.mark.parametrize("T", [4, 12])
@pytest.mark.parametrize("ty", [ULAW, 16])
def test_capacity_edge_above_2_32(dev, arena, ty, T):
    api = _api()
    g, eb = G48, EB[ty]
    fs, ms, hr, ch, rate = g
    xb, nat = _input(ty, g, T, seed=61, streams=S)
    fe = xb.shape[2] * xb.shape[3]
    offs, cap, inv = _edge_plan(eb, fe, T)
    assert cap * eb > 2 ** 32 and np.array_equal(api.plan_placed(ty, ch, xb.shape[3], offs, cap) != 0, inv)
    # encoder: silence for the invalid frames (the sample 0: the 16-bit call on the expanded input), flag 16 on them alone
    z = np.ascontiguousarray(np.where(inv[:, :, None, None], 0, nat).astype(np.int16))
    zb = z.view(np.uint8).reshape(z.shape + (2,))
    words = [np.array([[r] * T for r in _rates(g)], np.int32)]
    run = lambda feed: _enc_one(dev, g, T, feed, words[0])
    want = run(lambda bat: (dev.put(zb), 16))
    def feed(bat):
        for s in range(S):
            for t in range(T):
                if not inv[s, t]:
                    arena.write(int(offs[s, t]) * eb, _frame_flat(xb[s, t], 0))
        bat.set_pcm_placement(dev.put(offs), cap)
        return arena.base, ty
    with api.launch_census() as census:
        got = run(feed)
    _claims(census, _enc_kernels(g, T, "rates"))
    _same(got[0], want[0], "the 16-bit dense call with the invalid frames zeroed")
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], np.where(inv, ENC_FL_PCM_PLACE, 0).astype(np.uint8)) and not want[2].any()
    arena.restore()
    # decoder: nothing written for the invalid frames, status bit 4; the bytes from the valid frame's end on still hold the canary
    case = _dec_case(g, T, seed=63)
    case = (case[0][:, :T], case[1], case[2][:, :T])
    d = _amd().DecBatch(S, fs, ch, ms, hr, list(case[1]), device=0)
    dd = _amd().DecBatch(S, fs, ch, ms, hr, list(case[1]), device=0)
    try:
        nb = dev.put(np.repeat(np.asarray(case[1], np.int32)[:, None], T, axis=1))
        N = d.N
        d_pcm, d_st0, d_st = dev.zeros(S * T * ch * N * eb), dev.zeros(S * T), dev.put(np.full((S, T), 0xEE, np.uint8))
        dd.decode_device_sizes(dev.put(case[0]), case[0].shape[2], T, d_pcm, nb, dev.put(case[2]), d_st0, bps=ty, sync=True)
        wpcm, wst = dev.get(d_pcm, (S, T, ch, N, eb), np.uint8), dev.get(d_st0, (S, T), np.uint8)
        d.set_pcm_placement(dev.put(offs), cap)
        with api.launch_census() as census:
            d.decode_device_sizes(dev.put(case[0]), case[0].shape[2], T, arena.base, nb, dev.put(case[2]), d_st, bps=ty, sync=True)
        _claims(census, _dec_kernels(g, False))
        for s in range(S):
            for t in range(T):
                if inv[s, t]:
                    continue
                _check_windows_one(arena, int(offs[s, t]) * eb, _frame_flat(wpcm[s, t], 0), (s, t))
        tail = arena.read(cap * eb, (fe + 1) * eb + wo.GUARD)
        assert (tail == CANARY).all(), "bytes at or past the capacity were written"
        assert np.array_equal(dev.get(d_st, (S, T), np.uint8), wst | np.where(inv, DEC_ST_PCM_PLACE, 0).astype(np.uint8))
    finally:
        d.close()
        dd.close()
    _done(arena)


def _enc_one(dev, g, T, feed, rates):
    """one encode_device_rates call with constant per-frame bitrates (the call that reports flags) -> (bytes, num_bytes, flags)"""
    fs, ms, hr, ch, rate = g
    bat = _amd().Batch(S, fs, ch, ms, hr, _rates(g), device=0)
    try:
        d_pcm, word = feed(bat)
        stride = bat.stride
        d_out, d_nb, d_fl = dev.zeros(S * T * stride), dev.put(np.full((S, T), -1, np.int32)), dev.put(np.full((S, T), 0xEE, np.uint8))
        bat.encode_device_rates(d_pcm, word, T, d_out, stride, d_bitrates_ptr=dev.put(rates.astype(np.int32)), d_num_bytes_ptr=d_nb, d_flags_ptr=d_fl, sync=True)
        return dev.get(d_out, (S, T, stride), np.uint8), dev.get(d_nb, (S, T), np.int32), dev.get(d_fl, (S, T), np.uint8)
    finally:
        bat.close()


def _check_windows_one(arena, lo, body, who):
    G = wo.GUARD
    arena.written(lo, body.size)
    win = arena.read(lo - G, body.size + 2 * G)
    assert (win[:G] == CANARY).all() and (win[G + body.size:] == CANARY).all(), ("guard bytes were written", who, lo)
    assert np.array_equal(win[G:G + body.size], body), ("frame", who, "at byte", lo)


# ---- out of range in 64 bits, in range in 32 (small arenas: never skipped) ---------------------------------------------------------------------------------

def _small_plan(fe, T):
    """dense offsets with gaps in a small buffer; mask: the frames whose offset is replaced by its out-of-range alias"""
    valid = (np.arange(S * T, dtype=np.int64) * (fe + 64) + 32).reshape(S, T)
    cap = int(valid.max()) + fe + 32
    mask = np.array([[(s * 3 + t) % 4 == 1 for t in range(T)] for s in range(S)])
    bad = wo.alias_invalid(valid, cap)                                    # [CALLS, S, T]: call k uses the k-th kind
    assert bad.shape[0] == CALLS
    return valid, cap, mask, np.where(mask[None], bad, valid[None])


@pytest.mark.parametrize("T", [4, 12])
@pytest.mark.parametrize("ty,lay", [(16, 0), (F32, IL), (ULAW, 0)])
def test_encoder_offsets_in_range_only_when_narrowed(dev, ty, lay, T):
    """the frame such an offset aliases holds other PCM; the encoder takes silence, flags the frame and reads nothing of it"""
    api = _api()
    g, eb = G48ST, EB[ty]
    fs, ms, hr, ch, rate = g
    xb, nat = _input(ty, g, CALLS * T, seed=71, streams=S)
    decoy, _ = _input(ty, g, CALLS * T, seed=72, streams=S)
    fe = xb.shape[2] * xb.shape[3]
    valid, cap, mask, offs = _small_plan(fe, T)
    inv = np.concatenate([mask] * CALLS, axis=1)
    for k in range(CALLS):
        assert np.array_equal(api.plan_placed(ty | lay, ch, xb.shape[3], offs[k], cap) != 0, mask)
    words = [np.array([[r] * T for r in _rates(g)], np.int32)] * CALLS
    zty = F32 if ty == F32 else 16                                        # silence is the sample 0: for G.711 the 16-bit call on the expanded input
    z = np.ascontiguousarray(np.where(inv[:, :, None, None], 0, nat).astype(np.float32 if ty == F32 else np.int16))
    zb = z.view(np.uint8).reshape(z.shape + (z.dtype.itemsize,))
    want = _enc_calls(dev, g, T, "rates", _dense_feed(dev, zb, zty, T), words)
    def feed(bat, k):
        image = np.full(cap * eb + 64, 0x5A, np.uint8)
        for s in range(S):
            for t in range(T):
                src = decoy if mask[s, t] else xb
                image[int(valid[s, t]) * eb:(int(valid[s, t]) + fe) * eb] = _frame_flat(src[s, k * T + t], lay)
        bat.set_pcm_placement(dev.put(offs[k]), cap)
        return dev.put(image), ty | lay
    with api.launch_census() as census:
        got = _enc_calls(dev, g, T, "rates", feed, words)
    _claims(census, _enc_kernels(g, T, "rates"))
    _same(got[0], want[0], "the dense call with those frames zeroed")
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], np.where(inv, ENC_FL_PCM_PLACE, 0).astype(np.uint8))


@pytest.mark.parametrize("T", [4, 12])
@pytest.mark.parametrize("ty,lay", [(16, 0), (F32, IL), (S24LE, 0)])
def test_decoder_offsets_in_range_only_when_narrowed(dev, ty, lay, T):
    """nothing is written for such a frame, least of all at the valid offset it aliases; status bit 4"""
    api = _api()
    g, eb = G48ST, EB[ty]
    fs, ms, hr, ch, rate = g
    case = _dec_case(g, T)
    want, wst = _dec_calls(dev, g, case, T, ty)
    N = want.shape[3]
    fe = ch * N
    valid, cap, mask, offs = _small_plan(fe, T)

    def place(d, k):
        assert np.array_equal(api.plan_placed(ty | lay, ch, N, offs[k], cap) != 0, mask)
        d_buf = dev.put(np.full(cap * eb + 64, CANARY, np.uint8))
        d.set_pcm_placement(dev.put(offs[k]), cap)
        def after():
            image = np.full(cap * eb + 64, CANARY, np.uint8)
            for s in range(S):
                for t in range(T):
                    if not mask[s, t]:
                        image[int(valid[s, t]) * eb:(int(valid[s, t]) + fe) * eb] = _frame_flat(want[s, k * T + t], lay)
            bad = np.flatnonzero(dev.get(d_buf, (cap * eb + 64,), np.uint8) != image)
            assert bad.size == 0, ("call", k, "first differing bytes", bad[:6].tolist())
        return d_buf, ty | lay, after

    with api.launch_census() as census:
        _, st = _dec_calls(dev, g, case, T, ty, place=place)
    _claims(census, _dec_kernels(g, False))
    assert np.array_equal(st, wst | np.where(np.concatenate([mask] * CALLS, axis=1), DEC_ST_PCM_PLACE, 0).astype(np.uint8))


@pytest.mark.parametrize("T", [4, 12])
def test_packed_frames_and_probe_items_in_range_only_when_narrowed(dev, T):
    """decode_packed with a small frames_capacity: such a frame is invalid (status bit 2) and concealed, not decoded from the frame it aliases; the probe gives it
    the invalid record"""
    api = _api()
    g = G48
    fs, ms, hr, ch, rate = g
    case = _dec_case(g, T)
    frames, nbytes, bfi = case
    N = int(fs * ms / 1000)
    size = np.asarray(nbytes)
    valid = (np.arange(S * T, dtype=np.int64) * (int(size.max()) + 5) + 3).reshape(S, T)
    cap = int(valid.max()) + int(size.max()) + 1
    mask = np.array([[(s * 3 + t) % 4 == 1 for t in range(T)] for s in range(S)])
    offs = np.where(mask[None], wo.alias_invalid(valid, cap), valid[None])
    nb = np.repeat(size.astype(np.int32)[:, None], T, axis=1)
    # the slotted call with those frames flagged invalid: the same outcome by the header's rule (concealed, status bit 2); none of them is lost as well
    bfi, bfi2 = bfi.copy(), bfi.copy()
    bfi[np.concatenate([mask] * CALLS, axis=1)] = 0
    bfi2[np.concatenate([mask] * CALLS, axis=1)] = 2
    case = (frames, nbytes, bfi)
    want, wst = _dec_calls(dev, g, (frames, nbytes, bfi2), T, 16)
    bufs = []
    def packed(k):
        rc, eff, lost, inv, end, mx = api.dec_plan_packed_lenient(fs, ch, ms, hr, size.astype(np.int32), nb, offs[k], cap, int(size.max()), bfi[:, k * T:(k + 1) * T])
        assert rc == 0 and np.array_equal(inv != 0, mask)
        buf = np.full(cap + 8, 0x3C, np.uint8)
        for s in range(S):
            for t in range(T):
                buf[int(valid[s, t]):int(valid[s, t]) + size[s]] = frames[s, k * T + t, :size[s]]
        bufs.append((dev.put(buf), buf))
        return bufs[-1][0], cap, offs[k]
    with api.launch_census() as census:
        got, st = _dec_calls(dev, g, case, T, 16, packed=packed)
    _claims(census, ("lc3_dec_plan_packed_kernel",))
    assert np.array_equal(got, want) and np.array_equal(st, wst)
    assert np.array_equal((st & 2) != 0, np.concatenate([mask] * CALLS, axis=1) | ((wst & 2) != 0)) and ((st & 2) != 0).any()
    # the probe on the last call's items
    d = _amd().DecBatch(1, fs, ch, ms, hr, None, device=0)
    try:
        n, k = S * T, CALLS - 1
        for depth in (api.PROBE_SIDE, api.PROBE_FULL):
            res = {}
            for name, o in (("valid", valid), ("bad", offs[k])):
                d_info = dev.put(np.full((n, ch, api.FRAME_INFO_WORDS), 0x5A5A5A5A, np.int32))
                d.probe_device(bufs[k][0], cap, dev.put(o), dev.put(nb), int(size.max()), n, d_info, depth, sync=True)
                res[name] = dev.get(d_info, (n, ch, api.FRAME_INFO_WORDS), np.int32).reshape(S, T, ch, -1)
            assert (res["bad"][mask][:, :, 0] == 3).all() and not res["bad"][mask][:, :, 1:].any(), "not the invalid record (concealed | invalid, nothing else)"
            assert np.array_equal(res["bad"][~mask], res["valid"][~mask]) and (res["valid"][..., 0] & 2 == 0).all()
            if depth == api.PROBE_SIDE:
                for s in range(S):
                    for t in range(T):
                        side = api.frame_info_side(fs, ch, ms, hr, frames[s, k * T + t, :size[s]])
                        assert np.array_equal(res["valid"][s, t], side), (s, t)
    finally:
        d.close()


# ---- packed frames past 4 GiB -------------------------------------------------------------------------------------------------------------------------------

PACKED = [pytest.param(G48, (64000, 96000), "lc3_dec_parse_kernel_var_pk", id="mono-lds"), pytest.param(G48, (64000, 104000), "lc3_dec_parse_kernel_g_var_pk", id="mono-global"),
          pytest.param(G48ST, (128000, 192000), "lc3_dec_parse_kernel_var_pk", id="stereo-lds"),
          pytest.param(G48ST, (128000, 208000), "lc3_dec_parse_kernel_g_var_pk", id="stereo-global")]


def _packed_case(dev, arena, g, rates, parser, T, counts=None):
    api = _api()
    fs, ms, hr, ch, rate = g
    case = _dec_case(g, T, seed=81, rates=tuple(rates[s % 2] for s in range(S)))
    frames, nbytes, bfi = case
    size = np.asarray(nbytes)
    assert (size.max() > 128 * ch) == ("_g_" in parser)
    want, wst = _dec_calls(dev, g, case, T, 16, counts=counts)
    sizes = np.broadcast_to(size[None, :, None], (CALLS, S, T))
    offs, cap, _ = wo.plan_bytes(sizes, calls=CALLS, arena=arena.size, seed=83 + T)
    assert cap == arena.size
    def packed(k):
        arena.restore()
        for s in range(S):
            for t in range(T):
                arena.write(int(offs[k, s, t]), frames[s, k * T + t, :size[s]])
        return arena.base, cap, offs[k]
    with api.launch_census() as census:
        got, st = _dec_calls(dev, g, case, T, 16, counts=counts, packed=packed)
    if counts is None:
        _claims(census, (parser, "lc3_dec_plan_packed_kernel"))
    else:
        _claims(census, ("lc3_dec_plan_packed_kernel_rag",))
        assert any(n.startswith("lc3_dec_parse_kernel") for n in census), sorted(census)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=(2, 3, 4)))[:6].tolist()
    assert np.array_equal(st, wst)
    return case, offs, size


@pytest.mark.parametrize("T", [4, 12])
@pytest.mark.parametrize("g,rates,parser", PACKED)
def test_packed_frames_past_4g(dev, arena, g, rates, parser, T):
    api = _api()
    fs, ms, hr, ch, rate = g
    (frames, nbytes, bfi), offs, size = _packed_case(dev, arena, g, rates, parser, T)
    # the probe on the last call's items, still in the arena, against the same frames at low offsets of a small buffer: word for word
    k, n, mx = CALLS - 1, S * T, int(size.max())
    low = (np.arange(n, dtype=np.int64) * (mx + 3) + 1).reshape(S, T)
    buf = np.full(n * (mx + 3) + 8, 0x3C, np.uint8)
    for s in range(S):
        for t in range(T):
            buf[int(low[s, t]):int(low[s, t]) + size[s]] = frames[s, k * T + t, :size[s]]
    nb = dev.put(np.repeat(size.astype(np.int32)[:, None], T, axis=1))
    d = _amd().DecBatch(1, fs, ch, ms, hr, None, device=0)
    try:
        for depth in (api.PROBE_SIDE, api.PROBE_FULL):
            res = []
            for ptr, fcap, o in ((dev.put(buf), buf.size, low), (arena.base, arena.size, offs[k])):
                d_info = dev.put(np.full((n, ch, api.FRAME_INFO_WORDS), 0x5A5A5A5A, np.int32))
                d.probe_device(ptr, fcap, dev.put(o), nb, mx, n, d_info, depth, sync=True)
                res.append(dev.get(d_info, (n, ch, api.FRAME_INFO_WORDS), np.int32))
            assert np.array_equal(res[1], res[0]), ("depth", depth, np.argwhere((res[1] != res[0]).any(axis=(1, 2)))[:6].ravel().tolist())
            assert (res[0][:, :, 0] & 2 == 0).all() and (res[0][:, :, 0] == 0).any()
    finally:
        d.close()
    _done(arena)


def test_packed_frames_past_4g_ragged(dev, arena):
    T = 12
    counts = [[(T, 5, 0, T, 1, T)[(s + k) % S] for s in range(S)] for k in range(CALLS)]
    _packed_case(dev, arena, G48ST, (128000, 192000), "lc3_dec_parse_kernel_var_pk", T, counts=counts)
    _done(arena)


# ---- one HIP stream, no host wait, everything high ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", ["48k_10_128B", "48k_10_stereo_161B"])
def test_receive_path_and_re_encode_on_one_stream_past_4g(dev, arena, geom):
    """probe_device -> ingest_device -> set_frame_counts + decode_device_packed into placed PCM -> an encoder batch that reads the placed PCM back, queued on one
    HIP stream with one wait at the end.  The packets of test_gpu_ingest's receive buffer (duplicates, refused copies, a gap, late and early items) lie at planned
    byte offsets on both sides of every boundary (class 0), the PCM frames start on the boundaries (class 3)."""
    import hostile_frames as hf
    from test_gpu_ingest import _oracle, _scenario
    api = _api()
    fs, ms, hr, ch, _ = hf.GEOMS[geom]
    sc = _scenario(geom)
    B, T, N, n = len(sc["counts"]), hf.T, hf.frame_len(fs, ms), len(sc["stream"])
    # the packets: one planned frame per item (an empty item plans one byte and writes none)
    cols = -(-n // S)
    psz = np.full(S * cols, 1, np.int64)
    psz[:n] = np.maximum(sc["num_bytes"], 1)
    poffs = wo.plan_bytes(psz.reshape(1, S, cols), calls=1, arena=arena.size, seed=91)[0].reshape(-1)[:n]
    assert poffs.max() > 2 ** 32 and poffs.min() < 2 ** 31
    for i in range(n):
        z = int(sc["num_bytes"][i])
        if z:
            arena.write(int(poffs[i]), sc["buf"][int(sc["offsets"][i]):int(sc["offsets"][i]) + z])
    # the PCM: class 3 of every boundary, int16
    plo, pcap, aliases = wo.plan(2, ch, N, B, T, calls=CALLS, arena=arena.size, seed=93)
    plo, aliases = plo[3], aliases[3]
    fe = ch * N
    for i in range(n):                                                     # the two plans share the arena: they must not meet
        for e in plo.reshape(-1):
            assert int(poffs[i]) + int(psz[i]) <= int(e) * 2 or (int(e) + fe) * 2 + wo.GUARD <= int(poffs[i])
    assert int(plo.max()) * 2 >= wo.bounds(arena.size)[-1]
    rates = [64000 * ch] * B
    d = _amd().DecBatch(B, fs, ch, ms, hr, None, device=0)
    enc = _amd().Batch(B, fs, ch, ms, hr, rates, device=0)
    try:
        d_stream, d_seq, d_off, d_nb = dev.put(sc["stream"]), dev.put(sc["seq"]), dev.put(poffs), dev.put(sc["num_bytes"])
        d_base, d_floor = dev.put(sc["base"]), dev.put(sc["floor"])
        d_info = dev.put(np.zeros((n, ch, api.FRAME_INFO_WORDS), np.int32))
        d_oo, d_onb, d_ci = dev.put(np.full((B, T), -7, np.int64)), dev.put(np.full((B, T), -7, np.int32)), dev.put(np.full((B, T), -7, np.int32))
        d_counts, d_next, d_stats, d_ist = dev.put(np.full(B, -7, np.int32)), dev.put(np.full(B, -7, np.int32)), dev.put(np.full((B, 4), -7, np.int32)), dev.put(np.full(n, 0xEE, np.uint8))
        d_st, d_plo = dev.put(np.full((B, T), 0xEE, np.uint8)), dev.put(plo)
        d_out = dev.zeros(B * T * enc.stride)
        dev.sync()
        s1 = dev.stream()
        with api.launch_census() as census:
            d.probe_device(arena.base, arena.size, d_off, d_nb, sc["size"], n, d_info, api.PROBE_FULL, s1, sync=False)
            d.ingest_device(n, d_stream, d_seq, d_off, d_nb, d_base, T, d_oo, d_onb, d_ci, d_counts, 16, d_info, d_floor, d_next, d_stats, d_ist, s1, sync=False)
            d.set_frame_counts(d_counts)
            d.set_pcm_placement(d_plo, pcap)
            d.decode_device_packed(arena.base, arena.size, d_oo, T, arena.base, d_onb, sc["size"], None, d_st, 16, s1, sync=False)
            enc.set_pcm_placement(d_plo, pcap)
            enc.encode_device(arena.base, 16, T, d_out, enc.stride, hip_stream=s1, sync=False)
            dev.stream_sync(s1)
        _claims(census, ("lc3_dec_plan_packed_kernel_rag", "lc3_dec_synth_kernel_rag_plc", "lc3_enc_resample_plc_kernel", "lc3_enc_front4_kernel_plc"))
        # the tables: the host plan on the probe's records, all 64 bits of every offset
        info = dev.get(d_info, (n, ch, api.FRAME_INFO_WORDS), np.int32)
        plan = api.plan_ingest(B, ch, sc["stream"], sc["seq"], poffs, sc["num_bytes"], sc["base"], T, 16, info, sc["floor"])
        oo = dev.get(d_oo, (B, T), np.int64)
        assert np.array_equal(oo, plan["offsets"]) and oo.max() > 2 ** 32
        assert np.array_equal(dev.get(d_onb, (B, T), np.int32), plan["num_bytes"]) and np.array_equal(dev.get(d_onb, (B, T), np.int32), sc["sizes"])
        assert np.array_equal(dev.get(d_counts, (B,), np.int32), sc["counts"]) and np.array_equal(dev.get(d_ci, (B, T), np.int32), plan["cell_item"])
        assert np.array_equal(dev.get(d_ist, (n,), np.uint8), plan["item_status"])
        # the PCM: the oracle's decode of the chosen copies, between untouched guards; absent frames and alias windows hold the canary
        st = dev.get(d_st, (B, T), np.uint8)
        pcm = np.full((B, T, ch, N), -23131, np.int16)                 # 0xA5A5: what an absent frame's place holds
        for s, (wp, ws) in enumerate(_oracle(geom)):
            c = int(sc["counts"][s])
            assert np.array_equal(st[s, :c], ws) and (st[s, c:] == api.DEC_ST_ABSENT).all(), (s, st[s].tolist())
            pcm[s, :c] = wp
            for t in range(T):
                lo = int(plo[s, t]) * 2
                if t < c:                                                 # (a packet of class 0 ends where this frame starts: the packets are compared below)
                    body = np.ascontiguousarray(wp[t]).view(np.uint8).reshape(-1)
                    arena.written(lo, body.size)
                    win = arena.read(lo, body.size + wo.GUARD)
                    assert np.array_equal(win[:body.size], body), ("frame", s, t, "at byte", lo)
                    assert (win[body.size:] == CANARY).all(), ("guard bytes were written", s, t)
                else:
                    assert (arena.read(lo - wo.GUARD, fe * 2 + 2 * wo.GUARD) == CANARY).all(), ("an absent frame was written", s, t)
                for a_lo, a_hi in aliases[s][t]:
                    assert (arena.read(a_lo, a_hi - a_lo) == CANARY).all(), ("alias written", s, t)
        for i in range(n):                                                 # the decoder wrote into no packet
            z = int(sc["num_bytes"][i])
            assert np.array_equal(arena.read(int(poffs[i]), z), sc["buf"][int(sc["offsets"][i]):int(sc["offsets"][i]) + z]), ("packet", i)
        # the encoder read those frames: the dense encode of that PCM
        got = dev.get(d_out, (B, T, enc.stride), np.uint8)
        ref = _amd().Batch(B, fs, ch, ms, hr, rates, device=0)
        try:
            d_ref = dev.zeros(B * T * ref.stride)
            ref.encode_device(dev.put(pcm), 16, T, d_ref, ref.stride, sync=True)
            _same(got, dev.get(d_ref, (B, T, ref.stride), np.uint8), "the dense encode of the decoded PCM")
        finally:
            ref.close()
    finally:
        d.close()
        enc.close()
    _done(arena)


# ---- out_capacity is 64 bits ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("T", [4, 12])
def test_packed_output_capacity_is_64_bits(dev, T, order):
    """out_capacity = 2^32 + 10 cuts nothing (the offsets are the library's own scan from 0: the buffer holds the frames and no more); out_capacity = 10 cuts what
    api.plan_packed says.  A capacity narrowed to 32 bits would make the two calls alike."""
    api = _api()
    g = G48
    fs, ms, hr, ch, rate = g
    xb, _ = _input(16, g, T, seed=95, streams=S)
    def run(cap, size):
        bat = _amd().Batch(S, fs, ch, ms, hr, _rates(g), device=0)
        try:
            d_out, d_off, d_tot = dev.put(np.full(size, CANARY, np.uint8)), dev.put(np.full((S, T), -9, np.int64)), dev.put(np.full(1, -9, np.int64))
            d_nb, d_fl = dev.put(np.zeros((S, T), np.int32)), dev.put(np.full((S, T), 0xEE, np.uint8))
            with api.launch_census() as census:
                bat.encode_device_packed(dev.put(xb), 16, T, d_out, cap, order, d_offsets_ptr=d_off, d_total_ptr=d_tot, d_num_bytes_ptr=d_nb, d_flags_ptr=d_fl,
                                         sync=True)
            _claims(census, ("lc3_pack_offsets_kernel", "lc3_encode_kernel_pk" if T <= 8 else "lc3_enc_pack_kernel_pk"))
            return (dev.get(d_out, (size,), np.uint8), dev.get(d_off, (S, T), np.int64), int(dev.get(d_tot, (1,), np.int64)[0]), dev.get(d_nb, (S, T), np.int32),
                    dev.get(d_fl, (S, T), np.uint8))
        finally:
            bat.close()
    size = S * T * 400
    big, small = run(2 ** 32 + 10, size), run(10, size)
    total = big[2]
    exact = run(total, size)                                              # the exact total as the capacity
    assert not exact[4].any() and (exact[0][total:] == CANARY).all() and exact[2] == total
    rc, offs, tot, ovf = api.plan_packed(big[3], order, 10)
    assert rc == 0 and total == tot and np.array_equal(big[1], offs) and np.array_equal(small[1], offs) and np.array_equal(small[3], big[3]) and small[2] == total
    assert not big[4].any(), "a frame below 2^32 + 10 bytes was cut or flagged"
    assert np.array_equal(big[0], exact[0])
    assert np.array_equal(small[4], ovf) and ovf.any()
    image = np.full(size, CANARY, np.uint8)                               # what fits 10 bytes by the plan is there, nothing else is written
    for s in range(S):
        for t in range(T):
            if not ovf[s, t]:
                image[int(offs[s, t]):int(offs[s, t]) + int(big[3][s, t])] = exact[0][int(offs[s, t]):int(offs[s, t]) + int(big[3][s, t])]
    assert np.array_equal(small[0], image)


# ---- last: nothing else in the arena was written ---------------------------------------------------------------------------------------------------------------

def test_the_rest_of_the_arena_still_holds_the_canary(arena):
    """every earlier test has put its windows back: the whole arena, read back in pieces of 64 MiB through one pinned buffer, is 0xA5.  The one test that moves
    gigabytes; it prints its own time and the module's."""
    hip, piece = arena.hip, 1 << 26
    assert not arena.dirty
    p = C.c_void_p()
    assert hip.hipHostMalloc(C.byref(p), C.c_size_t(piece), C.c_uint(0)) == 0
    try:
        words = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), (piece // 8,))
        t0 = time.perf_counter()
        for lo in range(0, arena.size, piece):
            n = min(piece, arena.size - lo)
            assert n % 8 == 0 and hip.hipMemcpy(p, C.c_void_p(arena.base + lo), C.c_size_t(n), C.c_int(2)) == 0
            bad = np.flatnonzero(words[:n // 8] != 0xA5A5A5A5A5A5A5A5)
            assert bad.size == 0, ("the arena was written outside the tests' windows: first words", [lo + 8 * int(b) for b in bad[:6]])
        t1 = time.perf_counter()
    finally:
        hip.hipHostFree(p)
    print("wide offsets: arena %d bytes (%s), sweep %.2f s, module %.1f s" % (arena.size, "reduced" if arena.reduced else "full", t1 - t0, t1 - TIMES["start"]))
    _done(arena)
