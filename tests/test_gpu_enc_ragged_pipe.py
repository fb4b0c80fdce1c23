"""GPU tests of ragged encode calls on the pipelined kernels (include/lc3plus_batch.h: lc3plus_enc_batch_set_frame_counts; lc3_runtime.hip: enc_launch): a
ragged call of more than 8 frames without per-frame bitrates in the standard layout runs the _rag form of every step of the pipeline.  The rule of a ragged
call is unchanged, so the helpers of test_gpu_enc_ragged.py - sentinels everywhere, spoiling values in every absent entry - and the CPU oracle fed each stream's
frames densely remain the specification.  Every comparison is equality.

Schedule: calls of 20 frames - without the input-ready promise two runs of ten - with counts from {0, 1, 3, 9, 10, 11, 14, 20}: 1 and 3 cut a four-frame front
group, 9 / 10 / 11 straddle the run boundary, 14 ends inside the second run.  Every value occurs, every call holds a 0 and a 20, one stream is idle for two
consecutive calls, stream 0 has count 0 in the first call of a fresh batch, and every stream has 41 frames in all, so that a dense twin batch ends where it does."""
import functools

import numpy as np
import pytest

from lc3_harness import Oracle
from test_gpu_dec_varsize_device import _Hip
from test_gpu_enc_ragged import ABSENT, CAP, PLACE, _amd, _garbage_words, _plan, _ragged, _same_frames
from test_gpu_enc_rates_device import OracleStreams, SENT, check_frames, nbytes_of, run_calls, spoil_bws
from test_gpu_enc_varbw import bw_values
from test_gpu_enc_varrate import make_pcm, rate_plan
from test_gpu_pcm_placed import _enc_state_rows

pytestmark = pytest.mark.gpu
NF, T_TOTAL = 20, 41
VALUES = (0, 1, 3, 9, 10, 11, 14, 20)
SCHED = {5: np.array([[0, 10, 20, 9, 14], [20, 11, 0, 1, 10], [1, 20, 20, 0, 3], [0, 0, 0, 20, 0], [20, 0, 1, 11, 14]], np.int32),
         4: np.array([[0, 20, 14, 1], [20, 0, 3, 9], [1, 0, 10, 20], [20, 1, 0, 11], [0, 20, 14, 0]], np.int32)}
# geometry -> fs, frame_ms, hrmode, channels, rates, streams
GEOMS = {
    "48k_mono": (48000, 10.0, 0, 1, [40000, 64000, 96000, 128000, 272000], 5),       # lc3_enc_front4_kernel; an odd number of channel-streams
    "48k_stereo": (48000, 10.0, 0, 2, [128800, 160800, 200800, 96000], 4),           # a count is per stream, the two channels share it
    "16k_2p5": (16000, 2.5, 0, 1, [64000, 80000, 128000], 4),                        # lc3_enc_frontm_kernel, the short-frame front
    "32k_10": (32000, 10.0, 0, 1, [32000, 64000, 96000, 128000], 4),                 # N = 320: lc3_enc_front_kernel, the front for every frame length
    "48k_hr": (48000, 10.0, 1, 1, [128000, 256000, 400000, 500000], 4),              # high resolution in the standard layout: no bandwidths, so packed without words only
}


def test_the_schedule_is_what_the_module_says():
    for B, s in SCHED.items():
        assert s.shape == (5, B) and (s.sum(axis=0) == T_TOTAL).all() and set(s.ravel().tolist()) == set(VALUES)
        assert ((s == 0).any(axis=1) & (s == NF).any(axis=1)).all() and s[0, 0] == 0
        assert ((s[:-1] == 0) & (s[1:] == 0)).any()


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


@functools.lru_cache(maxsize=None)
def _case(geom, mode, T=T_TOTAL, seed=0):
    """The shared case of a geometry and mode (b bandwidths, n no words, r rates), computed once and left unchanged: PCM, the words with refused values among
    them, the rule's sizes and flags over each stream's dense frames, the oracle's frames, the schedule."""
    fs, ms, hr, ch, rates, B = GEOMS[geom] if geom in GEOMS else (96000, 10.0, 1, 1, [149600, 256000, 400000], 4)
    pcm = make_pcm(fs, ms, ch, B, T, seed=160 + seed)
    start = [rates[(b + 1) % len(rates)] for b in range(B)]
    stride = max(nbytes_of(fs, ch, ms, hr, r) for r in rates)
    br = rate_plan(rates, B, T, 170 + seed) if "r" in mode else None
    bw = spoil_bws(rate_plan(bw_values(fs), B, T, 172 + seed), 173 + seed) if "b" in mode else None
    nb, inf, fl, end = _plan(fs, ch, ms, hr, start, [0] * B, br, bw, stride, T)
    want = OracleStreams(fs, ch, ms, hr, start).encode(pcm, br, bw, nb, fl)
    c = dict(geom=geom, mode=mode, fs=fs, ms=ms, hr=hr, ch=ch, B=B, N=pcm.shape[3], T=T, pcm=pcm, br=br, bw=bw, start=start, stride=stride, nb=nb, inf=inf,
             fl=fl, end=end, want=want, sched=SCHED[B])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def _batch(c):
    return _amd().Batch(c["B"], c["fs"], c["ch"], c["ms"], c["hr"], c["start"], device=0)


def _records_words(bat, T):
    """words lc3plus_enc_batch_last_records returns for a call of T frames"""
    w = bat.lib.lc3plus_enc_batch_record_words()
    rec = np.zeros((bat.n_streams * bat.channels, T, w), np.float32)
    return int(bat.lib.lc3plus_enc_batch_last_records(bat.h, rec.ctypes.data, rec.size)), rec


def _ends_like(a, b, c):
    """state and configuration of two batches.  Every word of get_state() is compared but the ones in front of the MDCT memory in its slot, where the frame
    length has any (test_gpu_pcm_placed._enc_state_rows: no kernel reads them, a pipelined call hands them over from LDS it never wrote, and they differ from run
    to run of one and the same dense call); at 48 kHz / 10 ms the memory fills the slot and the comparison is of every byte."""
    B = c["B"]
    g = (c["fs"], c["ms"], c["hr"], c["ch"], 0)
    ra, rb = _enc_state_rows(a.get_state(), g, c["N"], B * c["ch"]), _enc_state_rows(b.get_state(), g, c["N"], B * c["ch"])
    assert np.array_equal(ra, rb), np.argwhere(ra != rb).tolist()[:20]
    if c["N"] == 480:
        assert a.get_state().tobytes() == b.get_state().tobytes()
    assert [a.num_bytes(s) for s in range(B)] == [b.num_bytes(s) for s in range(B)] == c["nb"][:, -1].tolist()
    if not c["hr"]:
        assert [a.bandwidth(s) for s in range(B)] == [b.bandwidth(s) for s in range(B)]


def _dense_twin(dev, c, cuts):
    """the same frames densely on a second batch, checked against the oracle: with bandwidths the call of run_calls, without words encode_device"""
    twin = _batch(c)
    if c["bw"] is not None:
        out, nb, fl = run_calls(dev, twin, c["pcm"], None, c["bw"], cuts, c["stride"])
        assert (fl == c["fl"]).all()
    else:
        B, stride, outs = c["B"], c["stride"], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            d_out = dev.put(np.full((B, b - a, stride), SENT, np.uint8))
            twin.encode_device(dev.put(np.ascontiguousarray(c["pcm"][:, a:b])), 16, b - a, d_out, stride)
            outs.append((d_out, b - a))
        dev.sync()
        out, nb = np.concatenate([dev.get(p, (B, n, stride), np.uint8) for p, n in outs], axis=1), c["nb"]
    check_frames(out, nb, c["want"])
    assert (nb == c["nb"]).all()
    return twin


# ---- 1. parity ----
@pytest.mark.parametrize("geom", [g for g in GEOMS if not GEOMS[g][2]])
def test_sequence_with_bandwidths_vs_oracle_and_dense_twin(dev, geom):
    c = _case(geom, "b")
    bat = _batch(c)
    got, nb, fl = _ragged(dev, bat, c, n_frames=NF)
    assert _records_words(bat, NF)[0] > 0                                   # the last call of the sequence ran the pipeline
    _same_frames(got, c["want"])
    assert (nb == c["nb"]).all() and (fl == c["fl"]).all() and (c["fl"] & 2).any() and (c["fl"] & 4).any()
    twin = _dense_twin(dev, c, (0, NF, T_TOTAL))
    _ends_like(bat, twin, c)
    bat.close(); twin.close()


@pytest.mark.parametrize("geom,mode", [(g, m) for g in GEOMS for m in ("n", "b") if not (GEOMS[g][2] and m == "b")])
def test_packed_sequence_in_both_orders_vs_oracle_and_dense_twin(dev, geom, mode):
    """order 0 with call 1's capacity one byte short of its total - the last present frame in the order is cut (flag bit 3) and still encoded: the frames
    behind it match - order 1 with nothing cut on a second batch, and the dense slotted calls on a third: one state"""
    c = _case(geom, mode)
    a, b = _batch(c), _batch(c)
    got, nb, fl = _ragged(dev, a, c, n_frames=NF, packed=0, cut=1)
    assert _records_words(a, NF)[0] > 0
    assert sum(g is None for row in got for g in row) == 1 and int(((fl & CAP) != 0).sum()) == 1
    _same_frames(got, c["want"], allow_cut=True)
    assert (nb == c["nb"]).all() and ((fl & (0xFF ^ CAP)) == c["fl"]).all()
    got2, nb2, fl2 = _ragged(dev, b, c, n_frames=NF, packed=1)
    _same_frames(got2, c["want"])
    assert (nb2 == c["nb"]).all() and (fl2 == c["fl"]).all()
    twin = _dense_twin(dev, c, (0, NF, T_TOTAL))
    _ends_like(a, b, c); _ends_like(a, twin, c)
    a.close(); b.close(); twin.close()


# ---- 2. the path was taken ----
def test_counts_all_20_leave_the_dense_call_s_records_and_state(dev, monkeypatch):
    c = _case("48k_mono", "b", T=NF, seed=1)
    B = c["B"]
    full = np.full((1, B), NF, np.int32)
    a, b = _batch(c), _batch(c)
    got, nb, fl = _ragged(dev, a, c, sched=full, n_frames=NF)
    out2, nb2, fl2 = run_calls(dev, b, c["pcm"], None, c["bw"], (0, NF), c["stride"])
    _same_frames(got, c["want"]); check_frames(out2, nb2, c["want"])
    assert (nb == nb2).all() and (fl == fl2).all()
    ra, rb = a.last_records(NF), b.last_records(NF)                         # raises where the call left none
    assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), np.argwhere(ra.view(np.uint32) != rb.view(np.uint32)).tolist()[:20]
    assert a.get_state().tobytes() == b.get_state().tobytes()
    # the switch, read when the batch is created: the one-wave path, the same bytes, no records
    monkeypatch.setenv("LC3PLUS_ENC_RAGGED_PIPE", "0")
    o = _batch(c)
    monkeypatch.delenv("LC3PLUS_ENC_RAGGED_PIPE")
    got3, nb3, fl3 = _ragged(dev, o, c, sched=full, n_frames=NF)
    assert _records_words(o, NF)[0] == 0
    _same_frames(got3, c["want"])
    assert (nb3 == nb).all() and (fl3 == fl).all()
    a.close(); b.close(); o.close()


def test_a_ragged_call_of_20_frames_leaves_records_and_zero_status_for_absent_frames(dev):
    c = _case("48k_stereo", "b")
    bat = _batch(c)
    sched = c["sched"][:1]
    got, nb, fl = _ragged(dev, bat, c, sched=sched, n_frames=NF)
    for s in range(c["B"]):
        _same_frames([got[s]], [c["want"][s]])
    n, rec = _records_words(bat, NF)
    assert n == rec.size > 0
    st = bat.last_status(NF)                                                # [channel-stream][frame]
    absent = np.arange(NF)[None, :] >= np.repeat(sched[0], c["ch"])[:, None]
    assert absent.any() and (st[absent] == 0).all()
    bat.close()


# ---- 3. the five-wave writer, three runs ----
def test_48_frames_of_80_bytes_run_the_five_wave_writer(dev):
    fs, ms, B, T = 48000, 10.0, 3, 48
    sched = np.array([[48, 17, 0], [5, 48, 31]], np.int32)
    total = int(sched.sum(axis=0).max())
    pcm = make_pcm(fs, ms, 1, B, total, seed=181)
    start = [64000] * B
    assert nbytes_of(fs, 1, ms, 0, 64000) == 80
    bw = spoil_bws(rate_plan(bw_values(fs), B, total, 182), 183)
    nb, inf, fl, end = _plan(fs, 1, ms, 0, start, [0] * B, None, bw, 80, total)
    want = OracleStreams(fs, 1, ms, 0, start).encode(pcm, None, bw, nb, fl)
    c = dict(B=B, ch=1, N=480, stride=80, pcm=pcm, br=None, bw=bw, nb=nb, sched=sched)
    bat = _amd().Batch(B, fs, 1, ms, 0, start, device=0)
    got, nbg, flg = _ragged(dev, bat, c, n_frames=T)
    assert _records_words(bat, T)[0] > 0
    _same_frames(got, want)
    for s in range(B):
        n = int(sched[:, s].sum())
        assert (nbg[s, :n] == nb[s, :n]).all() and (flg[s, :n] == fl[s, :n]).all()
    bat.close()


# ---- 4. PCM forms ----
@pytest.mark.parametrize("name", ["f32_interleaved_stereo", "s24_3be"])
def test_float_layout_and_wire_type_equal_the_native_call(dev, name):
    api = _amd().api
    if name == "s24_3be":
        c = _case("48k_mono", "b")
        fmt, native_fmt = api.PCM_S24_3BE, 24
        native = lambda x: x.astype(np.int32) * 256                          # the same samples at 24 bits
        conv = lambda x: api.pcm_from_native(fmt, native(x))
    else:
        c = _case("48k_stereo", "b")
        fmt, native_fmt = api.PCM_FLOAT32 | api.PCM_INTERLEAVED, 16
        native = lambda x: x
        conv = lambda x: np.ascontiguousarray((x.astype(np.float32) / 32768.0).transpose(0, 1, 3, 2).reshape(x.shape[0], -1, x.shape[2]))      # [stream][time][channel]
    sched = c["sched"][:3]
    a, b = _batch(c), _batch(c)
    got, nb, fl = _ragged(dev, a, c, sched=sched, n_frames=NF, fmt=fmt, conv=conv)
    got2, nb2, fl2 = _ragged(dev, b, c, sched=sched, n_frames=NF, fmt=native_fmt, conv=native)
    assert _records_words(a, NF)[0] > 0 and _records_words(b, NF)[0] > 0
    _same_frames(got, c["want"]); _same_frames(got2, c["want"])
    assert (nb == nb2).all() and (fl == fl2).all()
    assert np.array_equal(a.get_state(), b.get_state())
    a.close(); b.close()


def test_placed_pcm_equals_the_native_call(dev):
    """frames at offsets in an arena; absent frames get in-range and wildly out-of-range offsets alike and report exactly 32; one present frame has an invalid
    offset: flag 16 and the bytes of silence"""
    c = _case("48k_mono", "b")
    B, N, stride = c["B"], c["N"], c["stride"]
    sched = c["sched"][:3]
    cap = B * NF * N + 1000
    bad_at = (2, 0, 0)                                                      # call, stream, frame: present (stream 0 has one frame in call 2)
    assert sched[2, 0] == 1
    pos = np.zeros(B, np.int64)
    pcm_or = c["pcm"].copy()
    bat = _batch(c)
    calls = []
    for k in range(3):
        arena = np.full(cap, 0x7A5A, np.int16)
        offs = np.zeros((B, NF), np.int64)
        wild = np.array([-1, cap - N + 1, -2 ** 62, 2 ** 62, 3], np.int64)
        w = _garbage_words(B, NF)
        for s in range(B):
            n = int(sched[k, s])
            for t in range(NF):
                slot = 500 + ((s * NF + (t + 2 * k) % NF)) * N             # rings: the frames of a stream wrap inside its twenty slots
                if t < n:
                    offs[s, t] = slot
                    arena[slot:slot + N] = c["pcm"][s, pos[s] + t, 0]
                    w[s, t] = c["bw"][s, pos[s] + t]
                else:
                    offs[s, t] = slot if (s + t) % 2 else wild[(s + t) % 5]
        if k == bad_at[0]:
            offs[bad_at[1], bad_at[2]] = cap - N + 1
            pcm_or[bad_at[1], pos[bad_at[1]] + bad_at[2]] = 0
        calls.append(dict(cnt=sched[k].copy(), pos=pos.copy(), d_pcm=dev.put(arena), d_offs=dev.put(offs), d_w=dev.put(w), d_cnt=dev.put(sched[k]),
                          d_out=dev.put(np.full((B, NF, stride), SENT, np.uint8)), d_nb=dev.put(np.full((B, NF), -7, np.int32)),
                          d_fl=dev.put(np.full((B, NF), 0xEE, np.uint8))))
        pos += sched[k]
    for q in calls:
        bat.set_pcm_placement(q["d_offs"], cap)
        bat.set_frame_counts(q["d_cnt"])
        bat.encode_device_rates(q["d_pcm"], 16, NF, q["d_out"], stride, None, q["d_w"], q["d_nb"], q["d_fl"])
    dev.sync()
    assert _records_words(bat, NF)[0] > 0
    bat.set_frame_counts(None); bat.set_pcm_placement(None)
    want = OracleStreams(c["fs"], c["ch"], c["ms"], c["hr"], c["start"]).encode(pcm_or, None, c["bw"], c["nb"], c["fl"])
    c2 = dict(c); c2["pcm"] = pcm_or
    twin = _batch(c)
    got2, nb2, fl2 = _ragged(dev, twin, c2, sched=sched, n_frames=NF)       # the native call on the same samples
    _same_frames(got2, want)
    for k, q in enumerate(calls):
        out, nb, fl = dev.get(q["d_out"], (B, NF, stride), np.uint8), dev.get(q["d_nb"], (B, NF), np.int32), dev.get(q["d_fl"], (B, NF), np.uint8)
        for s in range(B):
            n = int(q["cnt"][s])
            assert (fl[s, n:] == ABSENT).all() and (nb[s, n:] == 0).all() and (out[s, n:] == SENT).all()
            for t in range(n):
                i = int(q["pos"][s]) + t
                bad = (k, s, t) == bad_at
                assert fl[s, t] == (c["fl"][s, i] | (PLACE if bad else 0)) and nb[s, t] == c["nb"][s, i] == nb2[s, i]
                assert np.array_equal(out[s, t, :nb[s, t]], want[s][i]) and (out[s, t, nb[s, t]:] == SENT).all(), (k, s, t)
    assert np.array_equal(bat.get_state(), twin.get_state())
    bat.close(); twin.close()


# ---- 5. a pending attack-detector reset waits for the stream's first present frame ----
def test_pending_reset_of_an_absent_stream_is_done_at_its_next_frame_once(dev):
    """Stream 0 encodes 4 frames with attack handling (96 kbit/s) on PCM with clicks; set_bitrate(64000) disables attack handling and asks for the one-shot
    detector reset, set_bitrate(128000) enables it again, no frame between.  The stream is absent from a ragged call of 20 frames and present with all 20 in the
    next - two runs: the reset belongs to the first.  Its frames are the oracle's, and those of a second batch that never skipped.  An oracle that never saw
    64000 gives other bytes, and so does one that clears the detector once more where the second run starts: the case would notice a lost reset and a repeated one."""
    fs, ms, B, N = 48000, 10.0, 4, 480
    rng = np.random.default_rng(22)                                         # (a seed with which both of the oracle's answers below differ from the right one)
    T = 4 + 2 * NF
    pcm = (rng.standard_normal((B, T, 1, N)) * 200).astype(np.int16)
    for b in range(B):
        for t in range(1, T, 2):
            k = int(rng.integers(0, N - 8))
            pcm[b, t, 0, k:k + 8] = 20000

    def oracle(with_reset, again=False):
        o = Oracle(fs, 1, ms, 0, 96000, portable_math=True)
        fr = [o.encode(pcm[0, t]) for t in range(4)]
        if with_reset:
            assert o.set_bitrate(64000) == 0
        assert o.set_bitrate(128000) == 0
        for t in range(4, 4 + NF):
            if again and t == 4 + NF // 2:                                  # where the call's second run starts
                assert o.set_bitrate(64000) == 0 and o.set_bitrate(128000) == 0
            fr.append(o.encode(pcm[0, t]))
        return fr
    want, lost, twice = oracle(True), oracle(False), oracle(True, True)
    assert any(not np.array_equal(a, b) for a, b in zip(want[4:], lost[4:])), "the detector's memory does not reach these frames: the case shows nothing"
    assert any(not np.array_equal(a, b) for a, b in zip(want[4 + NF // 2:], twice[4 + NF // 2:])), "a second reset at the run boundary would not show"
    c = dict(B=B, ch=1, N=N, stride=160, pcm=pcm, br=None, bw=np.zeros((B, T), np.int32), sched=None,
             nb=np.array([[160] * T] + [[120] * T] * 3, np.int32))
    res = []
    for skip in (True, False):
        bat = _amd().Batch(B, fs, 1, ms, 0, [96000] * B, device=0)
        out = bat.encode(pcm[:, :4])
        assert all(np.array_equal(out[0, t, :120], want[t]) for t in range(4))
        assert bat.set_bitrate(0, 64000) == 0 and bat.set_bitrate(0, 128000) == 0
        if skip:
            _ragged(dev, bat, c, sched=np.array([[0, NF, 9, 3]], np.int32), n_frames=NF, pos0=[4] * B)
            assert _records_words(bat, NF)[0] > 0
        got, nb, fl = _ragged(dev, bat, c, sched=np.array([[NF, 0, 11, 1]], np.int32), n_frames=NF, pos0=[4] * B)
        _same_frames([got[0]], [want[4:]])
        res.append(got[0])
        bat.close()
    assert all(np.array_equal(x, y) for x, y in zip(*res))


# ---- 6. between promised calls ----
def test_ragged_call_of_16_between_promised_dense_calls(dev):
    """under set_input_ready(1): two dense calls of 16 frames (the pipelined path, overlapping), a ragged call of 16 on the same path, two more dense calls;
    everything uploaded first, one wait at the end; every stream's frames are the oracle's, every untouched byte keeps its sentinel"""
    fs, ms, hr, ch, rates, B = GEOMS["48k_mono"]
    n = 16
    T = 5 * n
    pcm = make_pcm(fs, ms, ch, B, T, seed=191)
    start = [64000, 96000, 128000, 64000, 96000]
    sizes = np.array([nbytes_of(fs, ch, ms, hr, r) for r in start])
    stride = int(sizes.max())
    cnt = np.array([16, 0, 7, 1, 12], np.int32)
    want = OracleStreams(fs, ch, ms, hr, start).encode(pcm, nb=np.repeat(sizes[:, None], T, axis=1))
    bat = _amd().Batch(B, fs, ch, ms, hr, start, device=0)
    bat.set_input_ready(True)
    pos, plan = np.zeros(B, np.int64), []
    for kind in ("d", "d", "r", "d", "d"):
        x = np.full((B, n, ch, pcm.shape[3]), 0x7A5A, np.int16)
        take = np.full(B, n) if kind == "d" else cnt
        for s in range(B):
            x[s, :take[s]] = pcm[s, pos[s]:pos[s] + take[s]]
        plan.append((kind, take.copy(), pos.copy(), dev.put(x), dev.put(np.full((B, n, stride), SENT, np.uint8))))
        pos += take
    d_bw, d_cnt = dev.put(np.where(np.arange(n)[None, :] < cnt[:, None], 0, _garbage_words(B, n)).astype(np.int32)), dev.put(cnt)
    d_nb, d_fl = dev.put(np.full((B, n), -7, np.int32)), dev.put(np.full((B, n), 0xEE, np.uint8))
    for kind, take, p0, d_pcm, d_out in plan:
        if kind == "d":
            bat.encode_device(d_pcm, 16, n, d_out, stride)
        else:
            bat.set_frame_counts(d_cnt)
            bat.encode_device_rates(d_pcm, 16, n, d_out, stride, None, d_bw, d_nb, d_fl)
            bat.set_frame_counts(None)
    dev.sync()
    for kind, take, p0, d_pcm, d_out in plan:
        out = dev.get(d_out, (B, n, stride), np.uint8)
        for s in range(B):
            for t in range(n):
                if t < take[s]:
                    w = want[s][int(p0[s]) + t]
                    assert np.array_equal(out[s, t, :w.size], w) and (out[s, t, w.size:] == SENT).all(), (kind, s, t)
                else:
                    assert (out[s, t] == SENT).all()
    fl, nb = dev.get(d_fl, (B, n), np.uint8), dev.get(d_nb, (B, n), np.int32)
    present = np.arange(n)[None, :] < cnt[:, None]
    assert (fl == np.where(present, 0, ABSENT)).all() and (nb == np.where(present, sizes[:, None], 0)).all()
    bat.close()


# ---- 7. what stays on the one-wave kernels ----
def test_large_layout_and_per_frame_bitrates_stay_where_they_were(dev):
    """12 frames, more than the in-kernel writer's 8: 96 kHz high-resolution (the large layout) through encode_packed without words, and 48 kHz with per-frame
    bitrates - with them the dense call runs the one-wave kernel too.  Both match the oracle and leave no records."""
    for geom, mode, packed, sched in (("96k_hr", "n", 0, [[0, 12, 3, 9]]), ("48k_mono", "r", None, [[0, 12, 3, 9, 5]])):
        c = _case(geom, mode, T=12, seed=2)
        bat = _batch(c)
        sched = np.array(sched, np.int32)
        got, nb, fl = _ragged(dev, bat, c, sched=sched, n_frames=12, packed=packed)
        for s in range(c["B"]):
            n = int(sched[0, s])
            _same_frames([got[s]], [c["want"][s]])
            assert (nb[s, :n] == c["nb"][s, :n]).all() and (fl[s, :n] == c["fl"][s, :n]).all()
        assert _records_words(bat, 12)[0] == 0
        bat.close()
