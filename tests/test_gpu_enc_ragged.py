"""GPU tests of per-stream frame counts in the batched encoder (lc3plus_enc_batch_set_frame_counts, Batch.set_frame_counts): ragged calls of
encode_device_rates / encode_device_packed against the CPU oracle fed each stream's frames densely with the setters the lenient rule accepts
(test_gpu_enc_rates_device.OracleStreams).  Every comparison is equality: bytes, sizes, flags, state.  out, num_bytes, flags and offsets are filled with
sentinels before every call; the entries of absent frames - PCM, rates, bandwidths, placement - hold values that would be refused or change the result if
they were looked at.

One case per geometry and mode: every stream has 14 frames, dealt out over 8 calls of 6 frames with counts from {0, 1, 3, 4, 5, 6}, every call holding at
least one 0 and one 6 (_schedule).  A stream of 14 frames has at most two counts of 6, so eight such calls need four streams: the stereo and the
high-resolution geometry have four, one more than the fewest that would show a fault."""
import ctypes as C
import functools

import numpy as np
import pytest

from lc3_harness import Oracle
from test_enc_rates_device_cpu import _limits
from test_gpu_dec_varsize_device import _Hip
from test_gpu_enc_rates_device import OracleStreams, SENT, check_frames, nbytes_of, run_calls, spoil_bws, spoil_rates
from test_gpu_enc_varbw import bw_values
from test_gpu_enc_varrate import make_pcm, rate_plan
from test_gpu_pcm_placed import _enc_state_rows

pytestmark = pytest.mark.gpu
LC3_ERROR = 1
ABSENT, PLACE, CAP = 32, 16, 8
T_TOTAL, NF = 14, 6
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
# geometry -> fs, frame_ms, hrmode, channels, rates, streams
GEOMS = {
    "48k_mono": (48000, 10.0, 0, 1, [40000, 64000, 96000, 128000, 272000], 5),
    "48k_stereo": (48000, 10.0, 0, 2, [128800, 160800, 200800, 96000], 4),       # odd sizes; a count is per stream, the two channels share it
    "96k_hr": (96000, 10.0, 1, 1, [149600, 256000, 400000], 4),                  # the large layout
    "16k_2p5": (16000, 2.5, 0, 1, [64000, 80000, 128000], 4),
}


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


def _schedule(B, seed):
    """counts [K, B], K = 8: every column sums to 14, every entry is one of 0, 1, 3, 4, 5, 6, every row holds a 0 and a 6.  Streams
    0 .. K / 2 - 1 are pillars: pillar j has 6, 6, 1, 1 in calls 2j .. 2j + 3 (mod K) and 0 elsewhere; the others split their 14 frames at random."""
    K = 8
    rng = np.random.default_rng(seed)
    sched = np.zeros((K, B), np.int32)
    for j in range(K // 2):
        for i, c in enumerate((6, 6, 1, 1)):
            sched[(2 * j + i) % K, j] = c
    for s in range(K // 2, B):
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


def _plan(fs, ch, ms, hr, start, start_bw, br, bw, stride, T):
    rc, nb, inf, fl, end = _amd().api.enc_plan_rates_ragged(fs, ch, ms, hr, start, start_bw, bitrates=br, bandwidths=bw, out_stride=stride, n_frames=T)
    assert rc == 0
    return nb, inf, fl, end


@functools.lru_cache(maxsize=None)
def _case(geom, mode, T=T_TOTAL, seed=0, packed=False):
    """The shared case of a geometry and mode (r rates, b bandwidths, rb both, n neither), computed once and left unchanged: PCM, the words with refused
    values among them, the rule's sizes and flags over each stream's dense frames, the oracle's frames, the schedule.  packed: the rule of encode_packed, which has no slot to
    bound a frame with (a rate is refused only where set_bitrate refuses it)."""
    fs, ms, hr, ch, rates, B = GEOMS[geom]
    pcm = make_pcm(fs, ms, ch, B, T, seed=60 + seed)
    start = [rates[(b + 1) % len(rates)] for b in range(B)]
    stride = max(nbytes_of(fs, ch, ms, hr, r) for r in rates)
    br = spoil_rates(rate_plan(rates, B, T, 70 + seed), fs, ch, ms, hr, 71 + seed, _limits(fs, ch, ms, hr)[1]) if "r" in mode else None
    bw = spoil_bws(rate_plan(bw_values(fs), B, T, 72 + seed), 73 + seed) if "b" in mode else None
    nb, inf, fl, end = _plan(fs, ch, ms, hr, start, [0] * B, br, bw, 1 << 20 if packed else stride, T)
    want = OracleStreams(fs, ch, ms, hr, start).encode(pcm, br, bw, nb, fl)
    c = dict(geom=geom, mode=mode, fs=fs, ms=ms, hr=hr, ch=ch, B=B, N=pcm.shape[3], T=T, pcm=pcm, br=br, bw=bw, start=start, stride=stride, nb=nb, inf=inf,
             fl=fl, end=end, want=want, sched=_schedule(B, len(geom) + seed))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def _batch(c):
    return _amd().Batch(c["B"], c["fs"], c["ch"], c["ms"], c["hr"], c["start"], device=0)


def _garbage_words(B, n):
    """rates / bandwidths of absent frames: every one a value the rule refuses"""
    tt, ss = np.meshgrid(np.arange(n), np.arange(B))
    return np.array([-1, I32_MAX, I32_MIN, 7], np.int64)[(ss + tt) % 4].astype(np.int32)


def _ragged(dev, bat, c, sched=None, n_frames=NF, fmt=16, conv=None, packed=None, cut=None, hip_stream=None, async_counts=False, raw_counts=None, pos0=None):
    """The ragged calls of a schedule [K, B] on batch bat, stream s taking its next sched[k, s] frames in call k.  packed: None (slotted) or the order;
    cut: the call whose capacity is one byte short of its total.  raw_counts [K, B]: what is uploaded as counts in place of the schedule (which must be
    its clamp).  Asserts what holds for absent frames and for every byte outside the written frames, and returns the present frames gathered per stream:
    list [B] of lists of byte arrays (None for a frame cut by the capacity), sizes [B, sum], flags [B, sum]."""
    api = _amd().api
    sched = c["sched"] if sched is None else sched
    B, ch, N, stride = c["B"], c["ch"], c["N"], c["stride"]
    conv = conv or (lambda x: x)
    pos = np.zeros(B, np.int64) if pos0 is None else np.array(pos0, np.int64)
    calls = []
    for k in range(sched.shape[0]):
        cnt = sched[k]
        pcm = np.full((B, n_frames, ch, N), 0x7A5A, np.int16)
        r, w = _garbage_words(B, n_frames), _garbage_words(B, n_frames)[:, ::-1].copy()
        for s in range(B):
            p, n = int(pos[s]), int(cnt[s])
            pcm[s, :n] = c["pcm"][s, p:p + n]
            if c["br"] is not None:
                r[s, :n] = c["br"][s, p:p + n]
            if c["bw"] is not None:
                w[s, :n] = c["bw"][s, p:p + n]
        nb_k = np.zeros((B, n_frames), np.int32)
        for s in range(B):
            nb_k[s, :cnt[s]] = c["nb"][s, pos[s]:pos[s] + cnt[s]]
        up = (raw_counts[k] if raw_counts is not None else cnt).astype(np.int32)
        q = dict(cnt=cnt.copy(), pos=pos.copy(), nb=nb_k, d_pcm=dev.put(conv(pcm)), d_r=dev.put(r) if c["br"] is not None else None,
                 d_w=dev.put(w) if c["bw"] is not None else None, d_nb=dev.put(np.full((B, n_frames), -7, np.int32)),
                 d_fl=dev.put(np.full((B, n_frames), 0xEE, np.uint8)))
        if async_counts:
            q["d_cnt"], q["h_cnt"] = dev.put(np.full(B, -1, np.int32)), dev.pin(up)      # until the copy lands: nothing present
        else:
            q["d_cnt"] = dev.put(up)
        if packed is None:
            q["d_out"] = dev.put(np.full((B, n_frames, stride), SENT, np.uint8))
        else:
            _, offs, total, ovf = api.plan_packed(nb_k, order=packed)
            q["cap"] = total - 1 if cut == k else total + 40
            q["plan"] = api.plan_packed(nb_k, order=packed, capacity=q["cap"])
            q["d_out"] = dev.put(np.full(total + 104, SENT, np.uint8))
            q["d_offs"], q["d_tot"] = dev.put(np.full((B, n_frames), -99, np.int64)), dev.put(np.full(1, -99, np.int64))
        calls.append(q)
        pos += cnt
    for q in calls:
        if async_counts:
            dev.copy_async(q["d_cnt"], q["h_cnt"], hip_stream)
        bat.set_frame_counts(q["d_cnt"])
        if packed is None:
            bat.encode_device_rates(q["d_pcm"], fmt, n_frames, q["d_out"], stride, q["d_r"], q["d_w"], q["d_nb"], q["d_fl"], hip_stream=hip_stream)
        else:
            bat.encode_device_packed(q["d_pcm"], fmt, n_frames, q["d_out"], q["cap"], packed, q["d_r"], q["d_w"], q["d_offs"], q["d_tot"], q["d_nb"], q["d_fl"],
                                     hip_stream=hip_stream)
    dev.sync()
    total_frames = int(sched.sum(axis=0).max())
    got = [[None] * total_frames for _ in range(B)]
    nb_all, fl_all = np.full((B, total_frames), -1, np.int32), np.full((B, total_frames), 0xFF, np.uint8)
    base = np.zeros(B, np.int64) if pos0 is None else np.array(pos0, np.int64)
    for q in calls:
        nb, fl = dev.get(q["d_nb"], (B, n_frames), np.int32), dev.get(q["d_fl"], (B, n_frames), np.uint8)
        absent = np.arange(n_frames)[None, :] >= q["cnt"][:, None]
        assert (nb[absent] == 0).all() and (fl[absent] == ABSENT).all() and not (fl[~absent] & ABSENT).any()
        assert (nb == q["nb"]).all()
        if packed is None:
            out = dev.get(q["d_out"], (B, n_frames, stride), np.uint8)
            assert (out[absent] == SENT).all()                               # no byte of an absent frame's slot
            assert (out[np.arange(stride)[None, None, :] >= nb[:, :, None]] == SENT).all()      # nor behind a payload
        else:
            rc, offs, total, ovf = q["plan"]
            raw = dev.get(q["d_out"], (total + 104,), np.uint8)
            assert (dev.get(q["d_offs"], (B, n_frames), np.int64) == offs).all() and int(dev.get(q["d_tot"], (1,), np.int64)[0]) == total
            assert ((fl & CAP) == np.where(absent, 0, ovf)).all()
            written = np.zeros(raw.size, bool)
            for s in range(B):
                for t in range(int(q["cnt"][s])):
                    if not ovf[s, t]:
                        written[offs[s, t]:offs[s, t] + nb[s, t]] = True
            assert (raw[~written] == SENT).all()                            # no byte outside the written frames
        for s in range(B):
            for t in range(int(q["cnt"][s])):
                i = int(q["pos"][s] - base[s]) + t
                nb_all[s, i], fl_all[s, i] = nb[s, t], fl[s, t]
                if packed is None:
                    got[s][i] = out[s, t, :nb[s, t]]
                elif not ovf[s, t]:
                    got[s][i] = raw[offs[s, t]:offs[s, t] + nb[s, t]]
    bat.set_frame_counts(None)
    return [got[s][:int(sched[:, s].sum())] for s in range(B)], nb_all, fl_all


def _same_frames(got, want, t0=0, allow_cut=False):
    bad = [(s, t) for s in range(len(got)) for t in range(len(got[s]))
           if (got[s][t] is None and not allow_cut) or (got[s][t] is not None and not np.array_equal(got[s][t], want[s][t0 + t]))]
    assert not bad, (len(bad), bad[:8])


def _dense_twin(dev, c, cuts=(0, 6, T_TOTAL), fmt=16, conv=None):
    """the same frames densely with the same call on a second batch: out [B, T, stride], sizes, flags, the batch"""
    bat = _batch(c)
    pcm = c["pcm"] if conv is None else None
    assert pcm is not None
    out, nb, fl = run_calls(dev, bat, pcm, c["br"], c["bw"], cuts, c["stride"], bitdepth=fmt)
    return out, nb, fl, bat


# ---- 1. parity ----
@pytest.mark.parametrize("geom,mode", [(g, m) for g in GEOMS for m in ("r", "b", "rb") if not (GEOMS[g][2] and "b" in m)])
def test_ragged_sequence_vs_oracle_and_dense_twin(dev, geom, mode):
    c = _case(geom, mode)
    bat = _batch(c)
    got, nb, fl = _ragged(dev, bat, c)
    _same_frames(got, c["want"])
    assert (nb == c["nb"]).all() and (fl == c["fl"]).all()
    if "r" in mode:
        assert (c["fl"] & 1).any()                                          # the case has refused rates: the carry is exercised
    if "b" in mode:
        assert (c["fl"] & 2).any() and (c["fl"] & 4).any()
    out2, nb2, fl2, twin = _dense_twin(dev, c)
    check_frames(out2, nb2, c["want"])
    assert (nb2 == nb).all() and (fl2 == fl).all()
    assert np.array_equal(bat.get_state(), twin.get_state())
    B = c["B"]
    assert [bat.num_bytes(s) for s in range(B)] == [twin.num_bytes(s) for s in range(B)] == c["nb"][:, -1].tolist()
    if not c["hr"]:
        assert [bat.bandwidth(s) for s in range(B)] == [twin.bandwidth(s) for s in range(B)]
    bat.close(); twin.close()


# ---- 2. counts all equal to n_frames ----
@pytest.mark.parametrize("T,mode", [(4, "rb"), (12, "b"), (12, "r")])
def test_counts_all_n_frames_equal_the_call_without_counts(dev, T, mode):
    """bytes, sizes, flags, state and the configuration read back; with bandwidths alone the dense call of 12 frames runs the pipelined kernels, the ragged
    one the one-wave kernel: the result does not depend on the path"""
    c = _case("48k_mono", mode, T=T, seed=T)
    B = c["B"]
    a, b = _batch(c), _batch(c)
    got, nb, fl = _ragged(dev, a, c, sched=np.full((1, B), T, np.int32), n_frames=T)
    out2, nb2, fl2 = run_calls(dev, b, c["pcm"], c["br"], c["bw"], (0, T), c["stride"])
    check_frames(out2, nb2, c["want"])
    _same_frames(got, c["want"])
    assert (nb == nb2).all() and (fl == fl2).all() and (nb == c["nb"]).all() and (fl == c["fl"]).all()
    if mode == "b" and T > 8:
        # Two paths, one state: what differs between them is no state.  The slot's words in front of the MDCT memory (test_gpu_pcm_placed._enc_state_rows), and
        # the per-frame scalars that lc3_encode_kernel stores with the cross-frame ones and the pipelined kernels leave alone - fsc[9 ...] (normalised
        # correlation, gain) and isc[6 ... 15] (pitch lag, LTPF parameters, bandwidth index, SNS indices: lc3_kernels.hip, the fsc / isc maps), every one
        # written by its frame before that frame reads it.  Everything else is compared, and the two batches carry on alike.
        g = (c["fs"], c["ms"], c["hr"], c["ch"], 0)
        ra, rb = _enc_state_rows(a.get_state(), g, c["N"], B), _enc_state_rows(b.get_state(), g, c["N"], B)
        scal = ra.shape[1] - 660 + 384 + 194 + 2                           # LC3D_ST_SCAL
        for r in (ra, rb):
            r[:, scal + 9:scal + 16] = 0; r[:, scal + 16 + 6:scal + 32] = 0
        assert np.array_equal(ra, rb), np.argwhere(ra != rb).tolist()[:20]
        more = make_pcm(c["fs"], c["ms"], c["ch"], B, 3, seed=77)
        assert np.array_equal(a.encode(more), b.encode(more))
    else:
        assert np.array_equal(a.get_state(), b.get_state())
    assert [a.num_bytes(s) for s in range(B)] == [b.num_bytes(s) for s in range(B)]
    assert [a.bandwidth(s) for s in range(B)] == [b.bandwidth(s) for s in range(B)]
    a.close(); b.close()


# ---- 3. a stream that is idle through a sequence, with a pending attack-detector reset ----
def _state_rows(bat, stream):
    st = bat.get_state()
    rows = st.reshape(bat.n_streams * bat.channels, -1)
    return rows[stream * bat.channels:(stream + 1) * bat.channels].copy()


def test_idle_stream_keeps_state_configuration_and_its_pending_reset(dev):
    """Stream 0 encodes 4 frames with attack handling (96 kbit/s) on PCM with clicks, is then absent from three calls - set_bitrate(64000), which disables
    attack handling and asks for the one-shot detector reset, and set_bitrate(128000), which enables it again, are issued meanwhile - and then encodes 8
    frames.  Its state rows and configuration do not move while it is idle, and its later frames are the oracle's, which cleared the detector at
    set_bitrate(64000).  An oracle that never saw 64000 gives other bytes: the case would notice a lost reset."""
    fs, ms, B, N = 48000, 10.0, 4, 480
    rng = np.random.default_rng(5)
    T = 4 + 8
    pcm = (rng.standard_normal((B, T, 1, N)) * 200).astype(np.int16)
    for b in range(B):
        for t in range(1, T, 2):
            k = int(rng.integers(0, N - 8))
            pcm[b, t, 0, k:k + 8] = 20000
    start = [96000] * B
    c = dict(B=B, ch=1, N=N, stride=160, pcm=pcm, br=None, bw=np.zeros((B, T + 18), np.int32), nb=None, sched=None)
    amd = _amd()
    bat = amd.Batch(B, fs, 1, ms, 0, start, device=0)

    def oracle(with_reset):
        o = Oracle(fs, 1, ms, 0, 96000, portable_math=True)
        fr = [o.encode(pcm[0, t]) for t in range(4)]
        if with_reset:
            assert o.set_bitrate(64000) == 0
        assert o.set_bitrate(128000) == 0
        return fr + [o.encode(pcm[0, t]) for t in range(4, T)]
    want, wrong = oracle(True), oracle(False)
    assert any(not np.array_equal(a, b) for a, b in zip(want[4:], wrong[4:])), "the detector's memory does not reach these frames: the case shows nothing"
    # phase A: everybody present (stream 0: four frames)
    c["nb"] = np.full((B, T + 18), 120, np.int32)
    got, nb, fl = _ragged(dev, bat, c, sched=np.array([[4, 4, 4, 4]], np.int32))
    _same_frames([got[0]], [want[:4]])
    rows0, cfg0 = _state_rows(bat, 0), (bat.num_bytes(0), bat.bandwidth(0))
    # phase B: stream 0 idle, the others advance (their PCM is read again from frame 4 on: only stream 0 is compared)
    idle = np.array([[0, 6, 1, 3]], np.int32)
    _ragged(dev, bat, c, sched=idle, pos0=[4] * B)
    assert np.array_equal(_state_rows(bat, 0), rows0) and (bat.num_bytes(0), bat.bandwidth(0)) == cfg0
    assert bat.set_bitrate(0, 64000) == 0
    c["nb"] = np.array([[80] * (T + 18)] + [[120] * (T + 18)] * 3, np.int32)
    _ragged(dev, bat, c, sched=idle, pos0=[4] * B)
    assert np.array_equal(_state_rows(bat, 0), rows0) and bat.num_bytes(0) == 80
    assert bat.set_bitrate(0, 128000) == 0
    c["nb"] = np.array([[160] * (T + 18)] + [[120] * (T + 18)] * 3, np.int32)
    _ragged(dev, bat, c, sched=idle, pos0=[4] * B)
    assert np.array_equal(_state_rows(bat, 0), rows0) and bat.num_bytes(0) == 160
    # phase C: stream 0 present again, in two calls
    got, nb, fl = _ragged(dev, bat, c, sched=np.array([[3, 0, 6, 1], [5, 6, 0, 0]], np.int32), pos0=[4] * B)
    _same_frames([got[0][:8]], [want[4:]])
    bat.close()


@pytest.mark.parametrize("kind", ["ragged_then_encode_device", "ragged_then_packed", "dense_only"])
def test_pending_reset_is_done_once_by_the_dense_calls_that_follow(dev, kind):
    """set_bitrate(64000) - attack handling off, the one-shot reset asked for - and set_bitrate(128000) - on again - with no frame of stream 0 between
    them; with `ragged` a ragged call in which stream 0 is absent follows each, so that the reset waits in the device's configuration behind a stale host
    copy.  Then counts off and two dense calls, of two and of six frames: the first clears the detector, the second must not clear it again.  Stream 0
    against the oracle; an oracle without the reset gives other bytes in the first call, one that clears the detector once more in front of the second call
    other bytes there.  dense_only: the same two setters in front of dense calls alone."""
    fs, ms, B, N, T = 48000, 10.0, 4, 480, 12
    rng = np.random.default_rng(5)
    pcm = (rng.standard_normal((B, T, 1, N)) * 200).astype(np.int16)
    for b in range(B):
        for t in range(1, T, 2):
            k = int(rng.integers(0, N - 8))
            pcm[b, t, 0, k:k + 8] = 20000

    cuts = (4, 6, T)

    def oracle(with_reset, again=False):
        o = Oracle(fs, 1, ms, 0, 96000, portable_math=True)
        fr = [o.encode(pcm[0, t]) for t in range(4)]
        if with_reset:
            assert o.set_bitrate(64000) == 0
        assert o.set_bitrate(128000) == 0
        for t in range(4, T):
            if again and t == cuts[1]:
                assert o.set_bitrate(64000) == 0 and o.set_bitrate(128000) == 0
            fr.append(o.encode(pcm[0, t]))
        return fr
    want, lost, twice = oracle(True), oracle(False), oracle(True, True)
    assert any(not np.array_equal(a, b) for a, b in zip(want[4:6], lost[4:6])) and any(not np.array_equal(a, b) for a, b in zip(want[6:], twice[6:]))
    api = _amd().api
    bat = _amd().Batch(B, fs, 1, ms, 0, [96000] * B, device=0)
    out = bat.encode(pcm[:, :4])
    assert all(np.array_equal(out[0, t, :120], want[t]) for t in range(4))
    c = dict(B=B, ch=1, N=N, stride=160, pcm=pcm, br=None, bw=np.zeros((B, T + 18), np.int32), nb=np.full((B, T + 18), 120, np.int32), sched=None)
    idle = np.array([[0, 6, 1, 3]], np.int32)
    assert bat.set_bitrate(0, 64000) == 0
    if kind != "dense_only":
        _ragged(dev, bat, c, sched=idle, pos0=[4] * B)
    assert bat.set_bitrate(0, 128000) == 0
    if kind != "dense_only":
        _ragged(dev, bat, c, sched=idle, pos0=[4] * B)
    got = []
    for a, b in zip(cuts[:-1], cuts[1:]):                                   # nothing is read back between the two
        n = b - a
        d_pcm = dev.put(np.ascontiguousarray(pcm[:, a:b]))
        if kind == "ragged_then_packed":
            _, offs, total, _ = api.plan_packed(np.repeat(np.array([[160], [120], [120], [120]], np.int32), n, axis=1))
            d_out = dev.put(np.full(total, SENT, np.uint8))
            bat.encode_device_packed(d_pcm, 16, n, d_out, total, d_offsets_ptr=dev.put(np.zeros((B, n), np.int64)), d_total_ptr=dev.zeros(8))
            got.append((a, n, d_out, offs, total))
        else:
            d_out = dev.put(np.full((B, n, 160), SENT, np.uint8))
            bat.encode_device(d_pcm, 16, n, d_out, 160)
            got.append((a, n, d_out, None, 0))
    dev.sync()
    for a, n, d_out, offs, total in got:
        for t in range(n):
            fr = dev.get(d_out, (B, n, 160), np.uint8)[0, t] if offs is None else dev.get(d_out, (total,), np.uint8)[offs[0, t]:offs[0, t] + 160]
            assert np.array_equal(fr[:160], want[a + t]), (a, t)
    bat.close()


# ---- 4. out-of-range counts ----
def test_out_of_range_counts_behave_as_their_clamp(dev):
    c = _case("48k_mono", "rb")
    raw = np.array([[-3, NF + 9, I32_MIN, I32_MAX, 2]], np.int32)
    clamp = np.array([[0, NF, 0, NF, 2]], np.int32)
    a, b = _batch(c), _batch(c)
    ga, nba, fla = _ragged(dev, a, c, sched=clamp, raw_counts=raw)
    gb, nbb, flb = _ragged(dev, b, c, sched=clamp)
    _same_frames(ga, c["want"]); _same_frames(gb, c["want"])
    assert (nba == nbb).all() and (fla == flb).all()
    assert np.array_equal(a.get_state(), b.get_state())
    a.close(); b.close()


def test_four_frame_groups_cut_by_a_count(dev):
    """a call of 8 frames takes the plan kernel's four-frames-per-access path; counts that are no multiple of 4 cut inside a group"""
    c = _case("48k_mono", "rb")
    bat = _batch(c)
    sched = np.array([[0, 1, 3, 5, 8]], np.int32)
    got, nb, fl = _ragged(dev, bat, c, sched=sched, n_frames=8)
    for s in range(c["B"]):
        n = int(sched[0, s])
        _same_frames([got[s][:n]], [c["want"][s]])
        assert (nb[s, :n] == c["nb"][s, :n]).all() and (fl[s, :n] == c["fl"][s, :n]).all()
    bat.close()


# ---- 5. packed output ----
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("mode", ["rb", "n"])
def test_packed_output_with_counts(dev, mode, order):
    """both orders, with rates and bandwidths and with neither; call 1's capacity is one byte short of its total: the last present frame in the order is cut
    (flag bit 3), still encoded - the frames behind it match - and offsets and total are lc3plus_plan_packed of the ragged sizes"""
    c = _case("48k_mono", mode, packed=True)
    bat = _batch(c)
    got, nb, fl = _ragged(dev, bat, c, packed=order, cut=1)
    assert sum(g is None for row in got for g in row) == 1 and int(((fl & CAP) != 0).sum()) == 1
    _same_frames(got, c["want"], allow_cut=True)
    assert (nb == c["nb"]).all() and ((fl & (0xFF ^ CAP)) == c["fl"]).all()
    twin = _batch(c)
    _ragged(dev, twin, c, packed=1 - order)                                  # the other order, nothing cut: the same state
    assert np.array_equal(bat.get_state(), twin.get_state())
    bat.close(); twin.close()


# ---- 6. placed PCM from rings ----
def test_placed_pcm_with_counts(dev):
    """frames at offsets in an arena: absent frames get in-range and wildly out-of-range offsets alike and report exactly 32; one present frame has an
    invalid offset: flag 16 and the bytes of silence"""
    c = _case("48k_mono", "r")
    B, N, stride = c["B"], c["N"], c["stride"]
    bat = _batch(c)
    sched = c["sched"][:3]
    cap = B * NF * N + 1000
    bad_at = (2, 0, 0)                                                      # call, stream, frame: present (pillar 0 has 6, 6, 1 in calls 0 .. 2)
    assert sched[2, 0] == 1
    pos = np.zeros(B, np.int64)
    pcm_or = c["pcm"].copy()
    calls = []
    for k in range(3):
        arena = np.full(cap, 0x7A5A, np.int16)
        offs = np.zeros((B, NF), np.int64)
        wild = np.array([-1, cap - N + 1, -2 ** 62, 2 ** 62, 3], np.int64)
        r = _garbage_words(B, NF)
        for s in range(B):
            n = int(sched[k, s])
            for t in range(NF):
                slot = 500 + ((s * NF + (t + 2 * k) % NF)) * N             # rings: the frames of a stream wrap inside its six slots
                if t < n:
                    offs[s, t] = slot
                    arena[slot:slot + N] = c["pcm"][s, pos[s] + t, 0]
                    r[s, t] = c["br"][s, pos[s] + t]
                else:
                    offs[s, t] = slot if (s + t) % 2 else wild[(s + t) % 5]
        if k == bad_at[0]:
            offs[bad_at[1], bad_at[2]] = cap - N + 1
            pcm_or[bad_at[1], pos[bad_at[1]] + bad_at[2]] = 0
        calls.append(dict(cnt=sched[k].copy(), pos=pos.copy(), d_pcm=dev.put(arena), d_offs=dev.put(offs), d_r=dev.put(r), d_cnt=dev.put(sched[k]),
                          d_out=dev.put(np.full((B, NF, stride), SENT, np.uint8)), d_nb=dev.put(np.full((B, NF), -7, np.int32)),
                          d_fl=dev.put(np.full((B, NF), 0xEE, np.uint8))))
        pos += sched[k]
    for q in calls:
        bat.set_pcm_placement(q["d_offs"], cap)
        bat.set_frame_counts(q["d_cnt"])
        bat.encode_device_rates(q["d_pcm"], 16, NF, q["d_out"], stride, q["d_r"], None, q["d_nb"], q["d_fl"])
    dev.sync()
    done = int(pos.max())
    fs, ms, hr, ch = c["fs"], c["ms"], c["hr"], c["ch"]
    nbw, _, flw, _ = _plan(fs, ch, ms, hr, c["start"], [0] * B, c["br"], None, stride, T_TOTAL)
    want = OracleStreams(fs, ch, ms, hr, c["start"]).encode(pcm_or[:, :done], c["br"][:, :done], None, nbw[:, :done], flw[:, :done])
    for k, q in enumerate(calls):
        out, nb, fl = dev.get(q["d_out"], (B, NF, stride), np.uint8), dev.get(q["d_nb"], (B, NF), np.int32), dev.get(q["d_fl"], (B, NF), np.uint8)
        for s in range(B):
            n = int(q["cnt"][s])
            assert (fl[s, n:] == ABSENT).all() and (nb[s, n:] == 0).all() and (out[s, n:] == SENT).all()
            for t in range(n):
                i = int(q["pos"][s]) + t
                bad = (k, s, t) == bad_at
                assert fl[s, t] == (flw[s, i] | (PLACE if bad else 0)) and nb[s, t] == nbw[s, i]
                assert np.array_equal(out[s, t, :nb[s, t]], want[s][i]), (k, s, t)
    bat.close()


# ---- 7. formats ----
@pytest.mark.parametrize("name", ["ulaw", "f32_interleaved_stereo"])
def test_wire_type_and_float_layout(dev, name):
    api = _amd().api
    if name == "ulaw":
        c = dict(_case("48k_mono", "r"))
        fmt = api.PCM_ULAW
        wire = api.pcm_from_native(fmt, c["pcm"])
        native = api.pcm_to_native(fmt, wire)
        conv = lambda x: api.pcm_from_native(fmt, x)
    else:
        c = dict(_case("48k_stereo", "rb"))
        fmt = api.PCM_FLOAT32 | api.PCM_INTERLEAVED
        native = c["pcm"]
        conv = lambda x: np.ascontiguousarray((x.astype(np.float32) / 32768.0).transpose(0, 1, 3, 2).reshape(x.shape[0], -1, x.shape[2]))      # [stream][time][channel]
    want = OracleStreams(c["fs"], c["ch"], c["ms"], c["hr"], c["start"]).encode(native, c["br"], c["bw"], c["nb"], c["fl"])
    c["pcm"] = native
    bat = _batch(c)
    got, nb, fl = _ragged(dev, bat, c, fmt=fmt, conv=conv)
    _same_frames(got, want)
    assert (nb == c["nb"]).all() and (fl == c["fl"]).all()
    bat.close()


# ---- 8. ordering ----
def test_counts_produced_on_the_stream(dev):
    """every call's counts arrive by an asynchronous copy queued on the call's stream just before it (the array holds -1 until then: nothing present),
    sync = 0, nothing waited for until the end"""
    c = _case("48k_mono", "rb")
    bat = _batch(c)
    got, nb, fl = _ragged(dev, bat, c, hip_stream=dev.stream(), async_counts=True)
    _same_frames(got, c["want"])
    assert (nb == c["nb"]).all() and (fl == c["fl"]).all()
    bat.close()


def test_ragged_call_between_promised_dense_calls(dev):
    """under set_input_ready(1): two dense calls of 16 frames (the pipelined path, overlapping), a ragged call, two more dense calls; everything uploaded
    first, one wait at the end; every stream's frames are the oracle's"""
    fs, ms, hr, ch, rates, B = GEOMS["48k_mono"]
    T = 4 * 16 + NF
    pcm = make_pcm(fs, ms, ch, B, T, seed=91)
    start = [64000, 96000, 128000, 64000, 96000]
    sizes = np.array([nbytes_of(fs, ch, ms, hr, r) for r in start])
    stride = int(sizes.max())
    cnt = np.array([6, 0, 3, 1, 5], np.int32)
    want = OracleStreams(fs, ch, ms, hr, start).encode(pcm, nb=np.repeat(sizes[:, None], T, axis=1))
    bat = _amd().Batch(B, fs, ch, ms, hr, start, device=0)
    bat.set_input_ready(True)
    pos, plan = np.zeros(B, np.int64), []
    for kind in ("d", "d", "r", "d", "d"):
        n = 16 if kind == "d" else NF
        x = np.full((B, n, ch, pcm.shape[3]), 0x7A5A, np.int16)
        take = np.full(B, 16) if kind == "d" else cnt
        for s in range(B):
            x[s, :take[s]] = pcm[s, pos[s]:pos[s] + take[s]]
        plan.append((kind, n, take.copy(), pos.copy(), dev.put(x), dev.put(np.full((B, n, stride), SENT, np.uint8))))
        pos += take
    d_bw, d_cnt = dev.put(np.zeros((B, NF), np.int32)), dev.put(cnt)
    d_nb, d_fl = dev.put(np.full((B, NF), -7, np.int32)), dev.put(np.full((B, NF), 0xEE, np.uint8))
    for kind, n, take, p0, d_pcm, d_out in plan:
        if kind == "d":
            bat.encode_device(d_pcm, 16, n, d_out, stride)
        else:
            bat.set_frame_counts(d_cnt)
            bat.encode_device_rates(d_pcm, 16, n, d_out, stride, None, d_bw, d_nb, d_fl)
            bat.set_frame_counts(None)
    dev.sync()
    for kind, n, take, p0, d_pcm, d_out in plan:
        out = dev.get(d_out, (B, n, stride), np.uint8)
        for s in range(B):
            for t in range(n):
                if t < take[s]:
                    w = want[s][int(p0[s]) + t]
                    assert np.array_equal(out[s, t, :w.size], w) and (out[s, t, w.size:] == SENT).all(), (kind, s, t)
                else:
                    assert (out[s, t] == SENT).all()
    fl = dev.get(d_fl, (B, NF), np.uint8)
    assert (fl == np.where(np.arange(NF)[None, :] < cnt[:, None], 0, ABSENT)).all()
    bat.close()


# ---- 9. refusals ----
def test_other_calls_refuse_on_a_real_batch_and_work_again(dev):
    c = _case("48k_mono", "rb")
    amd = _amd()
    bat = _batch(c)
    B, stride = c["B"], c["stride"]
    sched = c["sched"]
    got, nb, fl = _ragged(dev, bat, c, sched=sched[:2])
    d_cnt = dev.put(sched[2])
    bat.set_frame_counts(d_cnt)
    x = np.ascontiguousarray(c["pcm"][:, :4])
    d_pcm, d_out = dev.put(x), dev.put(np.full((B, 4, stride), SENT, np.uint8))
    for call in (lambda: bat.encode(x), lambda: bat.encode(x, bitrates=np.full((B, 4), 64000, np.int32)),
                 lambda: bat.encode(x, bandwidths=np.full((B, 4), 8000, np.int32)), lambda: bat.encode_device(d_pcm, 16, 4, d_out, stride),
                 lambda: bat.encode_traced(x)):
        with pytest.raises(amd.LC3Error) as e:
            call()
        assert e.value.code == LC3_ERROR
    dev.sync()
    assert (dev.get(d_out, (B, 4, stride), np.uint8) == SENT).all()
    # the sequence goes on as if nothing had been tried
    done = sched[:2].sum(axis=0)
    got2, nb2, fl2 = _ragged(dev, bat, c, sched=sched[2:], pos0=done)
    for s in range(B):
        _same_frames([got[s][:done[s]] + got2[s][:T_TOTAL - done[s]]], [c["want"][s]])
    # counts off: the other calls are back, and continue from the configuration the ragged calls left
    sizes = np.repeat(c["nb"][:, -1:], 3, axis=1)
    tail = make_pcm(c["fs"], c["ms"], c["ch"], B, 3, seed=99)
    o = OracleStreams(c["fs"], c["ch"], c["ms"], c["hr"], c["start"])
    o.encode(c["pcm"], c["br"], c["bw"], c["nb"], c["fl"])
    w = o.encode(tail, nb=sizes)
    out = bat.encode(tail)
    for s in range(B):
        for t in range(3):
            assert np.array_equal(out[s, t, :sizes[s, t]], w[s][t]), (s, t)
    bat.close()


def test_sharded_batch_on_one_device_twice(dev):
    """devices {0, 0}: each shard takes its counts through the borrowed handle, with local stream indices, and gives the unsharded result; the sharded encode
    calls refuse while any shard has counts"""
    c = _case("48k_mono", "n")
    amd, api = _amd(), _amd().api
    B, stride, N = c["B"], c["stride"], c["N"]
    sb = amd.ShardedBatch(B, c["fs"], c["ch"], c["ms"], c["hr"], c["start"], [0, 0])
    try:
        blocks = [api.shard_block(B, 2, i) for i in range(2)]
        cnt = c["sched"][0]
        x = np.full((B, NF, 1, N), 0x7A5A, np.int16)
        for s in range(B):
            x[s, :cnt[s]] = c["pcm"][s, :cnt[s]]
        res = []
        for i, (first, count) in enumerate(blocks):
            sh = sb.shard(i)
            sh.set_frame_counts(dev.put(cnt[first:first + count]))
            d_out = dev.put(np.full((count, NF, stride), SENT, np.uint8))
            d_nb, d_fl = dev.put(np.full((count, NF), -7, np.int32)), dev.put(np.full((count, NF), 0xEE, np.uint8))
            d_bw = dev.put(np.zeros((count, NF), np.int32))
            sh.encode_device_rates(dev.put(np.ascontiguousarray(x[first:first + count])), 16, NF, d_out, stride, None, d_bw, d_nb, d_fl, sync=True)
            res.append((dev.get(d_out, (count, NF, stride), np.uint8), dev.get(d_nb, (count, NF), np.int32), dev.get(d_fl, (count, NF), np.uint8)))
        out, nb, fl = (np.concatenate([r[j] for r in res], axis=0) for j in range(3))
        for s in range(B):
            n = int(cnt[s])
            assert (fl[s] == [0] * n + [ABSENT] * (NF - n)).all() and (nb[s, n:] == 0).all() and (out[s, n:] == SENT).all()
            for t in range(n):
                assert nb[s, t] == c["nb"][s, t] and np.array_equal(out[s, t, :nb[s, t]], c["want"][s][t])
        with pytest.raises(amd.LC3Error) as e:
            sb.encode(np.ascontiguousarray(c["pcm"][:, :2]))
        assert e.value.code == LC3_ERROR
        ptrs = [dev.put(np.ascontiguousarray(x[f:f + n])) for f, n in blocks]
        outs = [dev.put(np.full((n, NF, stride), SENT, np.uint8)) for f, n in blocks]
        sb.shard(0).set_frame_counts(None)                                  # shard 1 alone still has counts: shard 0 must not be touched
        with pytest.raises(amd.LC3Error) as e:
            sb.encode_device(ptrs, 16, NF, outs, stride, sync=True)
        assert e.value.code == LC3_ERROR
        dev.sync()
        assert all((dev.get(p, (n, NF, stride), np.uint8) == SENT).all() for p, (f, n) in zip(outs, blocks))
        sb.shard(1).set_frame_counts(None)
        sb.encode_device(ptrs, 16, NF, outs, stride, sync=True)             # and works again
    finally:
        sb.close()
