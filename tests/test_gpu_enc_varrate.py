"""GPU tests of per-frame bitrates in the batched encoder (lc3plus_enc_batch_encode_bitrates, Batch.encode(bitrates=...)): streams whose
bitrate changes every one to three frames, against the CPU oracle given lc3_enc_set_bitrate before every frame (R/codec_exe.c:296-302).
Bar: bytes identical, frame for frame."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

from lc3_harness import Oracle, Trace, synth_pcm

pytestmark = pytest.mark.gpu
LC3_ERROR, LC3_BITRATE_ERROR = 1, 6
HERE = os.path.dirname(os.path.abspath(__file__))


def _amd():
    import audio_codec_amd
    return audio_codec_amd


def rate_plan(rates, B, T, seed, change=(1, 3)):
    """[B, T] bitrates drawn from `rates` anew every change[0] .. change[1] frames."""
    rng = np.random.default_rng(seed)
    out = np.zeros((B, T), np.int32)
    for b in range(B):
        t = 0
        while t < T:
            n = int(rng.integers(change[0], change[1] + 1))
            out[b, t:t + n] = int(rates[rng.integers(len(rates))])
            t += n
    return out


def make_pcm(fs, ms, channels, B, T, seed):
    N = int((48000 if fs == 44100 else fs) * ms / 1000)
    return synth_pcm(B * channels, T, N, fs, seed=seed).reshape(B, channels, T, N).transpose(0, 2, 1, 3).copy()


def oracle_frames(pcm, fs, ms, hr, br, traced=False):
    """The oracle with set_bitrate before every frame: list over streams of lists of frames (and the attack flags when traced)."""
    from audio_codec_amd.api import enc_plan_bitrates
    B, T, ch, N = pcm.shape
    nbytes = enc_plan_bitrates(fs, ch, ms, hr, br)[0]
    frames, att = [], np.zeros((B * ch, T), np.int32)
    for b in range(B):
        o = Oracle(fs, ch, ms, hr, int(br[b, 0]), portable_math=True)
        tr = o.enable_trace() if traced else None
        row = []
        for t in range(T):
            assert o.set_bitrate(int(br[b, t])) == 0
            o.nbytes = int(nbytes[b, t])                                    # the stream-frame's bytes: for an odd size not channels x the first channel's
            row.append(o.encode(pcm[b, t]))
            if traced:
                for c in range(ch):
                    att[b * ch + c, t] = tr[c].attack
        frames.append(row)
    return (frames, att) if traced else frames


def mismatches(got, nb, want, t0=0):
    bad = []
    for b in range(got.shape[0]):
        for t in range(got.shape[1]):
            w = want[b][t0 + t]
            if nb[b, t] != w.size or (got[b, t, :w.size] != w).any():
                bad.append((b, t0 + t))
    return bad


# operating points: tag, fs, frame_ms, hrmode, channels, bitrates (48 kHz / 10 ms crosses LPC weighting at 60 bytes, LTPF at 120, attack
# handling at 100 and 340 bytes; 32 kHz attack handling at 81 bytes, 44.1 kHz at 100 and 340 after the 441 / 480 scaling)
POINTS = [
    ("fb48k_10", 48000, 10.0, 0, 1, [40000, 47200, 48000, 64000, 79200, 80000, 95200, 96000, 128000, 271200, 272000, 320000]),
    ("fb48k_5", 48000, 5.0, 0, 1, [32000, 47200, 48000, 64000, 110400, 112000, 256000, 640000]),
    ("fb48k_2p5", 48000, 2.5, 0, 1, [64000, 76800, 128000, 256000, 320000, 1280000]),
    ("cd44k_10", 44100, 10.0, 0, 1, [14700, 44100, 64000, 73400, 73500, 128000, 249800, 249900, 294000]),
    ("swb32k_10", 32000, 10.0, 0, 1, [16000, 38400, 64000, 64000 + 800, 96000, 271200, 272000, 320000]),
    ("wb16k_10", 16000, 10.0, 0, 1, [16000, 24000, 32000, 64000, 128000, 320000]),
    ("nb8k_10", 8000, 10.0, 0, 1, [16000, 24000, 32000, 64000, 320000]),
    ("fb48k_10_stereo", 48000, 10.0, 0, 2, [80000, 96000, 128000, 128800, 160800, 200000, 232800, 544000, 640000]),
    ("hr48k_10", 48000, 10.0, 1, 1, [124800, 160000, 256000, 400000, 500000]),
    ("hr96k_2p5", 96000, 2.5, 1, 1, [198400, 256000, 400000, 672000]),
    ("hr96k_10", 96000, 10.0, 1, 1, [149600, 256000, 400000, 500000]),        # the large layout
]


@pytest.mark.parametrize("tag,fs,ms,hr,ch,rates", POINTS, ids=[p[0] for p in POINTS])
def test_parity_with_oracle_short_and_long_calls(tag, fs, ms, hr, ch, rates):
    B, Ts, Tl = 4, 6, 26
    T = Ts + Tl
    pcm = make_pcm(fs, ms, ch, B, T, seed=11)
    br = rate_plan(rates, B, T, seed=zlib.crc32(tag.encode()))
    want = oracle_frames(pcm, fs, ms, hr, br)
    b = _amd().Batch(B, fs, ch, ms, hr, [int(x) for x in br[:, 0]])
    bad = []
    for t0, n in ((0, Ts), (Ts, Tl)):                                       # a short call (in-kernel writer territory) and a long one
        out = b.encode(pcm[:, t0:t0 + n], bitrates=br[:, t0:t0 + n])
        bad += mismatches(out, b.last_num_bytes, want, t0)
    assert not bad, (tag, len(bad), bad[:8])
    assert [b.num_bytes(s) for s in range(B)] == [want[s][-1].size for s in range(B)]


def test_attack_detector_reset_and_restart():
    """Attack handling switched off and on again within calls, on PCM with transients: the detector is cleared by every frame whose rate
    disables it and restarts from there; its flag (stage trace) and the bytes equal the oracle's, and it fires after off -> on transitions."""
    fs, ms, B, T = 48000, 10.0, 6, 30
    N = 480
    rng = np.random.default_rng(5)
    pcm = (rng.standard_normal((B, T, 1, N)) * 200).astype(np.int16)
    for b in range(B):
        for t in range(1, T, 3):                                            # a click every third frame, at a different place each time
            k = int(rng.integers(0, N - 8))
            pcm[b, t, 0, k:k + 8] = 20000
    on, off = [96000, 128000, 200000], [64000, 320000]
    br = np.zeros((B, T), np.int32)
    for b in range(B):
        for t in range(T):
            br[b, t] = (on if (t // (1 + b % 3)) % 2 else off)[(b + t) % (2 if (t // (1 + b % 3)) % 2 == 0 else 3)]
    want, watt = oracle_frames(pcm, fs, ms, 0, br, traced=True)
    b = _amd().Batch(B, fs, 1, ms, 0, [int(x) for x in br[:, 0]])
    out, traces = b.encode_traced(pcm, bitrates=br)
    assert not mismatches(out, b.last_num_bytes, want)
    got = np.array([[Trace.from_buffer_copy(traces[s * T + t].tobytes()[:C.sizeof(Trace)]).attack for t in range(T)] for s in range(B)])
    assert (got == watt).all(), (got, watt)
    after = [(s, t) for s in range(B) for t in range(1, T) if br[s, t - 1] in off and br[s, t] in on and got[s, t:t + 3].any()]
    assert after, "no attack detected after an off -> on transition: the case does not exercise the reset"
    # and the untraced call gives the same bytes
    b2 = _amd().Batch(B, fs, 1, ms, 0, [int(x) for x in br[:, 0]])
    assert not mismatches(b2.encode(pcm, bitrates=br), b2.last_num_bytes, want)


@pytest.mark.parametrize("T", [3, 24])
def test_same_rate_everywhere_equals_encode(T):
    fs, ms, B = 48000, 10.0, 8
    rates = [64000, 96000, 128000, 32000, 256000, 80000, 48000, 160000]
    pcm = make_pcm(fs, ms, 1, B, T, seed=3)
    a = _amd().Batch(B, fs, 1, ms, 0, rates)
    v = _amd().Batch(B, fs, 1, ms, 0, rates)
    ref = a.encode(pcm)
    got = v.encode(pcm, bitrates=np.repeat(np.array(rates, np.int32)[:, None], T, axis=1))
    for s in range(B):
        assert (got[s, :, :rates[s] // 800] == ref[s, :, :rates[s] // 800]).all(), s
        assert (v.last_num_bytes[s] == rates[s] // 800).all()


def test_continuity_encode_and_checkpoint():
    fs, ms, B = 48000, 10.0, 4
    rates = [40000, 64000, 96000, 128000, 272000]
    pcm = make_pcm(fs, ms, 1, B, 40, seed=9)
    br = rate_plan(rates, B, 12, seed=4)
    last = br[:, -1]
    full = np.concatenate([br, np.repeat(last[:, None], 28, axis=1)], axis=1)
    want = oracle_frames(pcm, fs, ms, 0, full)
    b = _amd().Batch(B, fs, 1, ms, 0, [64000] * B)
    out = b.encode(pcm[:, :12], bitrates=br)
    assert not mismatches(out, b.last_num_bytes, want)
    assert [b.num_bytes(s) for s in range(B)] == [int(x) * 480 // 384000 for x in last]
    assert b.stride == max(int(x) * 480 // 384000 for x in last)
    out = b.encode(pcm[:, 12:28])                                           # encode() continues from each stream's last rate
    nb = np.array([[b.num_bytes(s)] * 16 for s in range(B)])
    assert not mismatches(out, nb, want, 12)
    st = b.get_state()
    c = _amd().Batch(B, fs, 1, ms, 0, [int(x) for x in last])              # a checkpoint resumes on a batch created with those rates
    c.set_state(st)
    out = c.encode(pcm[:, 28:40])
    assert not mismatches(out, np.array([[c.num_bytes(s)] * 12 for s in range(B)]), want, 28)


def test_validation_leaves_the_batch_unchanged():
    from audio_codec_amd.api import LC3Error
    fs, ms, B, T = 48000, 10.0, 3, 10
    pcm = make_pcm(fs, ms, 1, B, 2 * T, seed=2)
    br = rate_plan([48000, 64000, 96000, 128000], B, T, seed=8)
    a = _amd().Batch(B, fs, 1, ms, 0, [64000, 80000, 96000])
    ref = _amd().Batch(B, fs, 1, ms, 0, [64000, 80000, 96000])
    for bad_rate in (0, -1, 15999, 320001):
        bad = br.copy(); bad[2, T - 1] = bad_rate
        with pytest.raises(LC3Error) as e:
            a.encode(pcm[:, :T], bitrates=bad)
        assert e.value.code == LC3_BITRATE_ERROR
    out = np.zeros((B, T, 100), np.uint8)                                   # a stride below the call's largest frame (120 bytes)
    rc = a.lib.lc3plus_enc_batch_encode_bitrates(a.h, pcm.ctypes.data, 0, 16, np.ascontiguousarray(br).ctypes.data, T, out.ctypes.data, 100, 0,
                                                 None, None, 1)
    assert rc == LC3_ERROR
    assert [a.num_bytes(s) for s in range(B)] == [80, 100, 120] and a.stride == 120
    g1, g2 = a.encode(pcm[:, :T], bitrates=br), ref.encode(pcm[:, :T], bitrates=br)
    assert (g1 == g2).all()
    assert (a.encode(pcm[:, T:]) == ref.encode(pcm[:, T:])).all()


class _Dev:
    """Device buffers through ctypes (hipMalloc / hipMemcpy)."""
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so"); self.ptrs = []
    def put(self, arr):
        arr = np.ascontiguousarray(arr); p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(arr.nbytes)) == 0
        assert self.hip.hipMemcpy(p, C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), C.c_int(1)) == 0
        self.ptrs.append(p); return p.value
    def get(self, ptr, shape, dtype):
        out = np.zeros(shape, dtype)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), C.c_int(2)) == 0
        return out
    def sync(self):
        assert self.hip.hipDeviceSynchronize() == 0
    def free(self):
        for p in self.ptrs: self.hip.hipFree(p)
        self.ptrs = []


def test_device_pointers_sync0_and_untouched_tail():
    fs, ms, B, T, K = 48000, 10.0, 64, 16, 3
    rates = [48000, 64000, 96000, 128000, 200000]
    pcm = make_pcm(fs, ms, 1, B, K * T, seed=6)
    br = rate_plan(rates, B, K * T, seed=12)
    host = _amd().Batch(B, fs, 1, ms, 0, [64000] * B)
    dev = _amd().Batch(B, fs, 1, ms, 0, [64000] * B)
    d = _Dev()
    try:
        stride = 256
        for k in range(K):                                                  # K calls queued without a host synchronisation
            # the pcm of call k: frames k*T .. of every stream are not contiguous across streams, so each call gets its own copy
            dpk = d.put(pcm[:, k * T:(k + 1) * T])
            dok = d.put(np.full((B, T, stride), 0xA5, np.uint8))
            dev.encode_device(dpk, 16, T, dok, stride, sync=False, bitrates=br[:, k * T:(k + 1) * T])
            nb_k = dev.last_num_bytes.copy()
            d.sync()
            got = d.get(dok, (B, T, stride), np.uint8)
            want = host.encode(pcm[:, k * T:(k + 1) * T], bitrates=br[:, k * T:(k + 1) * T])
            assert (nb_k == host.last_num_bytes).all()
            for s in range(B):
                for t in range(T):
                    n = nb_k[s, t]
                    assert (got[s, t, :n] == want[s, t, :n]).all(), (k, s, t)
                    assert (got[s, t, n:] == 0xA5).all(), (k, s, t)
    finally:
        d.free()


def test_mixing_with_promised_encode_calls():
    """Under the input-ready promise per-frame calls run between promised encode() calls of the pipelined and the short path."""
    fs, ms, B = 48000, 10.0, 256
    rates = [64000, 96000, 128000]
    seq = [("fix", 16), ("var", 16), ("fix", 16), ("var", 4), ("fix", 4), ("fix", 24), ("var", 24), ("fix", 16)]
    T = sum(n for _, n in seq)
    pcm = make_pcm(fs, ms, 1, B, T, seed=21)
    br = rate_plan(rates, B, T, seed=22)
    init = [int(x) for x in br[:, 0]]
    ref = _amd().Batch(B, fs, 1, ms, 0, init)
    b = _amd().Batch(B, fs, 1, ms, 0, init)
    d = _Dev()
    try:
        b.set_input_ready(True)
        outs, t0 = [], 0
        for kind, n in seq:
            dp = d.put(pcm[:, t0:t0 + n]); do = d.put(np.zeros((B, n, 160), np.uint8))
            if kind == "var":
                b.encode_device(dp, 16, n, do, 160, sync=False, bitrates=br[:, t0:t0 + n])
                want = ref.encode(pcm[:, t0:t0 + n], bitrates=br[:, t0:t0 + n]); nb = ref.last_num_bytes.copy()
            else:
                b.encode_device(dp, 16, n, do, 160, sync=False)
                want = ref.encode(pcm[:, t0:t0 + n]); nb = np.array([[ref.num_bytes(s)] * n for s in range(B)])
            outs.append((do, n, want, nb))
            t0 += n
        d.sync()
        for i, (do, n, want, nb) in enumerate(outs):
            got = d.get(do, (B, n, 160), np.uint8)
            bad = [(s, t) for s in range(B) for t in range(n) if (got[s, t, :nb[s, t]] != want[s, t, :nb[s, t]]).any()]
            assert not bad, (i, seq[i], len(bad), bad[:6])
        b.set_input_ready(False)
    finally:
        d.free()


def test_last_status_reports_the_call():
    fs, ms, B, T = 48000, 10.0, 4, 12
    pcm = make_pcm(fs, ms, 2, B, T, seed=4)
    br = rate_plan([128000, 160800, 232800], B, T, seed=1)
    b = _amd().Batch(B, fs, 2, ms, 0, [128000] * B)
    b.encode(pcm, bitrates=br)
    st = np.full(B * 2 * T, 0xFF, np.uint8)
    n = b.lib.lc3plus_enc_batch_last_status(b.h, st.ctypes.data, st.size)
    assert n == B * 2 * T and (st == 0).all()


def test_reference_golden():
    """tests/golden/e2_variable_bitrates.npz: frames the ETSI reference encoder made with lc3_enc_set_bitrate before every frame."""
    z = np.load(os.path.join(HERE, "golden", "e2_variable_bitrates.npz"))
    tags = sorted({k.split("/")[0] for k in z.files})
    assert len(tags) == 11
    bad = {}
    for tag in tags:
        fs, ms, hr, ch = (int(x) if i != 1 else float(x) for i, x in enumerate(z[tag + "/cfg"]))
        pcm, br, frames, sizes = z[tag + "/pcm"], z[tag + "/bitrates"], z[tag + "/frames"], z[tag + "/sizes"]
        B, T = br.shape
        b = _amd().Batch(B, fs, ch, ms, hr, [int(x) for x in br[:, 0]])
        n = []
        for t0, m in ((0, 6), (6, T - 6)):
            out = b.encode(pcm[:, t0:t0 + m], bitrates=br[:, t0:t0 + m])
            assert (b.last_num_bytes == sizes[:, t0:t0 + m]).all(), tag
            n += [(s, t0 + t) for s in range(B) for t in range(m) if (out[s, t, :sizes[s, t0 + t]] != frames[s, t0 + t, :sizes[s, t0 + t]]).any()]
        if n:
            bad[tag] = n[:6]
    assert not bad, bad


def test_host_pointers_in_overlapped_runs_equal_device_pointers():
    """A host-pointer call large enough to be cut into several runs of frames (the in-kernel writer then addresses the call's frames by run
    offset) gives the bytes of the same call through device pointers."""
    fs, ms, B, T = 48000, 10.0, 4096, 32                                   # 126 MB of PCM: three runs
    pcm = np.ascontiguousarray(np.tile(make_pcm(fs, ms, 1, 64, T, seed=17), (B // 64, 1, 1, 1)))
    br = rate_plan([32000, 64000, 96000, 128000, 256000], B, T, seed=31)
    init = [int(x) for x in br[:, 0]]
    h = _amd().Batch(B, fs, 1, ms, 0, init)
    dv = _amd().Batch(B, fs, 1, ms, 0, init)
    stride = 320
    out_h = np.full((B, T, stride), 0x5A, np.uint8)
    rc = h.lib.lc3plus_enc_batch_encode_bitrates(h.h, pcm.ctypes.data, 0, 16, np.ascontiguousarray(br).ctypes.data, T, out_h.ctypes.data, stride, 0,
                                                 None, None, 1)
    assert rc == 0
    d = _Dev()
    try:
        dp = d.put(pcm); do = d.put(np.full((B, T, stride), 0x5A, np.uint8))
        dv.encode_device(dp, 16, T, do, stride, sync=True, bitrates=br)
        out_d = d.get(do, (B, T, stride), np.uint8)
    finally:
        d.free()
    nb = dv.last_num_bytes
    assert (nb == br * 480 // 384000).all()
    bad = [(s, t) for s in range(B) for t in range(T) if (out_h[s, t, :nb[s, t]] != out_d[s, t, :nb[s, t]]).any()]
    assert not bad, (len(bad), bad[:8])
    s, t = np.nonzero(nb < stride)
    assert (out_d[s, t, nb[s, t]] == 0x5A).all()                           # behind each frame: untouched (host calls: as encode() leaves them)


@pytest.mark.parametrize("fs,ms,channels,rates,g192", [(48000, 10.0, 1, [40000, 48000, 64000, 80000, 96000, 128000, 272000, 320000], 0),
                                                        (48000, 10.0, 1, [40000, 64000, 96000, 120000], 1),
                                                        (48000, 10.0, 2, [40000, 64000, 96000, 128000], 1),
                                                        (32000, 5.0, 1, [32000, 64000, 96000], 0)])
def test_cli_bitrate_switching_file_against_the_reference_cli(tmp_path, fs, ms, channels, rates, g192):
    """tools/lc3plus_enc_cli -swf against the reference CLI (oracle/_ref/LC3plus -E -swf) on a switching file with a new rate every 1-3 frames
    over more than one block of 256 frames, in the .lc3plus container and in G.192: identical files."""
    import subprocess
    from lc3_harness import ORACLE_DIR
    from test_gpu_parity import _write_wav
    ref_cli = os.path.join(ORACLE_DIR, "_ref", "LC3plus")
    if not os.path.exists(ref_cli):
        pytest.skip("the reference CLI (oracle/_ref/LC3plus) is not built")
    root = os.path.dirname(HERE)
    cli = os.path.join(root, "tools", "lc3plus_enc_cli")
    subprocess.check_call(["make", "-s", "-C", root, "cli"])
    rng = np.random.default_rng(fs + channels + g192)
    N = int(fs * ms / 1000); T = 600                                   # more than two blocks of 256 frames
    pcm = synth_pcm(channels, T, N, fs, seed=47)
    wav = tmp_path / "in.wav"
    _write_wav(wav, pcm.reshape(channels, -1).T.reshape(-1)[:T * N * channels - 77 * channels], fs, channels, 16)   # last frame partial
    plan = []
    while len(plan) < T:
        plan += [int(rates[rng.integers(len(rates))])] * int(rng.integers(1, 4))
    swf = tmp_path / "rates.swf"; np.array(plan[:T], dtype="<i8").tofile(swf)       # per channel (R/codec_exe.c:296-302)
    fmt = ["-formatG192"] if g192 else []
    ours, theirs = tmp_path / "ours.bit", tmp_path / "ref.bit"
    subprocess.check_call([cli, "-E", "-q", "-frame_ms", str(ms), "-swf", str(swf)] + fmt + [str(wav), str(ours), str(rates[0])])
    subprocess.check_call([ref_cli, "-E", "-q", "-frame_ms", str(ms), "-swf", str(swf)] + fmt + [str(wav), str(theirs), str(rates[0])],
                          stdout=subprocess.DEVNULL)
    got, ref = open(ours, "rb").read(), open(theirs, "rb").read()
    assert len(got) == len(ref) and got == ref
    if g192:
        assert open(str(ours) + ".cfg", "rb").read() == open(str(theirs) + ".cfg", "rb").read()
