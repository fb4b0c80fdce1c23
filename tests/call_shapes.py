"""The shape of a call (test helper beside size_sweep.py and launch_census.py, TEST INFRASTRUCTURE ONLY): how many frames a call holds, how many channel-streams
the batch has, and which call came before it on the same batch.

1. A Python restatement of every rule by which audio_codec_amd/csrc/lc3_runtime.hip sizes a launch from the call's shape (enc_launch, enc_pipelined, enc_run,
   enc_writer; dec_parse_lds, dec_parse, dec_chain): enc_shape(), dec_shape(), and from them expected_launches() - the launch counts of the kernels that expose a
   rule.  tests/test_call_shapes_cpu.py holds its constants against the #defines and defaults of the sources.
2. The sequences: one batch each and a list of consecutive call lengths in a fixed shuffled order, so that every path hands its state to every other one.  The
   lengths are the smallest at which each rule can go wrong and are produced from the restatement's constants (enc_ordered_lengths, dec_ordered_lengths ...).
3. The inputs, all from seeds: encoder PCM with onsets laid on call boundaries (enc_pcm), decoder bitstreams with the loss pattern laid out against the call
   boundaries, one role per stream (loss_roles, dec_case), and the oracle's continuous run over each (oracle_encode, oracle_decode).
4. all_enc_calls(): every encoder call of every sequence with its shape, from which tests/test_call_shapes_cpu.py takes its census - which rule is reached below, at
   and above its threshold, and which grid tail with remainders 0, 1 and unit - 1, in which kernel family.

tests/test_gpu_call_shapes.py makes the calls; every comparison there is equality with the CPU oracle (lc3_harness.Oracle with portable math through the oracle's
batch entry, and OracleDecoder)."""
import collections
import concurrent.futures
import ctypes as C
import functools
import os

import numpy as np

from lc3_harness import ORACLE_DIR, Oracle, OracleDecoder, synth_pcm

# ---- the constants of the restatement (lc3_runtime.hip, lc3_launch.h, lc3_plan.h; test_call_shapes_cpu.test_constants_are_the_sources) ------------------------
WAVE = 64
LC3D_RUN_FRAMES, LC3D_RUN_FRAMES_READY, LC3D_MAX_RUNS = 16, 64, 16
LC3D_FUSED_MAX_T, LC3D_FUSED_MAX_T_READY = 8, 5
LC3D_AHEAD_MAX_FRAMES = 256
FRONT_FPW, FM_F240, FM_SHORT, FRONT4_FPW = 4, 4, 8, 4
IMDCT_FPW, IMDCT4_FPW = 8, 4
RATE_WG = 4
LC3D_SETS = DEC_SETS = 3
PRE_RUNS = 3                                       # read_opts: LC3PLUS_ENC_PRE_RUNS
PACK_WPG = 4                                       # read_opts: LC3PLUS_ENC_PACK_WPG
W5_MIN_FRAMES, W5_MAX_BYTES = 48, 100              # enc_writer: dT >= 48 && max_nbytes <= 100
RATE_MEAN_BYTES, RATE_SHORT_CALL = 120, 32         # enc_pipelined want_rt: mean_nbytes >= 120 || n_frames <= 32
RATE_FRONT_LO, RATE_FRONT_HI, RATE_FRONT_MASK = 16, 24, 3      # enc_pipelined on_pre: !(mean < 120 && 16 <= n <= 24 && !(n & 3))
SHAPE_ON_PITCH_FRAMES, SHAPE_ON_PITCH_N = 128, 240             # enc_run sop: hr && N == 240 && n_frames >= 128
PARSE_LDS_MAX_BYTES, PARSE_MAX_WPG = 128, 4        # dec_parse_lds
PLAN_WG = 256                                      # dec_plan, dec_tail: stream-frames per workgroup
PLC_RAMP = 8                                       # the concealment's per-frame factor takes its last value at the eighth lost frame (R/plc_noise_substitution0.c)
TWIN_CALL = 12                                     # the twin batch takes the same frames in calls of 12

FRONTS = ("lc3_enc_front4_kernel", "lc3_enc_frontm_kernel", "lc3_enc_front_kernel", "lc3_enc_front_kernel_big")
WRITERS = ("lc3_enc_pack_kernel", "lc3_enc_pack_kernel_w5")
ONE_WAVE = ("lc3_encode_kernel", "lc3_encode_kernel_big")
RATES = ("lc3_enc_rate_kernel", "lc3_enc_rate_kernel_big")
PARSERS = ("lc3_dec_parse_kernel", "lc3_dec_parse_kernel_g", "lc3_dec_parse_kernel_var", "lc3_dec_parse_kernel_g_var")
IMDCTS = ("lc3_dec_imdct4_kernel", "lc3_dec_imdct_kernel", "lc3_dec_imdct_kernel_big")
ENC_KERNELS = FRONTS + WRITERS + ONE_WAVE + RATES + ("lc3_enc_hp50_kernel",)
DEC_KERNELS = PARSERS + IMDCTS


def _api():
    import audio_codec_amd
    return audio_codec_amd.api


def frame_len(fs, ms):
    return int(fs * ms / 1000)


def is_big(fs, ms):
    """LC3D_LAYOUT_BIG: 96 kHz / 10 ms and 96 kHz / 5 ms"""
    return fs == 96000 and ms >= 5.0


# ---- the families -------------------------------------------------------------------------------------------------------------------------------------------
# name -> fs, frame_ms, hrmode, channels, one bitrate per stream (five: odd, no multiple of RATE_WG, 5 * nt never a whole wave)
ENC_FAMILIES = collections.OrderedDict([
    # 50 ... 90 bytes: front4, pitch2, resample48, the five-wave writer.  (No stream above 100 bytes - 80 kbit/s: one would switch that writer off for the batch -
    # and none at 100, where attack handling starts: the family without the attack kernel.  96 kbit/s is in the stream-count batches, the limit itself - 100 and 101 bytes - in ENC_TAIL_BATCHES.)
    ("48k_10_small", (48000, 10.0, 0, 1, (40000, 48000, 56000, 64000, 72000))),
    ("48k_10_large", (48000, 10.0, 0, 1, (128000, 160000, 192000, 256000, 320000))),     # mean size >= 120: the other rate-stream rule, and the attack kernel
    ("48k_5_stereo", (48000, 5.0, 0, 2, (129600, 161600, 97600, 193600, 65600))),        # 81, 101, 61, 121, 41 bytes: frontm, pitch2_l64
    ("48k_2p5", (48000, 2.5, 0, 1, (64000, 96000, 128000, 195200, 259200))),             # front, pitch2_l32
    ("32k_10", (32000, 10.0, 0, 1, (32000, 48000, 64000, 96000, 128000))),               # front with the generic resampler; attack handling from 81 bytes
    ("96k_2p5_hr", (96000, 2.5, 1, 1, (198400, 256000, 320000, 400000, 480000))),        # N = 240: frontm, the shape kernel's stream at 128
    ("96k_10", (96000, 10.0, 1, 1, (149600, 256000, 400000, 300000, 200000))),           # the large layout
    ("16k_2p5", (16000, 2.5, 0, 1, (64000, 80000, 96000, 128000, 160000))),              # 20 ... 50 bytes, N = 40: frontm with eight frames a wave
])
ENC_READY_FAMILIES = collections.OrderedDict([
    ("48k_10_small", ENC_FAMILIES["48k_10_small"]),
    ("48k_10_stereo", (48000, 10.0, 0, 2, (128800, 160800, 96000, 200800, 80800))),      # 161, 201, 120, 251, 101 bytes
    ("48k_5_stereo", ENC_FAMILIES["48k_5_stereo"]),
    ("32k_10", ENC_FAMILIES["32k_10"]),
    ("96k_10", ENC_FAMILIES["96k_10"]),
])
COUNT_RATES = (40000, 64000, 96000, 48000, 80000)
# name -> fs, frame_ms, hrmode, channels, stream count, bitrates in turn
ENC_COUNT_BATCHES = collections.OrderedDict(
    [("mono_%d" % n, (48000, 10.0, 0, 1, n, COUNT_RATES)) for n in (1, 2, 63, 64, 65)] + [("stereo_3", (48000, 10.0, 0, 2, 3, (128800, 160800, 96000)))])
# One stream on either side of the five-wave writer's size limit: 100 bytes (that writer) and 101 (lc3_enc_pack_kernel), at a whole writer workgroup of frames and one
# frame either side - each writer's grid tail with remainders 255, 0 and 1, and max_nbytes <= 100 at 100 and above it (both below a mean of 120 bytes: the second
# rate-stream rule applies).
ENC_TAIL_BATCHES = collections.OrderedDict([("one_100B", (48000, 10.0, 0, 1, 1, (80000,))), ("one_101B", (48000, 10.0, 0, 1, 1, (80800,)))])
# name -> fs, frame_ms, hrmode, channels, stream-frame bytes of every stream
DEC_FAMILIES = collections.OrderedDict([
    ("48k_10_80B", (48000, 10.0, 0, 1, (80,) * 5)),                          # imdct4, the LDS parser
    ("48k_10_160B", (48000, 10.0, 0, 1, (160,) * 5)),                        # the global parser
    ("48k_10_stereo", (48000, 10.0, 0, 2, (161, 201, 121, 141, 181))),       # odd sizes: the channels differ in bytes
    ("32k_5", (32000, 5.0, 0, 1, (40,) * 5)),                                # imdct
    ("96k_10", (96000, 10.0, 1, 1, (250,) * 5)),                             # imdct_big
])
DEC_READY_FAMILIES = ("48k_10_80B", "32k_5")
STEREO_CORRUPT_STREAM = 2          # in stereo this stream's losses are corrupt first channels, not flags


def enc_family(name):
    if name in ENC_FAMILIES or name in ENC_READY_FAMILIES:
        return ENC_FAMILIES[name] if name in ENC_FAMILIES else ENC_READY_FAMILIES[name]
    fs, ms, hr, ch, n, rates = ENC_COUNT_BATCHES[name] if name in ENC_COUNT_BATCHES else ENC_TAIL_BATCHES[name]
    return fs, ms, hr, ch, tuple(rates[i % len(rates)] for i in range(n))


@functools.lru_cache(maxsize=None)
def enc_geometry(name):
    """what lc3hip_create and lc3hip_upload_chans keep of a batch: dict(fs, ms, hr, ch, rates, S, ncs, N, big, nbytes (stream-frames), chan_bytes, mean_nbytes,
    max_nbytes, any_attack)"""
    api = _api()
    fs, ms, hr, ch, rates = enc_family(name)
    nbytes = [int(api.enc_plan_bitrates(fs, ch, ms, hr, [[r]])[0][0, 0]) for r in rates]
    chan = [n // ch + (c < n % ch) for n in nbytes for c in range(ch)]
    return dict(name=name, fs=fs, ms=ms, hr=hr, ch=ch, rates=rates, S=len(rates), ncs=len(rates) * ch, N=frame_len(fs, ms), big=is_big(fs, ms), nbytes=nbytes,
                chan_bytes=chan, mean_nbytes=sum(chan) // len(chan), max_nbytes=max(chan),
                any_attack=any(api.plan_chan(fs, ms, hr, n)["attack_handling"] for n in chan))


@functools.lru_cache(maxsize=None)
def dec_geometry(name, S=None):
    fs, ms, hr, ch, sizes = DEC_FAMILIES[name]
    if S is not None:
        sizes = tuple(sizes[i % len(sizes)] for i in range(S))
    chan = [n // ch + (c < n % ch) for n in sizes for c in range(ch)]
    ltpf = [_api().plan_chan(fs, ms, hr, n)["ltpf_enable"] for n in chan]
    return dict(name=name, fs=fs, ms=ms, hr=hr, ch=ch, sizes=sizes, S=len(sizes), ncs=len(sizes) * ch, N=frame_len(fs, ms), big=is_big(fs, ms), chan_bytes=chan,
                ltpf=ltpf)


# ---- the restatement: encoder ---------------------------------------------------------------------------------------------------------------------------------
def front_of(g):
    """enc_run: (front kernel, frames per wave at full runs)"""
    if g["big"]:
        return "lc3_enc_front_kernel_big", FRONT_FPW
    if g["N"] == 480 and g["ms"] == 10.0:          # la == 180, ylen 400 or 480: a multiple of 16
        return "lc3_enc_front4_kernel", FRONT4_FPW
    if g["N"] == 240:                              # lc3hip_create: fm_frames
        return "lc3_enc_frontm_kernel", FM_F240
    if g["N"] == 40:                               # ... N <= 120 with radices up to 8 (a 20-point transform: 4 x 5)
        return "lc3_enc_frontm_kernel", FM_SHORT
    assert (g["fs"], g["ms"]) in ((48000, 2.5), (32000, 10.0)), g["name"]       # N = 120 (radices above 8) and N = 320: no frontm
    return "lc3_enc_front_kernel", FRONT_FPW


def enc_runs(n, ready=False, run_frames=0, runs=0):
    """enc_pipelined: (R, Tr, [run lengths]).  run_frames, runs: LC3PLUS_ENC_RUN_FRAMES, LC3PLUS_ENC_RUNS"""
    runf = run_frames or (LC3D_RUN_FRAMES_READY if ready else LC3D_RUN_FRAMES)
    R = max(1, min(LC3D_MAX_RUNS, -(-n // runf)))
    if runs:
        R = runs
    Tr = -(-n // R)
    return R, Tr, [min(Tr, n - tb) for tb in range(0, n, Tr)]


def enc_shape(g, n, ready=False, prev=None, run_frames=0):
    """What a dense device-pointer call of n frames does on batch g; prev: the shape of the call before it on the batch (None: the first call, or the promise
    was given or withdrawn in between)."""
    one_wave = n <= (LC3D_FUSED_MAX_T_READY if ready else LC3D_FUSED_MAX_T)
    sh = dict(n=n, ready=ready, path="one_wave" if one_wave else "pipelined", overlaps=False, R=0, Tr=0, runs=[], pieces=1, front=None, fpw=0, writer=None,
              rate_stream=None, shape_stream=None)
    if one_wave:
        return sh
    R, Tr, runs = enc_runs(n, ready, run_frames)
    front, fpw = front_of(g)
    mean = g["mean_nbytes"]
    want_rt = not g["big"] and (mean >= RATE_MEAN_BYTES or n <= RATE_SHORT_CALL)
    on_pre = not (g["big"] or (mean < RATE_MEAN_BYTES and RATE_FRONT_LO <= n <= RATE_FRONT_HI and not n & RATE_FRONT_MASK))
    w5 = not g["big"] and not g["hr"] and g["N"] == 480 and n >= W5_MIN_FRAMES and g["max_nbytes"] <= W5_MAX_BYTES
    sh.update(R=R, Tr=Tr, runs=runs, pieces=1 + -(-(n - runs[0]) // (PRE_RUNS * Tr)), front=front, fpw=fpw,
              front_fpw=[min(nt, FRONT_FPW) if front.startswith("lc3_enc_front_kernel") else fpw for nt in runs],
              writer=WRITERS[1] if w5 else WRITERS[0], rate_stream=("pitch" if on_pre else "front") if want_rt else "caller",
              shape_stream="pitch" if g["hr"] and g["N"] == SHAPE_ON_PITCH_N and n >= SHAPE_ON_PITCH_FRAMES else "front",
              overlaps=bool(ready and n <= LC3D_AHEAD_MAX_FRAMES and prev and prev["path"] == "pipelined" and prev["ready"] and prev["n"] == n and prev["R"] == R))
    return sh


def expected_enc_launches(g, sh):
    """launch counts of the kernels that expose a rule, every name of ENC_KERNELS (0: must not run)"""
    e = dict.fromkeys(ENC_KERNELS, 0)
    e["lc3_enc_hp50_kernel"] = sh["pieces"]                            # one launch per piece (the one-wave path: one in front of its kernel)
    if sh["path"] == "one_wave":
        e[ONE_WAVE[1] if g["big"] else ONE_WAVE[0]] = 1
        return e
    e[RATES[1] if g["big"] else RATES[0]] = len(sh["runs"])            # one launch per run
    e[sh["front"]] = len(sh["runs"])
    e[sh["writer"]] = 1
    return e


# ---- the restatement: decoder ---------------------------------------------------------------------------------------------------------------------------------
PARSE_STATIC_BYTES = 2 * (64 * 32 + 8) + 2 * (18 + 144) + 4096 + 4 * 176 + 4 * 45       # sizeof(ParseLds), lc3_launch.h (16-byte aligned below)


def parse_wpg(N, max_nb):
    """dec_parse_lds: (nw_max, waves per parse workgroup).  The rule yields PARSE_MAX_WPG for every frame there is: a lane stages at most 32 words (128 bytes) beside
    at most 15 words of the row (N > 480), 47 * 256 bytes per wave, and four of those fit beside the static tables
    (test_call_shapes_cpu.test_no_frame_takes_fewer_parse_waves) - so no geometry exercises a smaller workgroup."""
    nw_max = 0 if max_nb > PARSE_LDS_MAX_BYTES else (max_nb + 3) // 4 if max_nb > 0 else 1
    nlw = ((960 if N > 480 else 480) // 2 + 31) // 32
    per_wave = (nw_max + nlw) * WAVE * 4
    return nw_max, min(PARSE_MAX_WPG, (64 * 1024 - (PARSE_STATIC_BYTES + 15) // 16 * 16) // per_wave)


def dec_shape(g, n, how, max_nb):
    """how: "fixed" (decode_device without sizes), "hostsizes" (decode_device with host sizes and flags), "sizes" (decode_device_sizes).  max_nb: the largest channel
    frame the host knows of - fixed: of the configuration; hostsizes: of the call's frames that are not lost; sizes: a channel's share of in_stride."""
    nw_max, wpg = parse_wpg(g["N"], max_nb)
    parser = "lc3_dec_parse_kernel" + ("" if nw_max else "_g") + ("" if how == "fixed" else "_var")
    imdct, fpw = (IMDCTS[2], IMDCT_FPW) if g["big"] else (IMDCTS[0], IMDCT4_FPW) if g["N"] == 480 else (IMDCTS[1], IMDCT_FPW)
    return dict(n=n, how=how, parser=parser, wpg=wpg, imdct=imdct, fpw=fpw)


def expected_dec_launches(g, sh):
    e = dict.fromkeys(DEC_KERNELS, 0)
    e[sh["parser"]] = 1
    e[sh["imdct"]] = 1
    return e


def expected_launches(kind, g, sh):
    return expected_enc_launches(g, sh) if kind == "enc" else expected_dec_launches(g, sh)


# ---- the sequences --------------------------------------------------------------------------------------------------------------------------------------------
def _shuffled(lengths, seed):
    return tuple(int(x) for x in np.random.RandomState(seed).permutation(np.array(sorted(lengths))))


def enc_ordered_lengths():
    """1; both sides of the one-wave limit; one frame below, at and above one, two, three (the five-wave writer's 48) and four runs; 128 / 129 (the shape kernel's
    stream); the last length with runs of 16 and the first with runs of 17 (fifteen of 17 and one of 2); fifteen runs of 18 and one of 3"""
    r, m = LC3D_RUN_FRAMES, LC3D_MAX_RUNS
    assert W5_MIN_FRAMES == 3 * r
    return sorted({1, LC3D_FUSED_MAX_T, LC3D_FUSED_MAX_T + 1, r - 1, r, r + 1, 2 * r, 2 * r + 1, W5_MIN_FRAMES - 1, W5_MIN_FRAMES, W5_MIN_FRAMES + 1, 4 * r, 4 * r + 1,
                   SHAPE_ON_PITCH_FRAMES, SHAPE_ON_PITCH_FRAMES + 1, m * r, m * r + 1, (m - 1) * (r + 2) + 3})


def enc_count_lengths():
    return sorted({1, LC3D_FUSED_MAX_T + 1, LC3D_RUN_FRAMES + 1, W5_MIN_FRAMES})


def enc_ready_blocks():
    """equal calls per block: both sides of the promise's one-wave limit, 7, two short runs, one frame below, at and above a run of 64 (65: 33 + 32), 129, and both
    sides of the longest call that overlaps"""
    q, a = LC3D_FUSED_MAX_T_READY, LC3D_AHEAD_MAX_FRAMES
    return sorted({q, q + 1, q + 2, LC3D_RUN_FRAMES + 1, LC3D_RUN_FRAMES_READY - 1, LC3D_RUN_FRAMES_READY, LC3D_RUN_FRAMES_READY + 1, 2 * LC3D_RUN_FRAMES_READY + 1, a, a + 1})


ENC_READY_REPEAT = 5
ENC_SMALL_RUN_LENGTHS = (9, 18, 35)          # with LC3PLUS_ENC_RUN_FRAMES = 1 and 3: runs of 1, 2 and 3 frames (R is capped at 16)
ENC_SMALL_RUN_FRAMES = (1, 3)
# (batch, LC3PLUS_ENC_RUN_FRAMES): 63 streams in runs of one frame are the lane kernels' 63 (stream, frame) pairs - a wave less one lane
ENC_SMALL_RUN_CASES = (("48k_10_small", 1), ("48k_10_small", 3), ("mono_63", 1))


def enc_tail_lengths():
    """for one stream: a whole workgroup of the writer (one frame per lane) and one frame either side; and the upper end of the second rate-stream rule, which the
    ordered lengths reach from 32 only: a call inside it (20), at its end (24) and the first above (25)"""
    wg = PACK_WPG * WAVE
    return sorted({wg - 1, wg, wg + 1, RATE_FRONT_HI - RATE_FRONT_MASK - 1, RATE_FRONT_HI, RATE_FRONT_HI + 1})


def dec_ordered_lengths():
    """1; one below, at and above a group of four and of eight frames (3, 4, 5, 7, 8, 9); two groups of eight and one more; 33; a whole wave of frames per stream and
    one more; 129"""
    return sorted({1, IMDCT4_FPW - 1, IMDCT4_FPW, IMDCT4_FPW + 1, IMDCT_FPW - 1, IMDCT_FPW, IMDCT_FPW + 1, 2 * IMDCT_FPW, 2 * IMDCT_FPW + 1, 4 * IMDCT_FPW + 1, WAVE,
                   WAVE + 1, 2 * WAVE + 1})


def dec_whole_wg_lengths():
    return [PLAN_WG - 1, PLAN_WG, PLAN_WG + 1]


def dec_count_lengths():
    return [1, IMDCT4_FPW + 1, IMDCT_FPW + 1]


def dec_ready_blocks():
    return [1, IMDCT4_FPW - 1, IMDCT4_FPW, IMDCT4_FPW + 1, IMDCT_FPW + 1, 2 * IMDCT_FPW + 1]


DEC_READY_REPEAT = 6
# the seeds of the fixed shuffles (test_call_shapes_cpu.test_the_orders_hand_every_path_to_every_other holds what each order has to contain)
SEEDS = dict(enc_tails=0, enc_ordered=11, enc_count=1, enc_ready=2, dec_ordered=5, dec_count=0, dec_ready=1, dec_whole=0)


def sequence(name):
    """the consecutive call lengths of a sequence, in its fixed shuffled order"""
    if name == "enc_ordered":
        return _shuffled(enc_ordered_lengths(), SEEDS[name])
    if name == "enc_count":
        return _shuffled(enc_count_lengths(), SEEDS[name])
    if name == "enc_ready":
        return tuple(n for b in _shuffled(enc_ready_blocks(), SEEDS[name]) for n in [b] * ENC_READY_REPEAT)
    if name == "enc_small_runs":
        return ENC_SMALL_RUN_LENGTHS
    if name == "enc_tails":
        return _shuffled(enc_tail_lengths(), SEEDS[name])
    if name == "dec_ordered":
        return _shuffled(dec_ordered_lengths(), SEEDS[name])
    if name == "dec_whole":
        return _shuffled(dec_whole_wg_lengths(), SEEDS[name])
    if name == "dec_count":
        return _shuffled(dec_count_lengths(), SEEDS[name])
    if name == "dec_ready":
        return tuple(n for b in _shuffled(dec_ready_blocks(), SEEDS[name]) for n in [b] * DEC_READY_REPEAT)
    raise KeyError(name)


def _tag(name, seq):
    return sum(map(ord, name)) + 7 * sum(map(ord, seq))


def starts(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def twin_lengths(total):
    return [TWIN_CALL] * (total // TWIN_CALL) + ([total % TWIN_CALL] if total % TWIN_CALL else [])


def enc_shapes(g, lengths, ready=False, run_frames=0):
    out, prev = [], None
    for n in lengths:
        prev = enc_shape(g, n, ready, prev, run_frames)
        out.append(prev)
    return out


# ---- encoder inputs -------------------------------------------------------------------------------------------------------------------------------------------
def onset_frames(lengths):
    """(first frame of a call, last frame of another call): calls in the middle of the sequence, of at least three frames, not neighbours"""
    st = starts(lengths)
    long_ = [k for k, n in enumerate(lengths) if n >= 3 and k > 0]
    a, b = long_[0], long_[-1]
    assert b > a + 1, lengths
    return int(st[a]), int(st[b + 1] - 1)


@functools.lru_cache(maxsize=None)
def enc_pcm(name, seq):
    """int16 [S, total, ch, N], read-only: synth_pcm (channel c of stream s is its stream s + c * S, so stream 1's first channel is the pitched class), and in every
    channel with attack handling an onset - 30 dB up from the middle of the frame on - on the first frame of one call and on the last frame of another"""
    g = enc_geometry(name)
    lengths = sequence(seq)
    total, S, ch, N = int(sum(lengths)), g["S"], g["ch"], g["N"]
    x = synth_pcm(S * ch, total, N, g["fs"], seed=4100 + _tag(name, seq)).reshape(ch, S, total, N).transpose(1, 2, 0, 3).astype(np.float64)
    if g["any_attack"] and len(lengths) > 4:
        for t in onset_frames(lengths):
            x[:, t - 1:t] *= 0.03
            x[:, t, :, :N // 2] *= 0.03
            x[:, t, :, N // 2:] = np.clip(x[:, t, :, N // 2:] * 3.0, -30000, 30000)
    x = np.ascontiguousarray(np.clip(np.rint(x), -32768, 32767).astype(np.int16))
    x.flags.writeable = False
    return x


def _pm():
    L = C.CDLL(os.path.join(ORACLE_DIR, "liblc3_oracle_pm.so"))
    L.lc3o_encode_batch16_ch.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return L


@functools.lru_cache(maxsize=None)
def oracle_encode(name, seq):
    """the portable-math oracle's continuous run over enc_pcm: uint8 [S, total, stride] (zero behind a frame), read-only"""
    g = enc_geometry(name)
    pcm = enc_pcm(name, seq)
    out = np.zeros(pcm.shape[:2] + (max(g["nbytes"]),), np.uint8)
    br = np.array(g["rates"], np.int32)
    L = _pm()

    def one(s):        # a stream per thread (the C call releases the interpreter; the oracle encoder keeps everything it writes in the lc3o_enc it allocates)
        return L.lc3o_encode_batch16_ch(g["fs"], g["ms"], g["hr"], g["ch"], 1, pcm.shape[1], br[s:].ctypes.data, pcm[s].ctypes.data, out[s].ctypes.data, out.shape[2])
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        assert not any(ex.map(one, range(g["S"])))
    out.flags.writeable = False
    return out


def attack_flags(name, seq):
    """bool [ncs, total]: the exact-math oracle's attack decision per channel-frame (its trace)"""
    g = enc_geometry(name)
    pcm = enc_pcm(name, seq)
    out = np.zeros((g["ncs"], pcm.shape[1]), bool)
    for s in range(g["S"]):
        o = Oracle(g["fs"], g["ch"], g["ms"], g["hr"], int(g["rates"][s]))
        tr = o.enable_trace()
        for t in range(pcm.shape[1]):
            o.encode(pcm[s, t])
            for c in range(g["ch"]):
                out[s * g["ch"] + c, t] = tr[c].attack != 0
    return out


# ---- decoder inputs -------------------------------------------------------------------------------------------------------------------------------------------
ROLES = ("none", "boundary", "three_calls", "first", "last_two")


def role3_calls(lengths):
    """the first three consecutive calls that include a one-frame call and a call longer than the attenuation ramp"""
    for i in range(len(lengths) - 2):
        w = lengths[i:i + 3]
        if 1 in w and max(w) > PLC_RAMP:
            return i
    raise AssertionError(lengths)


def loss_roles(lengths, S, role0=0):
    """bool [S, total]: the frames stream s loses, by its role ROLES[(s + role0) % 5], laid out against the call boundaries"""
    st = starts(lengths)
    lost = np.zeros((S, int(st[-1])), bool)
    k3 = role3_calls(lengths) if len(lengths) >= 3 and 1 in lengths else None
    for s in range(S):
        role = ROLES[(s + role0) % len(ROLES)]
        for k, n in enumerate(lengths):
            a, b = int(st[k]), int(st[k + 1])
            if role == "boundary":                 # the last frame of every call and the first frame of the next
                lost[s, b - 1] = k + 1 < len(lengths) or lost[s, b - 1]
                lost[s, a] = k > 0 or lost[s, a]
            elif role == "three_calls":
                lost[s, a:b] = k3 is not None and k3 <= k < k3 + 3
            elif role == "first":
                lost[s, a] = True
            elif role == "last_two":
                lost[s, max(a, b - 2):b] = True
    return lost


def expected_status(lengths, S, role0=0):
    """what each role says of the status: its lost frames are concealed, every other frame is decoded"""
    return loss_roles(lengths, S, role0).astype(np.uint8)


def refuse(g, payload):
    """a copy of a stream-frame whose first channel the parser refuses (hostile_frames' crafted joint SNS index at its first invalid value)"""
    import hostile_frames as hf
    n0 = g_chan0(g, payload.size)
    out = payload.copy()
    out[:n0] = hf.edit(payload[:n0], g["fs"], g["ms"], g["hr"], msb=0, index=33460056)
    return out


def g_chan0(g, size):
    return size // g["ch"] + (0 < size % g["ch"])


@functools.lru_cache(maxsize=None)
def dec_case(name, seq, S=None, role0=0, refused=False):
    """-> dict(frames uint8 [S, total, stride], sizes int32 [S, total] (the stream's own, also where lost), bfi uint8 [S, total], lost bool [S, total], payload_lost:
    the frames whose loss is in their bytes, not in a flag - all of them with refused=True (a call without flags), else the stereo family's one stream), read-only.
    The bitstreams are the oracle encoder's on synth_pcm, stream 1's first channel the pitched class."""
    g = dec_geometry(name, S)
    lengths = sequence(seq)
    total, S, ch, N = int(sum(lengths)), g["S"], g["ch"], g["N"]
    pcm = np.ascontiguousarray(synth_pcm(S * ch, total, N, g["fs"], seed=4300 + _tag(name, seq)).reshape(ch, S, total, N).transpose(1, 2, 0, 3))
    api = _api()
    rates = np.zeros(S, np.int32)
    for s in range(S):
        rates[s] = g["sizes"][s] * 8 * g["fs"] // N
        assert int(api.enc_plan_bitrates(g["fs"], ch, g["ms"], g["hr"], [[int(rates[s])]])[0][0, 0]) == g["sizes"][s], (name, s)
    frames = np.zeros((S, total, max(g["sizes"])), np.uint8)
    assert _pm().lc3o_encode_batch16_ch(g["fs"], g["ms"], g["hr"], ch, S, total, rates.ctypes.data, pcm.ctypes.data, frames.ctypes.data, frames.shape[2]) == 0
    lost = loss_roles(lengths, S, role0)
    by_payload = np.zeros_like(lost)
    if refused:
        by_payload[:] = lost
    elif ch == 2:
        by_payload[STEREO_CORRUPT_STREAM] = lost[STEREO_CORRUPT_STREAM]
    for s, t in np.argwhere(by_payload).tolist():
        frames[s, t, :g["sizes"][s]] = refuse(g, frames[s, t, :g["sizes"][s]])
    c = dict(g=g, lengths=lengths, frames=frames, sizes=np.repeat(np.array(g["sizes"], np.int32)[:, None], total, axis=1), bfi=(lost & ~by_payload).astype(np.uint8),
             lost=lost, payload_lost=by_payload)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


@functools.lru_cache(maxsize=None)
def oracle_decode(name, seq, S=None, role0=0, refused=False):
    """the portable-math oracle decoder's continuous run over dec_case: (int16 [S, total, ch, N], status uint8 [S, total]), read-only"""
    c = dec_case(name, seq, S, role0, refused)
    g = c["g"]
    total = c["frames"].shape[1]
    pcm, st = np.zeros((g["S"], total, g["ch"], g["N"]), np.int16), np.zeros((g["S"], total), np.uint8)
    for s in range(g["S"]):                  # one stream after the other: the oracle decoder keeps scratch arrays of its own (not re-entrant)
        d = OracleDecoder(g["fs"], g["ch"], g["ms"], g["hr"], portable_math=True)
        for t in range(total):
            rc, x = d.decode(c["frames"][s, t, :g["sizes"][s]], int(c["bfi"][s, t]))
            assert rc in (0, 2), rc
            pcm[s, t], st[s, t] = x, rc == 2
    pcm.flags.writeable = False
    st.flags.writeable = False
    return pcm, st


def ltpf_active(c, s, t, channel=0):
    """the LTPF active flag of channel `channel` of frame (s, t)'s payload, by api.frame_info_side"""
    g = c["g"]
    info = _api().frame_info_side(g["fs"], g["ch"], g["ms"], g["hr"], c["frames"][s, t, :g["sizes"][s]])
    return info[channel, 0] == 0 and info[channel, 34] == 1


# ---- which rule is reached where ------------------------------------------------------------------------------------------------------------------------------
def all_enc_calls():
    """[(family or batch, shape)] over every encoder sequence"""
    out = []
    for name in ENC_FAMILIES:
        out += [(name, sh) for sh in enc_shapes(enc_geometry(name), sequence("enc_ordered"))]
    for name in ENC_COUNT_BATCHES:
        out += [(name, sh) for sh in enc_shapes(enc_geometry(name), sequence("enc_count"))]
    for name in ENC_READY_FAMILIES:
        out += [(name, sh) for sh in enc_shapes(enc_geometry(name), sequence("enc_ready"), ready=True)]
    for name in ENC_TAIL_BATCHES:
        out += [(name, sh) for sh in enc_shapes(enc_geometry(name), sequence("enc_tails"))]
    for name, rf in ENC_SMALL_RUN_CASES:
        out += [(name, sh) for sh in enc_shapes(enc_geometry(name), sequence("enc_small_runs"), run_frames=rf)]
    return out
