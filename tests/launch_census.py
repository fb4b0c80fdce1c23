"""The entry-point table of the launch census (test helper beside lc3_harness.py, TEST INFRASTRUCTURE ONLY).

SCENARIOS: one small self-contained case per way the host runtime (audio_codec_amd/csrc/lc3_runtime.hip) picks a kernel - geometry, channels, call kind and
arguments, sample type, pointer alignment, environment switches, call lengths - each with the entry points it is there for ("claims").  NOT_REACHED: the entry
points no public call reaches, each with the launch code that shows it.  tests/test_launch_census_cpu.py holds the two against the kernels of the built code
object; tests/test_gpu_launch_census.py runs every scenario under api.launch_census(), compares what it wrote with the CPU oracle for equality and asserts that
the claimed entry points were launched.

run_encoder / run_decoder are the two engines.  The expectation never comes from another GPU path: the encoder's bytes are those of lc3_harness.Oracle
(portable math) given set_bitrate / set_bandwidth before every frame as the host rule (api.enc_plan_rates_ragged) accepts them, over each stream's present frames
only; the decoder's samples and status are lc3_harness.OracleDecoder's at the output type's depth (_dec_same).  Sample types the oracle does not read go through api.pcm_from_native / api.pcm_to_native
on the host (float32 is fed on the 16-bit grid, where the format's rule gives the int16 sample); placed and packed calls are laid out with api.pcm_placed_offset,
api.plan_placed and api.plan_packed.  Every output buffer starts as sentinels and every byte a call may not write is checked untouched.

Shapes: 3 streams (lc3_enc_pitch2_kernel pairs streams 2k and 2k + 1: one stays unpaired), two consecutive calls (state and carried configuration cross a
launch) of 2 frames for the one-wave kernels, 12 for the pipelined ones, 6 under the input-ready promise, 48 for the five-wave writer, 128 for the shape kernel
on the pitch stream.  Stereo geometries have odd stream-frame sizes (161 and 201 bytes, 375 and 501 in the large layout): the channels differ in bytes and
channel 1's payload starts at an odd address."""
import functools
import os
import sys

import numpy as np

from lc3_harness import Oracle, OracleDecoder, synth_pcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT, NB_SENT, FL_SENT, ST_SENT = 0xA5, -7, 0xEE, 0xEE
FL_RATE, FL_BW, FL_CAP, FL_PLACE, FL_ABSENT = 1, 6, 8, 16, 32
ST_PLACE, ST_ABSENT = 4, 8

# geometry: fs, frame_ms, hrmode, channels, one bitrate per stream
G48 = (48000, 10.0, 0, 1, (64000, 96000, 40000))            # 80, 120 (attack handling: lc3_enc_attack_kernel), 50 bytes; front4, pitch2, resample48, imdct4
G48S = (48000, 10.0, 0, 2, (128800, 160800, 96000))         # 161, 201, 120 bytes: odd stream-frames
G48LS = (48000, 10.0, 0, 2, (320800, 400800, 272000))       # 401, 501, 340 bytes in stereo
G48_5S = (48000, 5.0, 0, 2, (129600, 161600, 96000))        # 81, 101, 60 bytes
G48_25S = (48000, 2.5, 0, 2, (259200, 195200, 128000))      # 81, 61, 40 bytes
G32S = (32000, 10.0, 0, 2, (128800, 160800, 96000))
G16S = (16000, 10.0, 0, 2, (64800, 96800, 48000))           # 81, 121, 60 bytes
G44S = (44100, 10.0, 0, 2, (118400, 147900, 92400))         # 161, 201, 125 bytes; frames of 480 samples that last 10.88 ms (tests/option_pairs.py)
G48HR = (48000, 10.0, 1, 1, (128000, 256000, 400000))       # high resolution in the standard layout
G96 = (96000, 10.0, 1, 1, (149600, 256000, 400000))         # the large layout
G96S = (96000, 10.0, 1, 2, (300000, 400800, 512000))        # 375, 501, 640 bytes
G96_5S = (96000, 5.0, 1, 2, (350400, 401600, 512000))       # 219, 251, 320 bytes
G96_25 = (96000, 2.5, 1, 1, (198400, 256000, 320000))       # N = 240 in the standard layout: lc3_enc_resample96_kernel_n240
G96_25S = (96000, 2.5, 1, 2, (400000, 515200, 640000))      # 125, 161, 200 bytes

WIRE_DEPTH = {"s16be": 16, "s24_3le": 24, "s24_3be": 24, "ulaw": 16, "alaw": 16}
SCENARIOS = []


def _add(kind, name, geom, claims, **kw):
    assert all(s["name"] != name for s in SCENARIOS), name
    SCENARIOS.append(dict(kw, kind=kind, name=name, geom=geom, claims=tuple(claims)))


def E(name, geom, claims, **kw):
    """encoder scenario.  calls: frames per call; how: device (encode_device), host (encode), hostwords (encode_device with host words), rates
    (encode_device_rates), packed (encode_device_packed); words: "", "r", "b", "rb"; form: 16, 24, 32, "f32" or a wire type's name; placed, ragged, ready
    (the input-ready promise); pad: bytes the PCM pointer lies off a 256-byte boundary; order: of packed output; reset: streams reset between the calls;
    layout: None, "interleaved" or "channel_major" (the device array is the default one permuted with api.pcm_offset); env: environment switches in force
    while the batch is created"""
    _add("enc", name, geom, claims, **kw)


def D(name, geom, claims, **kw):
    """decoder scenario.  how: host (decode), hostsizes (decode with num_bytes), device (decode_device), devhostsizes (decode_device with host num_bytes),
    sizes (decode_device_sizes), packed (decode_device_packed); placed, ragged, ready, layout, env as for the encoder; out: the output sample type, named as
    the encoder's form; pad: bytes the PCM output pointer lies off a 256-byte boundary (the bytes in front of and behind the buffer are checked untouched)"""
    _add("dec", name, geom, claims, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------------------------
PRE = ("lc3_enc_hp50_kernel",)
LANES = ("lc3_enc_scf_lane_kernel", "lc3_enc_snsvq_kernel", "lc3_enc_shape_lane_kernel")
PLAN = ("lc3_enc_plan_rates_kernel", "lc3_enc_rates_tail_kernel")
PLAN_RAG = ("lc3_enc_plan_rates_kernel_rag", "lc3_enc_rates_tail_kernel_rag", "lc3_enc_absent_kernel")
SCAN = ("lc3_pack_sums_kernel", "lc3_pack_base_kernel", "lc3_pack_offsets_kernel")
FORMS = (("", 16), ("_fmt", "f32"), ("_wire", "s16be"), ("_plc", 16))


def _one_wave():
    """lc3_runtime.hip enc_one_wave: LC3_OW_KERNELS x (plain, _fmt, _wire, _plc), calls of 2 frames.  Stereo with odd sizes in the plain and the placed form of
    every key (the kernels of one key are one source compiled four times)."""
    for big in (0, 1):
        for var, vbw, pk in ((0, 0, 0), (0, 0, 1), (1, 0, 0), (1, 0, 1), (0, 1, 0), (0, 1, 1), (1, 1, 0), (1, 1, 1)):
            if big and vbw:
                continue
            base = "lc3_encode_kernel" + ("_big" if big else "") + ("_var" if var else "") + ("_vbw" if vbw else "") + ("_pk" if pk else "")
            words = ("r" if var else "") + ("b" if vbw else "")
            how = "packed" if pk else "rates" if words else "device"
            for sfx, form in FORMS:
                stereo = sfx in ("", "_plc")
                geom = (G96S if stereo else G96) if big else (G48S if stereo else G48)
                extra = (SCAN if pk else ()) + (PLAN if words else ()) + (("lc3_pcm_placed_mark_kernel",) if sfx == "_plc" and how != "device" else ())
                # the pre-kernels run in front of the one-wave kernel of an untraced call (enc_size_set): the resampler for every shape where the typed ones do not apply
                E("ow%s%s" % (base[len("lc3_encode_kernel"):], sfx or "_plain"), geom, (base + sfx,) + extra, calls=(2, 2), how=how, words=words, form=form,
                  placed=sfx == "_plc")
    # the ragged forms (LC3_OW_RAG_KERNELS): always _var_pk; slotted with rates, packed with bandwidths, the large layout packed without words
    for base, geom, geom_s, words, how in (("lc3_encode_kernel_var_pk", G48, G48S, "r", "rates"), ("lc3_encode_kernel_var_vbw_pk", G48, G48S, "b", "packed"),
                                           ("lc3_encode_kernel_big_var_pk", G96, G96S, "", "packed")):
        for sfx, form in (("_rag", 16), ("_rag_fmt", "f32"), ("_rag_wire", "ulaw"), ("_rag_plc", 16)):
            stereo = sfx in ("_rag", "_rag_plc")
            E("ow%s%s" % (base[len("lc3_encode_kernel"):], sfx), geom_s if stereo else geom, (base + sfx,) + PLAN_RAG + (SCAN if how == "packed" else ()),
              calls=(2, 2), how=how, words=words, form=form, placed=sfx == "_rag_plc", ragged=True)


_one_wave()

# ---- the pipelined path (enc_pipelined, enc_run, enc_writer), calls of 12 frames ----
E("pipe_48_stereo", G48S, ("lc3_enc_resample48_kernel",) + PRE + ("lc3_enc_pitch2_kernel", "lc3_enc_front4_kernel", "lc3_enc_attack_kernel") + LANES +
  ("lc3_enc_rate_kernel", "lc3_enc_pack_kernel", "lc3_stream_state_kernel"), calls=(12, 12))
E("pipe_48_host", G48, ("lc3_enc_front4_kernel", "lc3_enc_pack_kernel"), calls=(12, 12), how="host")
E("pipe_48_off_alignment", G48, ("lc3_enc_resample_kernel",), calls=(12, 12), pad=2)                     # (dpcm & 15) != 0: the resampler for every shape
E("pipe_48_f32", G48S, ("lc3_enc_resample48f_kernel", "lc3_enc_front4_kernel_fmt"), calls=(12, 12), form="f32")
E("pipe_48_f32_off_alignment", G48, ("lc3_enc_resample_fmt_kernel",), calls=(12, 12), form="f32", pad=4)
E("pipe_48_wire", G48S, ("lc3_enc_resample48w_kernel", "lc3_enc_front4_kernel_wire"), calls=(12, 12), form="s24_3be")
E("pipe_48_wire_off_alignment", G48, ("lc3_enc_resample_wire_kernel",), calls=(12, 12), form="alaw", pad=1)      # (dpcm & 3) != 0
E("pipe_48_placed", G48S, ("lc3_enc_resample_plc_kernel", "lc3_enc_front4_kernel_plc"), calls=(12, 12), placed=True)
E("pipe_48_bw", G48S, ("lc3_enc_shape_lane_kernel_vbw",) + PLAN, calls=(12, 12), how="rates", words="b")
E("pipe_48_bw_host", G48, ("lc3_enc_shape_lane_kernel_vbw",), calls=(12, 12), how="hostwords", words="b")
E("pipe_48_packed", G48S, ("lc3_enc_pack_kernel_pk",) + SCAN, calls=(12, 12), how="packed", order=1)
E("pipe_48_ready", G48S, ("lc3_enc_front4_kernel", "lc3_enc_pack_kernel"), calls=(6, 6, 6), ready=True)
E("pipe_48_reset", G48, ("lc3_stream_state_kernel",), calls=(12, 12), reset=(1,))
E("pipe_48_w5", G48, ("lc3_enc_pack_kernel_w5",), calls=(48, 48), geom_rates=(64000, 40000, 72000))
E("pipe_48_w5_packed", G48, ("lc3_enc_pack_kernel_w5_pk",), calls=(48, 48), geom_rates=(64000, 40000, 72000), how="packed")
E("pipe_48_split", G48S, ("lc3_enc_pack_head_kernel", "lc3_enc_pack_code_kernel"), calls=(12, 12), env={"LC3PLUS_ENC_PACK_SPLIT": "1"})
E("pipe_48_split_packed", G48S, ("lc3_enc_pack_head_kernel_pk", "lc3_enc_pack_code_kernel_pk"), calls=(12, 12), how="packed", env={"LC3PLUS_ENC_PACK_SPLIT": "1"})
E("pipe_48_tailw", G48S, ("lc3_enc_tailw_kernel",), calls=(12, 12), env={"LC3PLUS_ENC_TAILW_BYTES": "100"})
E("pipe_48_shape_wave", G48S, ("lc3_enc_shape_kernel",), calls=(12, 12), env={"LC3PLUS_ENC_SHAPE_WAVE": "1"})
E("pipe_48_shape_wave_bw", G48S, ("lc3_enc_shape_kernel_vbw",), calls=(12, 12), how="rates", words="b", env={"LC3PLUS_ENC_SHAPE_WAVE": "1"})
E("pipe_48_pitch1", G48S, ("lc3_enc_pitch_kernel",), calls=(12, 12), env={"LC3PLUS_ENC_PITCH2": "0"})
E("pipe_48_5", G48_5S, ("lc3_enc_frontm_kernel", "lc3_enc_pitch2_kernel_l64"), calls=(12, 12))
E("pipe_48_25", G48_25S, ("lc3_enc_front_kernel", "lc3_enc_pitch2_kernel_l32"), calls=(12, 12))                  # N = 120: no frontm (lc3hip_create: fm_frames)
E("pipe_48_5_f32", G48_5S, ("lc3_enc_frontm_kernel_fmt", "lc3_enc_resample_fmt_kernel"), calls=(12, 12), form="f32")
E("pipe_48_5_wire", G48_5S, ("lc3_enc_frontm_kernel_wire", "lc3_enc_resample_wire_kernel"), calls=(12, 12), form="s24_3le")
E("pipe_48_5_placed", G48_5S, ("lc3_enc_frontm_kernel_plc",), calls=(12, 12), placed=True, form="f32")
E("pipe_32", G32S, ("lc3_enc_front_kernel", "lc3_enc_resample_kernel"), calls=(12, 12))
E("pipe_32_f32", G32S, ("lc3_enc_front_kernel_fmt",), calls=(12, 12), form="f32")
E("pipe_32_wire", G32S, ("lc3_enc_front_kernel_wire",), calls=(12, 12), form="ulaw")
E("pipe_32_placed", G32S, ("lc3_enc_front_kernel_plc",), calls=(12, 12), placed=True, form="s16be")
E("pipe_16_stereo", G16S, ("lc3_enc_pitch2_kernel",), calls=(12, 12))
E("pipe_48hr", G48HR, ("lc3_enc_rate_kernel",), calls=(12, 12))
E("pipe_96", G96S, ("lc3_enc_front_kernel_big", "lc3_enc_rate_kernel_big", "lc3_enc_resample_kernel"), calls=(12, 12))
E("pipe_96_f32", G96S, ("lc3_enc_front_kernel_big_fmt",), calls=(12, 12), form="f32")
E("pipe_96_wire", G96S, ("lc3_enc_front_kernel_big_wire",), calls=(12, 12), form="s24_3le")
E("pipe_96_placed", G96S, ("lc3_enc_front_kernel_big_plc",), calls=(12, 12), placed=True)
E("pipe_96_resample96", G96, ("lc3_enc_resample96_kernel_n960",), calls=(12, 12), env={"LC3PLUS_ENC_RESAMPLE96": "2"})
E("pipe_96_5_resample96", G96_5S, ("lc3_enc_resample96_kernel_n480", "lc3_enc_front_kernel_big"), calls=(12, 12), env={"LC3PLUS_ENC_RESAMPLE96": "2"})
E("pipe_96_25", G96_25S, ("lc3_enc_resample96_kernel_n240", "lc3_enc_frontm_kernel"), calls=(12, 12))
E("pipe_96_25_on_pitch", G96_25, ("lc3_enc_resample96_kernel_n240", "lc3_enc_shape_lane_kernel"), calls=(128, 128))      # enc_run: sop, n_frames >= 128
E("pipe_96_shape_wave", G96S, ("lc3_enc_shape_kernel_big",), calls=(12, 12), env={"LC3PLUS_ENC_SHAPE_WAVE": "1"})
E("pipe_96_tailw", G96S, ("lc3_enc_tailw_kernel_big",), calls=(12, 12), env={"LC3PLUS_ENC_TAILW_BYTES": "100"})
# ---- the ragged forms of the pipelined path: more than 8 frames, no per-frame bitrates, standard layout (enc_launch: rag_pipe) ----
RAG_PIPE = ("lc3_enc_hp50_kernel_rag", "lc3_enc_pitch_kernel_rag", "lc3_enc_scf_lane_kernel_rag", "lc3_enc_snsvq_kernel_rag", "lc3_enc_rate_kernel_rag",
            "lc3_enc_pack_kernel_pk_rag") + PLAN_RAG
# (the slotted call needs rates or bandwidths: the ragged call without words is a packed one)
E("rpipe_48", G48S, ("lc3_enc_resample_kernel_rag", "lc3_enc_front4_kernel_rag", "lc3_enc_attack_kernel_rag", "lc3_enc_shape_lane_kernel_rag") + RAG_PIPE + SCAN,
  calls=(12, 12), how="packed", ragged=True)
E("rpipe_48_bw", G48S, ("lc3_enc_shape_lane_kernel_vbw_rag",) + RAG_PIPE, calls=(12, 12), how="rates", words="b", ragged=True)
E("rpipe_48_f32", G48S, ("lc3_enc_resample_fmt_kernel_rag", "lc3_enc_front4_kernel_fmt_rag"), calls=(12, 12), how="rates", words="b", ragged=True, form="f32")
E("rpipe_48_wire", G48S, ("lc3_enc_resample_wire_kernel_rag", "lc3_enc_front4_kernel_wire_rag"), calls=(12, 12), how="rates", words="b", ragged=True, form="s24_3be")
E("rpipe_48_placed", G48S, ("lc3_enc_resample_plc_kernel_rag", "lc3_enc_front4_kernel_plc_rag"), calls=(12, 12), how="rates", words="b", ragged=True, placed=True)
E("rpipe_48_w5", G48, ("lc3_enc_pack_kernel_w5_pk_rag",), calls=(48, 48), geom_rates=(64000, 40000, 72000), how="rates", words="b", ragged=True)
E("rpipe_48_5", G48_5S, ("lc3_enc_frontm_kernel_rag",), calls=(12, 12), how="rates", words="b", ragged=True)
E("rpipe_48_5_f32", G48_5S, ("lc3_enc_frontm_kernel_fmt_rag",), calls=(12, 12), how="rates", words="b", ragged=True, form="f32")
E("rpipe_48_5_wire", G48_5S, ("lc3_enc_frontm_kernel_wire_rag",), calls=(12, 12), how="rates", words="b", ragged=True, form="alaw")
E("rpipe_48_5_placed", G48_5S, ("lc3_enc_frontm_kernel_plc_rag",), calls=(12, 12), how="rates", words="b", ragged=True, placed=True)
E("rpipe_32", G32S, ("lc3_enc_front_kernel_rag",), calls=(12, 12), how="rates", words="b", ragged=True)
E("rpipe_32_f32", G32S, ("lc3_enc_front_kernel_fmt_rag",), calls=(12, 12), how="rates", words="b", ragged=True, form="f32")
E("rpipe_32_wire", G32S, ("lc3_enc_front_kernel_wire_rag",), calls=(12, 12), how="rates", words="b", ragged=True, form="s16be")
E("rpipe_32_placed", G32S, ("lc3_enc_front_kernel_plc_rag",), calls=(12, 12), how="rates", words="b", ragged=True, placed=True)

# ---- the decoder (dec_plan, dec_parse, dec_chain, dec_tail) ----
CHAIN = ("lc3_dec_plc_kernel",)
D("dec_48_stereo", G48S, ("lc3_dec_parse_kernel", "lc3_dec_imdct4_kernel", "lc3_dec_synth_kernel", "lc3_stream_state_kernel") + CHAIN, calls=(2, 12), how="host")
D("dec_48_large", G48LS, ("lc3_dec_parse_kernel_g",), calls=(2, 12), how="device")
D("dec_48_hostsizes", G48S, ("lc3_dec_parse_kernel_var",), calls=(2, 12), how="hostsizes")
D("dec_48_hostsizes_large", G48LS, ("lc3_dec_parse_kernel_g_var",), calls=(2, 12), how="devhostsizes")
D("dec_48_sizes", G48S, ("lc3_dec_parse_kernel_var", "lc3_dec_plan_sizes_kernel", "lc3_dec_sizes_tail_kernel"), calls=(2, 12), how="sizes")
D("dec_48_sizes_large", G48LS, ("lc3_dec_parse_kernel_g_var", "lc3_dec_plan_sizes_kernel"), calls=(2, 12), how="sizes")
D("dec_48_packed", G48S, ("lc3_dec_parse_kernel_var_pk", "lc3_dec_plan_packed_kernel"), calls=(2, 12), how="packed")
D("dec_48_packed_large", G48LS, ("lc3_dec_parse_kernel_g_var_pk", "lc3_dec_plan_packed_kernel"), calls=(2, 12), how="packed")
D("dec_48_imdct", G48S, ("lc3_dec_imdct_kernel",), calls=(2, 12), how="device", env={"LC3PLUS_DEC_IMDCT4": "0"})
D("dec_48_5", G48_5S, ("lc3_dec_imdct_kernel",), calls=(2, 12), how="device")
D("dec_48_placed", G48S, ("lc3_dec_synth_kernel_plc", "lc3_pcm_placed_mark_kernel"), calls=(2, 12), how="sizes", placed=True)
D("dec_48_ready", G48S, ("lc3_dec_parse_kernel", "lc3_dec_imdct4_kernel"), calls=(6, 6, 6), how="device", ready=True)
D("dec_48_reset", G48, ("lc3_stream_state_kernel",), calls=(2, 12), how="device", reset=(1,))
D("dec_48_ragged", G48S, ("lc3_dec_plan_sizes_kernel_rag", "lc3_dec_plc_kernel_rag", "lc3_dec_imdct4_kernel_rag", "lc3_dec_synth_kernel_rag",
                          "lc3_dec_sizes_tail_kernel_rag"), calls=(2, 12), how="sizes", ragged=True)
D("dec_48_ragged_packed_placed", G48S, ("lc3_dec_plan_packed_kernel_rag", "lc3_dec_synth_kernel_rag_plc"), calls=(2, 12), how="packed", ragged=True, placed=True)
D("dec_48_5_ragged", G48_5S, ("lc3_dec_imdct_kernel_rag",), calls=(2, 12), how="sizes", ragged=True)
D("dec_96", G96S, ("lc3_dec_imdct_kernel_big", "lc3_dec_synth_kernel_big"), calls=(2, 12), how="device")
D("dec_96_placed", G96S, ("lc3_dec_synth_kernel_big_plc",), calls=(2, 12), how="sizes", placed=True)
D("dec_96_ragged", G96S, ("lc3_dec_imdct_kernel_big_rag", "lc3_dec_synth_kernel_big_rag"), calls=(2, 12), how="sizes", ragged=True)
D("dec_96_ragged_placed", G96S, ("lc3_dec_synth_kernel_big_rag_plc",), calls=(2, 12), how="packed", ragged=True, placed=True)
# ---- the test hook of lc3_fastmath.h ----
_add("fastmath", "fastmath_hook", None, ("lc3_fastmath_test_kernel",))

# entry point -> why no public call reaches it, by the launch code
NOT_REACHED = {}


def claimed():
    return sorted({k for s in SCENARIOS for k in s["claims"]})


def code_object_kernels():
    """the kernel symbols of the built library's gfx950 code object (tools/kernel_resources.py: the metadata notes, no GPU)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from audio_codec_amd import api
    return sorted(kr.kernels(api.lib_path(), "gfx950"))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# engines
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _api():
    import audio_codec_amd
    return audio_codec_amd.api


def nbytes_of(fs, ch, ms, hr, rate):
    return int(_api().enc_plan_bitrates(fs, ch, ms, hr, [[rate]])[0][0, 0])


def frame_len(fs, ms):
    return int((48000 if fs == 44100 else fs) * ms / 1000)


def counts_of(k, T, S):
    """a ragged call's per-stream counts: a full stream, an idle one and a cut one in every call, every stream idle once in three calls"""
    base = [T, 0, max(1, T // 2 - 1)] if k % 2 == 0 else [max(1, T // 4), T, T - max(1, T // 4)]
    return np.array([base[(s + k // 2) % 3] for s in range(S)], np.int32)


def _put(dev, arr, pad=0):
    """arr in device memory `pad` bytes behind a hipMalloc'd (256-byte aligned) address"""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    if not pad:
        return dev.put(raw if raw.size else np.zeros(1, np.uint8))
    return dev.put(np.concatenate([np.full(pad, 0x3C, np.uint8), raw])) + pad


def _pcm_forms(api, form, x):
    """int16 samples x [...] -> (format word, the array the device reads, the array and bit depth the oracle reads)"""
    if form == 16:
        return 16, x, x, 16
    if form in (24, 32):
        y = x.astype(np.int32) * (1 << (form - 16)) + (x.astype(np.int32) & ((1 << (form - 16)) - 1))      # the low bits carry signal too
        return form, y, y, form
    if form == "f32":
        return api.pcm_format(api.PCM_FLOAT32), (x.astype(np.float32) / np.float32(32768.0)), x, 16
    fmt, depth = api.pcm_format(form), WIRE_DEPTH[form]
    native = x if depth == 16 else x.astype(np.int32) * 256 + (x.astype(np.int32) & 255)
    wire = api.pcm_from_native(fmt, native)
    return fmt, wire, api.pcm_to_native(fmt, wire), depth


def _placement(api, fmt, ch, N, S, T, k, invalid):
    """offsets [S, T] of frames scattered over an arena (each stream's frames in reverse, odd gaps), its capacity in elements, and the invalid map of
    api.plan_placed; invalid: (stream, frame) whose offset lies one element past the last valid one, or None"""
    fe = ch * N
    cap = 11 + S * T * (fe + 3) + 5
    offs = np.zeros((S, T), np.int64)
    for s in range(S):
        for t in range(T):
            offs[s, t] = 11 + ((s * T + (T - 1 - t) + k) % (S * T)) * (fe + 3)
    if invalid is not None:
        offs[invalid] = cap - fe + 1
    return offs, cap, api.plan_placed(fmt, ch, N, offs, cap).astype(bool)


def _frame_elems(api, fmt, ch, N, off):
    """element indices [ch, N] of a frame placed at element off"""
    idx = np.zeros((ch, N), np.int64)
    step = ch if fmt & api.PCM_INTERLEAVED else 1
    for c in range(ch):
        a, b = api.pcm_placed_offset(fmt, ch, N, off, c, 0), api.pcm_placed_offset(fmt, ch, N, off, c, N - 1)
        assert a >= 0 and b - a == (N - 1) * step
        idx[c] = a + step * np.arange(N)
    return idx


def _dense_elems(api, fmt, ch, T, N, s, t):
    """element indices [ch, N] of frame (s, t) of a dense call of T frames in the layout of format word fmt (api.pcm_offset)"""
    idx = np.zeros((ch, N), np.int64)
    for c in range(ch):
        a, b = api.pcm_offset(fmt, ch, T, N, s, t, c, 0), api.pcm_offset(fmt, ch, T, N, s, t, c, N - 1)
        assert a >= 0 and (b - a) % (N - 1) == 0
        idx[c] = a + (b - a) // (N - 1) * np.arange(N)
    return idx


def _lay(api, fmt, arr):
    """arr [S, T, ch, N (, 3)] in the default layout -> the same samples in the layout of fmt, shape api.pcm_shape: a permutation placed with api.pcm_offset"""
    if not fmt & (api.PCM_INTERLEAVED | api.PCM_CHANNEL_MAJOR):
        return arr
    S, T, ch, N = arr.shape[:4]
    out = np.zeros((S * T * ch * N,) + arr.shape[4:], arr.dtype)
    for s in range(S):
        for t in range(T):
            out[_dense_elems(api, fmt, ch, T, N, s, t)] = arr[s, t]
    return out.reshape(api.pcm_shape(fmt, S, T, ch, N))


def _words(sc, fs, rates, S, T, k, lenient):
    """per-frame bitrates and bandwidths of call k, [S, T] int32 or None.  Device words (lenient) hold values the rule refuses as well."""
    t, s = np.meshgrid(np.arange(T), np.arange(S))
    br = bw = None
    if "r" in sc.get("words", ""):
        br = np.array(rates, np.int32)[(s + t + k) % len(rates)]
        if lenient:
            br[(s + 2 * t + k) % 5 == 4] = -1
    if "b" in sc.get("words", ""):
        top = min(fs, 40000) // 2
        vals = np.array([0, top, 4000, 8000, top - 1, top // 2 + 123] + ([top + 1, 7] if lenient else []), np.int32)
        bw = vals[(2 * s + t + k) % len(vals)]
    return br, bw


def run_encoder(dev, sc, amd):
    """runs the scenario's calls (the caller holds the census block around this) and compares with the oracle"""
    api = amd.api
    fs, ms, hr, ch, rates = sc["geom"]
    rates = list(sc.get("geom_rates", rates))
    S, N, calls, how = len(rates), frame_len(fs, ms), sc["calls"], sc.get("how", "device")
    ragged, placed, pad = bool(sc.get("ragged")), bool(sc.get("placed")), sc.get("pad", 0)
    lenient = how in ("rates", "packed")
    sizes0 = [nbytes_of(fs, ch, ms, hr, r) for r in rates]
    alts = [nbytes_of(fs, ch, ms, hr, r) for r in rates]
    stride = max(alts)
    total = sum(calls)
    x16 = synth_pcm(S * ch, total, N, fs, seed=211 + len(sc["name"])).reshape(S, ch, total, N).transpose(0, 2, 1, 3).copy()
    fmt, xdev, xora, depth = _pcm_forms(api, sc.get("form", 16), x16)
    if sc.get("layout"):
        fmt = api.pcm_format(fmt, sc["layout"])
    orc = [Oracle(fs, ch, ms, hr, int(r), portable_math=True) for r in rates]
    for o, n in zip(orc, sizes0):
        o.nbytes = n
    bat = amd.Batch(S, fs, ch, ms, hr, rates, device=0)
    if sc.get("ready"):
        bat.set_input_ready(True)
    if sc.get("before"):
        sc["before"](bat)                                                    # (tests/test_gpu_option_pairs.py: a refused call in front of the scenario's own)
    pos = np.zeros(S, np.int64)
    cur_rates, cur_bw = np.array(rates, np.int32), np.zeros(S, np.int32)
    queued = []
    for k, T in enumerate(calls):
        if k and sc.get("reset"):
            bat.reset_streams(list(sc["reset"]))
            for s in sc["reset"]:
                orc[s] = Oracle(fs, ch, ms, hr, int(cur_rates[s]), portable_math=True)
        cnt = counts_of(k, T, S) if ragged else np.full(S, T, np.int32)
        br, bw = _words(sc, fs, rates, S, T, k, lenient)
        present = np.arange(T)[None, :] < cnt[:, None]
        for w in (br, bw):
            if w is not None and ragged:
                w[~present] = np.array([-1, 2 ** 31 - 1, 7], np.int64)[(np.argwhere(~present).sum(axis=1)) % 3].astype(np.int32)
        rc, nb, inf, fl, end = api.enc_plan_rates_ragged(fs, ch, ms, hr, cur_rates, cur_bw, bitrates=br, bandwidths=bw,
                                                         out_stride=(1 << 20) if how == "packed" else stride, counts=cnt if ragged else None, n_frames=T)
        assert rc == 0
        if not lenient:
            assert not fl.any()
        # the PCM of the call: each stream's next cnt frames, garbage behind them; placed: scattered over an arena
        shape = (S, T) + xdev.shape[2:]
        arr = np.zeros(shape, xdev.dtype)
        arr.view(np.uint8)[...] = 0x5A
        for s in range(S):
            arr[s, :cnt[s]] = xdev[s, pos[s]:pos[s] + cnt[s]]
        inval = np.zeros((S, T), bool)
        d_offs = None
        if placed:
            bad = (S - 1, 0) if k == 0 and cnt[S - 1] > 0 else None
            offs, cap, inval = _placement(api, fmt, ch, N, S, T, k, bad)
            tail = arr.shape[4:]
            arena = np.zeros((cap,) + tail, arr.dtype)
            arena.view(np.uint8)[...] = 0x5A
            for s in range(S):
                for t in range(T):
                    if not inval[s, t]:
                        arena[_frame_elems(api, fmt, ch, N, int(offs[s, t]))] = arr[s, t]
            arr, d_offs = arena, dev.put(offs)
        else:
            arr = _lay(api, fmt, arr)
        # the oracle over the present frames, in the stream's order
        want = [[None] * T for _ in range(S)]
        for s in range(S):
            o = orc[s]
            for t in range(int(cnt[s])):
                if br is not None and not fl[s, t] & FL_RATE:
                    assert o.set_bitrate(int(br[s, t])) == 0
                o.nbytes = int(nb[s, t])
                if bw is not None and not fl[s, t] & FL_BW:
                    assert o.set_bandwidth(int(bw[s, t])) in (0, 18)
                frame = xora[s, pos[s] + t]
                want[s][t] = o.encode(np.zeros_like(frame) if inval[s, t] else frame, depth)
            if cnt[s]:
                cur_bw[s] = inf[s, cnt[s] - 1]
        cur_rates = end
        exp_fl = fl | np.where(inval & present, FL_PLACE, 0).astype(np.uint8)
        q = dict(T=T, cnt=cnt, nb=nb, fl=exp_fl, want=want, how=how)
        # the call
        if how == "host":
            q["out"] = bat.encode(arr, bitdepth=fmt, bitrates=br, bandwidths=bw)
            if br is not None or bw is not None:
                assert (bat.last_num_bytes == nb).all()
        else:
            d_pcm = _put(dev, arr, pad)
            if placed:
                bat.set_pcm_placement(d_offs, cap)
            d_cnt = dev.put(cnt) if ragged else None
            if ragged:
                bat.set_frame_counts(d_cnt)
            sync = not sc.get("ready")
            if how in ("device", "hostwords"):
                q["d_out"] = dev.put(np.full((S, T, stride), SENT, np.uint8))
                bat.encode_device(d_pcm, fmt, T, q["d_out"], stride, sync=sync, bitrates=br, bandwidths=bw)
                if br is not None or bw is not None:
                    assert (bat.last_num_bytes == nb).all()
            else:
                d_br = dev.put(br) if br is not None else None
                d_bw = dev.put(bw) if bw is not None else None
                q["d_nb"], q["d_fl"] = dev.put(np.full((S, T), NB_SENT, np.int32)), dev.put(np.full((S, T), FL_SENT, np.uint8))
                if how == "rates":
                    if d_br is None and d_bw is None and not ragged:
                        raise AssertionError("encode_device_rates needs words or counts")
                    q["d_out"] = dev.put(np.full((S, T, stride), SENT, np.uint8))
                    bat.encode_device_rates(d_pcm, fmt, T, q["d_out"], stride, d_br, d_bw, q["d_nb"], q["d_fl"], sync=sync)
                else:
                    order = sc.get("order", 0)
                    _, _, tot, _ = api.plan_packed(nb, order)
                    q["cap"] = tot + 24
                    q["plan"] = api.plan_packed(nb, order, q["cap"])
                    q["d_out"] = dev.put(np.full(q["cap"] + 40, SENT, np.uint8))
                    q["d_offs"], q["d_tot"] = dev.put(np.full((S, T), -99, np.int64)), dev.put(np.full(1, -99, np.int64))
                    bat.encode_device_packed(d_pcm, fmt, T, q["d_out"], q["cap"], order, d_br, d_bw, q["d_offs"], q["d_tot"], q["d_nb"], q["d_fl"], sync=sync)
            if ragged:
                bat.set_frame_counts(None)
            if placed:
                bat.set_pcm_placement(None)
        queued.append(q)
        pos += cnt
    dev.sync()
    bad = []
    for k, q in enumerate(queued):
        T, cnt, nb, want = q["T"], q["cnt"], q["nb"], q["want"]
        if "d_nb" in q:
            got_nb, got_fl = dev.get(q["d_nb"], (S, T), np.int32), dev.get(q["d_fl"], (S, T), np.uint8)
            assert (got_nb == nb).all(), (k, "num_bytes", got_nb.tolist(), nb.tolist())
            assert (got_fl == q["fl"]).all(), (k, "flags", got_fl.tolist(), q["fl"].tolist())
        if q["how"] == "packed":
            rc, offs, tot, ovf = q["plan"]
            assert not ovf.any()
            raw = dev.get(q["d_out"], (q["cap"] + 40,), np.uint8)
            assert (dev.get(q["d_offs"], (S, T), np.int64) == offs).all() and int(dev.get(q["d_tot"], (1,), np.int64)[0]) == tot
            exp = np.full(raw.size, SENT, np.uint8)
            for s in range(S):
                for t in range(int(cnt[s])):
                    exp[offs[s, t]:offs[s, t] + nb[s, t]] = want[s][t]
            for s in range(S):
                for t in range(int(cnt[s])):
                    if not np.array_equal(raw[offs[s, t]:offs[s, t] + nb[s, t]], want[s][t]):
                        bad.append((k, s, t))
            assert bad or np.array_equal(raw, exp), (k, "bytes outside the frames were written", np.flatnonzero(raw != exp)[:8].tolist())
        else:
            fill = 0 if q["how"] == "host" else SENT
            out = q["out"] if q["how"] == "host" else dev.get(q["d_out"], (S, T, stride), np.uint8)
            exp = np.full(out.shape, fill, np.uint8)
            for s in range(S):
                for t in range(int(cnt[s])):
                    exp[s, t, :nb[s, t]] = want[s][t]
            bad += [(k, s, t) for s, t in np.argwhere((out != exp).any(axis=2)).tolist()]
    bat.close()
    assert not bad, ("frames that differ from the oracle (call, stream, frame)", len(bad), bad[:10])


def _dec_streams(sc, fs, ms, hr, ch, rates, total, var):
    """the bitstreams: the oracle's stereo (or mono) encoder per stream; var: the stream's rate alternates between its own and its neighbour's every third frame"""
    S, N = len(rates), frame_len(fs, ms)
    pcm = synth_pcm(S * ch, total, N, fs, seed=307 + len(sc["name"])).reshape(S, ch, total, N).transpose(0, 2, 1, 3).copy()
    frames, sizes = [], np.zeros((S, total), np.int32)
    for s in range(S):
        o = Oracle(fs, ch, ms, hr, int(rates[s]), portable_math=True)
        row = []
        for t in range(total):
            r = rates[(s + (t // 3 if var else 0)) % S]
            assert o.set_bitrate(int(r)) == 0
            o.nbytes = nbytes_of(fs, ch, ms, hr, int(r))
            row.append(o.encode(pcm[s, t]))
            sizes[s, t] = row[-1].size
        frames.append(row)
    return frames, sizes


def _rha(v):
    """round half away from zero, float64 (np.round rounds half to even)"""
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def _dec_depths(out):
    """the depths the oracle decodes at for output type out: its own, the one a wire type stands for, 16 and 24 for float32"""
    return (16, 24) if out == "f32" else (WIRE_DEPTH[out],) if out in WIRE_DEPTH else (out,)


def _dec_same(api, out, fmt, got, want):
    """is a decoded frame - got: its elements as bytes [ch, N, element bytes] - the oracle's, want: the oracle's frame at every depth of _dec_depths(out).  Integer
    types: equality.  Wire types: equality with api.pcm_from_native (bytes swapped, 24 bits saturated, G.711 compressed) of the oracle's frame at the depth the
    type stands for.  float32: the sample rounded half away from zero equals the oracle's 16-bit and 24-bit sample
    (test_gpu_pcm_format.py: test_float_output_rounds_to_the_integer_outputs)."""
    got = np.ascontiguousarray(got)
    if out in (16, 24, 32):
        return np.array_equal(got.view(np.int16 if out == 16 else np.int32)[..., 0], want[0])
    if out == "f32":
        y = got.view(np.float32)[..., 0].astype(np.float64)
        if not np.abs(y).max() < 256.0:                                            # (what an int32 at 24 bits holds; a NaN fails here too)
            return False
        r16 = np.clip(_rha(y * 32768.0), -32768.0, 32767.0).astype(np.int16)
        return np.array_equal(r16, want[0]) and np.array_equal(_rha(y * float(1 << 23)).astype(np.int64), want[1].astype(np.int64))
    wire = np.ascontiguousarray(api.pcm_from_native(fmt & 0xFF, want[0]))
    return np.array_equal(got, wire.view(np.uint8).reshape(got.shape))


def run_decoder(dev, sc, amd):
    api = amd.api
    fs, ms, hr, ch, rates = sc["geom"]
    S, N, calls, how = len(rates), frame_len(fs, ms), sc["calls"], sc["how"]
    ragged, placed, pad = bool(sc.get("ragged")), bool(sc.get("placed")), sc.get("pad", 0)
    out = sc.get("out", 16)
    fmt = api.pcm_format(api.PCM_FLOAT32 if out == "f32" else out, sc.get("layout"))
    eb = api.load_library().lc3plus_pcm_elem_bytes(fmt)
    depths = _dec_depths(out)
    var = how in ("hostsizes", "devhostsizes", "sizes", "packed")
    lenient = how in ("sizes", "packed")
    total = sum(calls)
    frames, sizes = _dec_streams(sc, fs, ms, hr, ch, rates, total, var)
    stride = int(sizes.max())
    orc = [[OracleDecoder(fs, ch, ms, hr, portable_math=True) for _ in depths] for _ in range(S)]
    d = amd.DecBatch(S, fs, ch, ms, hr, None if var else [int(sizes[s, 0]) for s in range(S)], device=0)
    if sc.get("ready"):
        d.set_input_ready(True)
    if sc.get("before"):
        sc["before"](d)
    pos = np.zeros(S, np.int64)
    queued = []
    for k, T in enumerate(calls):
        if k and sc.get("reset"):
            d.reset_streams(list(sc["reset"]))
            for s in sc["reset"]:
                orc[s] = [OracleDecoder(fs, ch, ms, hr, portable_math=True) for _ in depths]
        cnt = counts_of(k, T, S) if ragged else np.full(S, T, np.int32)
        present = np.arange(T)[None, :] < cnt[:, None]
        fr = np.full((S, T, stride), 0x33, np.uint8)
        nb = np.full((S, T), 9999 if lenient else stride, np.int32)                # absent entries: a size the rule refuses
        bfi = np.zeros((S, T), np.uint8)
        for s in range(S):
            for t in range(int(cnt[s])):
                f = frames[s][pos[s] + t]
                fr[s, t, :f.size] = f
                nb[s, t] = f.size
        if T > 1:
            bfi[0, 1 % T] = cnt[0] > 1                                             # a frame flagged lost
            if var and cnt[S - 1] > 0:
                nb[S - 1, 0] = 0                                                   # size 0: lost
            if ch == 1 and cnt[1 % S] > 0:
                fr[1 % S, 0, 3:6] ^= 0x5D                                          # damage the decoder has to find itself
        # expectation
        inval = np.zeros((S, T), bool)
        if placed:
            bad = (0, 0) if k == 0 else None                              # stream 0 has every frame of call 0
            offs, cap, inval = _placement(api, fmt, ch, N, S, T, k, bad)
        want = [[None] * T for _ in range(S)]
        wst = np.full((S, T), ST_ABSENT, np.uint8)
        for s in range(S):
            for t in range(int(cnt[s])):
                n = int(nb[s, t])
                res = [o.decode(fr[s, t, :max(n, 1)], int(bfi[s, t]) if how != "device" else 0, dep, num_bytes=n) for o, dep in zip(orc[s], depths)]
                rc = res[0][0]
                assert rc in (0, 2) and all(r[0] == rc for r in res), [r[0] for r in res]
                want[s][t] = [r[1] for r in res]
                wst[s, t] = (rc == 2) | (ST_PLACE if inval[s, t] else 0)
        q = dict(T=T, cnt=cnt, want=want, wst=wst, inval=inval, present=present)
        if how in ("host", "hostsizes"):
            q["pcm"], q["st"] = d.decode(fr, bfi, bps=fmt, num_bytes=nb if how == "hostsizes" else None)
        else:
            d_fr = dev.put(fr)
            # the PCM: `pad` bytes of sentinels, the call's elements as sentinels, 64 bytes of sentinels
            q["n"] = cap if placed else S * T * ch * N
            q["bytes"] = pad + q["n"] * eb + 64
            q["d_base"] = dev.put(np.full(q["bytes"], 0x5A, np.uint8))
            q["d_pcm"] = q["d_base"] + pad
            if placed:
                q["offs"] = offs
                d.set_pcm_placement(dev.put(offs), cap)
            d_cnt = dev.put(cnt) if ragged else None
            if ragged:
                d.set_frame_counts(d_cnt)
            sync = not sc.get("ready")
            if how == "device":
                d.decode_device(d_fr, stride, T, q["d_pcm"], bps=fmt, sync=sync)
            elif how == "devhostsizes":
                d.decode_device(d_fr, stride, T, q["d_pcm"], bps=fmt, sync=sync, num_bytes=nb, bfi=bfi)
            else:
                q["d_st"] = dev.put(np.full((S, T), ST_SENT, np.uint8))
                d_nb, d_bfi = dev.put(nb), dev.put(bfi)
                if how == "sizes":
                    d.decode_device_sizes(d_fr, stride, T, q["d_pcm"], d_nb, d_bfi, q["d_st"], bps=fmt, sync=sync)
                else:
                    # packed: the frames back to back in the other stream order, a gap of one byte between them
                    po = np.zeros((S, T), np.int64)
                    at = 5
                    for s in range(S - 1, -1, -1):
                        for t in range(T):
                            po[s, t] = at
                            at += (int(nb[s, t]) if present[s, t] else 0) + 1
                    buf = np.full(at + 8, 0x33, np.uint8)
                    for s in range(S):
                        for t in range(int(cnt[s])):
                            buf[po[s, t]:po[s, t] + nb[s, t]] = fr[s, t, :nb[s, t]]
                    d.decode_device_packed(dev.put(buf), buf.size, dev.put(po), T, q["d_pcm"], d_nb, stride, d_bfi, q["d_st"], bps=fmt, sync=sync)
            if ragged:
                d.set_frame_counts(None)
            if placed:
                d.set_pcm_placement(None)
        queued.append(q)
        pos += cnt
    dev.sync()
    bad = []
    for k, q in enumerate(queued):
        T, cnt, want, wst = q["T"], q["cnt"], q["want"], q["wst"]
        if "pcm" in q:
            elems = np.ascontiguousarray(q["pcm"]).view(np.uint8).reshape(-1, eb)
            assert elems.shape[0] == S * T * ch * N and q["pcm"].shape == api.pcm_shape(fmt, S, T, ch, N)
            st = q["st"]
            assert (st == (wst & 1)).all(), (k, "status", st.tolist(), wst.tolist())
        else:
            raw = dev.get(q["d_base"], (q["bytes"],), np.uint8)
            elems = raw[pad:pad + q["n"] * eb].reshape(-1, eb)
        touched = np.zeros(elems.shape[0], bool)
        for s in range(S):
            for t in range(T):
                if not q["present"][s, t] or q["inval"][s, t]:
                    continue                                                # absent or refused: nothing written, the elements stay sentinels (below)
                idx = _frame_elems(api, fmt, ch, N, int(q["offs"][s, t])) if "offs" in q else _dense_elems(api, fmt, ch, T, N, s, t)
                touched[idx] = True
                if not _dec_same(api, out, fmt, elems[idx], want[s][t]):
                    bad.append((k, s, t))
        if "pcm" not in q:
            dirty = np.flatnonzero(np.concatenate([raw[:pad], np.where(touched[:, None], 0x5A, elems).reshape(-1), raw[pad + q["n"] * eb:]]) != 0x5A)
            assert bad or not dirty.size, (k, "samples outside the frames were written (byte offsets from the pointer)", (dirty[:8] - pad).tolist())
        if "d_st" in q:
            st = dev.get(q["d_st"], (S, T), np.uint8)
            assert (st == wst).all(), (k, "status", st.tolist(), wst.tolist())
    d.close()
    assert not bad, ("frames that differ from the oracle decoder (call, stream, frame)", len(bad), bad[:10])


@functools.lru_cache(maxsize=None)
def _fastmath_host(tmp):
    import importlib.util
    spec = importlib.util.spec_from_file_location("test_fastmath", os.path.join(ROOT, "tests", "test_fastmath.py"))
    tf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tf)
    return tf, tf.host_lib(tmp)


def run_fastmath(tmp_path, amd):
    """the test hook over a few thousand arguments against lc3_fastmath.h compiled for the host (which tools/fastmath_check.c pins to glibc)"""
    import ctypes as C
    tf, H = _fastmath_host(tmp_path)
    L = amd.load_library()
    L.lc3hip_test_fastmath.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_longlong]
    logs, ex = tf.sample_arguments(seed=5)
    for kind, x in ((0, logs[::97]), (1, logs[::89]), (2, ex[::83])):
        x = np.ascontiguousarray(x)
        got, want = np.zeros_like(x), np.zeros_like(x)
        assert L.lc3hip_test_fastmath(kind, x.ctypes.data, got.ctypes.data, x.size) == 0
        H.lc3m_host_eval(kind, x.ctypes.data, want.ctypes.data, x.size)
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), (kind, x[~same][:6], got[~same][:6], want[~same][:6])
