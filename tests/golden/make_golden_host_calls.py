"""Writes tests/golden/host_calls.json: what the host code of the batches (audio_codec_amd/csrc/lc3_host.c) answers and asks of the HIP runtime, recorded against the
build whose HIP side is tools/stub_shim.c (`make -C audio_codec_amd/csrc stub`).  No GPU is needed.

    python tests/golden/make_golden_host_calls.py            rewrites the file from the stub build of the working tree

Two parts, both computed by generate(), which tests/test_host_calls_cpu.py runs again and compares for equality:

  refusals   for every public batch and sharded entry of both sides, every lc3plus_*plan* hook and lc3plus_stream_state_header: the return code of the good call,
             of the call with each single bad argument, and of the call with each pair of bad arguments (the pairs pin the order of the checks).  Every case
             runs on handles of its own.  Only inputs whose handling is defined are used: a hook that does not check the frame length is given valid ones.
  scripts    call sequences on one handle: the return codes, both logs of the stub as one sequence per context (the second log holds the configuration traffic:
             uploads, downloads, lifecycle calls, the calls with words in device memory), and the getters afterwards (stride, num_bytes, bandwidth).

Shapes: 3 streams x 2 frames (2 shards get the uneven blocks 2 + 1), 48 kHz / 10 ms mono and stereo, 96 kHz / 10 ms hr for the hrmode refusals.
Pointers in the log are written as "buffer+offset" of the buffers the script passed, "null", or "internal" (the host's own scratch arrays)."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "host_calls.json")
STUB = os.path.join(ROOT, "audio_codec_amd", "_stub", "liblc3plus_stub.so")

S, T = 3, 2
GEOMS = {       # rate / rate2: two valid bitrates of a stream (all channels); nb / nb2: the stream-frame bytes they give; bw / bw2: two accepted bandwidths
    "mono":   dict(fs=48000, ch=1, ms=10.0, hr=0, rate=64000, rate2=96000, nb=80, nb2=120, N=480),
    "stereo": dict(fs=48000, ch=2, ms=10.0, hr=0, rate=128000, rate2=192000, nb=160, nb2=240, N=480),
    "hr96":   dict(fs=96000, ch=1, ms=10.0, hr=1, rate=200000, rate2=240000, nb=250, nb2=300, N=960),
}
DEV, DEV2, HSTREAM = 0x10000, 0x20000, 0x50      # stand-ins for device pointers (16-byte aligned) and a HIP stream: the host passes them on and never reads them

SIGS = {        # p pointer, i int, f float, q int64, z size_t; the result is an int unless named in RES
    "lc3plus_enc_batch_create": "piiifipi", "lc3plus_dec_batch_create": "piiifipi", "lc3plus_enc_batch_destroy": "p", "lc3plus_dec_batch_destroy": "p",
    "lc3plus_enc_batch_input_samples": "p", "lc3plus_enc_batch_stride": "p", "lc3plus_enc_batch_num_bytes": "pi", "lc3plus_enc_batch_bandwidth": "pi",
    "lc3plus_enc_batch_set_bitrate": "pii", "lc3plus_enc_batch_set_bandwidth": "pii", "lc3plus_enc_batch_set_pcm_placement": "ppq",
    "lc3plus_enc_batch_set_frame_counts": "pp", "lc3plus_enc_batch_set_input_ready": "pi", "lc3plus_enc_batch_last_status": "ppi",
    "lc3plus_enc_batch_last_records": "ppi", "lc3plus_enc_batch_work_buffer": "pipppp", "lc3plus_dec_batch_work_buffer": "pipppp",
    "lc3plus_enc_batch_encode": "ppiiipiipi", "lc3plus_enc_batch_encode_traced": "ppiipip", "lc3plus_enc_batch_encode_bitrates": "ppiipipiippi",
    "lc3plus_enc_batch_encode_bitrates_traced": "ppipipip", "lc3plus_enc_batch_encode_bandwidths": "ppiippipiippi",
    "lc3plus_enc_batch_encode_rates_device": "ppippipipppi", "lc3plus_enc_batch_encode_packed": "ppippiipqpppppi",
    "lc3plus_enc_batch_reset_streams": "ppippi", "lc3plus_enc_batch_export_streams": "ppipipi", "lc3plus_enc_batch_import_streams": "ppipippi",
    "lc3plus_enc_batch_state_size": "p", "lc3plus_enc_batch_get_state": "ppz", "lc3plus_enc_batch_set_state": "ppz", "lc3plus_enc_batch_stream_state_size": "p",
    "lc3plus_dec_batch_output_samples": "p", "lc3plus_dec_batch_delay": "p", "lc3plus_dec_batch_num_bytes": "pi", "lc3plus_dec_batch_set_num_bytes": "pii",
    "lc3plus_dec_batch_set_pcm_placement": "ppq", "lc3plus_dec_batch_set_frame_counts": "pp", "lc3plus_dec_batch_set_input_ready": "pi",
    "lc3plus_dec_batch_decode": "ppiipipiippi", "lc3plus_dec_batch_decode_traced": "ppipipipp", "lc3plus_dec_batch_decode_sizes": "ppiippipiippi",
    "lc3plus_dec_batch_decode_sizes_device": "ppippipippi", "lc3plus_dec_batch_decode_packed": "ppqppipipippi",
    "lc3plus_dec_batch_reset_streams": "ppippi", "lc3plus_dec_batch_export_streams": "ppipipi", "lc3plus_dec_batch_import_streams": "ppipippi",
    "lc3plus_dec_batch_state_size": "p", "lc3plus_dec_batch_get_state": "ppz", "lc3plus_dec_batch_set_state": "ppz", "lc3plus_dec_batch_stream_state_size": "p",
    "lc3plus_enc_plan_bandwidths": "ifiippip", "lc3plus_enc_plan_bitrates": "iifiipipp", "lc3plus_enc_plan_rates_lenient": "iifiippppiipppp",
    "lc3plus_enc_plan_rates_ragged": "iifiippppiippppp", "lc3plus_plan_chan": "ifiip", "lc3plus_dec_plan_sizes": "iifiipppiipppp",
    "lc3plus_dec_plan_sizes_lenient": "iifiipppiippppp", "lc3plus_dec_plan_packed_lenient": "iifiipppqipippppp", "lc3plus_dec_plan_counts": "piip",
    "lc3plus_plan_packed": "piiiqppp", "lc3plus_plan_placed": "iiipqqp", "lc3plus_frame_info_side": "iifipip", "lc3plus_stream_state_header": "iiifip",
    "lc3plus_stream_list_check": "ipi", "lc3plus_shard_block": "iiipp",
    "lc3plus_enc_sharded_create": "piiifippi", "lc3plus_dec_sharded_create": "piiifippi", "lc3plus_enc_sharded_destroy": "p", "lc3plus_dec_sharded_destroy": "p",
    "lc3plus_enc_sharded_shards": "p", "lc3plus_dec_sharded_shards": "p", "lc3plus_enc_sharded_shard": "pi", "lc3plus_dec_sharded_shard": "pi",
    "lc3plus_enc_sharded_device": "pi", "lc3plus_dec_sharded_device": "pi", "lc3plus_enc_sharded_owner": "pipp", "lc3plus_dec_sharded_owner": "pipp",
    "lc3plus_enc_sharded_input_samples": "p", "lc3plus_enc_sharded_num_bytes": "pi", "lc3plus_enc_sharded_stride": "p", "lc3plus_enc_sharded_set_bitrate": "pii",
    "lc3plus_enc_sharded_set_bandwidth": "pii", "lc3plus_enc_sharded_bandwidth": "pi", "lc3plus_enc_sharded_encode": "ppippipip",
    "lc3plus_enc_sharded_encode_device": "ppiipipi", "lc3plus_enc_sharded_state_size": "p", "lc3plus_enc_sharded_get_state": "ppz",
    "lc3plus_enc_sharded_set_state": "ppz", "lc3plus_dec_sharded_output_samples": "p", "lc3plus_dec_sharded_delay": "p", "lc3plus_dec_sharded_num_bytes": "pi",
    "lc3plus_dec_sharded_set_num_bytes": "pii", "lc3plus_dec_sharded_decode": "ppippipip", "lc3plus_dec_sharded_decode_device": "ppiipipi",
    "lc3plus_dec_sharded_state_size": "p", "lc3plus_dec_sharded_get_state": "ppz", "lc3plus_dec_sharded_set_state": "ppz",
}
CT = {"p": C.c_void_p, "i": C.c_int, "f": C.c_float, "q": C.c_int64, "z": C.c_size_t}
RES = {n: C.c_size_t for n in SIGS if n.endswith("state_size")}
RES.update({"lc3plus_enc_sharded_shard": C.c_void_p, "lc3plus_dec_sharded_shard": C.c_void_p})
KINDS = ["?", "encode", "decode", "get_state", "set_state", "wait", "placement", "counts"]


class Rec(C.Structure):                                              # lc3stub_rec (tools/stub_shim.c)
    _fields_ = [("ctx", C.c_int32), ("kind", C.c_int32), ("dec", C.c_int32), ("n_frames", C.c_int32), ("stride", C.c_int32), ("fmt", C.c_int32),
                ("on_device", C.c_int32), ("sync", C.c_int32), ("p", C.c_uint64 * 4), ("a", C.c_int64 * 3), ("b", C.c_int64 * 3), ("bytes", C.c_uint64),
                ("hip_stream", C.c_uint64)]


def load(path=STUB):
    L = C.CDLL(path)
    for name, sig in SIGS.items():
        f = getattr(L, name)
        f.argtypes = [CT[c] for c in sig]
        f.restype = RES.get(name, C.c_int)
    L.lc3stub_cfg_log.argtypes = [C.c_void_p, C.c_size_t]
    L.lc3stub_cfg_log.restype = C.c_size_t
    assert L.lc3stub_rec_sizeof() == C.sizeof(Rec)
    return L


def i32(x):
    return np.ascontiguousarray(x, dtype=np.int32)


def ptr(v):
    """An argument as ctypes takes it: arrays by address, everything else as it is."""
    return v.ctypes.data if isinstance(v, np.ndarray) else v


class Bufs:
    """The buffers of one geometry: every array a call may be given, by name, good and bad; kept alive here."""

    def __init__(self, g):
        ch, N, nb, nb2 = g["ch"], g["N"], g["nb"], g["nb2"]
        self.g = g
        self.stride = 700
        b = self.b = {}
        b["pcm"] = np.zeros(S * T * ch * N, np.int32)               # large enough for every format
        b["out"] = np.zeros(S * T * self.stride, np.uint8)          # also the decoder's frames
        b["rates"] = i32([[g["rate"], g["rate2"]]] * S)             # every stream ends on rate2
        b["rates_bad"] = i32([[g["rate"], g["rate"]], [g["rate"], g["rate"]], [g["rate"], 1000]])       # in the last shard's rows
        b["create_rates"] = i32([g["rate"]] * S)
        b["create_rates_bad"] = i32([g["rate"], g["rate"], 1000])
        b["bws"] = i32([[8000, 4000]] * S)
        b["bws_neg"] = i32([[8000, 4000], [8000, 4000], [8000, -5]])
        b["bws_refused"] = i32([[8000, 4000], [8000, 24000], [8000, 4000]])     # 2 * 24000 > 40000: refused as set_bandwidth refuses it, the value in force stays
        b["sizes"] = i32([[nb, nb2]] * S)
        b["sizes_bad"] = i32([[nb, nb2], [nb, nb2], [nb, 5 * ch]])
        b["create_sizes"] = i32([nb] * S)
        b["create_sizes_bad"] = i32([nb, nb, 5 * ch])
        b["bfi"] = np.array([[0, 1], [0, 0], [1, 0]], np.uint8)
        b["bfi_bad"] = np.array([[0, 1], [0, 0], [2, 0]], np.uint8)
        b["nb_out"] = np.full(S * T, -7, np.int32)
        b["status"] = np.zeros(S * T, np.uint8)
        b["streams"] = i32([2, 0])
        b["streams_twice"] = i32([2, 2])
        b["streams_range"] = i32([0, S])
        b["two_rates"] = i32([g["rate2"], g["rate"]])
        b["two_rates_bad"] = i32([g["rate2"], 1000])
        b["two_sizes"] = i32([nb2, nb])
        b["two_sizes_bad"] = i32([nb2, 5 * ch])
        b["blob"] = np.zeros(1 << 16, np.uint8)
        b["state"] = np.zeros(1 << 12, np.uint8)
        b["devices"] = i32([0, 0])
        b["devices_neg"] = i32([0, -1])
        b["devices4"] = i32([0, 0, 0, 0])
        b["words"] = np.zeros(64, np.int64)                         # small outputs of the hooks
        b["words2"] = np.zeros(64, np.int64)
        b["words3"] = np.zeros(64, np.int64)
        b["words4"] = np.zeros(64, np.int64)
        b["words5"] = np.zeros(64, np.int64)
        b["start_rates"] = i32([g["rate"]] * S)
        b["start_bw"] = i32([0] * S)
        b["start_sizes"] = i32([nb] * S)
        b["offsets"] = np.arange(S * T, dtype=np.int64) * self.stride
        b["pk_sizes"] = i32([nb] * (S * T))
        b["counts"] = i32([2, 0, 1])
        b["frame"] = np.zeros(self.stride, np.uint8)
        b["ptrs_a"] = (C.c_void_p * 2)(DEV, DEV + 0x1000)
        b["ptrs_b"] = (C.c_void_p * 2)(DEV2, DEV2 + 0x1000)
        b["ptrs_null"] = (C.c_void_p * 2)(DEV, None)
        b["ptrs_hs"] = (C.c_void_p * 2)(HSTREAM, None)

    def __getitem__(self, k):
        return self.b[k]

    def addr(self, v):
        if isinstance(v, np.ndarray):
            return v.ctypes.data
        if isinstance(v, C.Array):
            return C.addressof(v)
        return v

    def name_of(self, p):
        if p == 0:
            return "null"
        for k, v in self.b.items():
            a = self.addr(v)
            n = v.nbytes if isinstance(v, np.ndarray) else C.sizeof(v)
            if a <= p < a + n:
                return "%s+%d" % (k, p - a)
        for k, v in (("dev", DEV), ("dev2", DEV2)):
            if v <= p < v + 0x10000:
                return "%s+%d" % (k, p - v)
        return "internal"


# ------------------------------------------------------------------------------------------------------------------------------------------------
# handles
# ------------------------------------------------------------------------------------------------------------------------------------------------
def make(L, B, kind, sharded=False):
    g, h = B.g, C.c_void_p()
    cfg = B["create_rates"] if kind == "enc" else B["create_sizes"]
    if sharded:
        rc = getattr(L, "lc3plus_%s_sharded_create" % kind)(C.byref(h), S, g["fs"], g["ch"], g["ms"], g["hr"], ptr(cfg), ptr(B["devices"]), 2)
    else:
        rc = getattr(L, "lc3plus_%s_batch_create" % kind)(C.byref(h), S, g["fs"], g["ch"], g["ms"], g["hr"], ptr(cfg), 0)
    assert rc == 0 and h.value, (kind, sharded, rc)
    return h


def drop(L, kind, sharded, h):
    assert getattr(L, "lc3plus_%s_%s_destroy" % (kind, "sharded" if sharded else "batch"))(h) == 0


# ------------------------------------------------------------------------------------------------------------------------------------------------
# part 1: the refusal table
# ------------------------------------------------------------------------------------------------------------------------------------------------
H = "<handle>"              # the place of the handle among the arguments
PLACED, RAGGED, UNSAFE, STALE = "placed", "ragged", "bw_unsafe", "stale"       # states a handle is brought into before the call


def entries(B):
    """name -> (function, handle kind or None, sharded, [(argument name, good value)], {bad name: {argument name: bad value} or {state: 1}})."""
    g = B.g
    fs, ch, ms, hr, N, nb = g["fs"], g["ch"], g["ms"], g["hr"], g["N"], g["nb"]
    st = B.stride
    E = {}
    geom_bad = {"fs": {"fs": 47000}, "ch": {"ch": 3}, "ms": {"ms": 7.5}, "hr_low_fs": {"fs": 16000, "hr": 1}, "hr_32k": {"fs": 32000, "hr": 1},
                "hr_off_96k": {"fs": 96000, "hr": 0}, "hr_neg": {"hr": -1}}
    hook_bad = {k: v for k, v in geom_bad.items() if k != "ms"}      # the decoder's hooks do not check the frame length: valid ones only
    nch_bad = {k: v for k, v in geom_bad.items() if k != "ch"}       # one channel, not an argument

    def e(name, fn, kind, sharded, good, bad):
        E[name] = (fn, kind, sharded, good, bad)

    for kind, cfg in (("enc", "create_rates"), ("dec", "create_sizes")):
        out = C.c_void_p()
        B.b["handle_out_" + kind] = np.zeros(1, np.uint64)
        e(kind + "_batch_create", "lc3plus_%s_batch_create" % kind, None, False,
          [("out", B["handle_out_" + kind]), ("S", S), ("fs", fs), ("ch", ch), ("ms", ms), ("hr", hr), ("cfg", B[cfg]), ("device", 0)],
          dict(geom_bad, out_null={"out": None}, cfg_null={"cfg": None}, S0={"S": 0}, cfg_bad={"cfg": B[cfg + "_bad"]}))
        e(kind + "_sharded_create", "lc3plus_%s_sharded_create" % kind, None, False,
          [("out", B["handle_out_" + kind]), ("S", S), ("fs", fs), ("ch", ch), ("ms", ms), ("hr", hr), ("cfg", B[cfg]), ("devices", B["devices"]), ("nd", 2)],
          dict(geom_bad, out_null={"out": None}, cfg_null={"cfg": None}, S0={"S": 0}, cfg_bad={"cfg": B[cfg + "_bad"]}, devices_null={"devices": None},
               nd0={"nd": 0}, devices_neg={"devices": B["devices_neg"]}, devices_many={"devices": B["devices4"], "nd": 4}))
        del out
    hnull, stream_bad = {"b_null": {"b": None}}, {"stream_neg": {"stream": -1}, "stream_high": {"stream": S}}
    for sh in (False, True):
        pre = "enc_sharded_" if sh else "enc_batch_"
        fn = "lc3plus_" + pre
        e(pre + "stride", fn + "stride", "enc", sh, [("b", H)], hnull)
        e(pre + "input_samples", fn + "input_samples", "enc", sh, [("b", H)], hnull)
        e(pre + "num_bytes", fn + "num_bytes", "enc", sh, [("b", H), ("stream", 1)], dict(hnull, **stream_bad))
        e(pre + "bandwidth", fn + "bandwidth", "enc", sh, [("b", H), ("stream", 1)], dict(hnull, **stream_bad))
        e(pre + "set_bitrate", fn + "set_bitrate", "enc", sh, [("b", H), ("stream", 1), ("rate", g["rate2"])],
          dict(hnull, rate0={"rate": 0}, rate_low={"rate": 1000}, **stream_bad))
        e(pre + "set_bandwidth", fn + "set_bandwidth", "enc", sh, [("b", H), ("stream", 1), ("bw", 8000)],
          dict(hnull, bw_refused={"bw": 24000}, bw_low_cut={"bw": 10}, **stream_bad))
        e(pre + "state_size", fn + "state_size", "enc", sh, [("b", H)], hnull)
        for op in ("get_state", "set_state"):
            e(pre + op, fn + op, "enc", sh, [("b", H), ("state", B["state"]), ("size", 32 * S * ch)], dict(hnull, state_null={"state": None}, size={"size": 5}))
        pre = "dec_sharded_" if sh else "dec_batch_"
        fn = "lc3plus_" + pre
        e(pre + "output_samples", fn + "output_samples", "dec", sh, [("b", H)], hnull)
        e(pre + "delay", fn + "delay", "dec", sh, [("b", H)], hnull)
        e(pre + "num_bytes", fn + "num_bytes", "dec", sh, [("b", H), ("stream", 1)], dict(hnull, **stream_bad))
        e(pre + "set_num_bytes", fn + "set_num_bytes", "dec", sh, [("b", H), ("stream", 1), ("nb", g["nb2"])],
          dict(hnull, nb_low={"nb": 5 * ch}, nb_high={"nb": 5000}, **stream_bad))
        e(pre + "state_size", fn + "state_size", "dec", sh, [("b", H)], hnull)
        for op in ("get_state", "set_state"):
            e(pre + op, fn + op, "dec", sh, [("b", H), ("state", B["state"]), ("size", 32 * S * ch)], dict(hnull, state_null={"state": None}, size={"size": 5}))
    for kind in ("enc", "dec"):
        for op in ("shards",):
            e("%s_sharded_%s" % (kind, op), "lc3plus_%s_sharded_%s" % (kind, op), kind, True, [("b", H)], hnull)
        for op in ("shard", "device"):
            e("%s_sharded_%s" % (kind, op), "lc3plus_%s_sharded_%s" % (kind, op), kind, True, [("b", H), ("shard", 1)],
              dict(hnull, shard_neg={"shard": -1}, shard_high={"shard": 2}))
        e(kind + "_sharded_owner", "lc3plus_%s_sharded_owner" % kind, kind, True, [("b", H), ("stream", 2), ("shard", B["words"]), ("local", B["words2"])],
          dict(hnull, shard_null={"shard": None}, local_null={"local": None}, **stream_bad))
        e(kind + "_sharded_destroy", "lc3plus_%s_sharded_destroy" % kind, None, False, [("b", None)], {})
        e(kind + "_batch_destroy", "lc3plus_%s_batch_destroy" % kind, None, False, [("b", None)], {})
        pre = kind + "_batch_"
        fn = "lc3plus_" + pre
        e(pre + "set_pcm_placement", fn + "set_pcm_placement", kind, False, [("b", H), ("offsets", DEV), ("capacity", 1 << 20)],
          dict(hnull, capacity_neg={"capacity": -1}, offsets_null={"offsets": None}))
        e(pre + "set_frame_counts", fn + "set_frame_counts", kind, False, [("b", H), ("counts", DEV)], dict(hnull, counts_null={"counts": None}))
        e(pre + "set_input_ready", fn + "set_input_ready", kind, False, [("b", H), ("ready", 1)], hnull)
        e(pre + "stream_state_size", fn + "stream_state_size", kind, False, [("b", H)], hnull)
        e(pre + "work_buffer", fn + "work_buffer", kind, False,      # (the stub has no buffers: the good call is refused behind its checks)
          [("b", H), ("i", 0), ("name", B["words"]), ("ptr", B["words2"]), ("bytes", B["words3"]), ("elem", B["words4"])],
          dict(hnull, name_null={"name": None}, ptr_null={"ptr": None}, bytes_null={"bytes": None}, elem_null={"elem": None}))
        cfg = "two_rates" if kind == "enc" else "two_sizes"
        lst = {"streams_null": {"streams": None}, "n0": {"n": 0}, "streams_twice": {"streams": B["streams_twice"]}, "streams_range": {"streams": B["streams_range"]}}
        e(pre + "reset_streams", fn + "reset_streams", kind, False, [("b", H), ("streams", B["streams"]), ("n", 2), ("cfg", B[cfg]), ("hs", None), ("sync", 1)],
          dict(hnull, cfg_bad={"cfg": B[cfg + "_bad"]}, cfg_null={"cfg": None}, stale={STALE: 1}, **lst))
        e(pre + "export_streams", fn + "export_streams", kind, False,
          [("b", H), ("streams", B["streams"]), ("n", 2), ("blob", B["blob"]), ("on_dev", 0), ("hs", None), ("sync", 1)],
          dict(hnull, blob_null={"blob": None}, blob_dev_unaligned={"blob": DEV + 4, "on_dev": 1}, blob_dev={"blob": DEV, "on_dev": 1}, **lst))
        e(pre + "import_streams", fn + "import_streams", kind, False,
          [("b", H), ("streams", B["streams"]), ("n", 2), ("blob", "<blobs>"), ("on_dev", 0), ("status", B["status"]), ("hs", None), ("sync", 1)],
          dict(hnull, blob_null={"blob": None}, blob_dev_unaligned={"blob": DEV + 4, "on_dev": 1}, blob_dev={"blob": DEV, "on_dev": 1},
               blob_header={"blob": B["blob"]}, status_null={"status": None}, **lst))

    for op in ("last_status", "last_records"):
        e("enc_batch_" + op, "lc3plus_enc_batch_" + op, "enc", False, [("b", H), ("out", B["words"]), ("max", 8)],
          dict(hnull, out_null={"out": None}, max_neg={"max": -1}))

    # ---- the encode calls ----
    common = dict(hnull, pcm_null={"pcm": None}, out_null={"out": None}, fmt={"fmt": 17}, T0={"T": 0}, placed={PLACED: 1}, ragged={RAGGED: 1})
    e("enc_batch_encode", "lc3plus_enc_batch_encode", "enc", False,
      [("b", H), ("pcm", B["pcm"]), ("on_dev", 0), ("fmt", 16), ("T", T), ("out", B["out"]), ("stride", st), ("out_dev", 0), ("hs", None), ("sync", 1)],
      dict(common, stride={"stride": nb - 1}, stale={STALE: 1}, placed_dev_chmajor={PLACED: 1, "pcm": DEV, "on_dev": 1, "fmt": 16 | 0x200}))
    e("enc_batch_encode_traced", "lc3plus_enc_batch_encode_traced", "enc", False,
      [("b", H), ("pcm", B["pcm"]), ("fmt", 16), ("T", T), ("out", B["out"]), ("stride", st), ("traces", DEV)],
      dict(common, stride={"stride": nb - 1}, fmt_float={"fmt": 0x20}, fmt_layout={"fmt": 16 | 0x100}))
    e("enc_batch_encode_bitrates", "lc3plus_enc_batch_encode_bitrates", "enc", False,
      [("b", H), ("pcm", B["pcm"]), ("on_dev", 0), ("fmt", 16), ("rates", B["rates"]), ("T", T), ("out", B["out"]), ("stride", st), ("out_dev", 0),
       ("nb", B["nb_out"]), ("hs", None), ("sync", 1)],
      dict(common, rates_null={"rates": None}, rates_bad={"rates": B["rates_bad"]}, stride={"stride": g["nb2"] - 1}, nb_null={"nb": None}))
    e("enc_batch_encode_bitrates_traced", "lc3plus_enc_batch_encode_bitrates_traced", "enc", False,
      [("b", H), ("pcm", B["pcm"]), ("fmt", 16), ("rates", B["rates"]), ("T", T), ("out", B["out"]), ("stride", st), ("traces", DEV)],
      dict(common, rates_null={"rates": None}, rates_bad={"rates": B["rates_bad"]}, stride={"stride": g["nb2"] - 1}, traces_null={"traces": None},
           fmt_float={"fmt": 0x20}))
    e("enc_batch_encode_bandwidths", "lc3plus_enc_batch_encode_bandwidths", "enc", False,
      [("b", H), ("pcm", B["pcm"]), ("on_dev", 0), ("fmt", 16), ("bws", B["bws"]), ("rates", B["rates"]), ("T", T), ("out", B["out"]), ("stride", st),
       ("out_dev", 0), ("nb", B["nb_out"]), ("hs", None), ("sync", 1)],
      dict(common, bws_null={"bws": None}, bws_neg={"bws": B["bws_neg"]}, bws_refused={"bws": B["bws_refused"]}, rates_null={"rates": None},
           rates_bad={"rates": B["rates_bad"]}, stride={"stride": g["nb2"] - 1}, stride_no_rates={"rates": None, "stride": nb - 1}, unsafe={UNSAFE: 1}))
    e("enc_sharded_encode", "lc3plus_enc_sharded_encode", "enc", True,
      [("b", H), ("pcm", B["pcm"]), ("fmt", 16), ("bws", B["bws"]), ("rates", B["rates"]), ("T", T), ("out", B["out"]), ("stride", st), ("nb", B["nb_out"])],
      dict(hnull, pcm_null={"pcm": None}, out_null={"out": None}, fmt={"fmt": 17}, T0={"T": 0}, bws_null={"bws": None}, bws_neg={"bws": B["bws_neg"]},
           bws_refused={"bws": B["bws_refused"]}, rates_null={"rates": None}, rates_bad={"rates": B["rates_bad"]}, stride={"stride": g["nb2"] - 1},
           plain_stride={"bws": None, "rates": None, "stride": nb - 1}, nb_null={"nb": None}))
    e("enc_sharded_encode_device", "lc3plus_enc_sharded_encode_device", "enc", True,
      [("b", H), ("pcm", B["ptrs_a"]), ("fmt", 16), ("T", T), ("out", B["ptrs_b"]), ("stride", st), ("hs", B["ptrs_hs"]), ("sync", 1)],
      dict(hnull, pcm_null={"pcm": None}, out_null={"out": None}, pcm_one_null={"pcm": B["ptrs_null"]}, fmt={"fmt": 17}, T0={"T": 0}, stride={"stride": nb - 1},
           hs_null={"hs": None}))
    dev = dict(hnull, pcm_null={"pcm": None}, out_null={"out": None}, fmt={"fmt": 17}, T0={"T": 0}, placed_chmajor={PLACED: 1, "fmt": 16 | 0x200},
               no_words={"rates": None, "bws": None}, rates_null={"rates": None}, bws_null={"bws": None}, unsafe={UNSAFE: 1}, ragged={RAGGED: 1}, stale={STALE: 1})
    e("enc_batch_encode_rates_device", "lc3plus_enc_batch_encode_rates_device", "enc", False,
      [("b", H), ("pcm", DEV), ("fmt", 16), ("rates", DEV2), ("bws", DEV2 + 0x100), ("T", T), ("out", DEV + 0x1000), ("stride", st), ("nb", None), ("flags", None),
       ("hs", None), ("sync", 0)], dict(dev, stride={"stride": nb - 1}))
    e("enc_batch_encode_packed", "lc3plus_enc_batch_encode_packed", "enc", False,
      [("b", H), ("pcm", DEV), ("fmt", 16), ("rates", DEV2), ("bws", DEV2 + 0x100), ("T", T), ("order", 0), ("out", DEV + 0x1000), ("capacity", 1 << 20),
       ("offsets", None), ("total", None), ("nb", None), ("flags", None), ("hs", None), ("sync", 0)],
      dict(dev, order={"order": 2}, capacity_neg={"capacity": -1}))

    # ---- the decode calls ----
    dcommon = dict(hnull, frames_null={"frames": None}, pcm_null={"pcm": None}, fmt={"fmt": 17}, T0={"T": 0}, placed={PLACED: 1}, ragged={RAGGED: 1})
    e("dec_batch_decode", "lc3plus_dec_batch_decode", "dec", False,
      [("b", H), ("frames", B["out"]), ("f_dev", 0), ("stride", st), ("bfi", B["bfi"]), ("T", T), ("pcm", B["pcm"]), ("pcm_dev", 0), ("fmt", 16),
       ("status", B["status"]), ("hs", None), ("sync", 1)], dict(dcommon, stride={"stride": nb - 1}, bfi_null={"bfi": None}, stale={STALE: 1}))
    e("dec_batch_decode_traced", "lc3plus_dec_batch_decode_traced", "dec", False,
      [("b", H), ("frames", B["out"]), ("stride", st), ("bfi", B["bfi"]), ("T", T), ("pcm", B["pcm"]), ("fmt", 16), ("status", B["status"]), ("traces", DEV)],
      dict(dcommon, stride={"stride": nb - 1}, fmt_float={"fmt": 0x20}))
    e("dec_batch_decode_sizes", "lc3plus_dec_batch_decode_sizes", "dec", False,
      [("b", H), ("frames", B["out"]), ("f_dev", 0), ("stride", st), ("sizes", B["sizes"]), ("bfi", B["bfi"]), ("T", T), ("pcm", B["pcm"]), ("pcm_dev", 0),
       ("fmt", 16), ("status", B["status"]), ("hs", None), ("sync", 1)],
      dict(dcommon, stride={"stride": g["nb2"] - 1}, sizes_null={"sizes": None}, sizes_bad={"sizes": B["sizes_bad"]}, bfi_bad={"bfi": B["bfi_bad"]},
           bfi_null={"bfi": None}, stale={STALE: 1}))
    e("dec_sharded_decode", "lc3plus_dec_sharded_decode", "dec", True,
      [("b", H), ("frames", B["out"]), ("stride", st), ("sizes", B["sizes"]), ("bfi", B["bfi"]), ("T", T), ("pcm", B["pcm"]), ("fmt", 16), ("status", B["status"])],
      dict(hnull, frames_null={"frames": None}, pcm_null={"pcm": None}, fmt={"fmt": 17}, T0={"T": 0}, stride={"stride": g["nb2"] - 1},
           sizes_null={"sizes": None}, sizes_bad={"sizes": B["sizes_bad"]}, bfi_bad={"bfi": B["bfi_bad"]}, bfi_null={"bfi": None},
           plain_stride={"sizes": None, "stride": nb - 1}))
    e("dec_sharded_decode_device", "lc3plus_dec_sharded_decode_device", "dec", True,
      [("b", H), ("frames", B["ptrs_a"]), ("stride", st), ("T", T), ("pcm", B["ptrs_b"]), ("fmt", 16), ("hs", B["ptrs_hs"]), ("sync", 1)],
      dict(hnull, frames_null={"frames": None}, pcm_null={"pcm": None}, frames_one_null={"frames": B["ptrs_null"]}, fmt={"fmt": 17}, T0={"T": 0},
           stride={"stride": nb - 1}, hs_null={"hs": None}))
    ddev = dict(hnull, frames_null={"frames": None}, pcm_null={"pcm": None}, sizes_null={"sizes": None}, fmt={"fmt": 17}, T0={"T": 0},
                placed_chmajor={PLACED: 1, "fmt": 16 | 0x200}, ragged={RAGGED: 1}, stale={STALE: 1})
    e("dec_batch_decode_sizes_device", "lc3plus_dec_batch_decode_sizes_device", "dec", False,
      [("b", H), ("frames", DEV), ("stride", st), ("sizes", DEV2), ("bfi", None), ("T", T), ("pcm", DEV + 0x4000), ("fmt", 16), ("status", None), ("hs", None),
       ("sync", 0)], dict(ddev, stride0={"stride": 0}))
    e("dec_batch_decode_packed", "lc3plus_dec_batch_decode_packed", "dec", False,
      [("b", H), ("frames", DEV), ("capacity", 1 << 20), ("offsets", DEV2 + 0x100), ("sizes", DEV2), ("max", st), ("bfi", None), ("T", T), ("pcm", DEV + 0x4000),
       ("fmt", 16), ("status", None), ("hs", None), ("sync", 0)], dict(ddev, offsets_null={"offsets": None}, max0={"max": 0}, capacity_neg={"capacity": -1}))

    # ---- the hooks: no handle ----
    n0 = {"S0": {"S": 0}, "T0": {"T": 0}}
    e("enc_plan_bandwidths", "lc3plus_enc_plan_bandwidths", None, False,
      [("fs", fs), ("ms", ms), ("hr", hr), ("S", S), ("start", B["start_bw"]), ("bws", B["bws"]), ("T", T), ("in_force", B["words"].view(np.int32))],
      dict(nch_bad, start_null={"start": None}, bws_null={"bws": None}, in_force_null={"in_force": None}, bws_neg={"bws": B["bws_neg"]},
           bws_refused={"bws": B["bws_refused"]}, hr_48k={"fs": 48000, "hr": 1}, **n0))
    e("enc_plan_bitrates", "lc3plus_enc_plan_bitrates", None, False,
      [("fs", fs), ("ch", ch), ("ms", ms), ("hr", hr), ("S", S), ("rates", B["rates"]), ("T", T), ("nb", B["words"].view(np.int32)), ("max", B["words2"])],
      dict(geom_bad, rates_null={"rates": None}, nb_null={"nb": None}, max_null={"max": None}, rates_bad={"rates": B["rates_bad"]}, **n0))
    rates_host = [("fs", fs), ("ch", ch), ("ms", ms), ("hr", hr), ("S", S), ("start_rates", B["start_rates"]), ("start_bw", B["start_bw"]), ("rates", B["rates"]),
                  ("bws", B["bws"] if not hr else None), ("T", T), ("stride", st), ("nb", B["words"].view(np.int32)), ("bwf", B["words2"].view(np.int32)),
                  ("flags", B["words3"].view(np.uint8)), ("end", B["words4"].view(np.int32))]
    rates_bad = dict(geom_bad, start_rates_null={"start_rates": None}, start_bw_null={"start_bw": None}, nb_null={"nb": None}, bwf_null={"bwf": None},
                     flags_null={"flags": None}, end_null={"end": None}, no_words={"rates": None, "bws": None}, with_bws={"bws": B["bws"]},
                     start_rate_bad={"start_rates": B["create_rates_bad"]}, stride_low={"stride": nb - 1}, rates_bad={"rates": B["rates_bad"]}, **n0)
    e("enc_plan_rates_lenient", "lc3plus_enc_plan_rates_lenient", None, False, rates_host, rates_bad)
    e("enc_plan_rates_ragged", "lc3plus_enc_plan_rates_ragged", None, False, rates_host + [("counts", B["counts"])], dict(rates_bad, counts_null={"counts": None}))
    e("plan_chan", "lc3plus_plan_chan", None, False, [("fs", fs), ("ms", ms), ("hr", hr), ("nbytes", nb // ch), ("out", B["words"].view(np.int32))],
      dict(nch_bad, out_null={"out": None}, nbytes_low={"nbytes": 5}, nbytes_high={"nbytes": 5000}, hr_48k={"fs": 48000, "hr": 1}))
    sizes_host = [("fs", fs), ("ch", ch), ("ms", ms), ("hr", hr), ("S", S), ("start", B["start_sizes"]), ("sizes", B["sizes"]), ("bfi", B["bfi"]), ("T", T),
                  ("stride", st), ("eff", B["words"].view(np.uint16)), ("lost", B["words2"].view(np.uint8))]
    sizes_bad = dict(hook_bad, start_null={"start": None}, sizes_null={"sizes": None}, eff_null={"eff": None}, lost_null={"lost": None}, end_null={"end": None},
                     max_null={"max": None}, sizes_bad={"sizes": B["sizes_bad"]}, bfi_bad={"bfi": B["bfi_bad"]}, bfi_null={"bfi": None}, stride_low={"stride": nb})
    tail = [("end", B["words4"].view(np.int32)), ("max", B["words5"].view(np.int32))]
    e("dec_plan_sizes", "lc3plus_dec_plan_sizes", None, False, sizes_host + tail, sizes_bad)
    e("dec_plan_sizes_lenient", "lc3plus_dec_plan_sizes_lenient", None, False, sizes_host + [("invalid", B["words3"].view(np.uint8))] + tail,
      dict(sizes_bad, invalid_null={"invalid": None}))
    e("dec_plan_packed_lenient", "lc3plus_dec_plan_packed_lenient", None, False,
      [("fs", fs), ("ch", ch), ("ms", ms), ("hr", hr), ("S", S), ("start", B["start_sizes"]), ("sizes", B["sizes"]), ("offsets", B["offsets"]),
       ("capacity", S * T * st), ("max_bytes", st), ("bfi", B["bfi"]), ("T", T), ("eff", B["words"].view(np.uint16)), ("lost", B["words2"].view(np.uint8)),
       ("invalid", B["words3"].view(np.uint8))] + tail,
      dict({k: v for k, v in sizes_bad.items() if k != "stride_low"}, invalid_null={"invalid": None}, offsets_null={"offsets": None}, max_bytes0={"max_bytes": 0},
           capacity_low={"capacity": st}))
    e("dec_plan_counts", "lc3plus_dec_plan_counts", None, False, [("counts", B["counts"]), ("S", S), ("T", T), ("effective", B["words"].view(np.int32))],
      {"counts_null": {"counts": None}, "effective_null": {"effective": None}, "S_neg": {"S": -1}, "S0": {"S": 0}, "T0": {"T": 0}})
    e("plan_packed", "lc3plus_plan_packed", None, False,
      [("sizes", B["pk_sizes"]), ("S", S), ("T", T), ("order", 0), ("capacity", 1 << 20), ("offsets", B["words"]), ("total", B["words2"]), ("overflow", B["words3"].view(np.uint8))],
      dict(n0, sizes_null={"sizes": None}, offsets_null={"offsets": None}, order={"order": 2}, capacity_neg={"capacity": -1}, total_null={"total": None}))
    e("plan_placed", "lc3plus_plan_placed", None, False,
      [("fmt", 16), ("ch", ch), ("samples", N), ("offsets", B["offsets"]), ("n", S * T), ("capacity", 1 << 30), ("invalid", B["words"].view(np.uint8))],
      {"fmt": {"fmt": 17}, "fmt_chmajor": {"fmt": 16 | 0x200}, "ch0": {"ch": 0}, "samples0": {"samples": 0}, "n_neg": {"n": -1}, "n0": {"n": 0},
       "capacity_neg": {"capacity": -1}, "offsets_null": {"offsets": None}, "invalid_null": {"invalid": None}})
    e("frame_info_side", "lc3plus_frame_info_side", None, False,
      [("fs", fs), ("ch", ch), ("ms", ms), ("hr", hr), ("frame", B["frame"]), ("nb", nb), ("info", B["words"].view(np.int32))],
      dict(hook_bad, frame_null={"frame": None}, info_null={"info": None}, nb0={"nb": 0}, nb_bad={"nb": 5 * ch}))
    for decoder in (0, 1):
        e("stream_state_header_%s" % ("dec" if decoder else "enc"), "lc3plus_stream_state_header", None, False,
          [("decoder", decoder), ("fs", fs), ("ch", ch), ("ms", ms), ("hr", hr), ("header", B["words"].view(np.uint32))],
          dict(geom_bad, header_null={"header": None}, ms_unsupported={"fs": 8000, "ms": 2.5}))
    e("stream_list_check", "lc3plus_stream_list_check", None, False, [("n_streams", S), ("streams", B["streams"]), ("n", 2)],
      {"streams_null": {"streams": None}, "n0": {"n": 0}, "n_streams0": {"n_streams": 0}, "twice": {"streams": B["streams_twice"]}, "range": {"streams": B["streams_range"]}})
    e("shard_block", "lc3plus_shard_block", None, False, [("n_streams", S), ("n_shards", 2), ("shard", 1), ("first", B["words"]), ("count", B["words2"])],
      {"first_null": {"first": None}, "count_null": {"count": None}, "n_streams_neg": {"n_streams": -1}, "n_shards0": {"n_shards": 0}, "shard_neg": {"shard": -1},
       "shard_high": {"shard": 2}})
    return E


def apply_state(L, kind, h, state, B):
    """Brings a batch into the named state with calls that succeed."""
    g = B.g
    if state == PLACED:
        assert getattr(L, "lc3plus_%s_batch_set_pcm_placement" % kind)(h, DEV2 + 0x800, 1 << 20) == 0
    elif state == RAGGED:
        assert getattr(L, "lc3plus_%s_batch_set_frame_counts" % kind)(h, DEV2 + 0x900) == 0
    elif state == UNSAFE:                                            # a value set_bandwidth takes whose cut-off line is below 1
        L.lc3plus_enc_batch_set_bandwidth(h, 1, 10)                  # (refused in hrmode: the batch stays as it is)
    elif state == STALE and kind == "enc":                           # the configuration is on the device only, the stride bound raised to 300
        rc = L.lc3plus_enc_batch_encode_rates_device(h, DEV, 16, DEV2, None, T, DEV + 0x1000, max(300, g["nb"]), None, None, None, 0)
        assert rc == 0, rc
    elif state == STALE:
        assert L.lc3plus_dec_batch_decode_sizes_device(h, DEV, B.stride, DEV2, None, T, DEV + 0x4000, 16, None, None, 0) == 0


def run_case(L, B, entry, overrides):
    fn, kind, sharded, good, _ = entry
    vals = dict(good)
    states = [k for k in overrides if k in (PLACED, RAGGED, UNSAFE, STALE)]
    vals.update({k: v for k, v in overrides.items() if k not in states})
    h = make(L, B, kind, sharded) if kind else None
    if kind and not sharded:
        for s in (PLACED, RAGGED, UNSAFE, STALE):                    # a fixed order, whatever the order of the pair
            if s in states:
                apply_state(L, kind, h, s, B)
    if isinstance(vals.get("blob"), str):                          # two blobs with the batch's header
        size = getattr(L, "lc3plus_%s_batch_stream_state_size" % kind)(h)
        hdr = np.zeros(4, np.uint32)
        assert L.lc3plus_stream_state_header(kind == "dec", B.g["fs"], B.g["ch"], B.g["ms"], B.g["hr"], hdr.ctypes.data) == 0
        B.b["blobs"] = np.zeros(2 * size, np.uint8)
        for i in range(2):
            B.b["blobs"][i * size:i * size + 16] = hdr.view(np.uint8)
        vals["blob"] = B.b["blobs"]
    args = [h if v is H else (C.addressof(v) if isinstance(v, C.Array) else ptr(v)) for v in (vals[k] for k, _ in good)]
    rc = getattr(L, fn)(*args)
    if fn.endswith("_create"):                                       # a create that succeeded: the handle goes again
        out = vals["out"]
        if rc == 0 and out is not None and out[0]:
            drop(L, fn.split("_")[1], "sharded" in fn, C.c_void_p(int(out[0])))
            out[0] = 0
    if fn.endswith("sharded_shard"):
        rc = int(bool(rc))                                           # a pointer: there or not
    if h is not None:
        drop(L, kind, sharded, h)
    return int(rc)


def refusals(L):
    table = {}
    for gname, g in GEOMS.items():
        B = Bufs(g)
        for name, entry in entries(B).items():
            bad = entry[4]
            row = {"good": run_case(L, B, entry, {})}
            for k in sorted(bad):
                row[k] = run_case(L, B, entry, bad[k])
            for k1, k2 in itertools.combinations(sorted(bad), 2):
                if set(bad[k1]) & set(bad[k2]):
                    continue                                         # the two change the same argument
                row[k1 + " & " + k2] = run_case(L, B, entry, dict(bad[k1], **bad[k2]))
            table["%s %s" % (gname, name)] = row
    return table


# ------------------------------------------------------------------------------------------------------------------------------------------------
# part 2: the state scripts
# ------------------------------------------------------------------------------------------------------------------------------------------------
class Script:
    """One call sequence on one handle: every call's name and result, then the logs and the getters."""

    def __init__(self, L, B, kind, sharded=False):
        self.L, self.B, self.kind, self.sharded, self.calls = L, B, kind, sharded, []
        L.lc3stub_reset()
        L.lc3stub_cfg_enable(1)
        self.h = make(L, B, kind, sharded)
        self.pre = "lc3plus_%s_%s_" % (kind, "sharded" if sharded else "batch")

    def call(self, name, *args):
        rc = getattr(self.L, self.pre + name)(self.h, *[C.addressof(a) if isinstance(a, C.Array) else ptr(a) for a in args])
        self.calls.append([name, int(rc)])
        return rc

    def note(self, text):
        self.calls.append([text, None])

    def logs(self):
        L = self.L
        n = L.lc3stub_log(None, 0)
        recs = (Rec * max(n, 1))()
        assert L.lc3stub_log(recs, n) == n
        m = L.lc3stub_cfg_log(None, 0)
        text = C.create_string_buffer(m + 1)
        assert L.lc3stub_cfg_log(text, m) == m
        per_ctx = {}
        for line in text.raw[:m].decode().splitlines():
            ev = json.loads(line)
            if "rec" in ev:
                r = recs[ev.pop("rec")]
                assert KINDS[r.kind] == ev["call"] and r.ctx == ev["ctx"]
                ev.update(dec=r.dec, n_frames=r.n_frames, stride=r.stride, fmt=r.fmt, on_device=r.on_device, sync=r.sync, p=[self.B.name_of(p) for p in r.p],
                          a=list(r.a), b=list(r.b), bytes=r.bytes, hip_stream=r.hip_stream)
            per_ctx.setdefault(str(ev.pop("ctx")), []).append(ev)   # the shards' workers run side by side: the order is per context
        return per_ctx

    def done(self):
        f = lambda n, *a: int(getattr(self.L, self.pre + n)(self.h, *a))
        log = self.logs()                                            # before the getters: they may read the configuration back
        if self.kind == "enc":
            getters = {"stride": f("stride"), "num_bytes": [f("num_bytes", s) for s in range(S)], "bandwidth": [f("bandwidth", s) for s in range(S)]}
        else:
            getters = {"num_bytes": [f("num_bytes", s) for s in range(S)]}
        after = {c: ev[len(log.get(c, [])):] for c, ev in self.logs().items()}      # what the getters added: the read-backs
        self.L.lc3stub_cfg_enable(0)
        drop(self.L, self.kind, self.sharded, self.h)
        return {"calls": self.calls, "log": log, "getters": getters, "log_of_getters": after}


def scripts(L):
    out = {}
    for gname in ("mono", "stereo"):
        B = Bufs(GEOMS[gname])
        g, st = B.g, B.stride
        nb, nb2 = g["nb"], g["nb2"]
        enc = lambda s, stride=st, sync=1, hs=None: s.call("encode", B["pcm"], 0, 16, T, B["out"], stride, 0, hs, sync)
        enc_rates = lambda s, rates, hs=HSTREAM: s.call("encode_bitrates", B["pcm"], 0, 16, rates, T, B["out"], st, 0, B["nb_out"], hs, 0)
        enc_bws = lambda s, bws, rates=None, hs=HSTREAM: s.call("encode_bandwidths", B["pcm"], 0, 16, bws, rates, T, B["out"], st, 0, B["nb_out"], hs, 0)
        enc_dev = lambda s, rates=DEV2, bws=None, stride=st: s.call("encode_rates_device", DEV, 16, rates, bws, T, DEV + 0x1000, stride, None, None, HSTREAM, 0)
        enc_pk = lambda s, rates=None, bws=None: s.call("encode_packed", DEV, 16, rates, bws, T, 0, DEV + 0x1000, 1 << 20, None, None, None, None, None, 0)

        def script(name, kind="enc", sharded=False):
            def deco(fn):
                s = Script(L, B, kind, sharded)
                fn(s)
                out["%s %s" % (gname, name)] = s.done()
                return fn
            return deco

        @script("set_bitrate then encode: the reset is consumed and uploaded once")
        def _(s):
            s.call("set_bitrate", 1, 32000 * g["ch"])                # below the attack detector's range: a one-shot reset
            enc(s); enc(s)

        @script("encode_bitrates whose last rate differs: restride, async whole upload")
        def _(s):
            enc_rates(s, B["rates"]); enc_rates(s, B["rates"])       # the second: nothing changes, nothing uploaded

        @script("encode_bitrates ending on the rate in force, a reset pending")
        def _(s):
            s.call("set_bitrate", 2, 32000 * g["ch"])
            enc_rates(s, i32([[g["rate2"], g["rate"]], [g["rate"], g["rate"]], [g["rate"], 32000 * g["ch"]]]))

        @script("encode_bandwidths changing the bandwidth only: bw_only")
        def _(s):
            enc_bws(s, B["bws"]); enc_bws(s, B["bws"])

        @script("encode_bandwidths with rates")
        def _(s):
            enc_bws(s, B["bws"], B["rates"]); enc_bws(s, B["bws"], B["rates"])

        @script("encode_bandwidths with rates that stay: bandwidth words only")
        def _(s):
            enc_bws(s, B["bws"], i32([[g["rate2"], g["rate"]]] * S))

        @script("a refused bandwidth: LC3_BW_WARNING through to the result")
        def _(s):
            enc_bws(s, B["bws_refused"]); enc_bws(s, B["bws_refused"], B["rates"])

        @script("encode_bandwidths: a pending reset makes the upload whole")
        def _(s):
            s.call("set_bitrate", 0, 32000 * g["ch"])
            enc_bws(s, B["bws"])

        @script("encode_rates_device then num_bytes: one download")
        def _(s):
            enc_dev(s)
            s.call("num_bytes", 0); s.call("num_bytes", 1); s.call("stride")

        @script("encode_rates_device then encode below and above the bound")
        def _(s):
            enc_dev(s, stride=300)
            enc(s, stride=299); enc(s, stride=300); enc(s, stride=nb)       # the last after no read-back: still refused below the bound

        @script("encode_rates_device with bandwidths only keeps the bound at stride()")
        def _(s):
            enc_dev(s, rates=None, bws=DEV2, stride=300)
            enc(s, stride=nb); enc(s, stride=nb - 1)

        @script("set_bitrate then encode_rates_device: the pending reset goes with the call")
        def _(s):
            s.call("set_bitrate", 1, 32000 * g["ch"])
            enc_dev(s); enc_dev(s)
            enc(s)

        @script("set_bandwidth below cut bin 1 then encode_rates_device with and without bandwidths")
        def _(s):
            s.call("set_bandwidth", 1, 10)
            enc_dev(s, bws=DEV2 + 0x100); enc_dev(s); enc_dev(s, bws=DEV2 + 0x100)
            s.call("set_bandwidth", 1, 8000)
            enc_dev(s, bws=DEV2 + 0x100)                             # (the copy is read back, the stub's download changes nothing: 10 is gone, the flag clears)

        @script("set_bandwidth below cut bin 1 then encode_packed and encode_bandwidths")
        def _(s):
            s.call("set_bandwidth", 2, 10)
            enc_pk(s, bws=DEV2 + 0x100); enc_pk(s, rates=DEV2); enc_bws(s, B["bws"])

        @script("frame counts on, encode_packed with no words, frame counts off, encode: a read-back before the launch")
        def _(s):
            s.call("set_bitrate", 1, 32000 * g["ch"])
            s.call("set_frame_counts", DEV2 + 0x900)
            enc_pk(s)
            enc(s)                                                   # refused while the counts are on
            s.call("set_frame_counts", None)
            enc(s); enc(s)

        @script("encode_packed with no words ends like encode; with rates the bound is the geometry's")
        def _(s):
            s.call("set_bitrate", 0, 32000 * g["ch"])
            enc_pk(s); enc_pk(s)
            enc_pk(s, rates=DEV2)
            enc(s, stride=st); enc(s, stride=400 * g["ch"]); enc_pk(s)

        @script("reset_streams with and without rates")
        def _(s):
            s.call("reset_streams", B["streams"], 2, None, None, 1)
            s.call("reset_streams", B["streams"], 2, B["two_rates"], HSTREAM, 0)
            s.call("reset_streams", B["streams"], 2, B["two_rates_bad"], None, 1)
            enc(s, stride=nb); enc(s, stride=nb2)

        @script("reset_streams with rates while stale: a download first")
        def _(s):
            enc_dev(s)
            s.call("reset_streams", B["streams"], 2, B["two_rates"], None, 1)

        @script("export and import")
        def _(s):
            s.call("export_streams", B["streams"], 2, B["blob"], 0, None, 1)
            s.call("export_streams", B["streams"], 2, DEV, 1, HSTREAM, 0)
            s.call("import_streams", B["streams"], 2, DEV, 1, B["status"], HSTREAM, 0)
            s.call("import_streams", B["streams"], 2, B["blob"], 0, B["status"], None, 1)       # no header in it: refused before anything is queued

        dec = lambda s, stride=st: s.call("decode", B["out"], 0, stride, B["bfi"], T, B["pcm"], 0, 16, B["status"], None, 1)
        dec_sizes = lambda s, sizes: s.call("decode_sizes", B["out"], 0, st, sizes, B["bfi"], T, B["pcm"], 0, 16, B["status"], None, 1)
        dec_dev = lambda s: s.call("decode_sizes_device", DEV, st, DEV2, None, T, DEV + 0x4000, 16, None, HSTREAM, 0)

        @script("decode_sizes whose end sizes change: an upload", "dec")
        def _(s):
            dec_sizes(s, B["sizes"]); dec_sizes(s, B["sizes"])       # stream 0 loses its last frame: it ends on nb, the others on nb2
            dec_sizes(s, i32([[nb2, nb2]] * S))

        @script("decode_sizes_device then set_num_bytes: a download first", "dec")
        def _(s):
            dec_dev(s)
            s.call("set_num_bytes", 1, nb2); s.call("set_num_bytes", 2, nb2)
            dec(s)

        @script("decode_packed then decode: a download first", "dec")
        def _(s):
            s.call("decode_packed", DEV, 1 << 20, DEV2 + 0x100, DEV2, st, None, T, DEV + 0x4000, 16, None, None, 0)
            dec(s, stride=nb - 1); dec(s)

        @script("decoder reset_streams while stale", "dec")
        def _(s):
            s.call("reset_streams", B["streams"], 2, B["two_sizes"], None, 1)
            dec_dev(s)
            s.call("reset_streams", B["streams"], 2, i32([nb, nb2]), HSTREAM, 0)      # the host copy stays stale and is not written
            s.call("reset_streams", B["streams"], 2, None, None, 1)
            s.call("reset_streams", B["streams"], 2, B["two_sizes_bad"], None, 1)

        @script("decoder export and import", "dec")
        def _(s):
            s.call("export_streams", B["streams"], 2, B["blob"], 0, None, 1)
            s.call("import_streams", B["streams"], 2, DEV, 1, None, HSTREAM, 0)

        sh_enc = lambda s, bws=None, rates=None, stride=st: s.call("encode", B["pcm"], 16, bws, rates, T, B["out"], stride, B["nb_out"])

        def nb_out(s):
            s.note("num_bytes out: %s" % B["nb_out"].tolist())
            B["nb_out"][:] = -7

        @script("sharded encode, plain, with rates and with bandwidths, each with num_bytes out", "enc", True)
        def _(s):
            sh_enc(s); nb_out(s)
            sh_enc(s, rates=B["rates"]); nb_out(s)
            sh_enc(s, bws=B["bws"]); nb_out(s)
            sh_enc(s, bws=B["bws_refused"], rates=i32([[g["rate2"], g["rate"]]] * S)); nb_out(s)

        @script("a sharded encode whose second shard refuses", "enc", True)
        def _(s):
            sh_enc(s, rates=B["rates_bad"]); nb_out(s)               # the bad rate is in the second shard's rows: nothing runs on either
            sh_enc(s, bws=B["bws_neg"], rates=B["rates_bad"])
            sh_enc(s, stride=nb - 1)
            L.lc3stub_fail_ctx(1)
            s.note("the stub fails the second shard's context")
            sh_enc(s); nb_out(s)
            sh_enc(s, rates=B["rates"]); nb_out(s)
            L.lc3stub_fail_ctx(-1)
            sh_enc(s)

        @script("sharded encode_device and the setters", "enc", True)
        def _(s):
            s.call("set_bitrate", 2, g["rate2"]); s.call("set_bandwidth", 2, 8000); s.call("set_bitrate", 0, 32000 * g["ch"])
            s.call("encode_device", B["ptrs_a"], 16, T, B["ptrs_b"], st, B["ptrs_hs"], 1)
            s.call("encode_device", B["ptrs_a"], 16, T, B["ptrs_b"], nb2 - 1, None, 0)

        @script("sharded decode with sizes", "dec", True)
        def _(s):
            s.call("decode", B["out"], st, B["sizes"], B["bfi"], T, B["pcm"], 16, B["status"])
            s.call("decode", B["out"], st, None, B["bfi"], T, B["pcm"], 16, B["status"])
            s.call("decode", B["out"], st, B["sizes_bad"], B["bfi"], T, B["pcm"], 16, B["status"])
            s.call("set_num_bytes", 2, nb)
            s.call("decode_device", B["ptrs_a"], st, T, B["ptrs_b"], 16, None, 1)

        for kind in ("enc", "dec"):
            @script("sharded %s state round trip" % kind, kind, True)
            def _(s):
                size = getattr(L, s.pre + "state_size")(s.h)
                s.note("state_size %d" % size)
                B["state"][:] = 0xEE
                s.call("get_state", B["state"], size)
                s.note("state %s" % [int(B["state"][i]) for i in (0, size // 2, size - 1, size)])       # the stub fills a shard's slice with its context number
                s.call("set_state", B["state"], size)
                s.call("get_state", B["state"], size - 1)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the file's form: small enough to read.  A refusal row is the good call's code, the singles' codes in the order of "cases", and the pairs as one string per first
# case i: the codes of (i, j) for j > i, "x" where the two change the same argument; geometries that answer alike share one row.  A log event is a list: the call,
# then the values of log_fields[kind of the call]; an uploaded entry is the values of log_fields["enc entry"] or ["dec entry"].
# ------------------------------------------------------------------------------------------------------------------------------------------------
LOG_FIELDS = {"launch": ["dec", "n_frames", "stride", "fmt", "on_device", "sync", "p", "a", "b", "bytes", "hip_stream"],
              "configuration": ["first", "count", "bw_only", "mode", "on_stream", "sync", "entries"],
              "device words": ["n_frames", "stride", "fmt", "has_a", "has_b", "lim", "clear_resets", "capacity", "sync"],
              "list": ["blob_on_device", "hdr", "streams"],
              "enc entry": ["nbytes", "bitrate", "bandwidth", "bw_cut_bin", "bw_index", "reset_attack"], "dec entry": ["nbytes", "in_off"]}


def compact_event(ev):
    kind = "launch" if "p" in ev else "configuration" if "entries" in ev else "list" if "hdr" in ev else "device words"
    ev = dict(ev)
    if kind == "configuration":
        ev["entries"] = [[x[f] for f in LOG_FIELDS["enc entry" if "bitrate" in x else "dec entry"]] for x in ev["entries"]]
    assert set(ev) == set(LOG_FIELDS[kind]) | {"call"}, ev
    return [ev["call"]] + [ev[f] for f in LOG_FIELDS[kind]]


def compact(ref, scr):
    table = {}
    for name in sorted({k.split(" ", 1)[1] for k in ref}):
        cases = [c for c in ref["mono " + name] if c != "good" and " & " not in c]
        rows = {}
        for g in GEOMS:
            r = ref["%s %s" % (g, name)]
            assert [c for c in r if c != "good" and " & " not in c] == cases
            row = {"good": r["good"], "single": [r[c] for c in cases],
                   "pairs": [",".join(str(r.get("%s & %s" % (a, b), "x")) for b in cases[i + 1:]) for i, a in enumerate(cases[:-1])]}
            same = [k for k, v in rows.items() if v == row]
            rows[same[0] + "," + g if same else g] = rows.pop(same[0]) if same else row
        table[name] = dict(rows, cases=cases)
    for s in scr.values():
        for part in ("log", "log_of_getters"):
            s[part] = {c: [compact_event(ev) for ev in evs] for c, evs in s[part].items()}
    return {"log_fields": LOG_FIELDS, "refusals": table, "scripts": scr}


def refusal_rows(doc):
    """The refusal table of a document as {"geometry entry": {case: code}}, pairs as "a & b"."""
    out = {}
    for name, e in doc["refusals"].items():
        cases = e["cases"]
        for gs, row in e.items():
            if gs == "cases":
                continue
            r = dict(zip(cases, row["single"]), good=row["good"])
            for i, line in enumerate(row["pairs"]):
                r.update({"%s & %s" % (cases[i], b): int(c) for b, c in zip(cases[i + 1:], line.split(",")) if c != "x"})
            for g in gs.split(","):
                out["%s %s" % (g, name)] = r
    return out


def generate(path=STUB):
    L = load(path)
    return compact(refusals(L), scripts(L))


def dumps(doc):
    """One line per refusal row and per script part: small, and a change shows as the lines it touches."""
    lines = ["{", ' "log_fields": %s,' % json.dumps(doc["log_fields"], sort_keys=True, separators=(",", ":")), ' "refusals": {']
    rows = sorted(doc["refusals"])
    for i, k in enumerate(rows):
        lines.append("  %s: %s%s" % (json.dumps(k), json.dumps(doc["refusals"][k], sort_keys=True, separators=(",", ":")), "," if i + 1 < len(rows) else ""))
    lines += [" },", ' "scripts": {']
    names = sorted(doc["scripts"])
    for i, k in enumerate(names):
        lines.append("  %s: {" % json.dumps(k))
        parts = sorted(doc["scripts"][k])
        for j, p in enumerate(parts):
            lines.append("   %s: %s%s" % (json.dumps(p), json.dumps(doc["scripts"][k][p], sort_keys=True, separators=(",", ":")), "," if j + 1 < len(parts) else ""))
        lines.append("  }%s" % ("," if i + 1 < len(names) else ""))
    lines += [" }", "}"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "audio_codec_amd", "csrc"), "stub"])
    text = dumps(generate(sys.argv[1] if len(sys.argv) > 1 else STUB))
    with open(OUT, "w") as f:
        f.write(text)
    print("%s: %d bytes" % (OUT, len(text)))
